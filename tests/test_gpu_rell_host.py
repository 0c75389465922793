"""GPU test of the Bio++ mirror's RELL resampling (tests/cpp/test_rell_gpu.cpp): the local
bootstrap of an NNI-searched tree (NNIHomogeneousTreeLikelihood::computeLocalBootstrap) on 2000
simulated sites of a 12-taxon tree with one branch of length 1e-3, and
PairedSiteLikelihoods::computeExpectedLikelihoodWeights against a plain host loop over the same
draws.  tests/test_rell_cpu.py confirms the support figures for this alignment without a device."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_rell_resampling():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_rell_gpu")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
