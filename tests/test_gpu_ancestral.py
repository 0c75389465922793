"""GPU test of the mirror's ancestral reconstruction: tests/cpp/test_ancestral_gpu.cpp runs
MarginalAncestralStateReconstruction, DRTreeLikelihoodTools and the posterior-rate queries on
the MI355X against a brute-force sum over the ancestors' states and the rate classes."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_ancestral_reconstruction():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_ancestral_gpu")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
