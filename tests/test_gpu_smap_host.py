"""GPU test of the Bio++ mirror's DeviceStochasticMapping (tests/cpp/test_smap_gpu.cpp): its means
equal the sums of plk_smap_sample on a handle set up by hand; state frequencies within 6 binomial
standard errors of MarginalAncestralStateReconstruction; the total register's mean counts within 6
standard errors of SubstitutionMappingTools::computeSubstitutionVectors; kept replicates keep the
resolved leaves and their dwelling times sum to the branch length."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_stochastic_mapping():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_smap_gpu")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
