"""GPU test of the Bio++ mirror's NNI topology search (tests/cpp/test_nni_gpu.cpp):
NNITopologySearch (BETTER and FAST) over NNIHomogeneousTreeLikelihood on 2000 simulated sites of
a 10-taxon tree perturbed by three interchanges; one plk_nni_scores call per round."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_nni_topology_search():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_nni_gpu")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
