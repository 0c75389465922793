"""GPU test of the Bio++ mirror's parsimony classes (tests/cpp/test_parsimony_gpu.cpp):
DRTreeParsimonyScore on the reference's two goldens (score 9 with the gap as a state; score 3 and
its node states), and NNITopologySearch (BETTER and FAST) over it on 2000 simulated sites of a
10-taxon tree perturbed by three interchanges; one plk_pars_nni_scores call per round."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_parsimony():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_parsimony_gpu"), os.path.join(ROOT, "tests", "golden")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
