"""GPU test of the Bio++ mirror's route from an alignment to a refined tree
(tests/cpp/test_distance_gpu.cpp): DistanceEstimation (one plk_pair_distances call for all pairs)
equals a direct call, BioNJ on its matrix returns the true 12-taxon tree's bipartitions, and
NNITopologySearch (BETTER) from that tree makes no move."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_alignment_to_refined_tree():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_distance_gpu")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
