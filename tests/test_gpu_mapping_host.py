"""GPU test of the Bio++ mirror's substitution mapping (tests/cpp/test_mapping_gpu.cpp):
SubstitutionMappingTools::computeSubstitutionVectors over DecompositionSubstitutionCount on
20000 simulated sites, with the total and the comprehensive register, a constant rate and
Gamma(4), and a user-defined count through the host-matrix path."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_substitution_mapping():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_mapping_gpu")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
