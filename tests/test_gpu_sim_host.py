"""GPU test of the Bio++ mirror's DeviceSequenceSimulator (tests/cpp/test_simulation_gpu.cpp): on
the non-homogeneous test's tree and on a homogeneous GTR + Gamma(4) tree the container equals
plk_simulate on a handle set up by hand, character by character; internal sequences only when
asked for; replicates differ; tip frequencies within 5 binomial standard deviations of pi; and
the simulated alignment prefers the generating branch lengths to doubled ones."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_simulation():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_simulation_gpu")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
