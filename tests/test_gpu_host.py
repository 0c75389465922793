"""GPU test of the C++ Bio++ API mirror: the drop-in test program
(tests/cpp/test_likelihood_gpu.cpp) runs the reference's test_likelihood /
test_likelihood_clock calls on the MI355X and checks their goldens."""
import os
import subprocess

import pytest

import plk
from conftest import run_make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def test_cpp_drop_in_goldens():
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    r = subprocess.run([os.path.join(HOST, "bin", "test_likelihood_gpu")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout


def test_cpp_drop_in_nh():
    """tests/cpp/test_likelihood_nh_gpu.cpp: the reference's test_likelihood_nh.cpp calls
    (simulated alignments, per-branch theta recovered within 0.2 for both root
    parametrisations), per-theta evaluations recomputing one eigen-system, and the
    BrLenRoot / RootPosition derivatives against central differences."""
    assert plk.device_count() > 0, "no GPU visible"
    run_make("-s", "-j8", "-C", HOST)
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    r = subprocess.run([os.path.join(HOST, "bin", "test_likelihood_nh_gpu")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout


@pytest.mark.parametrize("name,goldens", [
    ("test_likelihood", (85.030942031997312824, 65.72293577214308868406)),
    ("test_likelihood_clock", (94.3957, 71.2657, 92.3295, 71.2657)),
    ("test_likelihood_nh", ()),
])
def test_reference_likelihood_test_runs_unchanged(name, goldens, tmp_path):
    """The reference's own test program (the reference's test/<name>.cpp, compiled unchanged
    against the Bio++ mirror where the reference is present, by `make -C oracle ref` as build()
    runs it: oracle/_ref/ref_<name>) runs on the MI355X and passes its own checks (exit status
    0: the goldens at its 0.001 / 0.0001 tolerances, the SR vs DR derivatives, the NH theta
    recovery).  The printed -lnL values are also checked here, in the order the program
    prints them."""
    assert plk.device_count() > 0, "no GPU visible"
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_" + name)
    assert os.path.exists(exe), f"{exe} missing: build it where the reference is present (make -C oracle ref)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout[-6000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    vals = []
    for line in r.stdout.splitlines():
        try:
            vals.append(float(line.strip()))
        except ValueError:
            pass
    for g in goldens:
        assert any(abs(v - g) <= 1e-3 for v in vals), (g, vals)
    if name == "test_likelihood_clock":
        # the clock half: initial 92.3295 after the unconstrained fit, final 71.2657
        assert abs(vals[2] - 92.3295) <= 1e-3 and abs(vals[3] - 71.2657) <= 1e-3, vals
