"""csrc/plk_topo.hpp on the CPU: the tree view over topo_kids and the KOp lists of the path,
root-pair and preorder passes (order of the ops and grouping into launches included) against
the literal arrays of tests/standalone/topo_check.cpp.  The header needs no HIP, so the
program is built with the host compiler, plainly and with ASan + UBSan; it is stand-alone,
nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

from test_sanitizers import _SAN_ENV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpp-phyl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "standalone", "topo_check.cpp")


def test_header_is_host_only():
    inc = [l.split()[1] for l in open(os.path.join(CSRC, "plk_topo.hpp")) if l.startswith("#include")]
    assert sorted(inc) == sorted(["<cstdint>", "<cstring>", "<vector>", '"../../include/plk.h"'])
    assert '#include "plk_topo.hpp"' in open(os.path.join(CSRC, "plk_kernels.hpp")).read()


def _build_and_run(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-o", exe, SRC],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=_SAN_ENV)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("PASSED"), r.stdout


def test_topo_check(tmp_path):
    _build_and_run(tmp_path, "topo", ["-O2"])


def test_topo_check_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "topo_san", ["-O0", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                          "-fno-sanitize-recover=all"])
