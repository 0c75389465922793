"""CPU side of plk_node_posteriors: the entry point is declared, bound and exported, fails
cleanly without a handle, and the mirror's host-only ancestral helpers (argmax with ties,
one-hot leaves, sampling, pattern -> site expansion) pass their stand-alone program, built
plainly and with ASan + UBSan.  Nothing loaded into Python runs under a sanitizer."""
import ctypes as ct
import os
import re
import subprocess

import plk
from conftest import run_make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_INC = os.path.join(ROOT, "bpp-phyl_amd", "host", "include")
SRC = os.path.join(ROOT, "tests", "standalone", "ancestral_helpers_check.cpp")


def _ensure_built():
    if not os.path.exists(plk.LIB_PATH):
        run_make("-s", "-C", os.path.join(ROOT, "bpp-phyl_amd"))


def test_header_declares_node_posteriors():
    hdr = open(os.path.join(ROOT, "include", "plk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+plk_node_posteriors\s*\(([^;]*)\)\s*;", code)
    assert m, "plk_node_posteriors is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7
    assert args[0].startswith("plk_handle") and "int32_t*" in args[2] and "uint8_t*" in args[6]
    assert sum("double*" in a for a in args) == 3
    assert re.search(r"#define\s+PLK_ABI_VERSION\s+2\b", hdr)      # additive: the version stays


def test_binding_lists_node_posteriors():
    assert "plk_node_posteriors" in plk.EXPORTS
    assert callable(getattr(plk.Engine, "node_posteriors", None))


def test_library_exports_node_posteriors():
    _ensure_built()
    out = subprocess.run(["nm", "-D", "--defined-only", plk.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT plk_node_posteriors$", out, flags=re.M)


def test_null_handle_is_an_argument_error():
    _ensure_built()
    lib = plk.load()
    nodes = (ct.c_int32 * 1)(4)
    best = (ct.c_uint8 * 8)()
    assert lib.plk_node_posteriors(None, 1, nodes, None, None, None, best) == -1
    assert b"null handle" in lib.plk_last_error(None)


def _build_and_run(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", *extra, "-I", HOST_INC, "-o", exe, SRC],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("PASSED"), r.stdout


def test_ancestral_helpers(tmp_path):
    _build_and_run(tmp_path, "helpers", ["-O2"])


def test_ancestral_helpers_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "helpers_san", ["-O0", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=all"])
