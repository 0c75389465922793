"""Workgroup task pool (plk_jit.hpp JitShape::wp) from the source and the code object, without a GPU.

tests/jit/jit_emit_wp.cpp emits the two direct-code wave-task programs -- one class per workgroup
with a quad unit (plk_jit_tree4c) and every class in the wave with rescaling (plk_jit_tree4) --
with the pool on and off.

  - without the pool the source is the wave-task program's text as tests/jit/jit_emit_wt.cpp
    emits it (the emitter called with wp = false), and names neither the pool's LDS word nor its
    map: cached code objects of the programs without it stay valid;
  - both are cross-compiled for gfx950: no scratch, no spilled register, a VGPR count not above
    the wave-task program's, static LDS larger by exactly one word, and no barrier in a loop;
  - the ticket -> task map (jit_pool_task; the generated kernel's POOL_TASK_ is the same
    expression's text) deals every task exactly once, evenly, and never comes back inside.
"""
import os
import subprocess

import pytest

from test_jit_wave_tasks import HIPCC, NAMES, OBJDUMP, READELF, ROOT, _loop_barriers, _note

pytestmark = pytest.mark.skipif(HIPCC is None or not os.path.exists(OBJDUMP) or not os.path.exists(READELF),
                                reason="hipcc / llvm-objdump / llvm-readelf not available")

POOL_WORD = "tk_pool_"
POOL_MAP = "POOL_TASK_"


def _build(d, name):
    exe = str(d / name)
    subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "bpp-phyl_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "jit", name + ".cpp")],
                   check=True, capture_output=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def emitters(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_emit_wp")
    return _build(d, "jit_emit_wp"), _build(d, "jit_emit_wt"), d


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, timeout=60).stdout.decode()


@pytest.fixture(scope="module")
def objects(emitters):
    """{(kind, wp): (source, disassembly, metadata notes)}, each kernel compiled once."""
    wp_exe, _, d = emitters
    out = {}
    for kind in NAMES:
        for wp in (0, 1):
            src = _run(wp_exe, kind, wp)
            path = d / f"k_{kind}_{wp}.hip"
            path.write_text("#include <hip/hip_runtime.h>\n" + src)
            co = str(path) + ".co"
            r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only",
                                "--no-gpu-bundle-output", "-O3", "-c", "-o", co, str(path)],
                               capture_output=True, timeout=600)
            assert r.returncode == 0, r.stderr.decode()[-4000:]
            dis = subprocess.run([OBJDUMP, "-d", co], check=True, capture_output=True, timeout=120).stdout.decode()
            notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, timeout=120).stdout.decode()
            out[(kind, wp)] = (src, dis, notes)
    return out


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_source_without_the_pool_is_the_wave_task_text(emitters, kind):
    wp_exe, wt_exe, _ = emitters
    off, on, wt = _run(wp_exe, kind, 0), _run(wp_exe, kind, 1), _run(wt_exe, kind, 1)
    assert off == wt                                       # byte for byte
    assert POOL_WORD not in off and POOL_MAP not in off
    assert POOL_WORD in on and POOL_MAP in on
    # the pool program takes no global ticket and does not read a.dyn in its loop
    assert "a.dyn" in off
    loop = on[on.index("for (int tk_nx = 0; tk < a.n_tasks; tk = tk_nx) {"):]
    assert "a.dyn" not in loop and "sbc_" not in loop and "__HIP_MEMORY_SCOPE_AGENT" not in loop.split("a.exit_ctr")[0]
    assert "i32 n_tasks;" in on and f"void {NAMES[kind]}(" in on


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_pool_kernel_registers_and_lds(objects, kind):
    off, on = objects[(kind, 0)][2], objects[(kind, 1)][2]
    print(f"{kind}: vgpr wp off {_note(off, 'vgpr_count')}, wp on {_note(on, 'vgpr_count')}; static LDS "
          f"{_note(off, 'group_segment_fixed_size')} -> {_note(on, 'group_segment_fixed_size')}")
    assert _note(on, "private_segment_fixed_size") == 0       # no scratch
    assert _note(on, "vgpr_spill_count") == 0
    assert _note(on, "vgpr_count") <= _note(off, "vgpr_count")
    assert _note(on, "agpr_count") <= _note(off, "agpr_count")
    # one word more: the metadata rounds the static segment up to the 16-byte alignment of the
    # dynamic array (the tables) that follows it, so 4 more bytes read as the next multiple of 16
    assert _note(on, "group_segment_fixed_size") == (_note(off, "group_segment_fixed_size") + 4 + 15) // 16 * 16
    src_off, src_on = objects[(kind, 0)][0], objects[(kind, 1)][0]
    assert src_on.count("__shared__") == src_off.count("__shared__") + 1
    assert src_on.count("__shared__ unsigned tk_pool_;") == 1


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_pool_loop_has_no_barrier(objects, kind):
    n_on, in_on = _loop_barriers(objects[(kind, 1)][1])
    assert in_on == 0
    assert n_on == 2              # after the staging, and behind the loop


def test_ticket_to_task_map(emitters):
    wp_exe, _, _ = emitters
    r = subprocess.run([wp_exe, "map"], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok", r.stdout.decode()[-2000:]
