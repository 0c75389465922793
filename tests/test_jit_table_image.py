"""The table image of the one-class-per-workgroup kernel (plk_jit.hpp JitShape::img) from the code
object, without a GPU.

tests/jit/jit_emit_img.cpp emits the 7-tip program of tests/jit/jit_emit_wp.cpp (a quad, a cherry
and a tip under the root; C = 4, two patterns per lane, wave tasks, pool off / on) with the table
image on: one module with the traversal (plk_jit_tree4c) and the two builder kernels
(plk_jit_tabs4c, plk_jit_tabs4c_l).  Cross-compiled for gfx950:

  - the traversal's prologue is a copy: no fp64 arithmetic instruction stands in front of its first
    s_barrier (the table build left the kernel), and the copy's global loads are 16 bytes wide;
  - no scratch, no spilled vector register, and vgpr_count / sgpr_spill_count not above what
    tests/test_jit_task_tail.py records for the parent's kernel of this program: 76 and 30 / 36
    (pool off / on);
  - still two barriers, none in a loop;
  - the builder kernels have no scratch;
  - the task loop's text is the parent's, byte for byte (the emitter with the image off gives the
    source jit_emit_wp gives), and with the image on it differs from it only in front of the loop
    and behind the traversal.
"""
import os
import re
import subprocess

import pytest

from test_jit_wave_tasks import HIPCC, OBJDUMP, READELF, ROOT

pytestmark = pytest.mark.skipif(HIPCC is None or not os.path.exists(OBJDUMP) or not os.path.exists(READELF),
                                reason="hipcc / llvm-objdump / llvm-readelf not available")

TRAV, BUILDERS = "plk_jit_tree4c", ("plk_jit_tabs4c", "plk_jit_tabs4c_l")
PARENT = {0: {"vgpr_count": 76, "sgpr_spill_count": 30}, 1: {"vgpr_count": 76, "sgpr_spill_count": 36}}
LOOP_HEAD = "for (int tk_nx = 0; tk < a.n_tasks; tk = tk_nx) {"
FP64 = re.compile(r"^v_(pk_)?(fma|fmac|mul|add|min|max|div|rcp|sqrt|ldexp|trig|frexp)\w*_f64")


def _build(d, name):
    exe = str(d / name)
    subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "bpp-phyl_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "jit", name + ".cpp")],
                   check=True, capture_output=True, timeout=600)
    return exe


def _run(exe, *args):
    return subprocess.run([exe, *map(str, args)], check=True, capture_output=True, timeout=60).stdout.decode()


@pytest.fixture(scope="module")
def emitters(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_table_image")
    return _build(d, "jit_emit_img"), _build(d, "jit_emit_wp"), d


@pytest.fixture(scope="module")
def objects(emitters):
    """{wp: (source, {kernel: [instruction text]}, {kernel: metadata note})}"""
    exe, _, d = emitters
    out = {}
    for wp in (0, 1):
        src = _run(exe, wp)
        path = d / f"k_{wp}.hip"
        path.write_text("#include <hip/hip_runtime.h>\n" + src)
        co = str(path) + ".co"
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output",
                            "-O3", "-c", "-o", co, str(path)], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        dis = subprocess.run([OBJDUMP, "-d", co], check=True, capture_output=True, timeout=120).stdout.decode()
        notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, timeout=120).stdout.decode()
        out[wp] = (src, _by_kernel(dis), _notes_by_kernel(notes))
    return out


def _by_kernel(dis):
    """{symbol: [(address, instruction text, line)]} of a llvm-objdump -d listing."""
    ks, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^([0-9A-Fa-f]+) <(\w+)>:", line)
        if m:
            cur = ks.setdefault(m.group(2), {"base": int(m.group(1), 16), "ins": []})
            continue
        m = re.search(r"^\s*(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and cur is not None:
            cur["ins"].append((int(m.group(2), 16), m.group(1), line))
    return ks


def _notes_by_kernel(notes):
    """{kernel name: its metadata entry's text} of llvm-readelf --notes (entries start at '- .agpr_count'
    or whichever key sorts first; every entry holds one '.name:')."""
    out = {}
    for entry in re.split(r"\n\s*- \.", notes):
        m = re.search(r"\.name:\s*(\w+)", entry)
        if m and re.search(r"vgpr_count:", entry):
            out[m.group(1)] = entry
    return out


def _note(entry, key):
    m = re.search(r"\b" + key + r":\s*(\d+)", entry)
    assert m, key
    return int(m.group(1))


@pytest.mark.parametrize("wp", [0, 1])
def test_prologue_is_a_copy(objects, wp):
    ins = [t for _, t, _ in objects[wp][1][TRAV]["ins"]]
    first = ins.index("s_barrier") if "s_barrier" in ins else next(i for i, t in enumerate(ins) if t.startswith("s_barrier"))
    head = ins[:first]
    fp = [t for t in head if FP64.match(t)]
    print(f"wp {wp}: {first} instructions in front of the first barrier, fp64 arithmetic among them: {fp}")
    assert not fp
    assert any(FP64.match(t) for t in ins[first:])                       # the pattern is not blind: the loop has them
    loads = [t for t in head if t.startswith("global_load")]
    wide = [t for t in loads if t.startswith("global_load_dwordx4")]
    lds = [t for t in head if t.startswith("ds_write_b128") or t.startswith("ds_write2_b64")]
    print(f"wp {wp}: global loads in the prologue {len(loads)} ({len(wide)} of 16 bytes), LDS stores {len(lds)}")
    assert len(wide) >= 3 and len(lds) >= 3                              # 1 104 doubles over 256 threads: three rounds of 16 B


@pytest.mark.parametrize("wp", [0, 1])
def test_resources_not_above_the_parent(objects, wp):
    e = objects[wp][2][TRAV]
    got = {k: _note(e, k) for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
    print(f"wp {wp}: {got}; parent {PARENT[wp]}")
    assert got["private_segment_fixed_size"] == 0
    assert got["vgpr_spill_count"] == 0
    assert got["vgpr_count"] <= PARENT[wp]["vgpr_count"]
    assert got["sgpr_spill_count"] <= PARENT[wp]["sgpr_spill_count"]


@pytest.mark.parametrize("wp", [0, 1])
def test_two_barriers_none_in_a_loop(objects, wp):
    k = objects[wp][1][TRAV]
    bars = [a for a, t, _ in k["ins"] if t.startswith("s_barrier")]
    back = []
    for a, t, line in k["ins"]:
        if t.startswith(("s_cbranch", "s_branch")):
            tg = re.search(r"<\w+\+0x([0-9A-Fa-f]+)>", line)
            assert tg, line
            if k["base"] + int(tg.group(1), 16) <= a:
                back.append((k["base"] + int(tg.group(1), 16), a))
    assert back                                                          # the task loop itself
    assert len(bars) == 2
    assert not [b for b in bars if any(lo <= b <= hi for lo, hi in back)]


@pytest.mark.parametrize("wp", [0, 1])
def test_builders_have_no_scratch(objects, wp):
    for name in BUILDERS:
        e = objects[wp][2][name]
        print(f"wp {wp} {name}: vgpr {_note(e, 'vgpr_count')}, LDS {_note(e, 'group_segment_fixed_size')} B")
        assert _note(e, "private_segment_fixed_size") == 0
        assert _note(e, "vgpr_spill_count") == 0
        assert any(FP64.match(t) for _, t, _ in objects[wp][1][name]["ins"])   # the build is here now


@pytest.mark.parametrize("wp", [0, 1])
def test_loop_text_is_the_parents(emitters, objects, wp):
    exe, exe_wp, _ = emitters
    parent = _run(exe_wp, "tree4q", wp)
    assert _run(exe, wp, 0) == parent                                    # image off: the same source
    src = objects[wp][0]
    assert src.count(LOOP_HEAD) == 1 and parent.count(LOOP_HEAD) == 1
    end = "  __syncthreads();\n  if (a.exit_ctr && threadIdx.x == 0) {"
    loop, loop_p = src.split(LOOP_HEAD)[1], parent.split(LOOP_HEAD)[1]
    assert loop.count(end) == 1 and loop_p.count(end) == 1
    assert loop.split(end)[0] == loop_p.split(end)[0]
    head = src.split(LOOP_HEAD)[0]
    assert "a.tab_img + ((i64)frag * C_ + c0) * TD_" in head and "kQuadD[q0_ + kk]" not in head
    assert "kQuadD[q0_ + kk]" in parent.split(LOOP_HEAD)[0]              # the build the image replaces
    assert "const double* tab_img;" in head and "i32 n_tasks;" in head
