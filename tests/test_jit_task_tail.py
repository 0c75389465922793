"""The task tail of the one-class-per-workgroup wave-task kernel (plk_jit.hpp reduce_root_cls and
the code rotation) from the code object, without a GPU.

tests/jit/jit_emit_wp.cpp emits the tree4q program (plk_jit_tree4c: a quad, a cherry and a tip
under the root) with the task pool on and off; each source is cross-compiled for gfx950 and the
task loop -- the backward-branch range that holds the non-temporal root-term stores -- is read:

  - loads.  The only global loads in the loop are the two code-prefetch loads of the next task
    (one per pattern of the lane; this program has three units, so the compiler narrows each
    16-byte word to the one dword in use).  The parent's loop held twelve: those two and ten
    global_load_dwordx2 of pi[0..3] and probs[c0], five per pattern of the lane, each behind its
    own s_waitcnt vmcnt(0);
  - stores.  Walking the loop in execution order (cyclically) from either root-term store, the
    next task's code-prefetch loads come before any s_waitcnt vmcnt: the stores drain under the
    next task's arithmetic.  (In the parent the second store was followed by vmcnt(1) and
    vmcnt(0) at the code rotation.)  In address order no such wait stands between the last
    store and the loop's back edge;
  - resources, against the parent's object of the same program (its emitter built once at the
    parent commit; pool off / on): vgpr_count 76 / 76, sgpr_spill_count 30 / 36, no scratch, no
    spilled vector register.  Now 76 / 76 and 30 / 30;
  - still two barriers, none in a loop.

The every-class-in-the-wave program (ciw, reduce_root) keeps reading pi and the probabilities
through the argument block: its loop is not changed.
"""
import os
import re
import subprocess

import pytest

from test_jit_wave_tasks import HIPCC, NAMES, OBJDUMP, READELF, ROOT, _loop_barriers, _note

pytestmark = pytest.mark.skipif(HIPCC is None or not os.path.exists(OBJDUMP) or not os.path.exists(READELF),
                                reason="hipcc / llvm-objdump / llvm-readelf not available")

KIND = "tree4q"
PARENT = {0: {"vgpr_count": 76, "sgpr_spill_count": 30}, 1: {"vgpr_count": 76, "sgpr_spill_count": 36}}
PARENT_LOOP_LOADS = 12      # 2 code-prefetch loads + 10 loads of pi[0..3] and probs[c0]


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    """{wp: (source, disassembly, metadata notes)}, each kernel compiled once."""
    d = tmp_path_factory.mktemp("jit_task_tail")
    exe = str(d / "jit_emit_wp")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "bpp-phyl_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "jit", "jit_emit_wp.cpp")],
                   check=True, capture_output=True, timeout=600)
    out = {}
    for wp in (0, 1):
        src = subprocess.run([exe, KIND, str(wp)], check=True, capture_output=True, timeout=60).stdout.decode()
        path = d / f"k_{wp}.hip"
        path.write_text("#include <hip/hip_runtime.h>\n" + src)
        co = str(path) + ".co"
        r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output",
                            "-O3", "-c", "-o", co, str(path)], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        dis = subprocess.run([OBJDUMP, "-d", co], check=True, capture_output=True, timeout=120).stdout.decode()
        notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, timeout=120).stdout.decode()
        out[wp] = (src, dis, notes)
    return out


def _task_loop(dis):
    """The task loop's instructions [(address, text)] in address order: the widest backward-branch
    range of the kernel that holds a non-temporal global store."""
    ins, base = [], None
    for line in dis.splitlines():
        m = re.match(r"^([0-9A-Fa-f]+) <(\w+)>:", line)
        if m and m.group(2) == NAMES[KIND]:
            base = int(m.group(1), 16)
        m = re.search(r"^\s*(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m:
            ins.append((int(m.group(2), 16), m.group(1), line))
    assert base is not None and ins
    nt = [a for a, t, _ in ins if t.startswith("global_store") and re.search(r"\bnt\b", t)]
    assert nt
    lo = hi = None
    for a, t, line in ins:
        if t.startswith(("s_cbranch", "s_branch")):
            tg = re.search(r"<\w+\+0x([0-9A-Fa-f]+)>", line)
            assert tg, line
            tgt = base + int(tg.group(1), 16)
            if tgt <= a and any(tgt <= s <= a for s in nt):
                lo, hi = (tgt if lo is None else min(lo, tgt)), (a if hi is None else max(hi, a))
    assert lo is not None
    assert all(lo <= s <= hi for s in nt)              # the root-term stores are the loop's only nt stores
    return [(a, t) for a, t, _ in ins if lo <= a <= hi]


@pytest.mark.parametrize("wp", [0, 1])
def test_loop_loads_are_the_code_prefetch_only(objects, wp):
    loop = _task_loop(objects[wp][1])
    loads = [t for _, t in loop if t.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))]
    print(f"wp {wp}: loads in the task loop: {loads}")
    assert len(loads) == PARENT_LOOP_LOADS - 10 == 2
    assert all(re.match(r"global_load_dword(x4)? ", t) for t in loads), loads
    assert not any(t.startswith("global_load_dwordx2") for _, t in loop)          # pi / prob, as the parent read them


@pytest.mark.parametrize("wp", [0, 1])
def test_no_wait_behind_the_root_term_stores(objects, wp):
    loop = [t for _, t in _task_loop(objects[wp][1])]
    stores = [i for i, t in enumerate(loop) if t.startswith("global_store_dwordx2") and re.search(r"\bnt\b", t)]
    assert len(stores) == 2                             # two patterns per lane
    for i in stores:
        # execution order: on from the store, through the back edge, to the next task's prefetch.
        # (Pool off: the a.dyn block in front of the prefetch takes a ticket from the fragment's
        # global counter and waits for its return at once -- the parent's code, run only under
        # JIT_DYN=1; the walk ends there, the static stride branches around it.)
        for k in range(1, len(loop) + 1):
            t = loop[(i + k) % len(loop)]
            if t.startswith(("global_load", "global_atomic")):
                break
            assert not (t.startswith("s_waitcnt") and "vmcnt" in t), (wp, i, k, t)
        else:
            pytest.fail("no code-prefetch load in the loop")
    # ... and in address order none between the last store and the back edge
    assert not any(t.startswith("s_waitcnt") and "vmcnt" in t for t in loop[stores[-1]:])


@pytest.mark.parametrize("wp", [0, 1])
def test_resources_not_above_the_parent(objects, wp):
    notes = objects[wp][2]
    got = {k: _note(notes, k) for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
    print(f"wp {wp}: {got}; parent {PARENT[wp]}")
    assert got["private_segment_fixed_size"] == 0       # no scratch
    assert got["vgpr_spill_count"] == 0
    assert got["vgpr_count"] <= PARENT[wp]["vgpr_count"]
    assert got["sgpr_spill_count"] <= PARENT[wp]["sgpr_spill_count"]
    n, inside = _loop_barriers(objects[wp][1])
    assert (n, inside) == (2, 0)                        # after the staging, and behind the loop


def test_root_constants_are_read_per_launch(objects):
    """From the source: the constants are loaded from the argument block's pointers in front of
    the loop (never numbers in the text), reduce_root_cls takes them as values, and JArgs keeps
    its fields."""
    for wp in (0, 1):
        src = objects[wp][0]
        head, loop = src.split("for (int tk_nx = 0; tk < a.n_tasks; tk = tk_nx) {")
        assert "uniform_d(a.pi[s_])" in head and "uniform_d(a.probs[c0])" in head
        assert "a.pi" not in loop and "a.probs" not in loop
        assert "reduce_root_cls<PW_>(a, A0, rpi_, rpr_, c0, p, gv);" in loop
        assert loop.index("ROT_\n") < loop.index("reduce_root_cls<PW_>(")
        assert "i32 n_tasks;  // wave tasks (64 * PW_ patterns each)\n};" in head
