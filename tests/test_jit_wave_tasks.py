"""Wave tasks (plk_jit.hpp JitShape::wt) from the code object, without a GPU.

tests/jit/jit_emit_wt.cpp emits the two direct-code programs whose waves share nothing in the
loop -- one class per workgroup with a quad unit (plk_jit_tree4c) and every class in the wave
with rescaling (plk_jit_tree4) -- with the wave-task schedule on and off.  Each source is
cross-compiled for gfx950 and the two code objects of a program are compared:

  - barriers.  The super-block schedule has one `__syncthreads()`, inside its loop.  Wave tasks
    keep two, both outside: one after the table staging and one in front of the exit ticket.  So
    a plain count of s_barrier instructions in the object cannot go down (1 -> 2, measured on
    both programs); what goes down is the count inside a loop, i.e. between the target of a
    backward branch and that branch, which is the count that costs time: >= 1 -> 0.  The test
    asserts that, and that the two barriers outside are all there is;
  - no scratch, no spilled vector register;
  - the VGPR count is not above the super-block kernel's, so occupancy cannot have dropped.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin") if HIPCC else ""
OBJDUMP = shutil.which("llvm-objdump") or os.path.join(LLVM, "llvm-objdump")
READELF = shutil.which("llvm-readelf") or os.path.join(LLVM, "llvm-readelf")

pytestmark = pytest.mark.skipif(HIPCC is None or not os.path.exists(OBJDUMP) or not os.path.exists(READELF),
                                reason="hipcc / llvm-objdump / llvm-readelf not available")

NAMES = {"tree4q": "plk_jit_tree4c", "ciw": "plk_jit_tree4"}


@pytest.fixture(scope="module")
def emitter(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_emit_wt")
    exe = str(d / "jit_emit_wt")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "bpp-phyl_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "jit", "jit_emit_wt.cpp")],
                   check=True, capture_output=True, timeout=600)
    return exe, d


def _emit(emitter, kind, wt):
    exe, _ = emitter
    return subprocess.run([exe, kind, str(wt)], check=True, capture_output=True, timeout=60).stdout.decode()


def _loop_barriers(dis):
    """(s_barrier instructions, those inside a loop) of a llvm-objdump -d listing: a loop is the
    address range from the target of a backward branch to that branch."""
    bars, loops = [], []
    for line in dis.splitlines():
        m = re.search(r"^\s*(s_\w+).*//\s*([0-9A-Fa-f]+):", line)
        if not m:
            continue
        op, addr = m.group(1), int(m.group(2), 16)
        if op == "s_barrier":
            bars.append(addr)
        elif op.startswith(("s_cbranch", "s_branch")):
            t = re.search(r"<\w+\+0x([0-9A-Fa-f]+)>", line)
            assert t, line
            loops.append((addr, int(t.group(1), 16)))
    assert loops
    # branch targets are offsets from the kernel's symbol: its address from a forward branch
    base = None
    for line in dis.splitlines():
        m = re.match(r"^([0-9A-Fa-f]+) <(\w+)>:", line)
        if m and m.group(2) in NAMES.values():
            base = int(m.group(1), 16)
    assert base is not None
    back = [(base + t, a) for a, t in loops if base + t <= a]
    assert back                                           # the persistent loop itself
    inside = [b for b in bars if any(lo <= b <= hi for lo, hi in back)]
    return len(bars), len(inside)


@pytest.fixture(scope="module")
def objects(emitter):
    """{(kind, wt): (source, disassembly, metadata notes)}, each kernel compiled once."""
    _, d = emitter
    out = {}
    for kind in NAMES:
        for wt in (0, 1):
            src = _emit(emitter, kind, wt)
            path = d / f"k_{kind}_{wt}.hip"
            path.write_text("#include <hip/hip_runtime.h>\n" + src)
            co = str(path) + ".co"
            r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only",
                                "--no-gpu-bundle-output", "-O3", "-c", "-o", co, str(path)],
                               capture_output=True, timeout=600)
            assert r.returncode == 0, r.stderr.decode()[-4000:]
            dis = subprocess.run([OBJDUMP, "-d", co], check=True, capture_output=True, timeout=120).stdout.decode()
            notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, timeout=120).stdout.decode()
            out[(kind, wt)] = (src, dis, notes)
    return out


def _note(notes, key):
    m = re.search(r"\." + key + r":\s*(\d+)", notes)
    assert m, key
    return int(m.group(1))


def test_default_shape_is_the_super_block_schedule(emitter):
    """JitShape::wt is off unless asked for: the wt-off source has the super-block loop and no
    trace of the wave-task one (n_tasks included: its JArgs ends where it did)."""
    for kind in NAMES:
        off, on = _emit(emitter, kind, 0), _emit(emitter, kind, 1)
        assert "sb_next_lds" in off and "n_tasks" not in off and "tk_nx" not in off
        assert "sb_next_lds" not in on and "i32 n_tasks;" in on and "tk_nx" in on
        assert f"void {NAMES[kind]}(" in off and f"void {NAMES[kind]}(" in on


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_wave_task_loop_has_no_barrier(objects, kind):
    n_off, in_off = _loop_barriers(objects[(kind, 0)][1])
    n_on, in_on = _loop_barriers(objects[(kind, 1)][1])
    print(f"{kind}: s_barrier total / in a loop: wt off {n_off} / {in_off}, wt on {n_on} / {in_on}")
    assert in_off >= 1            # the parent's per-super-block barrier
    assert in_on == 0             # fewer: none
    assert in_on < in_off
    assert n_on == 2              # after the staging, and in front of the exit ticket


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_wave_task_kernel_registers(objects, kind):
    off, on = objects[(kind, 0)][2], objects[(kind, 1)][2]
    print(f"{kind}: vgpr wt off {_note(off, 'vgpr_count')}, wt on {_note(on, 'vgpr_count')}")
    assert _note(on, "private_segment_fixed_size") == 0       # no scratch
    assert _note(on, "vgpr_spill_count") == 0
    assert _note(on, "vgpr_count") <= _note(off, "vgpr_count")
    assert _note(on, "agpr_count") <= _note(off, "agpr_count")
