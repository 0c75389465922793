"""bench.py's plain run on the GPU: the line carries the headline fields and none of the
--full measurements, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plk
import workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# more than one 4096-pattern block, and no multiple of the block
N_PATTERNS = 3 * 4096 + 123


def test_plain_run_dumps_last_step_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--patterns", str(N_PATTERNS), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == "site-pattern x node partial updates/s" and rec["unit"] == "updates/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(N_PATTERNS * rec["config"]["internal_nodes"] / (rec["ms_per_step"] * 1e-3))
    assert "cpu_baseline" not in rec and "strong" not in rec
    assert sorted(os.listdir(out)) == ["block_sums.npy", "lnl.npy"]
    lnl, blocks = np.load(out / "lnl.npy"), np.load(out / "block_sums.npy")
    assert lnl.dtype == np.float64 and lnl.shape == (1,) and lnl[0] == rec["lnl"]
    assert blocks.dtype == np.float64 and blocks.shape == ((N_PATTERNS + plk.BLOCK - 1) // plk.BLOCK,)
    # the same seeded workload evaluated here: the dumped arrays are the step's own, bitwise
    wl = workload.make_workload("gtr_g4_dna_1M_64", n_patterns=N_PATTERNS)
    ev = workload.Evaluator(wl, 0, 0, N_PATTERNS, extra_flags=plk.PLK_FLAG_LNL_ONLY)
    lnl_here, _, blocks_here = ev.step()
    ev.eng.close()
    assert lnl_here == lnl[0] and np.array_equal(blocks_here, blocks)
