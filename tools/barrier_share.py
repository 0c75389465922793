#!/usr/bin/env python3
"""Barrier-wait share of the 4-state generated kernel's loop, per wave (PLK_DEBUG_CLOCK=3).

Runs one bench config in the bench's mode (lnL only) over the driver's window -- 5 warm-up and
20 timed evaluations by default -- with the diagnostic build of the same traversal program in
which every wave records its loop ticks and the ticks it spends between arriving at the
per-super-block barrier and leaving it (plk_jit.hpp, level 3).  Prints one JSON line: per timed
evaluation the mean and the worst wave's wait share, the mean and longest loop in shader-clock
ticks and the waves that ran; and the medians over the timed evaluations.

  PLK_TUNE=JIT_WT=0 tools/barrier_share.py [--config gtr_g4_dna_1M_64] [--patterns N]

With wave tasks (JIT_WT=1) the loop has no barrier: the shares are 0 and only the loop ticks
say anything.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("bpp-phyl_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
os.environ["PLK_DEBUG_CLOCK"] = "3"
os.environ.setdefault("PLK_JIT_CACHE", os.path.join(ROOT, ".jit_cache"))

import numpy as np  # noqa: E402

import plk  # noqa: E402
import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64", choices=sorted(workload.CONFIGS))
    ap.add_argument("--patterns", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    wl = workload.make_workload(args.config, n_patterns=args.patterns)
    P = wl.n_patterns
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_LNL_ONLY)
    lnl = None
    for _ in range(args.warmup + args.steps):
        lnl, _, _ = ev.step()
    rec = np.asarray(ev.eng.clock_records(), dtype=np.float64).reshape(-1, 5)
    # one record per traversal: with several tiers the last of an evaluation holds every tier's waves
    timed = rec[-args.steps:]
    med = np.median(timed, axis=0)
    print(json.dumps({"config": args.config, "patterns": int(P), "tune": os.environ.get("PLK_TUNE", ""),
                      "kernel_path": ev.eng.kernel_path(), "lnl": lnl,
                      "fields": ["wait_share_mean", "wait_share_worst_wave", "loop_ticks_mean", "loop_ticks_max", "waves"],
                      "median": [float(x) for x in med],
                      "timed": [[float(x) for x in r] for r in timed]}))


if __name__ == "__main__":
    main()
