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

--spread adds where the gap between the mean and the longest wave lies, from every wave's own
loop ticks (Engine.clock_waves), per timed evaluation and as medians:

  within_wg          mean over the workgroups of (longest wave - mean wave of that workgroup)
  long_* / short_*   mean, minimum and maximum over the workgroups of the workgroup's longest
                     wave (its last wave's end: the waves of a workgroup start the loop together),
                     apart for the workgroups that walk R rounds under the static stride (at least
                     one wave has R = ceil(tasks / waves) tasks there) and those that walk R - 1
                     -- the same two sets whatever schedule ran, so before and after compare
  longest            the loop's longest wave overall

--tail adds the task tail's share of a wave's loop (one class per workgroup; Engine.clock_waves
with tail=True): the ticks between the end of a task's last contraction and the top of the next
task -- the root reduction and the rotation of the prefetched codes -- summed over the wave's
tasks, over the wave's loop ticks:

  tail_share_mean / _worst   mean over the waves that ran / the worst wave
  tail_ticks_per_task        tail ticks of all waves over the tasks they walked
  task_ticks                 loop ticks of all waves over the same tasks

(One launch per traversal is assumed, as in config 2: with several tiers the workgroups per
fragment are the last tier's.)
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


def spread(waves, gx):
    """The --spread figures of one evaluation: waves[workgroup, wave] = (loop ticks, tasks)."""
    ticks, tasks = waves[:, :, 0], waves[:, :, 1]
    nwg, nwt = ticks.shape
    gx = max(gx, 1)
    x = np.arange(nwg) % gx
    # tasks of a (fragment, class): what its gx workgroups walked
    n_tasks = tasks.reshape(-1, gx, nwt).sum(axis=(1, 2)).repeat(gx)
    rounds = np.ceil(n_tasks / (gx * nwt))
    long_wg = x * nwt < n_tasks - (rounds - 1) * gx * nwt     # wave 0 walks `rounds` under the static stride
    ran = tasks > 0
    live = ran.any(axis=1)
    wg_max = ticks.max(axis=1)
    wg_mean = np.where(live, ticks.sum(axis=1) / np.maximum(ran.sum(axis=1), 1), 0.0)
    out = {"within_wg": float((wg_max - wg_mean)[live].mean()) if live.any() else 0.0}
    for name, sel in (("long", live & long_wg), ("short", live & ~long_wg)):
        v = wg_max[sel]
        out[name + "_wgs"] = int(sel.sum())
        out[name + "_mean"] = float(v.mean()) if v.size else 0.0
        out[name + "_min"] = float(v.min()) if v.size else 0.0
        out[name + "_max"] = float(v.max()) if v.size else 0.0
    out["wave_mean"] = float(ticks[ran].mean()) if ran.any() else 0.0
    out["longest"] = float(ticks.max()) if ticks.size else 0.0
    out["tasks_per_wg_min"] = float(tasks.sum(axis=1)[live].min()) if live.any() else 0.0
    out["tasks_per_wg_max"] = float(tasks.sum(axis=1).max()) if live.any() else 0.0
    return out


def tail(waves, gx):
    """The --tail figures of one evaluation: waves[workgroup, wave] = (loop ticks, tasks, tail ticks)."""
    ticks, tasks, tl = waves[:, :, 0], waves[:, :, 1], waves[:, :, 2]
    ran = tasks > 0
    if not ran.any():
        return {"tail_share_mean": 0.0, "tail_share_worst": 0.0, "tail_ticks_per_task": 0.0, "task_ticks": 0.0}
    share = tl[ran] / ticks[ran]
    return {"tail_share_mean": float(share.mean()), "tail_share_worst": float(share.max()),
            "tail_ticks_per_task": float(tl[ran].sum() / tasks[ran].sum()),
            "task_ticks": float(ticks[ran].sum() / tasks[ran].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64", choices=sorted(workload.CONFIGS))
    ap.add_argument("--patterns", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spread", action="store_true",
                    help="within- and between-workgroup spread of the waves' loop ticks")
    ap.add_argument("--tail", action="store_true",
                    help="the task tail's (root reduction, code rotation) share of a wave's loop")
    args = ap.parse_args()
    wl = workload.make_workload(args.config, n_patterns=args.patterns)
    P = wl.n_patterns
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_LNL_ONLY)
    lnl = None
    spreads, tails = [], []
    for i in range(args.warmup + args.steps):
        lnl, _, _ = ev.step()
        if args.spread and i >= args.warmup:
            spreads.append(spread(*ev.eng.clock_waves()))
        if args.tail and i >= args.warmup:
            tails.append(tail(*ev.eng.clock_waves(tail=True)))
    rec = np.asarray(ev.eng.clock_records(), dtype=np.float64).reshape(-1, 5)
    # one record per traversal: with several tiers the last of an evaluation holds every tier's waves
    timed = rec[-args.steps:]
    med = np.median(timed, axis=0)
    out = {"config": args.config, "patterns": int(P), "tune": os.environ.get("PLK_TUNE", ""),
           "kernel_path": ev.eng.kernel_path(), "lnl": lnl,
           "fields": ["wait_share_mean", "wait_share_worst_wave", "loop_ticks_mean", "loop_ticks_max", "waves"],
           "median": [float(x) for x in med],
           "timed": [[float(x) for x in r] for r in timed]}
    if spreads:
        out["spread_median"] = {k: float(np.median([s[k] for s in spreads])) for k in spreads[0]}
        out["spread_timed"] = spreads
    if tails:
        out["tail_median"] = {k: float(np.median([t[k] for t in tails])) for k in tails[0]}
        out["tail_timed"] = tails
    print(json.dumps(out))


if __name__ == "__main__":
    main()
