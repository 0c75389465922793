"""Stochastic mapping on the device (plk_smap_sample): sampled histories on every branch, next to
one pass of the expectations the same handle already serves.

    python tools/bench_smap.py [--config gtr_g4_dna_1M_64] [--patterns N] [--replicates R] [--reps K]

One JSON line:
  * `sample_kernel_ms`: HIP-event time of the sampling launch over R replicates (plk_set_timing,
    PLK_TIME_PARTIALS), `tables_kernel_ms` that of the table launch; `ms_per_replicate` the former
    divided by R, `samples_per_s` site x branch samples per second of the sampling launch;
    `call_ms` the wall time of the whole synchronising call;
  * `lds_off_ms_per_replicate` (4 states): the same with the tables read from global memory
    (PLK_TUNE SMAP_LDS=0);
  * `expectations_ms`: wall time of one plk_node_posteriors (best state of every internal node) plus
    one plk_branch_counts (totals of every branch) on the same handle -- context, not a gate;
  * `mean_jumps_per_branch`, `mean_changes_per_site`: what the sampled work was.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bpp-phyl_amd"))
import phylo  # noqa: E402
import plk  # noqa: E402
import workload  # noqa: E402


def timed_sample(eng, root, br, t, mi, R, reps):
    eng.smap_sample(root, br, t, 1, 0, R, models=mi)  # warm-up (allocates, builds R^n)
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_PARTIALS | plk.PLK_TIME_TABLES)
    t0 = time.perf_counter()
    for k in range(reps):
        eng.smap_sample(root, br, t, 1, (k + 1) * R, R, models=mi)
    wall = (time.perf_counter() - t0) / reps
    tm = eng.get_timing()
    eng.set_timing(0)
    return tm["partials_ms"] / reps, tm["tables_ms"] / reps, wall * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    wl.n_patterns = args.patterns or wl.n_patterns
    P, R = wl.n_patterns, args.replicates
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_DOUBLE_RECURSIVE)
    eng, et = ev.eng, wl.et
    br = np.asarray(ev.branches, dtype=np.int32)
    t = et.brlen[br]
    eng.update_pmatrices(br, t, ev.model_idx, deriv_mask=7)
    eng.update_partials(ev.ops)
    lnl, _, _ = eng.root_loglik(et.root)
    ty = np.ones((wl.S, wl.S), dtype=np.uint8)
    np.fill_diagonal(ty, 0)
    eng.smap_set_types(1, ty)
    for k, m in enumerate(wl.models):
        eng.smap_set_generator(k, m.Q)
        eng.set_count_types(k, phylo.total_register(m.Q))
    samp_ms, tab_ms, call_ms = timed_sample(eng, et.root, br, t, ev.model_idx, R, args.reps)
    assert eng.smap_launches() <= 3
    totals = eng.smap_totals(br)
    rec = {
        "metric": "stochastic mapping: site x branch sampled histories/s (plk_smap_sample)",
        "config": args.config, "patterns": P, "branches": int(len(br)), "states": wl.S, "classes": wl.C,
        "replicates": R, "reps": args.reps, "lnl": lnl,
        "sample_kernel_ms": samp_ms, "tables_kernel_ms": tab_ms, "call_ms": call_ms,
        "ms_per_replicate": samp_ms / R, "samples_per_s": P * len(br) * R / (samp_ms * 1e-3),
        "n_bad": eng.smap_bad(), "tree_length": float(t.sum()),
        "mean_changes_per_site": float(totals.sum() / (R * P)),
    }
    if wl.S == 4:
        old = os.environ.get("PLK_TUNE", "")
        os.environ["PLK_TUNE"] = (old + "," if old else "") + "SMAP_LDS=0"
        off_ms, _, _ = timed_sample(eng, et.root, br, t, ev.model_idx, R, args.reps)
        os.environ["PLK_TUNE"] = old
        rec["lds_off_ms_per_replicate"] = off_ms / R
    # the expectations of the same handle: one posteriors pass and one counts pass
    eng.update_count_matrices(br, t, ev.model_idx)
    nodes = np.arange(et.n_tips, et.n_nodes, dtype=np.int32)
    eng.node_posteriors(nodes, states=False, best=True)
    want = eng.branch_counts(br, counts=False)["totals"]  # warm-up: the preorder pass is done
    t0 = time.perf_counter()
    eng.node_posteriors(nodes, states=False, best=True)
    eng.branch_counts(br, counts=False)
    rec["expectations_ms"] = (time.perf_counter() - t0) * 1e3
    rec["expected_changes_per_site"] = float(want.sum() / P)
    eng.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
