"""Pairwise ML distances on the device (plk_pair_counts / plk_pair_distances): all pairs of the
config's tips, from the tip codes to the distance matrix.

    python tools/bench_dist.py --config gtr_g4_dna_1M_64 [--patterns N] [--reps K] [--max-pairs N]

One JSON line:
  * `count_kernel_ms`: HIP-event time of the count launches (pair_count_kernel and pair_sum_kernel,
    one pair of launches per chunk of pairs), `updates` = pairs x patterns table updates, `updates_per_s`,
    and `input_bytes`: the tip codes (one byte per tip and pattern) and the weights (8 per
    pattern), each read once from HBM if every re-read hits a cache;
  * `newton_kernel_ms`, `passes`: HIP-event time of the Newton launches (pair_basis_kernel is
    not inside the events) and the evaluation passes of the slowest pair;
  * `counts_wall_ms`: plk_pair_counts end to end (the tables copied to the host included);
    `wall_ms`: plk_pair_distances end to end.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-pairs", type=int, default=0, help="only the first N pairs")
    ap.add_argument("--max-iter", type=int, default=40)
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    wl.n_patterns = args.patterns or wl.n_patterns
    P, T = wl.n_patterns, wl.et.n_tips
    m = wl.models[0]
    eng = plk.Engine(0, wl.S, wl.C, P, T, 1, 1, plk.PLK_FLAG_NONNEG_GUARD)
    eng.set_code_table(wl.alphabet.init_table)
    st = wl.simulate(0, P)
    for i in range(T):
        eng.set_tip_codes(i, phylo.states_to_codes(st[i]))
    eng.set_category_rates(wl.rates, wl.probs)
    eng.set_root_frequencies(m.pi)
    eng.set_eigen(0, m.V, m.Vinv, m.lam)
    pairs = [(a, b) for a in range(T) for b in range(a + 1, T)]
    if args.max_pairs:
        pairs = pairs[:args.max_pairs]
    ta = np.array([a for a, _ in pairs], dtype=np.int32)
    tb = np.array([b for _, b in pairs], dtype=np.int32)

    def run():
        return eng.pair_distances(ta, tb, t_max=10000.0, tol=1e-8, max_iter=args.max_iter)

    run()  # warm-up (buffers allocated)
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_TABLES | plk.PLK_TIME_ROOT)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        out = run()
    wall = (time.perf_counter() - t0) / args.reps
    tm = eng.get_timing()
    eng.set_timing(False)
    t0 = time.perf_counter()
    counts = eng.pair_counts(ta, tb)
    counts_wall = time.perf_counter() - t0
    count_ms, newton_ms = tm["tables_ms"] / args.reps, tm["root_ms"] / args.reps
    updates = len(pairs) * P
    rec = {
        "metric": "pairwise ML distances (all pairs of the tips)", "config": args.config, "patterns": P, "tips": T,
        "pairs": len(pairs), "states": wl.S, "classes": wl.C, "codes_in_use": int(len(np.unique(st))),
        "max_iter": args.max_iter, "count_kernel_ms": count_ms, "updates": updates,
        "updates_per_s": updates / (count_ms * 1e-3) if count_ms > 0 else None, "input_bytes": T * P + 8 * P,
        "newton_kernel_ms": newton_ms, "passes": out["passes"], "converged": int(np.sum(out["status"] == 0)),
        "counts_wall_ms": counts_wall * 1e3, "wall_ms": wall * 1e3,
        "weight_sum_ok": bool(np.all(counts.sum(axis=(1, 2)) == P)),
        "t_opt_min": float(out["t_opt"].min()), "t_opt_max": float(out["t_opt"].max()),
    }
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
