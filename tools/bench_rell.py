"""RELL resampling on the device: log rho rows of every NNI move of the config's tree
(plk_nni_site_rows), R replicate weight vectors, and their product (plk_replicate_sums), next to
the only route to the same numbers without them: per replicate plk_set_pattern_weights +
plk_nni_scores(max_iter = 0), timed on a few replicates and scaled to R.

    python tools/bench_rell.py --config gtr_g4_dna_1M_64 [--patterns N] [--replicates R] [--reps K]

One JSON line: `rows_ms` (wall, all moves), `sums_ms` (wall) and `sums_kernel_ms` (HIP events of
the block-partial launches), `old_route_ms` (scaled from `--old-replicates` replicates) and
`speedup` = old_route_ms / (rows_ms + sums_ms).  Two rooflines of the block-partial kernel:
fp64 MFMA (2 R M P flops against 78.6 TF) and HBM (W read once per 64-row tile, the rows once
per 64-replicate tile, against 8 TB/s; `ideal_bytes` reads both once).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bpp-phyl_amd"))
import plk  # noqa: E402
import workload  # noqa: E402

from bench_nni import all_moves  # noqa: E402

HBM_PEAK = 8000.0    # GB/s
MFMA_PEAK = 78.6     # fp64 TF
TILE = 64


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return out, (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--old-replicates", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    wl.n_patterns = args.patterns or wl.n_patterns
    P, R = wl.n_patterns, args.replicates
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_DOUBLE_RECURSIVE)
    eng, et = ev.eng, wl.et
    eng.update_pmatrices(ev.branches, et.brlen[ev.branches], ev.model_idx, deriv_mask=7)
    eng.update_partials(ev.ops)
    eng.root_loglik(et.root)
    moves, _, par = all_moves(et)
    son = np.array([s for s, _ in moves], dtype=np.int32)
    uncle = np.array([u for _, u in moves], dtype=np.int32)
    t0 = np.array([et.brlen[par[s]] for s in son])
    model = None if wl.model_of_node is None else np.array([wl.model_of_node[par[s]] for s in son], dtype=np.int32)
    M = len(moves)
    rng = np.random.default_rng(1)
    W = rng.integers(0, 4, (R, P), dtype=np.int8).astype(np.float64)   # counts; the values cost nothing
    eng.site_rows_reserve(M)
    eng.set_replicate_weights(W)
    _, rows_ms = wall(lambda: eng.nni_site_rows(son, uncle, t0, 0, model=model), args.reps)
    eng.replicate_sums(0, M)
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_ROOT)
    G, sums_ms = wall(lambda: eng.replicate_sums(0, M), args.reps)
    kernel_ms = eng.get_timing()["root_ms"] / (args.reps + 1)
    eng.set_timing(False)
    passes = eng.replicate_passes()

    # the parent route: one weight upload and one scoring pass per replicate
    def old(r):
        eng.set_pattern_weights(W[r])
        return eng.nni_scores(son, uncle, t0, max_iter=0, model=model)["delta"]
    old(0)
    t1 = time.perf_counter()
    deltas = np.stack([old(r) for r in range(args.old_replicates)])
    old_ms = (time.perf_counter() - t1) / args.old_replicates * 1e3 * R
    scale = np.abs(W[:args.old_replicates]).sum(axis=1)[:, None]
    agree = float((np.abs(G[:args.old_replicates] - deltas) / scale).max())
    flops = 2.0 * R * M * P
    tiles_m, tiles_r = -(-M // TILE), -(-R // TILE)
    read = 8.0 * P * (R * tiles_m + M * tiles_r)
    ideal = 8.0 * P * (R + M)
    k = kernel_ms * 1e-3
    print(json.dumps({
        "metric": "RELL replicate sums over all NNI moves", "config": args.config, "patterns": P, "moves": M,
        "replicates": R, "rows_ms": rows_ms, "sums_ms": sums_ms, "sums_kernel_ms": kernel_ms, "passes": passes,
        "old_route_ms": old_ms, "old_replicates_timed": args.old_replicates,
        "speedup": old_ms / (rows_ms + sums_ms), "max_abs_diff_per_unit_weight": agree,
        "mfma_roofline": {"bound": "fp64 mfma", "achieved": flops / k / 1e12, "peak": MFMA_PEAK, "unit": "TF",
                          "frac": flops / k / 1e12 / MFMA_PEAK},
        "hbm_roofline": {"bound": "hbm", "achieved": read / k / 1e9, "peak": HBM_PEAK, "unit": "GB/s",
                         "frac": read / k / 1e9 / HBM_PEAK, "tile_bytes": read, "ideal_bytes": ideal},
    }), flush=True)


if __name__ == "__main__":
    main()
