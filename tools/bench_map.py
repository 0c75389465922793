"""Substitution mapping on the device (plk_update_count_matrices, plk_branch_counts): the
posterior expected number of substitutions per branch, pattern and type, next to the DR pass
that leaves L_v and U_v in HBM.

    python tools/bench_map.py --config gtr_g4_dna_1M_64 [--patterns N] [--reps K] [--counts-branches N]

One JSON line per type count (T = 1, the total register; for DNA also T = 12, the
comprehensive register; the engine fixes T per handle, so each gets a handle of its own):
  * `count_matrix_kernel_ms`: HIP-event time of the count-matrix launch over every branch;
  * `map_totals_kernel_ms`: HIP-event time of the map launch over every branch with totals
    only (no per-pattern row written), and its algorithmic HBM rate: per branch and pattern
    U_v read (8 C S), L_v read for an internal branch (8 C S; a tip branch reads one code byte);
  * `map_counts_kernel_ms` / `map_counts_ms`: kernel and end-to-end time with per-pattern
    counts on the first `--counts-branches` branches (the answer is 8 T bytes per branch and
    pattern on the host), `map_counts_bytes_per_pattern` the rows that launch writes besides;
  * `post_best_kernel_ms`: plk_node_posteriors(best only) over all internal nodes on the same
    handle -- the yardstick, which reads the same L and U rows per node.
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
from bench_post import post_bytes  # noqa: E402


def map_bytes(wl, branches):
    """Algorithmic HBM bytes per pattern of the totals-only map launch over `branches`."""
    CS8 = 8 * wl.C * wl.S
    tips = int(np.sum(np.asarray(branches) < wl.et.n_tips))
    return len(branches) * CS8 + (len(branches) - tips) * CS8 + tips


def kernel_ms(eng, fn, reps, key="partials_ms"):
    fn()  # warm-up (U is current afterwards: no preorder pass, no tip fill)
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_PARTIALS | plk.PLK_TIME_PMAT)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    wall = (time.perf_counter() - t0) / reps
    tm = eng.get_timing()
    eng.set_timing(False)
    return tm[key] / reps, wall * 1e3, tm["launches"] / reps


def run(args, wl, T):
    P = wl.n_patterns
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_DOUBLE_RECURSIVE)
    eng, et = ev.eng, wl.et
    eng.update_pmatrices(ev.branches, et.brlen[ev.branches], ev.model_idx, deriv_mask=7)
    eng.update_partials(ev.ops)
    lnl, _, _ = eng.root_loglik(et.root)
    for k, m in enumerate(wl.models):
        eng.set_count_types(k, phylo.total_register(m.Q) if T == 1 else phylo.comprehensive_register(m.Q))
    br = np.asarray(ev.branches, dtype=np.int32)
    cm_ms, _, _ = kernel_ms(eng, lambda: eng.update_count_matrices(br, et.brlen[br], ev.model_idx), args.reps, "pmat_ms")
    tot_ms, tot_wall, launches = kernel_ms(eng, lambda: eng.branch_counts(br, counts=False), args.reps)
    totals = eng.branch_counts(br, counts=False)["totals"]
    nb = min(args.counts_branches, len(br))
    cnt_ms, cnt_wall, _ = kernel_ms(eng, lambda: eng.branch_counts(br[:nb], totals=False), 1)
    nodes = np.arange(et.n_tips, et.n_nodes, dtype=np.int32)
    post_ms, _, _ = kernel_ms(eng, lambda: eng.node_posteriors(nodes, states=False, best=True), args.reps)
    b = map_bytes(wl, br)
    pb = post_bytes(wl)
    rec = {
        "metric": "branch x site-pattern x type expected substitution counts/s (totals of every branch)",
        "config": args.config, "patterns": P, "branches": int(len(br)), "states": wl.S, "classes": wl.C, "types": T,
        "lnl": lnl, "count_matrix_kernel_ms": cm_ms,
        "map_totals_kernel_ms": tot_ms, "map_totals_ms": tot_wall, "map_totals_launches": launches,
        "map_counts_kernel_ms": cnt_ms, "map_counts_ms": cnt_wall, "map_counts_branches": int(nb),
        "map_counts_bytes_per_pattern": map_bytes(wl, br[:nb]) + 8 * T * nb,
        "post_best_kernel_ms": post_ms,
        "map_totals_vs_post_per_row_set": (tot_ms / len(br)) / (post_ms / len(nodes)),
        "map_updates_per_s": len(br) * P * T / (tot_ms * 1e-3),
        "roofline": {"bound": "hbm", "achieved": b * P / (tot_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": b * P / (tot_ms * 1e-3) / 1e9 / 8000.0, "algorithmic_bytes_per_pattern": b},
        "post_roofline_frac": pb * P / (post_ms * 1e-3) / 1e9 / 8000.0, "post_bytes_per_pattern": pb,
        "tree_length": float(et.brlen[br].sum()),
        "total_count_per_pattern": float(totals.sum() / P),
    }
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts-branches", type=int, default=4,
                    help="time per-pattern counts on the first N branches only")
    ap.add_argument("--types", type=int, nargs="*", default=None, help="type counts to run (default: 1, and 12 for DNA)")
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    wl.n_patterns = args.patterns or wl.n_patterns
    for T in args.types or ([1, 12] if wl.S == 4 else [1]):
        if T not in (1, wl.S * (wl.S - 1)) or T > 16:
            raise SystemExit(f"--types {T}: only the total (1) and, for DNA, the comprehensive (12) register")
        run(args, wl, T)


if __name__ == "__main__":
    main()
