"""Node posteriors on the device (plk_node_posteriors): marginal ancestral states and
posterior rate classes of every internal node, next to the DR pass that leaves L_v and U_v
in HBM.

    python tools/bench_post.py --config gtr_g4_dna_1M_64 [--patterns N] [--reps K] [--states-nodes N]

One JSON line:
  * `dr_kernels_ms`: HIP-event time of the DR pass's kernels (plk_all_branch_derivatives) on
    this handle, in this process -- the yardstick;
  * `post_best_kernel_ms`: HIP-event time of the posterior kernel with only best_state asked
    for, over all internal nodes, and its algorithmic HBM rate: per internal node and pattern
    L_v and U_v read (8 C S each; no U at the root) and one byte written;
  * `post_best_ms` / `post_states_ms`: end-to-end times of the call (kernel, device-to-host
    copies, the host's reordering into [node][pattern][state]) with best_state and with
    state_post.
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


def post_bytes(wl):
    """Algorithmic HBM bytes per pattern of the best_state-only pass over all internal nodes."""
    CS8 = 8 * wl.C * wl.S
    n = wl.et.n_internal
    return n * (CS8 + 1) + (n - 1) * CS8


def post_flops(wl):
    """Per non-root internal node and class the contraction P_v^T u: 2 S^2 flops."""
    return (wl.et.n_internal - 1) * wl.C * 2 * wl.S * wl.S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states-nodes", type=int, default=0,
                    help="time state_post on the first N internal nodes only (0: all; the answer is "
                         "8 S bytes per node and pattern on the host)")
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    P = args.patterns or wl.n_patterns
    wl.n_patterns = P
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_DOUBLE_RECURSIVE)
    eng, et = ev.eng, wl.et
    eng.update_pmatrices(ev.branches, et.brlen[ev.branches], ev.model_idx, deriv_mask=7)
    eng.update_partials(ev.ops)
    lnl, _, _ = eng.root_loglik(et.root)
    nodes = np.arange(et.n_tips, et.n_nodes, dtype=np.int32)
    eng.all_branch_derivatives()  # warm-up
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_PARTIALS)
    for _ in range(args.reps):
        eng.all_branch_derivatives()
    dr_ms = eng.get_timing()["partials_ms"] / args.reps
    eng.node_posteriors(nodes, states=False, best=True)  # warm-up (U is current: no preorder pass)
    eng.reset_timing()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        out = eng.node_posteriors(nodes, states=False, best=True)
    t_best = (time.perf_counter() - t0) / args.reps
    tm = eng.get_timing()
    k_ms = tm["partials_ms"] / args.reps
    eng.set_timing(False)
    best = out["best"]
    t0 = time.perf_counter()
    ns = args.states_nodes or len(nodes)
    out = eng.node_posteriors(nodes[:ns], states=True, best=False)
    t_states = time.perf_counter() - t0
    agree = float(np.mean(out["states"].argmax(axis=2) == best[:ns]))
    b = post_bytes(wl)
    fl = post_flops(wl)
    rec = {
        "metric": "node x site-pattern posteriors/s (best_state of every internal node)",
        "config": args.config, "patterns": P, "internal_nodes": int(len(nodes)), "states": wl.S, "classes": wl.C,
        "lnl": lnl, "dr_kernels_ms": dr_ms, "post_best_kernel_ms": k_ms,
        "post_best_kernel_launches": tm["launches"] / args.reps,
        "post_kernel_vs_dr_kernels": k_ms / dr_ms,
        "post_best_ms": t_best * 1e3, "post_states_ms": t_states * 1e3, "post_states_nodes": int(ns),
        "post_updates_per_s": len(nodes) * P / (k_ms * 1e-3),
        "roofline": {"bound": "hbm", "achieved": b * P / (k_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": b * P / (k_ms * 1e-3) / 1e9 / 8000.0, "algorithmic_bytes_per_pattern": b},
        "flop_rate_TFLOPs": fl * P / (k_ms * 1e-3) / 1e12,
        "underflowed_cells": int(np.sum(best == 255)),
        "argmax_of_state_post_equals_best_state": agree,
    }
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
