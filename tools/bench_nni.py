"""NNI scoring on the device (plk_nni_scores): every nearest-neighbour interchange of the
config's tree, the length of the move's branch kept (max_iter = 0) and re-estimated (max_iter =
20), next to the DR pass that leaves L_v and U_v in HBM.

    python tools/bench_nni.py --config gtr_g4_dna_1M_64 [--patterns N] [--reps K] [--max-moves N]

One JSON line per max_iter:
  * `build_kernel_ms`: HIP-event time of the coefficient launches (one per chunk of moves) and
    their algorithmic HBM rate: per move and pattern U_g (8 C S; nothing at the root), L of every
    internal subtree read (8 C S each; a tip reads one code byte), C S + 2 rows written;
  * `eval_kernel_ms`, `passes`, `eval_ms_per_pass`: HIP-event time of the evaluation launches
    and the passes the call took (chunks x (1 + Newton passes)).  With max_iter = 0 every pass
    reads all C S + 2 rows of every move, which gives `eval_roofline`; with max_iter > 0
    converged moves drop out, so only the time per pass is reported;
  * `wall_ms`: the call end to end (launches, block-sum copies and the host's Newton steps).
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

HBM_PEAK = 8000.0  # GB/s


def all_moves(et):
    sons, par = {}, {}
    for p, ch in et.ops:
        sons.setdefault(p, []).extend(ch)
        for c in ch:
            par[c] = p
    out = []
    for s in sorted(par):
        p = par[s]
        if p == et.root:
            continue
        g = par[p]
        if len(sons[p]) > 3 or len(sons[g]) > 3:
            continue
        out += [(s, u) for u in sons[g] if u != p]
    return out, sons, par


def build_bytes(et, moves, sons, par, CS):
    """Algorithmic HBM bytes per pattern of the coefficient build over `moves`."""
    b = 0
    for s, u in moves:
        p = par[s]
        g = par[p]
        kids = [s, u] + [o for o in sons[g] if o not in (p, u)] + [o for o in sons[p] if o != s]
        b += sum(1 if k < et.n_tips else 8 * CS for k in kids)
        b += 0 if g == et.root else 8 * CS
        b += 8 * (CS + 2)
    return b


def timed(eng, fn, reps):
    fn()  # warm-up (U is current afterwards: no preorder pass)
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_PARTIALS | plk.PLK_TIME_ROOT)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    wall = (time.perf_counter() - t0) / reps
    tm = eng.get_timing()
    eng.set_timing(False)
    return out, tm["partials_ms"] / reps, tm["root_ms"] / reps, tm["launches"] / reps, wall * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-moves", type=int, default=0, help="score only the first N moves")
    ap.add_argument("--max-iter", type=int, nargs="*", default=[0, 20])
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    wl.n_patterns = args.patterns or wl.n_patterns
    P = wl.n_patterns
    ev = workload.Evaluator(wl, 0, 0, P, extra_flags=plk.PLK_FLAG_DOUBLE_RECURSIVE)
    eng, et = ev.eng, wl.et
    eng.update_pmatrices(ev.branches, et.brlen[ev.branches], ev.model_idx, deriv_mask=7)
    eng.update_partials(ev.ops)
    lnl, _, _ = eng.root_loglik(et.root)
    moves, sons, par = all_moves(et)
    if args.max_moves:
        moves = moves[:args.max_moves]
    son = np.array([s for s, _ in moves], dtype=np.int32)
    uncle = np.array([u for _, u in moves], dtype=np.int32)
    t0 = np.array([et.brlen[par[s]] for s in son])
    model = None if wl.model_of_node is None else np.array([wl.model_of_node[par[s]] for s in son], dtype=np.int32)
    CS = wl.C * wl.S
    bb = build_bytes(et, moves, sons, par, CS)
    eb = len(moves) * 8 * (CS + 2) + 8
    for mi in args.max_iter:
        out, build_ms, eval_ms, chunks, wall = timed(
            eng, lambda: eng.nni_scores(son, uncle, t0, tol=1e-8, max_iter=mi, model=model), args.reps)
        rec = {
            "metric": "NNI moves scored (all of the tree)", "config": args.config, "patterns": P, "moves": len(moves),
            "states": wl.S, "classes": wl.C, "max_iter": mi, "lnl": lnl, "chunks": chunks, "passes": out["passes"],
            "build_kernel_ms": build_ms, "eval_kernel_ms": eval_ms, "eval_ms_per_pass": eval_ms / out["passes"],
            "wall_ms": wall, "converged": int(np.sum(out["status"] == 0)), "improving": int(np.sum(out["delta"] > 0)),
            "best_delta": float(out["delta"].max()),
            "build_roofline": {"bound": "hbm", "achieved": bb * P / (build_ms * 1e-3) / 1e9, "peak": HBM_PEAK,
                               "unit": "GB/s", "frac": bb * P / (build_ms * 1e-3) / 1e9 / HBM_PEAK,
                               "algorithmic_bytes_per_pattern": bb},
        }
        if mi == 0:
            rec["eval_roofline"] = {"bound": "hbm", "achieved": eb * P / (eval_ms * 1e-3) / 1e9, "peak": HBM_PEAK,
                                    "unit": "GB/s", "frac": eb * P / (eval_ms * 1e-3) / 1e9 / HBM_PEAK,
                                    "algorithmic_bytes_per_pattern": eb}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
