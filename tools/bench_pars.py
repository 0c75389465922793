"""Fitch parsimony on the engine: one plk_pars_update (lower pairs, upper pairs and the root of
the whole tree, one launch) and one plk_pars_nni_scores over every eligible move (one launch).

    python tools/bench_pars.py --config gtr_g4_dna_1M_64 [--patterns N] [--reps K]

One JSON line: the wall time of each call (both synchronise, so the time holds the launch and
the completion wait), its algorithmic HBM bytes and their share of the 8 TB/s roofline.
Algorithmic bytes per pattern, sets of w bytes (1 for up to 8 states) and scores of 2:
  * update: per op every input once (a tip: its 1-byte code; a lower or upper pair: w + 2) and
    the output pair once (w + 2); the weight (8) at the root;
  * nni: per move the inputs of gf and of pp once each and the weight (8).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gtr_g4_dna_1M_64")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    wl = workload.make_workload(args.config)
    P = args.patterns or wl.n_patterns
    wl.n_patterns = P
    ev = workload.Evaluator(wl, 0, 0, P)
    eng, et = ev.eng, wl.et
    nt = et.n_tips
    w = 1 if wl.S <= 8 else 4 if wl.S <= 32 else 8
    pair = w + 2
    kids = {}
    for p, ch in et.ops:
        kids.setdefault(p, []).extend(ch)
    parent = {c: p for p, ch in kids.items() for c in ch}
    size = lambda v: 1 if v < nt else pair  # noqa: E731

    # update: a lower op per internal node, an upper op per internal node but the root
    up_bytes = 8
    for v, ch in kids.items():
        up_bytes += sum(size(c) for c in ch) + pair
        if v != et.root:
            f = parent[v]
            up_bytes += (pair if f != et.root else 0) + sum(size(c) for c in kids[f] if c != v) + pair
    moves, nni_bytes = [], 0
    for s, p in sorted(parent.items()):
        if p == et.root:
            continue
        g = parent[p]
        for u in kids[g]:
            if u == p:
                continue
            moves.append((s, u))
            nni_bytes += (pair if g != et.root else 0) + sum(size(o) for o in kids[g] if o not in (p, u)) + size(s)
            nni_bytes += sum(size(o) for o in kids[p] if o != s) + size(u) + 8
    son, uncle = (np.array(x, dtype=np.int32) for x in zip(*moves))

    eng.pars_update(ev.ops)  # warm-up (allocates the arrays)
    score = eng.pars_score()
    eng.pars_nni_scores(son, uncle)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        eng.pars_update(ev.ops)
    t_up = (time.perf_counter() - t0) / args.reps
    t0 = time.perf_counter()
    for _ in range(args.reps):
        delta = eng.pars_nni_scores(son, uncle)
    t_nni = (time.perf_counter() - t0) / args.reps
    assert eng.pars_launches() == 1 and eng.pars_score() == score

    def roof(bytes_pp, t):
        gbps = bytes_pp * P / t / 1e9
        return {"bound": "hbm", "achieved": gbps, "peak": 8000.0, "unit": "GB/s", "frac": gbps / 8000.0,
                "algorithmic_bytes_per_pattern": bytes_pp}

    print(json.dumps({
        "metric": "Fitch parsimony: whole-tree update and all NNI moves, wall time per call",
        "config": args.config, "patterns": P, "taxa": nt, "states": wl.S, "set_bytes": w,
        "score": score, "best_delta": int(delta.min()),
        "update_ms": t_up * 1e3, "update_node_patterns_per_s": (2 * len(kids) - 1) * P / t_up,
        "update_roofline": roof(up_bytes, t_up),
        "nni_moves": len(moves), "nni_ms": t_nni * 1e3, "nni_move_patterns_per_s": len(moves) * P / t_nni,
        "nni_roofline": roof(nni_bytes, t_nni),
    }), flush=True)


if __name__ == "__main__":
    main()
