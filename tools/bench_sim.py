"""Simulation on the engine against the host route: one plk_simulate with PLK_SIM_SET_TIPS (the
cumulative tables and the walk, two launches, tip codes left where the next traversal reads them)
versus generating the same number of sites on the host (phylo.simulate: numpy's generator and the
same inverse-CDF rule, one core) and uploading every tip with plk_set_tip_codes.

    python tools/bench_sim.py [--config gtr_g4_dna_1M_64 | all] [--patterns N] [--reps K] [--host-patterns M]

One JSON line per config.  Device times are HIP events on the handle's stream (plk_set_timing:
the table build under PLK_TIME_TABLES, the walk under PLK_TIME_PARTIALS), averaged over the
repetitions after one warm-up call; call_ms is the wall time of the whole synchronising call.
The walk's algorithmic HBM bytes per site: one state byte stored per node and one loaded per
non-root node, the class byte, and with SET_TIPS one code byte per tip; the cumulative rows are
gathered from a table that stays in cache.  --host-patterns M times the host generator on M sites
only (it is linear in the sites) and reports the time scaled to the config's site count as
host_generate_ms, with host_patterns saying so."""
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

CONFIGS = ["gtr_g4_dna_1M_64", "lg08_g4_protein_200k_256", "yn98_codon_50k_128"]


def run(config, patterns, reps, host_patterns):
    wl = workload.make_workload(config)
    P = patterns or wl.n_patterns
    et = wl.et
    flags = (plk.PLK_FLAG_SCALING if wl.scaling else 0) | plk.PLK_FLAG_NONNEG_GUARD | plk.PLK_FLAG_LNL_ONLY
    eng = plk.Engine(0, wl.S, wl.C, P, et.n_tips, et.n_internal, 1, flags)
    eng.set_code_table(wl.alphabet.init_table)
    eng.set_category_rates(wl.rates, wl.probs)
    eng.set_root_frequencies(wl.root_freqs)
    m = wl.models[0]
    eng.set_eigen(0, m.V, m.Vinv, m.lam)
    br = np.array([n for n in range(et.n_nodes) if n != et.root], dtype=np.int32)
    t = et.brlen[br]
    eng.update_pmatrices(br, t)
    ops = phylo.split_ops(et.ops)

    eng.simulate(ops, et.root, seed=1, replicate=0)  # warm-up (allocates the arrays)
    assert eng.sim_launches() == 2
    eng.set_timing(plk.PLK_TIME_PARTIALS | plk.PLK_TIME_TABLES)
    eng.reset_timing()
    t0 = time.perf_counter()
    for r in range(reps):
        eng.simulate(ops, et.root, seed=1, replicate=1 + r)
    call = (time.perf_counter() - t0) / reps
    tm = eng.get_timing()
    eng.set_timing(0)
    walk_ms, cdf_ms = tm["partials_ms"] / reps, tm["tables_ms"] / reps
    lnl_sim, _ = eng.evaluate(br, t, ops, et.root)

    # the host route: generate, then one upload per tip
    hp = host_patterns or P
    t0 = time.perf_counter()
    states = phylo.simulate(et, wl.models, None, wl.rates, hp, seed=1, root_freqs=wl.root_freqs)
    gen = (time.perf_counter() - t0) * (P / hp)
    codes = [np.ascontiguousarray(np.resize(phylo.states_to_codes(states[i]), P)) for i in range(et.n_tips)]
    t0 = time.perf_counter()
    for i in range(et.n_tips):
        eng.set_tip_codes(i, codes[i])
    up = time.perf_counter() - t0
    lnl_host, _ = eng.evaluate(br, t, ops, et.root)

    bytes_pp = et.n_nodes + (et.n_nodes - 1) + 1 + et.n_tips
    gbps = bytes_pp * P / (walk_ms * 1e-3) / 1e9
    out = {
        "metric": "simulation: plk_simulate with SET_TIPS against host generation + plk_set_tip_codes",
        "config": config, "patterns": P, "taxa": et.n_tips, "states": wl.S, "classes": wl.C, "reps": reps,
        "sim_cdf_ms": cdf_ms, "sim_walk_ms": walk_ms, "sim_device_ms": cdf_ms + walk_ms, "sim_call_ms": call * 1e3,
        "sim_node_sites_per_s": et.n_nodes * P / (walk_ms * 1e-3),
        "walk_roofline": {"bound": "hbm", "achieved": gbps, "peak": 8000.0, "unit": "GB/s", "frac": gbps / 8000.0,
                          "algorithmic_bytes_per_pattern": bytes_pp},
        "host_patterns": hp, "host_generate_ms": gen * 1e3, "host_upload_ms": up * 1e3,
        "host_route_ms": (gen + up) * 1e3, "speedup_call": (gen + up) / call,
        "lnl_per_site_simulated": lnl_sim / P, "lnl_per_site_host": lnl_host / P,
    }
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all")
    ap.add_argument("--patterns", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-patterns", type=int, default=0)
    args = ap.parse_args()
    for config in (CONFIGS if args.config == "all" else [args.config]):
        run(config, args.patterns, args.reps, args.host_patterns)


if __name__ == "__main__":
    main()
