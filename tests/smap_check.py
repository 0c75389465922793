"""What tests/test_smap_cpu.py and tests/test_gpu_smap.py share: small trees, the transition /
transversion event types, analytic count and reward integrals by block expm, and the convergence
statistics of group C (sample means against posterior expectations, in standard errors)."""
from types import SimpleNamespace

import numpy as np
from scipy.linalg import expm

import phylo
import sim_rule as sr

# (ops, root, tips), as tests/test_gpu_sim.py
TREE5 = ([(5, (0, 1), 0), (6, (2, 3), 0), (7, (5, 6, 4), 0)], 7, 5)            # the root has three sons
TREE7 = ([(7, (0, 1), 0), (8, (2, 3), 0), (9, (7, 8), 0), (10, (4, 5), 0), (11, (9, 10, 6), 0)], 11, 7)
TREE6 = ([(6, (0, 1), 0), (7, (2, 3), 0), (8, (6, 7), 0), (9, (8, 4, 5), 0)], 9, 6)
STAR5 = ([(6, (0, 1), 0), (7, (6, 2, 3), 0), (7, (4, 5), 1)], 7, 6)             # five sons at node 7
SCRAMBLED = ([(6, (0, 1), 0), (5, (2, 3), 0), (4, (6, 5), 0)], 4, 4)            # the root is the lowest internal node
ROOT2 = ([(4, (0, 1), 0), (5, (2, 3), 0), (6, (4, 5), 0)], 6, 4)                # a two-son root

C_SEED, C_SITES, C_REPLICATES = 20260, 64, 2048   # group C
Z_BOUND = 6.0


def tree_et(tree):
    """The namespace tests/xref.py reads: ops as (parent, sons) with accumulate ops merged."""
    ops, root, nt = tree
    merged = []
    for p, ch, fl in ops:
        if fl:
            i = [k for k, (q, _) in enumerate(merged) if q == p][0]
            merged[i] = (p, merged[i][1] + tuple(ch))
        else:
            merged.append((p, tuple(ch)))
    nn = max(p for p, _, _ in ops) + 1
    return SimpleNamespace(ops=merged, root=root, n_tips=nt, n_nodes=nn, n_internal=nn - nt)


def branch_lengths(n_nodes, root, seed):
    t = np.random.default_rng(seed).uniform(0.05, 0.6, size=n_nodes)
    t[root] = 0.0
    return t


def ts_tv_types():
    """type_of [4][4] over A, C, G, T: 1 a transition, 2 a transversion."""
    ty = np.full((4, 4), 2, dtype=np.uint8)
    for x, y in ((0, 2), (2, 0), (1, 3), (3, 1)):
        ty[x, y] = 1
    np.fill_diagonal(ty, 0)
    return ty


def total_types(S):
    ty = np.ones((S, S), dtype=np.uint8)
    np.fill_diagonal(ty, 0)
    return ty


def register_B(Q, type_of, T):
    """B [T][S][S] of plk_set_count_types for the event types."""
    return np.stack([np.where(type_of == k + 1, Q, 0.0) for k in range(T)])


def integral(Q, B, tau):
    """int_0^tau e^{Qs} B e^{Q(tau - s)} ds: the upper right block of expm([[Q, B], [0, Q]] tau)."""
    S = Q.shape[0]
    M = np.zeros((2 * S, 2 * S))
    M[:S, :S] = M[S:, S:] = Q * tau
    M[:S, S:] = B * tau
    return expm(M)[:S, S:]


def count_matrices(Q, Bs, rates, t):
    """W [T][C][S][S]: expected counts of each type times P, at tau = r_c t."""
    return np.stack([np.stack([integral(Q, B, r * t) for r in rates]) for B in Bs])


def reward_matrices(Q, rates, t):
    """W [S][C][S][S]: the expected time spent in each state (in units of t) times P."""
    S = Q.shape[0]
    E = np.zeros((S, S, S))
    E[np.arange(S), np.arange(S), np.arange(S)] = 1.0
    return np.stack([np.stack([integral(Q, E[s], r * t) / r for r in rates]) for s in range(S)])


def tip_codes(tree, model, rates, probs, t, n, seed, ambiguous=()):
    """Tip codes [tip][n] simulated by the rule of plk_simulate; ambiguous: (tip, site, code)."""
    ops, root, nt = tree
    nn = len(t)
    P = {v: np.stack([model.pij(t[v] * r) for r in rates]) for v in range(nn) if v != root}
    _, states = sr.simulate(ops, root, P, probs, model.pi, seed, 0, 0, n)
    codes = np.stack([states[v] for v in range(nt)]).astype(np.uint8)
    for tip, site, code in ambiguous:
        codes[tip, site] = code
    return codes


def case_c():
    """Group C: GTR + Gamma4 on the 7-tip tree, 64 sites, two ambiguous cells."""
    model = phylo.gtr(a=1.2, b=0.4, c=0.6, d=0.8, e=0.5, piA=0.30, piC=0.20, piG=0.25, piT=0.25)
    rates, probs = phylo.gamma_rates(4, 0.7)
    ops, root, nt = TREE7
    t = branch_lengths(12, root, 11)
    codes = tip_codes(TREE7, model, rates, probs, t, C_SITES, seed=5, ambiguous=((2, 3, 14), (5, 40, 5)))
    return SimpleNamespace(tree=TREE7, et=tree_et(TREE7), model=model, rates=rates, probs=probs, t=t, codes=codes,
                           type_of=ts_tv_types(), T=2, br=[v for v in range(12) if v != root],
                           internal=list(range(nt, 12)))


def z_tally(tally, post, R):
    """Tallies pooled over sites against R sum_p q with variance R sum_p q (1 - q): tally, post
    [..., n, K] -> the largest |z| (a cell without variance must hit its expectation)."""
    tally = np.asarray(tally, dtype=np.float64)
    q = np.asarray(post, dtype=np.float64)
    obs, want, var = tally.sum(axis=-2), R * q.sum(axis=-2), R * (q * (1 - q)).sum(axis=-2)
    flat = var < 1e-9
    assert np.all(np.abs(obs - want)[flat] < 1e-6)
    return float(np.max(np.abs(obs - want)[~flat] / np.sqrt(var[~flat])))


def z_mean(per_replicate, expected):
    """Per-replicate values pooled over sites, [R, ...], against the expectation summed over sites,
    with the sample's own standard error: the largest |z|."""
    x = np.asarray(per_replicate, dtype=np.float64)
    R = x.shape[0]
    se = x.std(axis=0, ddof=1) / np.sqrt(R)
    assert np.all(se > 0)
    return float(np.max(np.abs(x.mean(axis=0) - np.asarray(expected, dtype=np.float64)) / se))
