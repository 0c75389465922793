"""CPU tests of the definition of plk_smap_sample as tests/smap_rule.py restates it: the
uniformisation tables against scipy's expm, the weighted draw's edge cases, the invariants of a
sampled path, and the convergence of the rule's own sample means (group C of tests/test_gpu_smap.py,
same case and seed) to numpy posteriors from tests/xref.py -- checked here before the GPU is asked.
No GPU, no libplk.

Largest |z| of group C with the rule alone (seed 20260, 2048 replicates, 64 sites, bound 6):
state tallies 1.45, class tallies 1.68, counts 2.35, dwelling times 1.92."""
import functools

import numpy as np
import pytest
from scipy.linalg import expm

import phylo
import sim_rule as sr
import smap_check as sc
import smap_rule as sm
import xref


@pytest.mark.parametrize("name,tau", [("GTR", 0.9), ("GTR", 0.01), ("T92", 3.0), ("LG08", 0.7), ("YN98", 0.4)])
def test_poisson_mixture_of_powers_is_expm(name, tau):
    m = {"GTR": phylo.gtr(a=1.2, b=0.4, c=0.6, d=0.8, e=0.5, piA=0.30, piC=0.20, piG=0.25, piT=0.25),
         "T92": phylo.t92(3.0, 0.4), "LG08": phylo.lg08(), "YN98": phylo.yn98(2.0, 0.3)}[name]
    tab = sm.tables(m.Q, np.array([1.0, 2.5]), tau)
    assert tab["mu"] * 2.5 * tau <= 32
    assert np.all(tab["R"] >= 0) and np.allclose(tab["R"].sum(axis=1), 1.0, atol=1e-14)
    for c, r in enumerate((1.0, 2.5)):
        mix = np.einsum("n,nxy->xy", tab["pois"][c], tab["Rpow"])
        err = np.max(np.abs(mix - expm(m.Q * tau * r)))
        print(f"smap expm {name} tau={tau * r}: {err:.2e}")
        assert err <= 1e-13


def test_poisson_tail_beyond_the_cut_is_negligible():
    from scipy.stats import poisson
    assert poisson.sf(sm.N_MAX, 32.0) < 1e-30


def test_weighted_draw_rule():
    w = np.array([[0.2, 0.0, 0.3, 0.0], [0.0, -1.0, np.nan, 0.0], [1e-300, 0.5, 0.5, 0.0]])
    u = np.array([0.5, 0.3, 0.0])
    assert sm.weighted_draw(w, u).tolist() == [2, 0, 0]              # 0.25 >= 0.2; no positive weight: 0; thr 0 < 1e-300
    assert sm.weighted_draw(w[:1], np.array([1 - 2.0**-53])).tolist() == [2]
    # a threshold no cumulative value exceeds takes the largest index of positive weight
    assert sm.weighted_draw(w[:1], None, thr=np.array([0.6])).tolist() == [2]
    # a product weight is rounded before it is added: the draw sees fl(p q), as the device's __dmul_rn
    p, q = np.array([[1 + 2.0**-30, 1.0]]), np.array([[1 + 2.0**-30, 1.0]])
    assert sr.cumulative(p * q)[0, -1] == (p * q)[0, 0] + 1.0


def test_streams_do_not_share_draws():
    site = np.arange(64, dtype=np.uint64)
    rep = np.zeros(64, dtype=np.uint64)
    assert np.array_equal(sm.uniform(9, rep, site, 1, 0), sr.uniform(9, 0, site, 1))
    a = [sm.uniform(9, rep, site, 1, c3) for c3 in (0, 1, 2, 3)]
    for i in range(4):
        for j in range(i):
            assert not np.any(a[i] == a[j])
    k = np.arange(64, dtype=np.uint64) % np.uint64(7)
    mixed = sm.uniform(9, rep, site, k, 5)
    for kk in range(7):
        assert np.array_equal(mixed[k == kk], sm.uniform(9, rep, site, kk, 5)[k == kk])


def _path_inputs(n=4000, t=0.9):
    m = phylo.gtr(a=1.2, b=0.4, c=0.6, d=0.8, e=0.5, piA=0.30, piC=0.20, piG=0.25, piT=0.25)
    rates = np.array([0.5, 2.0])
    tab = sm.tables(m.Q, rates, t)
    P = np.stack([expm(m.Q * t * r) for r in rates])
    rng = np.random.default_rng(3)
    a, b, cls = rng.integers(0, 4, n), rng.integers(0, 4, n), rng.integers(0, 2, n)
    return m, rates, tab, P, a, b, cls


def test_path_invariants_and_means():
    """Per endpoint pair: dwell sums to t, counts are the real changes, the mean count is
    W[a][b] / P[a][b] within 6 standard errors."""
    t = 0.9
    m, rates, tab, P, a, b, cls = _path_inputs(24000, t)
    ty = sc.total_types(4)
    site = np.arange(len(a), dtype=np.uint64)
    rep = np.zeros(len(a), dtype=np.uint64)
    n, counts, dwell, forced = sm.draw_path(a, b, cls, P, tab, t, ty, 1, 77, rep, site, v=3)
    assert not forced.any()
    assert np.allclose(dwell.sum(axis=1), t, rtol=1e-12, atol=0)
    assert np.all(counts[:, 0] <= n) and np.all((counts[:, 0] == 0) <= (a == b)) and np.all(n[a != b] >= 1)
    assert np.all(dwell[np.arange(len(a)), a] > 0) and np.all(dwell[np.arange(len(a)), b] > 0)
    W = sc.count_matrices(m.Q, sc.register_B(m.Q, ty, 1), rates, t)[0]
    worst = 0.0
    for c in range(2):
        for x in range(4):
            for y in range(4):
                sel = (cls == c) & (a == x) & (b == y)
                k = counts[sel, 0]
                z = abs(k.mean() - W[c, x, y] / P[c, x, y]) / (k.std(ddof=1) / np.sqrt(len(k)))
                worst = max(worst, z)
    print(f"smap path means: worst z {worst:.2f}")
    assert worst <= 6.0


def test_zero_length_branch_stays():
    m, rates, tab, P, a, b, cls = _path_inputs(100)
    tab0 = sm.tables(m.Q, rates, 0.0)
    P0 = np.stack([np.eye(4)] * 2)
    site = np.arange(100, dtype=np.uint64)
    n, counts, dwell, forced = sm.draw_path(a, a, cls, P0, tab0, 0.0, sc.total_types(4), 1, 1, site * 0, site, v=2)
    assert not n.any() and not counts.any() and not dwell.any() and not forced.any()


@functools.lru_cache(maxsize=None)
def rule_sample_c():
    """The rule on group C's case from numpy P and the reference's lower partials."""
    case = sc.case_c()
    et, m = case.et, case.model
    P = np.zeros((et.n_nodes, 4, 4, 4))
    for v in case.br:
        P[v] = np.stack([m.pij(case.t[v] * r) for r in case.rates])
    low = xref.lower(et, case.codes, phylo.DNA.init_table, P)
    L = {v: np.asarray(low[0][v], dtype=np.float64) for v in range(et.n_nodes)}
    tabs = {v: sm.tables(m.Q, case.rates, case.t[v]) for v in case.br}
    order = sr.preorder(sr.kids_of_ops(case.tree[0]), et.root)
    out = sm.sample(order, et.root, {v: P[v] for v in case.br}, L, case.probs, m.pi, tabs, {v: case.t[v] for v in case.br},
                    case.type_of, case.T, sc.C_SEED, np.arange(sc.C_REPLICATES), np.arange(sc.C_SITES))
    return case, P, low, out


def expectations_c(case, P, low):
    """Posterior state and class probabilities, expected counts and dwelling times of group C."""
    et, m = case.et, case.model
    post = xref.posteriors(et, case.codes, phylo.DNA.init_table, P, case.probs, m.pi, case.internal, lower=low)
    Wc = {v: sc.count_matrices(m.Q, sc.register_B(m.Q, case.type_of, case.T), case.rates, case.t[v]) for v in case.br}
    Wd = {v: sc.reward_matrices(m.Q, case.rates, case.t[v]) for v in case.br}
    cnt = xref.branch_counts(et, case.codes, phylo.DNA.init_table, P, Wc, case.probs, m.pi, case.br, lower=low).counts
    dw = xref.branch_counts(et, case.codes, phylo.DNA.init_table, P, Wd, case.probs, m.pi, case.br, lower=low).counts
    return post.states, post.classes[0], cnt, dw


def test_group_c_the_rule_alone_converges():
    case, P, low, out = rule_sample_c()
    assert out["n_bad"] == 0
    st, cl, cnt, dw = (np.asarray(x, dtype=np.float64) for x in expectations_c(case, P, low))
    assert np.allclose(dw.sum(axis=2), np.array([case.t[v] for v in case.br])[:, None], rtol=1e-10)
    R, S = sc.C_REPLICATES, 4
    tally = np.stack([(out["states"][v][:, :, None] == np.arange(S)).sum(axis=0) for v in case.internal])
    z_state = sc.z_tally(tally, st, R)
    z_class = sc.z_tally((out["classes"][:, :, None] == np.arange(4)).sum(axis=0), cl, R)
    z_count = sc.z_mean(np.stack([out["counts"][v].sum(axis=1) for v in case.br], axis=1), cnt.sum(axis=1))
    z_dwell = sc.z_mean(np.stack([out["dwell"][v].sum(axis=1) for v in case.br], axis=1), dw.sum(axis=1))
    print(f"smap rule C: z states {z_state:.2f} classes {z_class:.2f} counts {z_count:.2f} dwell {z_dwell:.2f}")
    assert max(z_state, z_class, z_count, z_dwell) <= sc.Z_BOUND
    # resolved tips keep their state, the ambiguous ones move within their code
    for tip in range(case.et.n_tips):
        res = case.codes[tip] < 4
        assert np.all(out["states"][tip][:, res] == case.codes[tip][res])
    assert set(np.unique(out["states"][5][:, 40])) == {0, 2}  # R
    assert len(np.unique(out["states"][2][:, 3])) >= 3        # N
