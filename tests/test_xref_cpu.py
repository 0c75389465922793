"""The extended-range reference (tests/xref.py) checked before tests/test_gpu_xref.py relies
on it: against the fp64 oracle where the oracle has the quantity, against central differences
of its own longdouble lnL where it has not (root pairs, per-branch models), and against three
planted errors that it must be able to tell from the truth.

Measured on the CPU (the worst over the cases of each test; every test prints its own):
  per-pattern lnL vs oracle.tree_loglik, relative      2.7e-16 unscaled, 2.7e-16 scaled  (bound 1e-13)
  d1 / d2 vs oracle.dr_derivatives, _close metric      3.0e-14 (the 300-taxon tree)      (bound 1e-12)
  d1 vs central differences of the longdouble lnL      1.1e-11                           (bound 1e-7)
  d2 vs central differences of the analytic d1         4.2e-14                           (bound 1e-7)
    (both with the h^2 term taken out, see _central: the plain difference at h = 1e-5 is off by
    up to 4.9e-7 in d1 from truncation alone)
  planted errors, smallest move of d2 in the _close metric (they must pass 1e-10):
    2 alpha beta -> alpha beta 1.7e-2, g^2 dropped 1.2, d2P of one branch times (1 + 1e-8) 5.4e-10
"""
import numpy as np
import pytest

import oracle
import phylo
import workload
import xref
from test_gpu_parity import _random_problem

LD = np.longdouble
PAIRS = ((0.3, 0.7), (0.25, -0.25), (1.0, 0.0), (0.0, 1.0))
POLY = "((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2);"
# the same with a fifth son (a tip) at the root: root sons one and five fall in different chunks of three
ROOT5 = "((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2,j:0.15);"
# S, C, taxa, patterns, ambiguity codes (the 4- and 20-state ones)
SHAPES = [(4, 4, 12, 400, True), (20, 2, 8, 150, True), (64, 1, 6, 130, False), (64, 1, 24, 130, False),
          (4, 4, 300, 300, True)]
FLOORS = {}


def _close_err(a, b):
    """|a - b| / max(1, |a|, |b|): _close(a, b, rel) of the GPU tests is _close_err <= rel."""
    return float(abs(a - b) / max(1.0, abs(a), abs(b)))


def _note(key, v):
    FLOORS[key] = max(FLOORS.get(key, 0.0), float(v))
    print(f"{key}: {float(v):.3g} (worst so far {FLOORS[key]:.3g})")


def _oracle_matrices(et, m, rates):
    """P, r Q P, r^2 Q^2 P in fp64 from the oracle's own expm (test_gpu_dr.test_dr_vs_oracle_restatement)."""
    C = len(rates)
    P = np.zeros((et.n_nodes, C, m.S, m.S))
    dP, d2P = np.zeros_like(P), np.zeros_like(P)
    for v in range(et.n_nodes):
        if v != et.root:
            for c, r in enumerate(rates):
                e = oracle.reversible_pij(m.Q, m.pi, et.brlen[v] * r)
                P[v, c], dP[v, c], d2P[v, c] = e, r * m.Q @ e, r ** 2 * m.Q @ m.Q @ e
    return P, dP, d2P


def _poly_problem(n, newick=POLY):
    et = phylo.engine_tree(phylo.Tree.from_newick(newick))
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(4, 0.5)
    wl = workload.Workload("p", et, [m], None, rates, probs, m.pi, phylo.DNA, n, False, True, 9)
    return et, m, phylo.DNA, rates, probs, wl.simulate(0, n).astype(np.int32)


@pytest.mark.parametrize("S,C,n_taxa,n_pat,amb", SHAPES)
def test_lnl_vs_oracle(S, C, n_taxa, n_pat, amb):
    """Per-pattern lnL against oracle.tree_loglik, unscaled and scaled, on the same fp64 P(t)."""
    et, m, alph, rates, probs, states = _random_problem(S, C, n_taxa, n_pat, seed=100 + S + C, amb=amb)
    P, _, _ = _oracle_matrices(et, m, rates)
    x = xref.updown(et, states, alph.init_table, P, None, None, probs, m.pi)
    ss, sons, lr = et.son_arrays()
    for scaling in (False, True):
        lnl, site, _, _ = oracle.tree_loglik(ss, sons, lr, et.root, states, alph.init_table, P, probs, m.pi,
                                             use_patterns=False, scaling=scaling, want_sites=True)
        err = float(np.max(np.abs(x.logl - site) / np.abs(site)))
        _note("lnl scaled" if scaling else "lnl unscaled", err)
        assert err <= 1e-13
        assert abs(float(x.lnl) - lnl) <= 1e-13 * abs(lnl)


@pytest.mark.parametrize("case", list(range(len(SHAPES))) + ["poly"])
def test_derivatives_vs_oracle(case):
    """d1 and d2 of every branch against oracle.dr_derivatives (flat, unscaled fp64)."""
    if case == "poly":
        et, m, alph, rates, probs, states = _poly_problem(1000)
    else:
        S, C, n_taxa, n_pat, amb = SHAPES[case]
        et, m, alph, rates, probs, states = _random_problem(S, C, n_taxa, n_pat, seed=100 + S + C, amb=amb)
    P, dP, d2P = _oracle_matrices(et, m, rates)
    x = xref.updown(et, states, alph.init_table, P, dP, d2P, probs, m.pi)
    ss, sons, lr = et.son_arrays()
    o1, o2 = oracle.dr_derivatives(ss, sons, lr, et.root, states, alph.init_table, P, dP, d2P, probs, m.pi)
    assert x.d1[et.root] == 0 and x.d2[et.root] == 0
    worst = 0.0
    for b in range(et.n_nodes):
        if b != et.root:
            e1, e2 = _close_err(x.d1[b], o1[b]), _close_err(x.d2[b], o2[b])
            worst = max(worst, e1, e2)
            assert e1 <= 1e-12 and e2 <= 1e-12, (b, x.d1[b], o1[b], x.d2[b], o2[b], x.abs1[b], x.abs2[b])
    _note("derivatives", worst)


# ---------------------------------------------------------------- central differences of xref's own lnL

class _Line:
    """A problem whose matrices are rebuilt by xref.eigen_matrices at any branch lengths, a model
    per branch."""

    def __init__(self, et, models, mon, rates, probs, pi, alph, states, weights=None):
        self.et, self.models, self.rates, self.probs, self.pi = et, models, rates, probs, pi
        self.mon = np.zeros(et.n_nodes, dtype=int) if mon is None else mon
        self.init, self.states, self.w = alph.init_table, states, weights
        self.mats0 = self.matrices(et.brlen)

    def matrices(self, brlen, old=None, changed=None):
        et, S, C = self.et, self.models[0].S, len(self.rates)
        if old is None:
            P = np.zeros((et.n_nodes, C, S, S), dtype=LD)
            out, changed = (P, P.copy(), P.copy()), [v for v in range(et.n_nodes) if v != et.root]
        else:
            out = tuple(a.copy() for a in old)
        for v in changed:
            m = self.models[self.mon[v]]
            for c, r in enumerate(self.rates):
                out[0][v, c], out[1][v, c], out[2][v, c] = xref.eigen_matrices(m.V, m.Vinv, m.lam, brlen[v], r)
        return out

    def shifted(self, move):
        """Matrices with brlen[v] + dt for (v, dt) in move."""
        bl = self.et.brlen.astype(LD)
        for v, dt in move:
            bl[v] += dt
        return self.matrices(bl, self.mats0, [v for v, _ in move])

    def lnl(self, mats):
        return xref.updown(self.et, self.states, self.init, mats[0], None, None, self.probs, self.pi, self.w).lnl


H = LD("1e-5")


def _fd_tol(ref):
    return 1e-7 * max(1.0, abs(float(ref)))


def _central(f):
    """f(h) is a central difference with step h.  At h = 1e-5 its truncation h^2 f'''/6 alone
    measured up to 4.9e-7 here (the third derivative of a sum over 300 patterns on branches of
    length 0.1 reaches 3e4; the error fell by 4.0 and 101.6 from 2h to h to h/10, so it is
    truncation), above the 1e-7 this check allows.  So the h^2 term is taken out with the
    difference at 2h (Richardson): what is left is h^4 f'''''/30 and the round-off
    eps_ld |lnL| / h ~ 1e-10, a margin of about a thousand under the tolerance."""
    return (4 * f(H) - f(2 * H)) / 3


def _three_model_problem(n_taxa=12, n=300, seed=74):
    """A rooted tree (the root keeps its two sons) with three GTR models over the branches, the
    two root sons on different models."""
    rng = np.random.default_rng(seed)
    et = phylo.engine_tree(phylo.balanced_tree(n_taxa, seed=seed, lo=0.01, hi=0.3), unroot=False)
    models = [phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5)) for _ in range(3)]
    mon = rng.integers(0, 3, et.n_nodes).astype(np.int32)
    kids = [c for p, ch in et.ops if p == et.root for c in ch]
    assert len(kids) == 2
    mon[kids[0]], mon[kids[1]] = 0, 2
    rates, probs = phylo.gamma_rates(4, 0.5)
    wl = workload.Workload("r", et, models, mon, rates, probs, models[0].pi, phylo.DNA, n, False, True, seed)
    states = wl.simulate(0, n).astype(np.int32)
    return _Line(et, models, mon, rates, probs, models[0].pi, phylo.DNA, states), kids


def _small_problem(newick, unroot, n=200, seed=5):
    rng = np.random.default_rng(seed)
    et = phylo.engine_tree(phylo.Tree.from_newick(newick), unroot=unroot)
    m = phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5))
    rates, probs = phylo.gamma_rates(4, 0.5)
    wl = workload.Workload("s", et, [m], None, rates, probs, m.pi, phylo.DNA, n, False, True, seed)
    states = wl.simulate(0, n).astype(np.int32)
    kids = [c for p, ch in et.ops if p == et.root for c in ch]
    return _Line(et, [m], None, rates, probs, m.pi, phylo.DNA, states), kids


def _pair_cases():
    line, kids = _three_model_problem()
    yield "nh12", line, kids[0], kids[1]
    # three taxa, rooted: an interior node and a tip under the root; and the trifurcation, two tips
    line, kids = _small_problem("((a:0.1,b:0.2):0.15,c:0.3);", unroot=False)
    assert len(kids) == 2
    yield "rooted3", line, kids[0], kids[1]
    line, kids = _small_problem("(a:0.1,b:0.2,c:0.3);", unroot=True)
    assert all(k < line.et.n_tips for k in kids)
    yield "tips3", line, kids[0], kids[1]
    et, m, alph, rates, probs, states = _poly_problem(300, ROOT5)
    line = _Line(et, [m], None, rates, probs, m.pi, alph, states)
    kids = [c for p, ch in et.ops if p == et.root for c in ch]
    assert len(kids) == 5 and kids[4] < et.n_tips
    yield "poly", line, kids[0], kids[4]


@pytest.mark.parametrize("name", ["nh12", "rooted3", "tips3", "poly"])
def test_root_pair_vs_central_differences(name):
    line, a, b = next(c[1:] for c in _pair_cases() if c[0] == name)
    et = line.et
    args = (et, line.states, line.init)
    terms = xref.root_pair_terms(*args, *line.mats0, line.probs, line.pi, a, b)
    for alpha, beta in PAIRS:
        d1, d2 = xref.root_pair(*args, *line.mats0, line.probs, line.pi, a, b, alpha, beta, terms=terms)
        def lnl_diff(h):
            return (line.lnl(line.shifted([(a, LD(alpha) * h), (b, LD(beta) * h)])) -
                    line.lnl(line.shifted([(a, -LD(alpha) * h), (b, -LD(beta) * h)]))) / (2 * h)

        def d1_diff(h):
            mp = line.shifted([(a, LD(alpha) * h), (b, LD(beta) * h)])
            mm = line.shifted([(a, -LD(alpha) * h), (b, -LD(beta) * h)])
            return (xref.root_pair(*args, *mp, line.probs, line.pi, a, b, alpha, beta)[0] -
                    xref.root_pair(*args, *mm, line.probs, line.pi, a, b, alpha, beta)[0]) / (2 * h)

        fd1, fd2 = _central(lnl_diff), _central(d1_diff)
        _note("fd d1", abs(d1 - fd1) / max(1.0, abs(float(fd1))))
        _note("fd d2", abs(d2 - fd2) / max(1.0, abs(float(fd2))))
        assert abs(d1 - fd1) <= _fd_tol(fd1), (alpha, beta, d1, fd1)
        assert abs(d2 - fd2) <= _fd_tol(fd2), (alpha, beta, d2, fd2)
    # one branch alone is the ordinary branch derivative of the up-down pass
    x = xref.updown(*args, *line.mats0, line.probs, line.pi)
    d1, d2 = xref.root_pair(*args, *line.mats0, line.probs, line.pi, a, b, 1.0, 0.0, terms=terms)
    assert _close_err(d1, x.d1[a]) <= 1e-15 and _close_err(d2, x.d2[a]) <= 1e-15


def test_per_branch_models_vs_central_differences():
    """Every branch of the three-model tree: d1 against the difference of lnL, d2 against the
    difference of the analytic d1."""
    line, _ = _three_model_problem()
    et = line.et
    args = (et, line.states, line.init)
    x = xref.updown(*args, *line.mats0, line.probs, line.pi)
    for v in range(et.n_nodes):
        if v == et.root:
            continue
        def lnl_diff(h):
            return (line.lnl(line.shifted([(v, h)])) - line.lnl(line.shifted([(v, -h)]))) / (2 * h)

        def d1_diff(h):
            return (xref.updown(*args, *line.shifted([(v, h)]), line.probs, line.pi).d1[v] -
                    xref.updown(*args, *line.shifted([(v, -h)]), line.probs, line.pi).d1[v]) / (2 * h)

        fd1, fd2 = _central(lnl_diff), _central(d1_diff)
        _note("fd d1", abs(x.d1[v] - fd1) / max(1.0, abs(float(fd1))))
        _note("fd d2", abs(x.d2[v] - fd2) / max(1.0, abs(float(fd2))))
        assert abs(x.d1[v] - fd1) <= _fd_tol(fd1), (v, x.d1[v], fd1)
        assert abs(x.d2[v] - fd2) <= _fd_tol(fd2), (v, x.d2[v], fd2)


# ---------------------------------------------------------------- it can fail

GPU_TOL = 1e-10


def test_planted_errors_are_caught():
    """Three errors, each planted on the 4-state three-model tree, move the result past the
    tolerance of the GPU tests (_close at 1e-10): a reference that agreed with an engine
    carrying one of them would not have checked it."""
    line, (a, b) = _three_model_problem()
    et = line.et
    args = (et, line.states, line.init)
    P, dP, d2P = line.mats0
    l, la, lb, laa, lbb, lab = xref.root_pair_terms(*args, P, dP, d2P, line.probs, line.pi, a, b)
    d2P_bad = d2P.copy()
    d2P_bad[a] *= LD(1) + LD("1e-8")
    for alpha, beta in PAIRS[:2]:   # both branches move: the cross term is there
        _, d2 = xref.root_pair(*args, P, dP, d2P, line.probs, line.pi, a, b, alpha, beta)
        al, be = LD(alpha), LD(beta)
        g1 = al * la + be * lb
        half = (al * al * laa + al * be * lab + be * be * lbb - g1 * g1).sum()
        no_g2 = (al * al * laa + 2 * al * be * lab + be * be * lbb).sum()
        for key, wrong in (("plant alpha beta", half), ("plant no g^2", no_g2)):
            FLOORS[key] = min(FLOORS.get(key, np.inf), _close_err(wrong, d2))
            print(f"{key}: moves d2 by {_close_err(wrong, d2):.3g}")
            assert _close_err(wrong, d2) > GPU_TOL, (key, alpha, beta, wrong, d2)
    # d2P of branch a larger by 1e-8, seen along a alone (alpha^2 does not shrink it)
    _, d2 = xref.root_pair(*args, P, dP, d2P, line.probs, line.pi, a, b, 1.0, 0.0)
    _, scaled = xref.root_pair(*args, P, dP, d2P_bad, line.probs, line.pi, a, b, 1.0, 0.0)
    print(f"plant d2P: moves d2 by {_close_err(scaled, d2):.3g}")
    assert _close_err(scaled, d2) > GPU_TOL, (scaled, d2)
    # the same d2P error through the up-down pass
    x, xb = xref.updown(*args, P, dP, d2P, line.probs, line.pi), xref.updown(*args, P, dP, d2P_bad, line.probs, line.pi)
    print(f"plant d2P (updown): moves d2 by {_close_err(xb.d2[a], x.d2[a]):.3g}")
    assert _close_err(xb.d2[a], x.d2[a]) > GPU_TOL
    others = [v for v in range(et.n_nodes) if v not in (a, et.root)]
    assert all(xb.d2[v] == x.d2[v] for v in others) and np.array_equal(xb.d1, x.d1)
