"""The extended-range reference (tests/xref.py) checked before tests/test_gpu_xref.py and
tests/test_gpu_xref_consumers.py rely on it: against the fp64 oracle where the oracle has the
quantity, against central differences of its own longdouble lnL where it has not (root pairs,
per-branch models), posteriors, counts and NNI scores against the fp64 references of the
consumers' own GPU tests, and against planted errors that it must be able to tell from the
truth.

Measured on the CPU (the worst over the cases of each test; every test prints its own):
  per-pattern lnL vs oracle.tree_loglik, relative      2.7e-16 unscaled, 2.7e-16 scaled  (bound 1e-13)
  d1 / d2 vs oracle.dr_derivatives, _close metric      3.0e-14 (the 300-taxon tree)      (bound 1e-12)
  d1 vs central differences of the longdouble lnL      1.1e-11                           (bound 1e-7)
  d2 vs central differences of the analytic d1         4.2e-14                           (bound 1e-7)
    (both with the h^2 term taken out, see _central: the plain difference at h = 1e-5 is off by
    up to 4.9e-7 in d1 from truncation alone)
  planted errors, smallest move of d2 in the _close metric (they must pass 1e-10):
    2 alpha beta -> alpha beta 1.7e-2, g^2 dropped 1.2, d2P of one branch times (1 + 1e-8) 5.4e-10
  posteriors vs the clamping reference, absolute             6.7e-16                      (bound 1e-13)
  counts vs plain pruning on Van Loan's W, / max(1, |ref|)   2.1e-15                      (bound 2e-13)
  NNI delta vs test_nni_cpu.Pruning, weight sums             3.8e-14                      (bound 1e-12)
  NNI d1 / d2 vs test_nni_cpu.Restatement, / max(wsum, |ref|)
    the fp64 restatement                                     1.0e-14 / 1.7e-14            (bound 1e-12)
    the same restatement held in longdouble                  2.7e-18 / 6.7e-18            (bound 5e-16)
    (with the trial P in the unit form I + V expm1(lambda r t) Vinv, xref.eigen_matrices.  With
    V exp(lambda r t) Vinv the restatement, which sums the short-length form d + sum gamma expm1,
    was 5.8e-12 / 1.1e-11 away at t = 1e-6, 7.4e-11 weight sums in d1 on 64 states, in doubles and
    in longdouble alike: V Vinv - I of an eigen system held in doubles, not rounding.)
  planted errors in the consumers (they must pass 1e-10): a sibling left out of up_v moves a joint
    posterior by 0.52, W of one type times (1 + 1e-8) a count by 8.8e-9 (the total per weight by
    2.9e-10), the pair swapped in p's son list only delta by at least 0.12 weight sums
  the seeds of the GPU cases: no best_state cell inside the 1e-8 gap; group G regimes 60 % to 92 %
"""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import phylo
import workload
import xref
import test_nni_cpu as nni_ref
from test_count_matrices_cpu import van_loan
from test_gpu_mapping import _pruning_counts
from test_gpu_parity import _random_problem
from test_gpu_posteriors import _clamp_joint
from test_gpu_posteriors import _lower as _fp64_lower

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


# ---------------------------------------------------------------- posteriors, counts, NNI

CONSUMER_SHAPES = SHAPES[:4]


def _consumer_problem(case):
    if case == "poly":
        return _poly_problem(300)
    S, C, n_taxa, n_pat, amb = CONSUMER_SHAPES[case]
    return _random_problem(S, C, n_taxa, n_pat, seed=100 + S + C, amb=amb)


def _internal(et):
    return list(range(et.n_tips, et.n_nodes))


def _branches(et):
    return [v for v in range(et.n_nodes) if v != et.root]


def _all_moves(et):
    """Every (son, uncle) whose father is not the root, whatever the number of sons (the
    reference serves the polytomies the engine leaves out)."""
    sons, par = nni_ref.sons_of(et.ops), nni_ref.parents_of(et.ops)
    return [(s, u) for s in sorted(par) if par[s] != et.root for u in sons[par[par[s]]] if u != par[s]]


@pytest.mark.parametrize("case", list(range(len(CONSUMER_SHAPES))) + ["poly"])
def test_posteriors_vs_clamping(case):
    """joint, state and class posteriors of every internal node against the clamping
    reference of test_gpu_posteriors.py (fp64: prune with L_v zeroed except at x)."""
    et, m, alph, rates, probs, states = _consumer_problem(case)
    P, _, _ = _oracle_matrices(et, m, rates)
    nodes = _internal(et)
    x = xref.posteriors(et, states, alph.init_table, P, probs, m.pi, nodes)
    L = _fp64_lower(et, states, alph.init_table, P)
    worst = 0.0
    for i, v in enumerate(nodes):
        J = _clamp_joint(et, L, P, probs, m.pi, v)
        J = J / J.sum(axis=(1, 2))[:, None, None]
        worst = max(worst, float(np.abs(x.joint[i] - J).max()), float(np.abs(x.states[i] - J.sum(axis=1)).max()),
                    float(np.abs(x.classes[i] - J.sum(axis=2)).max()))
        assert np.array_equal(x.best[i], x.states[i].argmax(axis=1))
    _note("posteriors", worst)
    assert worst <= 1e-13
    assert float(np.abs(x.joint.sum(axis=(2, 3)) - 1).max()) <= 1e-17


@pytest.mark.parametrize("case", list(range(len(CONSUMER_SHAPES))) + ["poly"])
def test_counts_vs_pruning(case):
    """Counts of every branch against _pruning_counts of test_gpu_mapping.py with Van Loan's W
    (DNA: the twelve comprehensive types; 20 and 64 states: the total register)."""
    et, m, alph, rates, probs, states = _consumer_problem(case)
    P, _, _ = _oracle_matrices(et, m, rates)
    B = phylo.comprehensive_register(m.Q) if m.S == 4 else phylo.total_register(m.Q)
    br = _branches(et)
    W = {v: np.stack([van_loan(m.Q, B, et.brlen[v] * r) for r in rates], axis=1) for v in br}
    x = xref.branch_counts(et, states, alph.init_table, P, W, probs, m.pi, br)
    L = _fp64_lower(et, states, alph.init_table, P)
    worst = 0.0
    for i, v in enumerate(br):
        ref = _pruning_counts(et, L, P, W, probs, m.pi, v)
        worst = max(worst, float((np.abs(x.counts[i] - ref) / np.maximum(1.0, np.abs(ref))).max()))
    _note("counts", worst)
    assert worst <= 2e-13
    assert np.array_equal(x.totals, x.counts.sum(axis=1))


def _trial(m, rates, t):
    mats = [xref.trial_matrices(m.V, m.Vinv, m.lam, ti, rates) for ti in t]
    return tuple([mm[k] for mm in mats] for k in range(3))


@pytest.mark.parametrize("case", list(range(len(CONSUMER_SHAPES))) + ["poly"])
def test_nni_vs_pruning_and_restatement(case):
    """delta of every move against test_nni_cpu.Pruning (the oracle on the swapped son arrays) at
    t_cur, t_cur / 2, 1e-6 and 3; d1 and d2 against test_nni_cpu.Restatement (the engine's
    gamma / eigen formulation in numpy), d2 relative as in test_gpu_nni.py."""
    et, m, alph, rates, probs, states = _consumer_problem(case)
    P, _, _ = _oracle_matrices(et, m, rates)
    P[et.root] = np.eye(m.S)[None]
    moves = _all_moves(et)
    if len(moves) > 12:
        moves = moves[::len(moves) // 12]
    par = nni_ref.parents_of(et.ops)
    rng = np.random.default_rng(7)
    w = rng.integers(1, 9, states.shape[1]).astype(np.float64)
    wsum = w.sum()
    args = (states, alph.init_table, P, rates, probs, m.pi, m, w)
    pr = nni_ref.Pruning(et.ops, et.root, et.n_nodes, et.n_tips, *args)
    rs = nni_ref.Restatement(et.ops, et.root, et.n_tips, *args)
    ml = SimpleNamespace(V=m.V.astype(LD), Vinv=m.Vinv.astype(LD), lam=m.lam.astype(LD))
    rl = nni_ref.Restatement(et.ops, et.root, et.n_tips, states, alph.init_table, P.astype(LD), rates.astype(LD),
                             probs.astype(LD), m.pi.astype(LD), ml, w.astype(LD))
    t_cur = np.array([et.brlen[par[s]] for s, _ in moves])
    for t0 in (t_cur, 0.5 * t_cur, np.full(len(moves), 1e-6), np.full(len(moves), 3.0)):
        x = xref.nni(et, states, alph.init_table, P, probs, m.pi, moves, *_trial(m, rates, t0), weights=w)
        r = rs.scores(moves, t0)
        for i, (s, u) in enumerate(moves):
            _, l1, l2 = _evaluate_ld(rl, s, u, t0[i])
            ed = abs(float(x.delta[i]) - pr.delta(s, u, t0[i])) / wsum
            e1 = float(abs(x.d1[i] - l1)) / max(wsum, abs(r["d1"][i]))
            e2 = float(abs(x.d2[i] - l2)) / max(wsum, abs(r["d2"][i]))
            f1 = abs(float(x.d1[i]) - r["d1"][i]) / max(wsum, abs(r["d1"][i]))
            f2 = abs(float(x.d2[i]) - r["d2"][i]) / max(wsum, abs(r["d2"][i]))
            fa = abs(float(x.d1[i]) - r["d1"][i]) / wsum
            for key, v in (("nni delta", ed), ("nni d1", e1), ("nni d2", e2), ("nni d1 fp64", f1), ("nni d2 fp64", f2),
                           ("nni d1 fp64 per weight", fa)):
                _note(key, v)
            assert max(ed, f1, f2) <= 1e-12 and max(e1, e2) <= 5e-16, (s, u, t0[i], ed, e1, e2, f1, f2)


def _evaluate_ld(rl, s, u, t):
    """test_nni_cpu.evaluate of a Restatement held in longdouble, the sums left in longdouble
    (evaluate itself returns Python floats)."""
    gam, d = rl.coefficients(s, u)
    mu = rl.rates[:, None] * rl.model.lam[None, :]
    e = np.exp(mu * LD(t))
    r0 = d + np.einsum("pck,ck->p", gam, np.expm1(mu * LD(t)))   # the short-length form at every t
    g1 = np.einsum("pck,ck->p", gam, e * mu) / r0
    g2 = np.einsum("pck,ck->p", gam, e * mu * mu) / r0
    return (rl.w * np.log(r0)).sum(), (rl.w * g1).sum(), (rl.w * (g2 - g1 * g1)).sum()


def test_planted_errors_in_the_consumers_are_caught():
    """Each new function tells a planted error from the truth at the GPU tests' tolerance: a
    sibling left out of up_v (posteriors, 1e-10 absolute), W of one type times 1 + 1e-8 (counts,
    1e-10 max(1, |ref|)), the pair swapped in the son list of p but not of g (NNI delta,
    1e-10 weight sums)."""
    et, m, alph, rates, probs, states = _consumer_problem(0)
    P, _, _ = _oracle_matrices(et, m, rates)
    n, C, S = states.shape[1], len(rates), m.S
    # a sibling left out of up_v
    sons, par = nni_ref.sons_of(et.ops), nni_ref.parents_of(et.ops)
    v = next(v for v in _internal(et) if v != et.root)
    sib = next(o for o in sons[par[v]] if o != v)
    x = xref.posteriors(et, states, alph.init_table, P, probs, m.pi, [v])
    Pl, pl, pil = xref._ld(P), xref._ld(probs), xref._ld(m.pi)
    L, q = xref._lower(et, states, alph.init_table, Pl)
    q_bad = dict(q)
    q_bad[sib] = np.ones((n, C, S), dtype=LD)
    _, up = xref._father_sides(et, q_bad, pil, Pl, n, C, S, [v])
    J = pl[None, :, None] * L[v] * up[v]
    J = J / J.sum(axis=(1, 2))[:, None, None]
    move = float(np.abs(J - x.joint[0]).max())
    print(f"plant sibling: moves joint by {move:.3g}")
    FLOORS["plant sibling"] = move
    assert move > GPU_TOL
    # W of one type larger by 1e-8
    B = phylo.comprehensive_register(m.Q)
    br = _branches(et)
    W = {b: np.stack([van_loan(m.Q, B, et.brlen[b] * r) for r in rates], axis=1) for b in br}
    W_bad = {b: W[b].astype(LD) for b in br}
    for b in br:
        W_bad[b][3] *= LD(1) + LD("1e-8")
    c = xref.branch_counts(et, states, alph.init_table, P, W, probs, m.pi, br)
    cb = xref.branch_counts(et, states, alph.init_table, P, W_bad, probs, m.pi, br)
    wsum = LD(n)
    move = float((np.abs(cb.totals - c.totals) / wsum / np.maximum(1.0, np.abs(c.totals) / wsum)).max())
    movec = float((np.abs(cb.counts - c.counts) / np.maximum(1.0, np.abs(c.counts))).max())
    print(f"plant W: moves counts by {movec:.3g}, totals / weight sum by {move:.3g}")
    FLOORS["plant W"] = movec
    assert movec > GPU_TOL
    others = [k for k in range(12) if k != 3]
    assert np.array_equal(cb.counts[:, :, others], c.counts[:, :, others])
    # the swapped pair not swapped in the son list of g
    moves = _all_moves(et)[::5]
    t_cur = np.array([et.brlen[par[s]] for s, _ in moves])
    tm = _trial(m, rates, t_cur)

    def half_swap(sons, par, s, u):
        p = par[s]
        return {p: [u if o == s else o for o in sons[p]]}

    good = xref.nni(et, states, alph.init_table, P, probs, m.pi, moves, *tm)
    bad = xref.nni(et, states, alph.init_table, P, probs, m.pi, moves, *tm, swap=half_swap)
    move = float(np.abs(bad.delta - good.delta).min() / wsum)
    print(f"plant half swap: moves delta by at least {move:.3g} weight sums")
    FLOORS["plant half swap"] = move
    assert move > GPU_TOL


# ---------------------------------------------------------------- the GPU cases, as far as the CPU can judge them

def _eigen_P(case):
    """fp64 V exp(lambda r t) Vinv of every branch (the engine's own matrices differ in the last
    digits: nothing here is that sensitive)."""
    et = case.et
    P = np.zeros((et.n_nodes, case.C, case.S, case.S))
    for v in case.br:
        m = case.models[0 if case.mon is None else int(case.mon[v])]
        P[v] = np.stack([m.pij(r * et.brlen[v]) for r in case.rates])
    return P


def _gpu_cases():
    import test_gpu_xref_consumers as cons
    from test_gpu_posteriors import _six_nodes
    from test_gpu_xref import _case_bc1, _case_deep, _case_very_deep
    yield "E C=3", _case_very_deep(4, 3), _six_nodes
    yield "E C=8", _case_very_deep(4, 8), _six_nodes
    yield "F S=20", _case_deep(20), _six_nodes
    yield "F S=64", _case_deep(64), _six_nodes
    yield "H flat", _case_bc1(False), _internal
    yield "H scaled", _case_bc1(True), _internal
    for name in sorted(cons.G_CASES):
        yield "G " + name, cons._case_g(name), _internal


@pytest.mark.parametrize("group", ["E C=3", "E C=8", "F S=20", "F S=64", "H flat", "H scaled", "G binary-C4", "G binary-C8",
                                   "G poly-C4", "G poly-C4-fused", "G tri-C4", "G tri-C8", "G tri-S20"])
def test_gpu_cases_best_state_and_regime(group):
    """The seeds of tests/test_gpu_xref_consumers.py: the reference alone leaves at most 1 % of the
    best_state cells inside the 1e-8 gap; the group G cases reach their regime (the product of
    the stored vectors' joint maxima below 2^-1022 on a quarter of the patterns) while the lower
    pass, carried out by the traversal's rule, keeps every stored partial a normal double."""
    import test_gpu_xref_consumers as cons
    case, pick = next(c[1:] for c in _gpu_cases() if c[0] == group)
    P = _eigen_P(case)
    low = xref.lower(case.et, case.states, case.alph.init_table, P)
    nodes = pick(case.et)
    x = xref.posteriors(case.et, case.states, case.alph.init_table, P, case.probs, case.pi, nodes, lower=low)
    top = np.sort(x.states, axis=2)
    skipped = 1.0 - float(np.asarray(top[:, :, -1] - top[:, :, -2] > 1e-8).mean())
    print(f"{group}: best_state cells inside the 1e-8 gap {skipped:.2%}, smallest likelihood 2^{float(np.log2(x.l.min())):.0f}")
    assert skipped <= 0.01
    if not group.startswith("G "):
        return
    Lmax, Umax, Ls = cons._stored(case, P, low)
    (mv_share, mv), (f_share, f) = cons._regime(case, Lmax, Umax)
    print(f"{group}: regime on {mv_share:.0%} of the patterns at the move {mv}, {f_share:.0%} at the father {f}")
    want_move, want_father = {"binary": (True, False), "tri": (True, True), "poly": (False, True)}[group.split()[1].split("-")[0]]
    assert (mv_share >= 0.25 or not want_move) and (f_share >= 0.25 or not want_father)
    for v in range(case.et.n_tips, case.et.n_nodes):
        m = Ls[v].max(axis=(1, 2))
        assert np.all((m == 0) | (m >= LD(2) ** -1022)), v


# ---------------------------------------------------------------- the rescaling rule restated (tests/rescale_rule.py)

def test_rescale_rule_check_points():
    """Once per node, after every three sons, and the rule whose running products never hold more
    than three stored vectors between two checks."""
    import rescale_rule as rr
    assert rr.check_points(9, False, True) == {9} and rr.check_points(9, False, False) == {3, 6, 9}
    assert rr.check_points(5, False, False) == {3, 5} and rr.check_points(5, True) == {3, 5}
    assert rr.check_points(9, True) == {3, 5, 6, 8, 9} and rr.check_points(10, True) == {3, 5, 6, 8, 9, 10}
    for n in range(1, 4):
        assert rr.check_points(n, True) == rr.check_points(n, False, True) == rr.check_points(n, False, False) == {n}
    for n in range(1, 20):   # at most three factors between two checks: the carried product and two sons, or three sons
        pts = sorted(rr.check_points(n, True))
        assert pts[0] <= 3 and all(b - a <= 2 for a, b in zip(pts, pts[1:])) and pts[-1] == n


RESCALE_CASES = ["I-C1", "I-C4", "I-C8", "I-S20", "I-S64", "J5-C1", "J5-C4", "J5-S20", "J5-S64", "J9-C4", "J9-C8", "J9-S20",
                 "Js-C4", "Js-C8", "Js-S20", "K-C1", "K-C4", "K-S20"]


@pytest.mark.parametrize("name", RESCALE_CASES)
def test_rescale_cases_regime(name):
    """The cases of tests/test_gpu_xref_rescale.py, as conditions on their inputs.  Under the
    rule up to now (one step per check), on the check points of the path the case targets, at
    least a quarter of the patterns end with an all-zero root partial: the fused and the
    levelwise points alike for I, J9 and Js (Js: an all-zero U of some node as well); the fused
    ones for J5 and K, where a check after every three sons still kept the product alive; on
    K-C1 and K-S20 every pattern.  Under the new rule no running product's joint maximum falls
    below 2^-1022 and every stored joint maximum lies in [2^-256, 1].  The reference's smallest
    likelihood is far inside its range, and where the GPU tests compare best_state at most 1 %
    of its cells lie inside the 1e-8 gap."""
    import rescale_rule as rr
    import test_gpu_xref_rescale as resc
    assert sorted(RESCALE_CASES) == sorted(resc.CASES)
    case = resc.case_of(name)
    et = case.et
    tree = resc.CASES[name][0]
    assert max(len(ch) for _, ch in et.ops) == {"i": 3, "root5": 5, "root9": 9, "son": 9, "star": et.n_tips}[tree]
    P = _eigen_P(case)
    args = (et, case.states, case.alph.init_table, P, case.pi)
    x = xref.updown(*args[:4], None, None, case.probs, case.pi)
    assert x.l.min() > xref.RANGE_MIN
    if tree in ("i", "son"):
        top = np.sort(xref.posteriors(*args[:4], case.probs, case.pi, _internal(et)).states, axis=2)
        assert 1.0 - float(np.asarray(top[:, :, -1] - top[:, :, -2] > 1e-8).mean()) <= 0.01
    shares = {}
    for fused in (True, False):
        old = rr.stored_once(*args, fused)
        shares[fused] = (float(rr.lost_lower(old, et).mean()), float(rr.lost_upper(old).mean()) if old.U else 0.0)
    assert shares[True][0] >= (1.0 if name in ("K-C1", "K-S20") else 0.25), shares
    if tree in ("i", "root9", "son"):
        assert shares[False][0] >= 0.25, shares
    if tree == "son":
        assert shares[True][1] >= 0.25 and shares[False][1] >= 0.25, shares
    new = rr.stored_new(*args)
    steps = max(int((new.k[p] - sum(new.k[c] for c in ch)).max()) for p, ch in et.ops)
    print(f"{name}: root partial all zero under one step per check on {shares[True][0]:.0%} of the patterns (fused), "
          f"{shares[False][0]:.0%} (levelwise), some stored U on {shares[True][1]:.0%}; new rule: smallest running maximum "
          f"2^{float(np.log2(new.low.min())):.0f}, most steps in one node {steps}; smallest likelihood "
          f"2^{float(np.log2(x.l.min())):.0f}")
    assert new.low.min() >= rr.NORMAL_MIN
    assert rr.in_range(new, et)
    assert not rr.lost_lower(new, et).any() and not (new.U and rr.lost_upper(new).any())
    assert steps >= 2
    # the counts are those of the reference's own magnitudes: L_ref 2^(256 k) has its joint maximum in [2^-256, 1)
    L, _ = xref.lower(*args[:4])
    for v in range(et.n_tips, et.n_nodes):
        m = rr.scaled_reference(L[v], new.k[v]).max(axis=(1, 2))
        assert np.all((m >= LD(2) ** -256) & (m < 1)), v
