"""The engine against the extended-range reference (tests/xref.py: one up-down pass in 80-bit
longdouble, never rescaled, checked on the CPU by tests/test_xref_cpu.py) on the engine's
own P, r dP, r^2 d2P.

  A  lnL under rescaling that fires (600 / 120 / 150-taxon caterpillars), per pattern at 1e-12:
     the 2^256 scheme against numbers that carry no scale counts at all.
  B  plk_branch_derivatives and C plk_all_branch_derivatives of one PLK_FLAG_DOUBLE_RECURSIVE
     engine, every branch (path: 12 chosen branches on trees above 40 taxa): per-branch models
     (4, 20, 64 states), class counts off the fused kernels (3, 8), rescaling that fires,
     zero-length and saturated branches, a polytomy under fractional weights, the
     per-subtree-compressed handle; and per-pattern lnL below -1022 ln 2, where a path vector
     of one sign once left the double range (test_bc10_path_vectors_of_one_sign).
  D  plk_root_pair_derivatives: per-branch models, tip sons, 20 and 64 states, a five-son root
     (the pair in one and in two PLK_OP_ACCUMULATE chunks), root sons of 150 tips each whose
     five scratch products carry scale counts of their own, weights.

Tolerances are the project's: lnL relative 1e-12 (test_gpu_parity.REL); derivatives _close at
1e-10, 1e-9 where the case's smallest per-pattern lnL is below -256 ln 2 (test_gpu_dr.py).
A derivative miss reports abs1 / abs2, the sum of the magnitudes that were added: a miss of the
order of 1e-16 of it is cancellation, anything larger a wrong term.  Every test prints its
worst difference ("xref <group> ..."): a record, not a tolerance.
"""
import functools

import numpy as np
import pytest

import phylo
import plk
import workload
import xref
from test_gpu_parity import MODES, REL, _caterpillar, _random_problem, _random_topology, engine_for, engine_pmats, run_engine

pytestmark = pytest.mark.gpu

DR = plk.PLK_FLAG_DOUBLE_RECURSIVE
SC = plk.PLK_FLAG_SCALING
GUARD = plk.PLK_FLAG_NONNEG_GUARD
SUB = plk.PLK_FLAG_SUBTREE_PATTERNS
FLAGS = dict(MODES, subtree=SUB)
RESCALED = -256 * np.log(2)
PAIRS = ((0.3, 0.7), (0.25, -0.25), (1.0, 0.0), (0.0, 1.0))
POLY = "((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2);"
# the same with a fifth son (a tip) at the root: root sons one and five fall in different chunks of three
ROOT5 = "((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2,j:0.15);"


def _expected_path(S, C, mode):
    """What serves the traversal (Engine.kernel_path): the fused kernels take 4 states with 1, 2
    or 4 classes, 20 states with up to 4, 64 states with one."""
    if mode == "subtree":
        return "subtree_patterns"
    if mode == "levelwise" or (S == 4 and C not in (1, 2, 4)) or (S == 64 and C != 1) or C > 4:
        return "levelwise"
    return {4: "jit_tree4", 20: "jit_treeM", 64: "treeM"}[S]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


# ---------------------------------------------------------------- helpers

def _close_err(a, b):
    """_close(a, b, rel) of test_gpu_dr.py is _close_err(a, b) <= rel."""
    return float(abs(a - b) / max(1.0, abs(a), abs(b)))


class Case:
    """A problem: tree, one model per branch (mon) or one for all, data, optional weights."""

    def __init__(self, et, models, mon, alph, C, n, seed, amb=0.0, alpha=0.5, weights=None):
        self.et, self.models, self.alph, self.n, self.w = et, models, alph, n, weights
        self.mon = None if mon is None else np.asarray(mon, dtype=np.int32)
        self.S, self.C, self.pi = models[0].S, C, models[0].pi
        self.rates, self.probs = phylo.gamma_rates(C, alpha) if C > 1 else (np.ones(1), np.ones(1))
        wl = workload.Workload("x", et, models, self.mon, self.rates, self.probs, self.pi, alph, n, False, True, seed)
        self.states = wl.simulate(0, n).astype(np.int32)
        if amb:
            rng = np.random.default_rng(seed + 1)
            mask = rng.random(self.states.shape) < amb
            self.states[mask] = rng.integers(self.S, alph.n_codes, size=mask.sum())
        self.br = np.array([v for v in range(et.n_nodes) if v != et.root], dtype=np.int32)
        self.kids = [c for p, ch in et.ops if p == et.root for c in ch]
        self._ref = None

    def engine(self, mode, extra=0, expect=None):
        """An engine with P, dP, d2P of every branch, after one traversal: (engine, per-pattern
        lnL, lnL).  expect: the kernel path to assert where a tuning knob changes it (JIT=0)."""
        eng = engine_for(self.et, self.S, self.C, self.n, self.states, self.alph.init_table, self.rates, self.probs,
                         self.pi, self.models, model_of_node=self.mon, flags=GUARD | FLAGS[mode] | extra)
        eng.update_pmatrices(self.br, self.et.brlen[self.br], None if self.mon is None else self.mon[self.br],
                             deriv_mask=7)
        if self.w is not None:
            eng.set_pattern_weights(self.w)
        lnl, site, _ = run_engine(eng, self.et)
        want = _expected_path(self.S, self.C, mode) if expect is None else expect
        assert eng.kernel_path() == want, (eng.kernel_path(), self.S, self.C, mode)
        return eng, site, lnl

    def matrices(self, eng):
        P = engine_pmats(eng, self.et)
        dP, d2P = np.zeros_like(P), np.zeros_like(P)
        for v in self.br:
            dP[v], d2P[v] = eng.get_dpmatrix(int(v), 1), eng.get_dpmatrix(int(v), 2)
        return P, dP, d2P

    def reference(self, eng, derivatives=True):
        """xref.updown on this engine's matrices; computed once per case and shared while the
        engines of the case hold bitwise the same matrices (they do: one P(t) kernel per state
        count, whatever the traversal mode)."""
        mats = self.matrices(eng)
        if self._ref is None or not all(np.array_equal(a, b) for a, b in zip(mats, self._ref[0])):
            x = xref.updown(self.et, self.states, self.alph.init_table, mats[0], mats[1] if derivatives else None,
                            mats[2] if derivatives else None, self.probs, self.pi, self.w)
            self._ref = (mats, x)
        return self._ref


def _check_lnl(group, site, lnl, x):
    assert np.all(np.isfinite(site))
    logl = x.logl.astype(np.float64)
    err = float(np.max(np.abs(site - logl) / np.abs(logl)))
    print(f"xref {group} lnL: per-pattern {err:.3g}, total {abs(lnl - float(x.lnl)) / abs(float(x.lnl)):.3g}, "
          f"smallest per-pattern lnL {site.min():.1f}")
    assert np.allclose(site, logl, rtol=REL, atol=0), err
    assert abs(lnl - float(x.lnl)) <= REL * abs(float(x.lnl)), (lnl, x.lnl)


def _tol(site):
    return 1e-9 if site.min() < RESCALED else 1e-10


def _path_branches(et):
    """Every branch up to 40 taxa; above, 12: the first and last tip, the deepest tip's father,
    two root sons, seven spread evenly by index."""
    br = [v for v in range(et.n_nodes) if v != et.root]
    if et.n_tips <= 40:
        return br
    parent = {c: p for p, ch in et.ops for c in ch}

    def depth(v):
        d = 0
        while v in parent:
            v, d = parent[v], d + 1
        return d

    deepest = max(range(et.n_tips), key=depth)
    kids = [c for p, ch in et.ops if p == et.root for c in ch]
    pick = [0, et.n_tips - 1, parent[deepest], kids[0], kids[1]]
    rest = [b for b in br if b not in pick]
    pick += [rest[int(i)] for i in np.linspace(0, len(rest) - 1, 9)[1:-1]]
    assert len(set(pick)) == 12
    return pick


def _check_derivatives(group, case, eng, site, x, dr=True):
    et, tol = case.et, _tol(site)
    worst = 0.0

    def cmp(what, b, got, want, mag):
        nonlocal worst
        e = _close_err(got, want)
        worst = max(worst, e)
        assert e <= tol, (f"{what} of branch {b}: engine {got!r}, reference {float(want)!r}, miss {e:.3g} of "
                          f"tolerance {tol:g}; sum of magnitudes {float(mag):.6g}, eps of it "
                          f"{2.2e-16 * float(mag) / max(1.0, abs(float(want))):.3g}")

    if dr:
        d1, d2 = eng.all_branch_derivatives()
        assert d1[et.root] == 0.0 and d2[et.root] == 0.0
        for b in case.br:
            cmp("DR d1", b, d1[b], x.d1[b], x.abs1[b])
            cmp("DR d2", b, d2[b], x.d2[b], x.abs2[b])
        print(f"xref {group} C (all-branch) worst {worst:.3g} over {len(case.br)} branches")
        worst = 0.0
    pick = _path_branches(et)
    for b in pick:
        p1, p2 = eng.branch_derivatives(int(b))
        cmp("path d1", b, p1, x.d1[b], x.abs1[b])
        cmp("path d2", b, p2, x.d2[b], x.abs2[b])
    print(f"xref {group} B (path) worst {worst:.3g} over {len(pick)} branches")


def _run_bc(group, case, mode, scaling, dr=True, rescaled=False):
    eng, site, lnl = case.engine(mode, (SC if scaling else 0) | (DR if dr else 0))
    _, x = case.reference(eng)
    assert x.l.min() > 1e-400
    if rescaled:
        assert site.min() < RESCALED, site.min()
    _check_lnl(group, site, lnl, x)
    _check_derivatives(group, case, eng, site, x, dr=dr)
    return eng


def _gtrs(rng, k):
    return [phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5)) for _ in range(k)]


def _rand_model(rng, S):
    """A random reversible model, as test_gpu_parity._random_problem builds its "rand" one."""
    E = rng.uniform(0.1, 2.0, (S, S))
    E = E + E.T
    pi = rng.dirichlet(np.ones(S) * 5)
    Q = phylo.reversible_generator(E, pi)
    V, Vinv, lam = phylo.reversible_eigen(Q, pi)
    return phylo.Model("rand", S, Q, pi, V, Vinv, lam)


def _fractional_weights(n, seed):
    """k / 8 with k in 0..56 (exact in binary), about 10 % exact zeros, the last pattern 7
    (test_gpu_weights._fractional_weights)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 57, size=n) / 8.0
    w[rng.random(n) < 0.1] = 0.0
    w[-1] = 7.0
    return w


def _model(S):
    return {4: (phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25), phylo.DNA), 20: (phylo.lg08(), phylo.PROTEIN),
            64: (phylo.yn98(2.0, 0.3), phylo.CODON)}[S]


# ---------------------------------------------------------------- A. lnL under rescaling

@functools.lru_cache(maxsize=None)
def _case_a(name):
    S, C, taxa, n, lo, hi, amb = {"A1": (4, 2, 600, 100, 0.5, 1.5, 0.05), "A2": (20, 1, 120, 100, 0.1, 0.5, 0.05),
                                  "A3": (64, 1, 150, 64, 0.1, 0.5, 0.0)}[name]
    et = phylo.engine_tree(_caterpillar(taxa, seed=3, lo=lo, hi=hi))
    m, alph = _model(S)
    return Case(et, [m], None, alph, C, n, seed=5, amb=amb)


@pytest.mark.parametrize("name,mode", [("A1", "lnl_only"), ("A1", "materialize"), ("A1", "levelwise"), ("A1", "subtree"),
                                       ("A2", "lnl_only"), ("A2", "levelwise"), ("A3", "lnl_only"), ("A3", "levelwise")])
def test_lnl_under_rescaling(name, mode):
    case = _case_a(name)
    eng = engine_for(case.et, case.S, case.C, case.n, case.states, case.alph.init_table, case.rates, case.probs,
                     case.pi, case.models, flags=GUARD | SC | FLAGS[mode])
    lnl, site, _ = run_engine(eng, case.et)
    assert eng.kernel_path() == _expected_path(case.S, case.C, mode), eng.kernel_path()
    P = engine_pmats(eng, case.et)
    if case._ref is None or not np.array_equal(P, case._ref[0]):
        case._ref = (P, xref.updown(case.et, case.states, case.alph.init_table, P, None, None, case.probs, case.pi))
    x = case._ref[1]
    assert x.l.min() > 1e-400
    # A1: the likelihood itself underflows a double; A2, A3: the partials went through rescaling
    assert site.min() < (-745 if name == "A1" else RESCALED), site.min()
    _check_lnl(f"A {name} {mode}", site, lnl, x)


# ---------------------------------------------------------------- B, C. branch derivatives

@functools.lru_cache(maxsize=None)
def _case_bc1(scaling):
    rng = np.random.default_rng(311)
    lo, hi = (0.3, 1.0) if scaling else (0.02, 0.3)
    et = phylo.engine_tree(_random_topology(20, rng, lo, hi), unroot=False)
    return Case(et, _gtrs(rng, 3), rng.integers(0, 3, et.n_nodes), phylo.DNA, 4, 300, seed=12, amb=0.10)


@pytest.mark.parametrize("mode", ["lnl_only", "materialize", "levelwise"])
@pytest.mark.parametrize("scaling", [False, True])
def test_bc1_per_branch_models(scaling, mode):
    """Three GTR models over the branches of a rooted random topology: deriv_kernel<4,4> and the
    fused preorder dr_pre_s4_kernel<4> (flat) and <4,true> (PLK_FLAG_SCALING)."""
    _run_bc(f"BC1 {'scaled' if scaling else 'flat'} {mode}", _case_bc1(scaling), mode, scaling)


@pytest.mark.parametrize("S,mode", [(20, "lnl_only"), (64, "materialize")])
def test_bc2_per_branch_models_20_64(S, mode):
    """Two models over the branches for 20 states (two random reversible models) and 64 states
    (two YN98 with different kappa and omega): levelwise substitution for the path, the
    levelwise preorder for all branches."""
    rng = np.random.default_rng(320 + S)
    et = phylo.engine_tree(_random_topology(10, rng, 0.02, 0.3), unroot=False)
    if S == 20:
        models, alph, C, n = [_rand_model(rng, 20), _rand_model(rng, 20)], phylo.PROTEIN, 2, 150
    else:
        models, alph, C, n = [phylo.yn98(2.0, 0.3), phylo.yn98(3.5, 0.8)], phylo.CODON, 1, 100
    mon = rng.integers(0, 2, et.n_nodes)
    mon[:2] = (0, 1)   # both models in use
    _run_bc(f"BC2 S={S}", Case(et, models, mon, alph, C, n, seed=13), mode, False)


@pytest.mark.parametrize("C,mode,scaling", [(3, "lnl_only", False), (8, "materialize", True)])
def test_bc3_class_counts_off_the_fused_kernels(C, mode, scaling):
    """3 and 8 classes: dr_branch_kernel for all branches, the levelwise substitution and
    deriv_reduce_kernel for the path."""
    et, m, alph, rates, probs, states = _random_problem(4, C, 12, 200, seed=330 + C, amb=True)
    case = Case(et, [m], None, alph, C, 200, seed=14, amb=0.10)
    _run_bc(f"BC3 C={C}", case, mode, scaling)


@functools.lru_cache(maxsize=None)
def _case_deep(S):
    C, taxa, n = {4: (4, 300, 200), 20: (1, 120, 100), 64: (1, 150, 64)}[S]
    et = phylo.engine_tree(_caterpillar(taxa, seed=3, lo=0.1, hi=0.5))
    m, alph = _model(S)
    return Case(et, [m], None, alph, C, n, seed=4, alpha=0.6)


@pytest.mark.parametrize("S,mode", [(4, "lnl_only"), (4, "levelwise"), (20, "lnl_only"), (64, "lnl_only")])
def test_bc4_6_rescaling_that_fires(S, mode):
    """Deep caterpillars, the smallest per-pattern lnL below -256 ln 2: the stored upper vectors
    and, for 20 and 64 states, the dP / d2P-substituted path vectors (mixed sign) go through the
    levelwise kernels' rescaling."""
    _run_bc(f"BC{ {4: 4, 20: 5, 64: 6}[S]} {mode}", _case_deep(S), mode, True, rescaled=True)


@functools.lru_cache(maxsize=None)
def _case_very_deep(S, C):
    taxa, n, lo, hi = {4: (600, 100, 0.5, 1.5), 20: (400, 64, 0.3, 1.0), 64: (300, 64, 0.5, 1.5)}[S]
    et = phylo.engine_tree(_caterpillar(taxa, seed=3, lo=lo, hi=hi))
    m, alph = _model(S)
    return Case(et, [m], None, alph, C, n, seed=5)


@pytest.mark.parametrize("S,C", [(4, 3), (4, 8), (20, 1), (64, 1)])
def test_bc10_path_vectors_of_one_sign(S, C):
    """Per-pattern lnL below -1022 ln 2 on a caterpillar, the path derivatives of its deepest
    branches through the levelwise substitution (partials_generic_kernel, partials_s4_kernel<8>,
    partials_sgpr_kernel<20>, partials_mfma64_kernel).  Carried up a long path a dP- or
    d2P-substituted vector tends to (pi . v) 1: every entry of one sign, for about half the
    patterns the negative one.  Rescaled by its largest value such a vector was never rescaled
    again and left the double range before the root: d1 and d2 of the deepest branches came out
    finite and wrong in the first digit (misses of 0.7 to 1.6 in the _close metric at these
    shapes), all shallower branches right.  The substitution ops now rescale by the largest
    magnitude (kOpSigned).  The shallower cases BC3 to BC6 cannot show it: below about 700
    in -lnL the unrescaled vector is still a normal double and the scale counts account for it."""
    case = _case_very_deep(S, C)
    eng, site, lnl = case.engine("lnl_only", SC | DR)
    assert site.min() < -1022 * np.log(2), site.min()
    _, x = case.reference(eng)
    assert x.l.min() > 1e-4000
    _check_lnl(f"BC10 S={S} C={C}", site, lnl, x)
    _check_derivatives(f"BC10 S={S} C={C}", case, eng, site, x)


@pytest.mark.parametrize("S,C,mode", [(4, 4, "lnl_only"), (20, 2, "levelwise")])
def test_bc7_zero_and_saturated_branches(S, C, mode):
    """t = 0 (P forced to the identity, dP and d2P from the eigen sum: r Q and r^2 Q^2) on two
    internal branches and on one tip of each of two cherries, t = 60 on two internal branches."""
    et, m, alph, rates, probs, _ = _random_problem(S, C, 16, 300, seed=370 + S)
    case = Case(et, [m], None, alph, C, 300, seed=15)   # data simulated on the positive lengths
    rng = np.random.default_rng(S)
    internal = rng.permutation([v for v in range(et.n_tips, et.n_nodes) if v != et.root])
    cherries = [kids for _, kids in et.ops if all(k < et.n_tips for k in kids)]
    zero = [int(internal[0]), int(internal[1]), int(cherries[0][0]), int(cherries[1][0])]
    long_ = [int(internal[2]), int(internal[3])]
    et.brlen[zero] = 0.0
    et.brlen[long_] = 60.0
    eng = _run_bc(f"BC7 S={S}", case, mode, False)
    qmax = max(1.0, float(np.abs(m.Q).max()))
    for b in zero:
        assert np.array_equal(eng.get_pmatrix(b), np.broadcast_to(np.eye(S), (C, S, S)))
        for c, r in enumerate(case.rates):
            assert np.max(np.abs(eng.get_dpmatrix(b, 1)[c] - r * m.Q)) <= 1e-13 * qmax, (b, c)


def test_bc8_polytomy_fractional_weights():
    """The five-son polytomy under weights k / 8 with exact zeros (the levelwise preorder and
    dr_branch_kernel; deriv_kernel<4,4> for the path): the weights go straight to the reference."""
    et = phylo.engine_tree(phylo.Tree.from_newick(POLY))
    assert any(len(ch) == 5 for _, ch in et.ops)
    case = Case(et, [_model(4)[0]], None, phylo.DNA, 4, 300, seed=9, weights=_fractional_weights(300, 8))
    assert (case.w == 0).any() and case.w[-1] == 7.0
    _run_bc("BC8", case, "materialize", False)


def test_bc9_subtree_pattern_handle():
    """Path derivatives of every branch of a per-subtree-compressed handle (no DR: the flags
    exclude each other): the compressed slots are expanded once, then deriv_kernel<4,4>."""
    et, m, alph, rates, probs, _ = _random_problem(4, 4, 24, 500, seed=390)
    _run_bc("BC9", Case(et, [m], None, alph, 4, 500, seed=16), "subtree", False, dr=False)


# ---------------------------------------------------------------- D. root pair derivatives

def _check_root_pair(group, case, mode, scaling, pairs, rescaled=False):
    eng, site, lnl = case.engine(mode, SC if scaling else 0)
    mats = case.matrices(eng)
    args = (case.et, case.states, case.alph.init_table, *mats, case.probs, case.pi)
    if rescaled:
        assert site.min() < RESCALED, site.min()
    tol, worst = _tol(site), 0.0
    for a, b in pairs:
        terms = xref.root_pair_terms(*args, a, b)
        assert terms[0].min() > 1e-400
        logl = np.log(terms[0]).astype(np.float64)
        assert np.allclose(site, logl, rtol=REL, atol=0)
        for alpha, beta in PAIRS:
            d1, d2 = eng.root_pair_derivatives(int(a), int(b), alpha, beta)
            r1, r2 = xref.root_pair(*args, a, b, alpha, beta, weights=case.w, terms=terms)
            e1, e2 = _close_err(d1, r1), _close_err(d2, r2)
            worst = max(worst, e1, e2)
            assert e1 <= tol and e2 <= tol, (a, b, alpha, beta, d1, float(r1), e1, d2, float(r2), e2)
            if beta == 0.0:   # one branch only: the ordinary branch derivative
                p1, p2 = eng.branch_derivatives(int(a))
                assert _close_err(d1, p1) <= 1e-10 and _close_err(d2, p2) <= 1e-10, (a, d1, p1, d2, p2)
    print(f"xref {group} D (root pair) worst {worst:.3g}, smallest per-pattern lnL {site.min():.1f}")


def _case_d1(weights=None):
    """A rooted 12-taxon tree, three GTR models over the branches, the two root sons on
    different ones."""
    rng = np.random.default_rng(74)
    et = phylo.engine_tree(phylo.balanced_tree(12, seed=74, lo=0.01, hi=0.3), unroot=False)
    mon = rng.integers(0, 3, et.n_nodes)
    kids = [c for p, ch in et.ops if p == et.root for c in ch]
    assert len(kids) == 2
    mon[kids[0]], mon[kids[1]] = 0, 2
    return Case(et, _gtrs(rng, 3), mon, phylo.DNA, 4, 300, seed=74, weights=weights)


def test_d1_per_branch_models():
    case = _case_d1()
    _check_root_pair("D1", case, "lnl_only", False, [case.kids[:2]])


@pytest.mark.parametrize("newick,unroot", [("((a:0.1,b:0.2):0.15,c:0.3);", False), ("(a:0.1,b:0.2,c:0.3);", True)])
def test_d2_three_taxa(newick, unroot):
    """Three taxa under PLK_FLAG_SCALING: rooted (an interior son and a tip son) and the
    trifurcation (two tip sons: both substituted vectors come from scratch tip rows)."""
    et = phylo.engine_tree(phylo.Tree.from_newick(newick), unroot=unroot)
    case = Case(et, _gtrs(np.random.default_rng(5), 1), None, phylo.DNA, 4, 200, seed=5)
    assert len(case.kids) == (3 if unroot else 2) and sum(k < et.n_tips for k in case.kids[:2]) == (2 if unroot else 1)
    _check_root_pair("D2", case, "materialize", True, [case.kids[:2]])


@pytest.mark.parametrize("S,C,taxa,n,mode,scaling", [(20, 2, 10, 150, "levelwise", True), (64, 1, 8, 130, "lnl_only", False)])
def test_d3_d4_20_and_64_states(S, C, taxa, n, mode, scaling):
    et, m, alph, rates, probs, _ = _random_problem(S, C, taxa, n, seed=430 + S)
    case = Case(et, [m], None, alph, C, n, seed=17)
    _check_root_pair(f"D{3 if S == 20 else 4}", case, mode, scaling, [case.kids[:2]])


def test_d5_accumulate_chunks():
    """A root of five sons is formed by two ops (three sons, then two with PLK_OP_ACCUMULATE):
    the pair in different chunks (first and fifth son, a tip), then both in the first."""
    et = phylo.engine_tree(phylo.Tree.from_newick(ROOT5))
    case = Case(et, [_model(4)[0]], None, phylo.DNA, 4, 300, seed=9)
    k = case.kids
    assert len(k) == 5 and k[4] < et.n_tips
    _check_root_pair("D5", case, "materialize", False, [(k[0], k[4]), (k[0], k[1])])


def _cat(prefix, n, rng, lo, hi):
    s = "%s0:%.4f" % (prefix, rng.uniform(lo, hi))
    for i in range(1, n):
        s = "(%s,%s%d:%.4f):%.4f" % (s, prefix, i, rng.uniform(lo, hi), rng.uniform(lo, hi))
    return s


def test_d6_deep_rescaling():
    """Two 150-tip long caterpillars joined at the root: the root slot and each of the five
    scratch products carry scale counts of their own (k0 - kx[v] in pair_reduce_kernel)."""
    rng = np.random.default_rng(46)
    tree = phylo.Tree.from_newick("(%s,%s);" % (_cat("u", 150, rng, 0.5, 1.5), _cat("v", 150, rng, 0.5, 1.5)))
    et = phylo.engine_tree(tree, unroot=False)
    case = Case(et, [_model(4)[0]], None, phylo.DNA, 2, 100, seed=18)
    assert len(case.kids) == 2 and et.n_tips == 300
    _check_root_pair("D6", case, "lnl_only", True, [case.kids], rescaled=True)


def test_d7_weights():
    case = _case_d1(weights=_fractional_weights(300, 8))
    _check_root_pair("D7", case, "lnl_only", False, [case.kids[:2]])
