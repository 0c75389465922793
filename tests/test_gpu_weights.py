"""Pattern weights (plk_set_pattern_weights: the reference's rootWeights_, the count of each
site pattern after compression) in every lnL and derivative reduction, and inputs changed on
a handle that has already evaluated.

The reference needs no weights of its own: a pattern of integer weight w is that column
w times (DRASRTreeLikelihoodData.cpp:218-332), so the weighted engine run on `states` with
weights `w` is checked against the unweighted oracle on np.repeat(states, w, axis=1) --
lnL by oracle.tree_loglik, every branch's d1 / d2 by oracle.dr_derivatives, the root-pair
derivatives by central differences of the expanded lnL.

Every lnL case first asserts, from the oracle alone, that the wrong weight vectors a kernel
could plausibly read (all ones, shifted by one pattern or one wave, reversed, their mean, the
last pattern dropped) move the weighted lnL by more than 1e-6 |lnL| (tolerance: 1e-12), so no
case can pass with such a kernel; the derivative cases assert the counterpart on d2.

Tolerances: per-pattern lnL and weighted lnL relative 1e-12 (REL: every site lnL is
negative, so 1e-12 per pattern bounds the weighted sum by the same); a block sum against
math.fsum of w * site within 80 * 2^-53 of the sum of magnitudes (one multiply, six butterfly
adds, a chain of 4096 / 64 = 64 adds: 71 roundings); derivatives relative 1e-10 as
test_gpu_dr.test_dr_vs_oracle_restatement.

Reduction reached by each case (asserted through kernel_path / table_nodes where the
library reports it):
  cls-*            jit_tree4, quad units  -> cls_blocks_kernel<1|2|4> (both launches: with and
                                            without the per-pattern lnL)
  gen4-*           jit_tree4, no quads    -> the generated 4-state kernel's own root fragment
                                            (classes in one workgroup; in one wave with rescaling)
  tree4-*          tree4                  -> tree4_kernel
  mat4 / sub4-*    jit_tree4 / subtree_patterns, then root_kernel on the stored root partial
  lev4-* / gen-c*  levelwise              -> root_kernel
  jitm-*           jit_treeM              -> the generated 20-state kernel
  treeM20          treeM (20 states)      -> treeM_kernel + site_wave_sums_kernel
  treeM64-*        treeM (64 states)      -> treeM_kernel's own 64-pattern wave sums
"""
import math

import numpy as np
import pytest

import oracle
import phylo
import plk
import workload
from conftest import set_tune
from test_gpu_parity import (MODES, _caterpillar, _random_problem, _random_topology, check, engine_for, engine_pmats,
                             oracle_for, run_engine)

pytestmark = pytest.mark.gpu
REL = 1e-12
DR = plk.PLK_FLAG_DOUBLE_RECURSIVE
SUB = plk.PLK_FLAG_SUBTREE_PATTERNS
FLAGS = dict(MODES, subtree=SUB)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


# ---------------------------------------------------------------- helpers

def _weights(n, seed):
    """Integer weights 1..7; the last pattern 7, and around the first wave boundary 1 | 6, so
    that neither the edge of a wave nor the ragged tail is neutral."""
    w = np.random.default_rng(seed).integers(1, 8, size=n).astype(np.float64)
    w[-1] = 7.0
    if n > 64:
        w[63], w[64] = 1.0, 6.0
    return w


def _fractional_weights(n, seed):
    """k / 8 with k in 0..56 (exact in binary), about 10 % exact zeros, the last pattern 7."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 57, size=n) / 8.0
    w[rng.random(n) < 0.1] = 0.0
    w[-1] = 7.0
    return w


def _expanded(states, w):
    return np.repeat(states, w.astype(int), axis=1)


def _assert_weights_matter(w, so):
    """The can-fail precondition, from the oracle's per-pattern lnL alone."""
    L = math.fsum(w * so)
    wrong = {"ones": np.ones_like(w), "roll1": np.roll(w, 1), "roll64": np.roll(w, 64), "reversed": w[::-1],
             "mean": np.full_like(w, w.mean()), "last0": np.concatenate([w[:-1], [0.0]])}
    for name, v in wrong.items():
        assert abs(math.fsum(v * so) - L) > 1e-6 * abs(L), (name, math.fsum(v * so), L)


def _tune(monkeypatch, tune):
    for kv in tune.split():
        k, v = kv.split("=")
        set_tune(monkeypatch, k, v)


class Problem:
    """A seeded problem on a tree shape the suite already compiles kernels for."""

    def __init__(self, S, C, tree_kind, n, data="", scaling=False):
        seed = {4: 23, 20: 31, 64: 29}[S]
        if tree_kind.startswith("balanced"):
            tree = phylo.balanced_tree(int(tree_kind[8:]), seed=seed, lo=0.05, hi=0.4)
        elif tree_kind.startswith("caterpillar"):
            tree = _caterpillar(int(tree_kind[11:]), seed=5)
        else:  # "polyN": random joins with polytomies
            tree = _random_topology(int(tree_kind[4:]), np.random.default_rng(seed), 0.05, 0.4, poly=0.5)
        self.et = et = phylo.engine_tree(tree)
        rng = np.random.default_rng(C * 13 + n)
        if S == 4:
            self.m, self.alph = phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5)), phylo.DNA
        elif S == 20:
            self.m, self.alph = phylo.lg08(), phylo.PROTEIN
        else:
            self.m, self.alph = phylo.yn98(2.0, 0.3), phylo.CODON
        self.S, self.C, self.n, self.scaling = S, C, n, scaling
        self.rates, self.probs = phylo.gamma_rates(C, 0.5) if C > 1 else (np.ones(1), np.ones(1))
        self.pi = self.m.pi
        wl = workload.Workload("m", et, [self.m], None, self.rates, self.probs, self.pi, self.alph, n, scaling, True, 5)
        self.states = wl.simulate(0, n).astype(np.int32)
        if data == "amb":
            mask = rng.random(self.states.shape) < 0.05
            self.states[mask] = rng.integers(S, self.alph.n_codes, size=mask.sum())
        self.br = np.array([v for v in range(et.n_nodes) if v != et.root], dtype=np.int32)
        self.ops = phylo.split_ops(et.ops)

    @classmethod
    def of(cls, et, m, alph, rates, probs, states, scaling=False):
        """The same record around a problem of test_gpu_parity._random_problem."""
        p = cls.__new__(cls)
        p.et, p.m, p.alph, p.rates, p.probs, p.states, p.pi = et, m, alph, rates, probs, states, m.pi
        p.S, p.C, p.n, p.scaling = m.S, len(rates), states.shape[1], scaling
        p.br = np.array([v for v in range(et.n_nodes) if v != et.root], dtype=np.int32)
        p.ops = phylo.split_ops(et.ops)
        return p

    def engine(self, flags, w=None, device=0, deriv=False):
        if device == 0:
            eng = engine_for(self.et, self.S, self.C, self.n, self.states, self.alph.init_table, self.rates, self.probs,
                             self.pi, [self.m], flags=flags | (plk.PLK_FLAG_SCALING if self.scaling else 0))
        else:   # a list of devices: one handle sharding the patterns (engine_for takes device 0)
            et = self.et
            eng = plk.Engine(device, self.S, self.C, self.n, et.n_tips, et.n_internal, 1, flags)
            eng.set_code_table(self.alph.init_table)
            for i in range(et.n_tips):
                eng.set_tip_codes(i, self.states[i].astype(np.uint8))
            eng.set_category_rates(self.rates, self.probs)
            eng.set_root_frequencies(self.pi)
            eng.set_eigen(0, self.m.V, self.m.Vinv, self.m.lam)
            eng.update_pmatrices(self.br, et.brlen[self.br])
        if deriv:
            eng.update_pmatrices(self.br, self.et.brlen[self.br], deriv_mask=7)
        if w is not None:
            eng.set_pattern_weights(w)
        return eng

    def oracle(self, eng, states=None, probs=None, pi=None):
        """Oracle (lnL, per-pattern lnL) on the engine's own P(t)."""
        return oracle_for(self.et, self.states if states is None else states, self.alph.init_table, self.rates,
                          self.probs if probs is None else probs, self.pi if pi is None else pi, [self.m],
                          scaling=self.scaling, pmats=engine_pmats(eng, self.et))


def _check_blocks(lnl, blocks, site, w):
    """lnl is the left-to-right sum of the block sums, bitwise; every block sum is the weighted
    sum of its patterns' lnL within 71 (<= 80) roundings of the magnitudes."""
    BLOCK = plk.load().plk_block_size()
    s = 0.0
    for v in blocks:
        s += v
    assert s == lnl
    assert len(blocks) == (len(w) + BLOCK - 1) // BLOCK
    for b in range(len(blocks)):
        t = w[b * BLOCK:(b + 1) * BLOCK] * site[b * BLOCK:(b + 1) * BLOCK]
        err, bound = abs(blocks[b] - math.fsum(t)), 80 * 2.0 ** -53 * math.fsum(np.abs(t))
        assert err <= bound, (b, blocks[b], math.fsum(t), err, bound)


def _check_weighted(p, eng, res, w, **kw):
    """Section 1's assertions on an engine result (lnl, site, blocks) under integer weights w."""
    lnl, site, blocks = res
    _, so = p.oracle(eng, **kw)
    _assert_weights_matter(w, so)
    L_exp, _ = p.oracle(eng, states=_expanded(p.states, w), **kw)
    check(lnl, site, L_exp, so)    # per-pattern lnL unweighted, the total weighted
    _check_blocks(lnl, blocks, site, w)


# ---------------------------------------------------------------- 1. weighted lnL on every root-reduction path

LNL_CASES = [
    # id, S, C, tree, n, mode, scaling, data, tune, guard, kernel_path, quads
    # one class per workgroup with quad units, direct codes, two patterns per lane (the default)
    ("cls-c4-2blocks", 4, 4, "balanced64", 4096 + 130, "lnl_only", False, "", "", True, "jit_tree4", True),
    ("cls-c4-n7", 4, 4, "balanced64", 7, "lnl_only", False, "", "", True, "jit_tree4", True),
    ("cls-c2-n129", 4, 2, "balanced64", 129, "lnl_only", False, "", "", True, "jit_tree4", True),
    ("cls-c1-n130", 4, 1, "balanced64", 130, "lnl_only", False, "", "", True, "jit_tree4", True),
    ("cls-pw1", 4, 4, "balanced64", 700, "lnl_only", False, "", "JIT_PW=1", True, "jit_tree4", True),
    ("cls-dc0", 4, 4, "balanced64", 700, "lnl_only", False, "", "JIT_DC=0", True, "jit_tree4", True),
    ("cls-g3", 4, 4, "balanced64", 700, "lnl_only", False, "", "JIT_G=3", True, "jit_tree4", True),
    ("cls-noguard", 4, 4, "balanced64", 777, "lnl_only", False, "", "", False, "jit_tree4", True),
    # the generated kernel's own root fragment
    ("gen4-noquads", 4, 4, "balanced64", 4096 + 130, "lnl_only", False, "", "JIT_QUAD_KB=0", True, "jit_tree4", False),
    ("gen4-amb", 4, 4, "balanced64", 4096 + 130, "lnl_only", False, "amb", "", True, "jit_tree4", False),
    ("gen4-scaled", 4, 4, "balanced64", 4096 + 130, "lnl_only", True, "", "", True, "jit_tree4", False),
    # the interpreter
    ("tree4", 4, 4, "caterpillar40", 777, "lnl_only", False, "amb", "JIT=0", True, "tree4", False),
    ("tree4-scaled", 4, 4, "caterpillar40", 777, "lnl_only", True, "amb", "JIT=0", True, "tree4", False),
    # root_kernel
    ("mat4", 4, 4, "balanced64", 777, "materialize", False, "amb", "", True, "jit_tree4", False),
    ("lev4", 4, 4, "balanced64", 777, "levelwise", False, "amb", "", True, "levelwise", False),
    ("lev4-noguard", 4, 4, "balanced64", 777, "levelwise", False, "", "", False, "levelwise", False),
    ("gen-c3", 4, 3, "balanced12", 300, "materialize", False, "amb", "", True, "levelwise", False),
    ("gen-c8", 4, 8, "balanced12", 300, "lnl_only", False, "amb", "", True, "levelwise", False),
    ("sub4-poly", 4, 4, "poly40", 700, "subtree", False, "", "", True, "subtree_patterns", False),
    # 20 states
    ("jitm-c4", 20, 4, "balanced64", 333, "lnl_only", False, "amb", "", True, "jit_treeM", False),
    ("jitm-c1-scaled", 20, 1, "balanced64", 333, "lnl_only", True, "", "", True, "jit_treeM", False),
    ("jitm-2blocks", 20, 4, "balanced12", 4096 + 70, "lnl_only", False, "", "", True, "jit_treeM", False),
    ("treeM20", 20, 4, "balanced64", 333, "lnl_only", False, "amb", "JITM=0", True, "treeM", False),
    # 64 states
    ("treeM64", 64, 1, "balanced8", 130, "lnl_only", False, "", "", True, "treeM", False),
    ("treeM64-2blocks", 64, 1, "balanced8", 4096 + 70, "lnl_only", False, "", "", True, "treeM", False),
]


@pytest.mark.parametrize("S,C,tree_kind,n,mode,scaling,data,tune,guard,path,quads",
                         [c[1:] for c in LNL_CASES], ids=[c[0] for c in LNL_CASES])
def test_weighted_lnl_vs_expanded_oracle(S, C, tree_kind, n, mode, scaling, data, tune, guard, path, quads,
                                         monkeypatch):
    """Integer weights on every root-reduction path against the oracle on the alignment with
    pattern p repeated w[p] times: per-pattern lnL (weights must not leak into it), weighted
    lnL, block sums, and the same doubles from a second evaluation with and without the
    per-pattern lnL (one class per workgroup: two different cls_blocks_kernel launches)."""
    _tune(monkeypatch, tune)
    p = Problem(S, C, tree_kind, n, data, scaling)
    if tree_kind.startswith("poly"):
        assert max(len(ch) for _, ch in p.et.ops) > 3
    w = _weights(n, seed=n + C)
    eng = p.engine((plk.PLK_FLAG_NONNEG_GUARD if guard else 0) | FLAGS[mode], w)
    res = run_engine(eng, p.et)
    assert eng.kernel_path() == path
    if quads:
        assert eng.traversal_work()["table_nodes"] > 0
    _check_weighted(p, eng, res, w)
    l2, _, b2 = run_engine(eng, p.et, sites=False)
    l3, s3, b3 = run_engine(eng, p.et)
    assert l2 == res[0] and np.array_equal(b2, res[2])
    assert l3 == res[0] and np.array_equal(s3, res[1]) and np.array_equal(b3, res[2])
    if mode in ("materialize", "subtree") and path != "levelwise":
        # the stored root partial through root_kernel (the same weights set again drop the
        # traversal's own root reduction)
        eng.set_pattern_weights(w)
        r4 = eng.root_loglik(p.et.root, want_sites=True, want_blocks=True)
        _check_weighted(p, eng, r4, w)


def test_quads_replace_table_nodes(monkeypatch):
    """The cls-* cases above do run with quad units: more table nodes than the same problem
    without (as test_jit_tree4_quads_bitwise), so they are no copy of gen4-noquads."""
    p = Problem(4, 4, "balanced64", 700)
    tn = []
    for kb in (None, "0"):
        if kb is not None:
            set_tune(monkeypatch, "JIT_QUAD_KB", kb)
        eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | plk.PLK_FLAG_LNL_ONLY, _weights(700, 1))
        run_engine(eng, p.et)
        tn.append(eng.traversal_work()["table_nodes"])
        eng.close()
    assert tn[0] > tn[1] > 0


# ---------------------------------------------------------------- 2. fractional and zero weights

@pytest.mark.parametrize("S,tree_kind,n,mode,tune,path", [
    (4, "balanced64", 4096 + 130, "lnl_only", "", "jit_tree4"),
    (4, "balanced64", 4096 + 130, "lnl_only", "JIT_QUAD_KB=0", "jit_tree4"),
    (4, "balanced64", 4096 + 130, "levelwise", "", "levelwise"),
    (20, "balanced64", 333, "lnl_only", "", "jit_treeM")], ids=["cls", "gen4", "root_kernel", "jitm"])
def test_fractional_and_zero_weights(S, tree_kind, n, mode, tune, path, monkeypatch):
    """Weights k / 8 with exact zeros (a zero weight on a finite site lnL: plain data, every
    site likelihood positive) and 7.0 on the last pattern of the ragged tail: the block sums
    within the rounding bound of the weighted per-pattern lnL, the lnL against math.fsum of
    w * oracle site lnL at 1e-12."""
    _tune(monkeypatch, tune)
    p = Problem(S, 4, tree_kind, n)
    w = _fractional_weights(n, seed=n + S)
    assert 0.05 * n < np.count_nonzero(w == 0.0) < 0.2 * n and w[-1] == 7.0
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | FLAGS[mode], w)
    lnl, site, blocks = run_engine(eng, p.et)
    assert eng.kernel_path() == path
    _, so = p.oracle(eng)
    assert np.all(np.isfinite(so))
    _assert_weights_matter(w, so)
    L = math.fsum(w * so)
    check(lnl, site, L, so)
    _check_blocks(lnl, blocks, site, w)


# ---------------------------------------------------------------- 3. the re-launch branches

def test_cls_relaunch_after_evaluate():
    """plk_evaluate on the one-class-per-workgroup path forms the block sums without the
    per-pattern lnL; plk_root_loglik with want_sites then launches cls_blocks_kernel again:
    the same lnL and block sums bitwise, the per-pattern lnL the oracle's."""
    n = 4096 + 130
    p = Problem(4, 4, "balanced64", n)
    w = _weights(n, seed=n + 4)
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | plk.PLK_FLAG_LNL_ONLY, w)
    lnl, blocks = eng.evaluate(p.br, p.et.brlen[p.br], p.ops, p.et.root)
    assert eng.kernel_path() == "jit_tree4" and eng.traversal_work()["table_nodes"] > 0
    res = eng.root_loglik(p.et.root, want_sites=True, want_blocks=True)
    assert res[0] == lnl and np.array_equal(res[2], blocks)
    _check_weighted(p, eng, res, w)


def test_multi_device_handle_weighted_vs_oracle():
    """A two-shard handle (weights sliced per shard at a block boundary) against the
    expanded oracle, not only against a one-device handle."""
    n = 4096 + 130
    p = Problem(4, 4, "balanced64", n)
    w = _weights(n, seed=n + 4)
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | plk.PLK_FLAG_LNL_ONLY, w, device=[0, 0])
    assert eng.shard_count() == 2
    res = run_engine(eng, p.et)
    assert eng.kernel_path() == "jit_tree4"
    _check_weighted(p, eng, res, w)


# ---------------------------------------------------------------- 4. weighted derivatives

def _close(a, b, rel):
    return abs(a - b) <= rel * max(1.0, abs(a), abs(b))


def _oracle_derivatives(p, states):
    """oracle.dr_derivatives as in test_gpu_dr.test_dr_vs_oracle_restatement: P, r Q P, r^2 Q^2 P
    from the oracle's own expm."""
    et, m = p.et, p.m
    P = np.zeros((et.n_nodes, p.C, p.S, p.S))
    dP, d2P = np.zeros_like(P), np.zeros_like(P)
    for v in p.br:
        for c, r in enumerate(p.rates):
            e = oracle.reversible_pij(m.Q, m.pi, et.brlen[v] * r)
            P[v, c], dP[v, c], d2P[v, c] = e, r * m.Q @ e, r ** 2 * m.Q @ m.Q @ e
    ss, sons, lr = et.son_arrays()
    return oracle.dr_derivatives(ss, sons, lr, et.root, states, p.alph.init_table, P, dP, d2P, p.probs, p.pi)


def _weighted_oracle_derivatives(p, w):
    """(d1, d2) per branch of the expanded alignment; asserts that they cannot be had from
    the compressed alignment with a constant weight (the can-fail precondition)."""
    o1, o2 = _oracle_derivatives(p, _expanded(p.states, w))
    _, c2 = _oracle_derivatives(p, p.states)
    assert any(abs(o2[b] - w.mean() * c2[b]) > 1e-6 * max(1.0, abs(o2[b])) for b in p.br)
    return o1, o2


DERIV_SHAPES = {"s4c4": (4, 4, 12, 400), "s4c1": (4, 1, 12, 400), "s4c3": (4, 3, 12, 300), "s4c8": (4, 8, 12, 300),
                "s20c2": (20, 2, 8, 150), "s64c1": (64, 1, 6, 130)}


def _deriv_problem(shape, scaling=False):
    S, C, n_taxa, n = DERIV_SHAPES[shape]
    return Problem.of(*_random_problem(S, C, n_taxa, n, seed=100 + S + C), scaling=scaling), _weights(n, seed=n + S)


@pytest.mark.parametrize("mode", ["lnl_only", "materialize"])
@pytest.mark.parametrize("shape", ["s4c4", "s4c1", "s4c3", "s20c2", "s64c1"])
def test_weighted_path_derivatives(shape, mode):
    """plk_branch_derivatives of every branch under weights (deriv_kernel for 4 states with
    1 / 4 classes, deriv_reduce_kernel otherwise) against the oracle's derivatives of the
    expanded alignment."""
    p, w = _deriv_problem(shape)
    o1, o2 = _weighted_oracle_derivatives(p, w)
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | MODES[mode], w, deriv=True)
    run_engine(eng, p.et)
    for b in p.br:
        d1, d2 = eng.branch_derivatives(int(b))
        assert _close(d1, o1[b], 1e-10), (b, d1, o1[b])
        assert _close(d2, o2[b], 1e-10), (b, d2, o2[b])


@pytest.mark.parametrize("shape,mode,scaling", [
    ("s4c4", "lnl_only", False), ("s4c4", "lnl_only", True), ("s4c1", "lnl_only", False),   # dr_pre_s4_kernel
    ("s20c2", "lnl_only", False),                                                           # dr_pre_m20_kernel
    ("s64c1", "lnl_only", False),                                      # levelwise preorder, dr_branch_mfma_kernel
    ("s4c4", "levelwise", False),                            # dr_pre_s4_kernel on levelwise partials
    ("s4c8", "materialize", False), ("s4c3", "lnl_only", False)])    # 3 / 8 classes: dr_branch_kernel
def test_weighted_double_recursive_derivatives(shape, mode, scaling):
    """plk_all_branch_derivatives under weights against the oracle's derivatives of the
    expanded alignment (flat, unscaled: these small trees do not underflow, so the rescaling
    variant of the kernels computes the same numbers)."""
    p, w = _deriv_problem(shape, scaling)
    o1, o2 = _weighted_oracle_derivatives(p, w)
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | MODES[mode] | DR, w, deriv=True)
    run_engine(eng, p.et)
    d1, d2 = eng.all_branch_derivatives()
    for b in p.br:
        assert _close(d1[b], o1[b], 1e-10), (b, d1[b], o1[b])
        assert _close(d2[b], o2[b], 1e-10), (b, d2[b], o2[b])


def test_weighted_double_recursive_polytomy():
    """A father of five sons takes 4 states and 4 classes off the fused preorder: the
    levelwise preorder and dr_branch_kernel, under weights."""
    t = phylo.Tree.from_newick("((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2);")
    et = phylo.engine_tree(t)
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(4, 0.5)
    n = 300
    wl = workload.Workload("p", et, [m], None, rates, probs, m.pi, phylo.DNA, n, False, True, 9)
    p = Problem.of(et, m, phylo.DNA, rates, probs, wl.simulate(0, n).astype(np.int32))
    w = _weights(n, seed=n)
    o1, o2 = _weighted_oracle_derivatives(p, w)
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | DR, w, deriv=True)
    run_engine(eng, p.et)
    d1, d2 = eng.all_branch_derivatives()
    for b in p.br:
        assert _close(d1[b], o1[b], 1e-10) and _close(d2[b], o2[b], 1e-10), (b, d1[b], o1[b], d2[b], o2[b])


@pytest.mark.parametrize("S,C,n_taxa,mode", [(4, 4, 12, "lnl_only"), (20, 2, 10, "materialize")])
def test_weighted_root_pair_derivatives(S, C, n_taxa, mode):
    """plk_root_pair_derivatives (pair_reduce_kernel) under weights, on a rooted tree for 4
    states, against central differences of the oracle's lnL of the expanded alignment: steps
    and tolerances of test_root_pair_derivatives_vs_oracle_finite_differences."""
    n = 300
    if S == 4:   # rooted: the two sons of the root are the whole pair
        tree = phylo.balanced_tree(n_taxa, seed=74, lo=0.01, hi=0.3)
        et = phylo.engine_tree(tree, unroot=False)
        rng = np.random.default_rng(74)
        m = phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5))
        rates, probs = phylo.gamma_rates(C, 0.5)
        wl = workload.Workload("r", et, [m], None, rates, probs, m.pi, phylo.DNA, n, False, True, 74)
        p = Problem.of(et, m, phylo.DNA, rates, probs, wl.simulate(0, n).astype(np.int32))
    else:
        p = Problem.of(*_random_problem(S, C, n_taxa, n, seed=70 + S + C + n_taxa))
    et = p.et
    kids = [c for q, ch in et.ops if q == et.root for c in ch]
    assert S != 4 or len(kids) == 2
    a, b = kids[0], kids[1]
    w = _weights(n, seed=n + S)
    big = _expanded(p.states, w)
    eng = p.engine(plk.PLK_FLAG_NONNEG_GUARD | MODES[mode], w, deriv=True)
    run_engine(eng, et)
    checked_mean = False
    for alpha, beta in ((0.3, 0.7), (0.25, -0.25), (1.0, 0.0)):
        d1, d2 = eng.root_pair_derivatives(int(a), int(b), alpha, beta)

        def lnl_at(s, states=big):
            bl = et.brlen.copy()
            bl[a] += alpha * s
            bl[b] += beta * s
            e2 = phylo.EngineTree(et.n_tips, et.n_internal, et.root, et.tip_names, et.ops, bl, {}, [], [])
            return oracle_for(e2, states, p.alph.init_table, p.rates, p.probs, p.pi, [p.m])[0]

        h, h2 = 1e-5, 1e-4
        fd1 = (lnl_at(h) - lnl_at(-h)) / (2 * h)
        fd2 = (lnl_at(h2) - 2 * lnl_at(0.0) + lnl_at(-h2)) / h2 ** 2
        if not checked_mean:   # can-fail: not the unweighted derivative times the mean weight
            c2 = (lnl_at(h2, p.states) - 2 * lnl_at(0.0, p.states) + lnl_at(-h2, p.states)) / h2 ** 2
            assert abs(fd2 - w.mean() * c2) > 10 * 2e-4 * max(1.0, abs(fd2))
            checked_mean = True
        assert abs(d1 - fd1) <= 1e-6 * max(1.0, abs(fd1)), (alpha, beta, d1, fd1)
        assert abs(d2 - fd2) <= 2e-4 * max(1.0, abs(fd2)), (alpha, beta, d2, fd2)


# ---------------------------------------------------------------- 5. inputs changed after an evaluation

def _changed(p, what, w0):
    """(weights, class probabilities, root frequencies) after the change of `what`."""
    rng = np.random.default_rng(17)
    w, probs, pi = w0, p.probs, p.pi
    if what == "weights":
        w = _weights(p.n, seed=p.n + 99)
    elif what == "probs":   # the rates stay, so every P(t) stays valid
        probs = rng.dirichlet(np.ones(p.C) * 3)
    else:
        pi = rng.dirichlet(np.ones(p.S) * 5)
    return w, probs, pi


def _apply(eng, p, what, w, probs, pi):
    if what == "weights":
        eng.set_pattern_weights(w)
    elif what == "probs":
        eng.set_category_rates(p.rates, probs)
    else:
        eng.set_root_frequencies(pi)


def _fresh(p, flags, w, probs, pi):
    """A handle built with the changed input from the start, and its evaluation."""
    q = Problem.of(p.et, p.m, p.alph, p.rates, probs, p.states, scaling=p.scaling)
    q.pi = pi
    eng = q.engine(flags, w)
    return eng, run_engine(eng, p.et)


@pytest.mark.parametrize("what", ["weights", "probs", "freqs"])
@pytest.mark.parametrize("S,n,mode", [(4, 777, "materialize"), (4, 777, "levelwise"), (4, 777, "subtree"),
                                      (20, 333, "materialize"), (20, 333, "levelwise"), (20, 333, "subtree")])
def test_input_change_with_stored_root(S, n, mode, what):
    """Weights, class probabilities or root frequencies changed after an evaluation on a
    handle that stores the root partial: plk_root_loglik without a new traversal must not
    reuse the traversal's own root reduction -- it returns what a handle built with the new
    input returns, bitwise, and that is the weighted oracle's.

    The call is served by root_kernel on the stored root partial.  The fresh handle B, which
    never saw the old input, is asked the same way (its input set once more, then
    plk_root_loglik): bitwise.  B's first evaluation reduces the root inside the traversal
    kernel where there is one (materialising 4 and 20 states): jit_tree4 keeps root_kernel's
    order of operations, so that too is bitwise for 4 states; the 20-state kernel sums the
    states on the matrix cores in another order, and its per-pattern lnL agrees with
    root_kernel's at the 1e-12 that test_s20_modes_vs_oracle holds both to (observed: last-bit
    differences in the per-pattern lnL, the same lnL)."""
    p = Problem(S, 4, "balanced64" if S == 4 else "balanced12", n, "amb")
    flags = plk.PLK_FLAG_NONNEG_GUARD | FLAGS[mode]
    w0 = _weights(n, seed=n + 4)
    A = p.engine(flags, w0)
    before = run_engine(A, p.et)
    w, probs, pi = _changed(p, what, w0)
    _apply(A, p, what, w, probs, pi)
    after = A.root_loglik(p.et.root, want_sites=True, want_blocks=True)
    B, fresh = _fresh(p, flags, w, probs, pi)
    assert abs(before[0] - fresh[0]) > 1e-6 * abs(fresh[0])   # a stale value would show
    _apply(B, p, what, w, probs, pi)
    same = B.root_loglik(p.et.root, want_sites=True, want_blocks=True)
    assert after[0] == same[0] and np.array_equal(after[1], same[1]) and np.array_equal(after[2], same[2])
    if S == 4 or mode != "materialize":
        assert after[0] == fresh[0] and np.array_equal(after[1], fresh[1]) and np.array_equal(after[2], fresh[2])
    else:
        check(after[0], after[1], fresh[0], fresh[1])
        assert np.allclose(after[2], fresh[2], rtol=REL, atol=0)
    _check_weighted(p, A, after, w, probs=probs, pi=pi)


@pytest.mark.parametrize("what", ["weights", "probs", "freqs"])
@pytest.mark.parametrize("S,tune", [(4, ""), (4, "JIT_QUAD_KB=0"), (20, "")], ids=["cls", "gen4", "jitm"])
def test_input_change_lnl_only(S, tune, what, monkeypatch):
    """The same on lnL-only handles, whose root partial is not stored: plk_root_loglik without
    a new traversal either fails with PLK_ERR_STATE or returns the fresh value, never the one
    from before the change; after plk_update_partials it is a fresh handle's, bitwise.
    (Observed: PLK_ERR_STATE, "root has no partial" -- INTEGRATION.md, call order.)"""
    _tune(monkeypatch, tune)
    n = 777 if S == 4 else 333
    p = Problem(S, 4, "balanced64" if S == 4 else "balanced12", n)
    flags = plk.PLK_FLAG_NONNEG_GUARD | plk.PLK_FLAG_LNL_ONLY
    w0 = _weights(n, seed=n + 4)
    A = p.engine(flags, w0)
    before = run_engine(A, p.et)
    assert A.kernel_path() == ("jit_tree4" if S == 4 else "jit_treeM")
    w, probs, pi = _changed(p, what, w0)
    _apply(A, p, what, w, probs, pi)
    B, fresh = _fresh(p, flags, w, probs, pi)
    assert abs(before[0] - fresh[0]) > 1e-6 * abs(fresh[0])
    try:
        after = A.root_loglik(p.et.root, want_sites=True, want_blocks=True)
    except plk.PlkError as e:
        assert e.code == -5
    else:
        assert after[0] == fresh[0] and np.array_equal(after[1], fresh[1]) and np.array_equal(after[2], fresh[2])
    again = run_engine(A, p.et)
    assert again[0] == fresh[0] and np.array_equal(again[1], fresh[1]) and np.array_equal(again[2], fresh[2])
    _check_weighted(p, A, again, w, probs=probs, pi=pi)


@pytest.mark.parametrize("shape", ["s4c4", "s20c2"])
def test_derivatives_after_weight_change(shape):
    """New weights after an evaluation: path and double-recursive derivatives are those of a
    handle that had the new weights from the start."""
    p, w0 = _deriv_problem(shape)
    w = _weights(p.n, seed=p.n + 99)
    flags = plk.PLK_FLAG_NONNEG_GUARD | DR
    A = p.engine(flags, w0, deriv=True)
    run_engine(A, p.et)
    a_old = A.all_branch_derivatives()
    A.set_pattern_weights(w)
    B = p.engine(flags, w, deriv=True)
    run_engine(B, p.et)
    b1, b2 = B.all_branch_derivatives()
    assert any(not _close(a_old[1][b], b2[b], 1e-6) for b in p.br)   # a stale value would show
    a1, a2 = A.all_branch_derivatives()
    for b in p.br:
        assert _close(a1[b], b1[b], 1e-12) and _close(a2[b], b2[b], 1e-12), (b, a1[b], b1[b], a2[b], b2[b])
        x1, x2 = A.branch_derivatives(int(b))
        y1, y2 = B.branch_derivatives(int(b))
        assert _close(x1, y1, 1e-12) and _close(x2, y2, 1e-12), (b, x1, y1, x2, y2)
