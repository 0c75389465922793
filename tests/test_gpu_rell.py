"""RELL resampling on the device: site rows (plk_site_row_*, plk_site_row_from_root,
plk_nni_site_rows), replicate weights and plk_replicate_sums.

Bounds.  replicate_sums: |G - exact| <= P 2^-53 Gabs, the worst case of ANY order of P fused
multiply-adds (each step rounds once, by at most 2^-53 of a partial sum that never exceeds the sum
of absolute values), so it is derived and not measured; `exact` is math.fsum of the fp64 products,
whose own rounding (2^-53 per product) is inside that bound for P >= 2 and absent for P = 1 (one
fma from +0.0 is the rounded product).  Gabs is held to the same bound against fsum of |w| |x|.
Bitwise checks use test_rell_cpu.py's restatement of the summation rule on data whose products are
exact.  Site rows: bitwise against root_loglik(want_sites=True); log rho rows within 1e-10 per
pattern of the engine's own site lnL of the swapped tree minus the current one, and their
weighted sum within 1e-10 weight sums of nni_scores' delta (test_gpu_nni.py's bound, per unit
weight and summed)."""
import math

import numpy as np
import pytest

import phylo
import plk
import workload
from conftest import set_tune

import test_nni_cpu as ref
import test_rell_cpu as rule
from test_gpu_nni import ARG, STATE, UNSUPPORTED, DR, GUARD, Problem, _code
from test_gpu_parity import MODES, _caterpillar, engine_for
from test_gpu_posteriors import _prepare

pytestmark = pytest.mark.gpu


def bare_engine(P, device=0):
    """The smallest legal handle: the rows and weights need no tree."""
    return plk.Engine(device, 2, 1, P, 0, 1, 1, 0)


def load_rows(eng, X, first=0):
    for i, x in enumerate(X):
        eng.site_row_set(first + i, x)


# ---------------------------------------------------------------- 1. replicate sums

def _weights(kind, rng, R, P):
    if kind == "counts":
        return rng.multinomial(P, np.full(P, 1.0 / P), size=R).astype(np.float64)
    return rng.normal(0.0, 2.0, (R, P))                        # mixed signs


def _fsum(W, X):
    return np.array([[math.fsum((w * x).tolist()) for x in X] for w in W])


SUM_CASES = [
    # P, replicates, rows, weights
    (1, 1, 1, "counts"), (1, 17, 16, "real"), (63, 15, 16, "real"), (65, 16, 17, "counts"),
    (4096, 17, 33, "real"), (4097, 70, 1, "counts"), (4097, 1, 33, "real"), (2 * 4096 + 5, 17, 17, "real"),
    (2 * 4096 + 5, 70, 33, "counts"),
]


@pytest.mark.parametrize("P,R,M,kind", SUM_CASES)
def test_replicate_sums_vs_fsum(P, R, M, kind):
    rng = np.random.default_rng(P + 7 * R + M)
    W = _weights(kind, rng, R, P)
    X = -rng.gamma(2.0, 3.0, (M, P))
    X[::2] *= rng.choice([-1.0, 1.0], (len(X[::2]), P))        # every other row with mixed signs
    eng = bare_engine(P)
    eng.site_rows_reserve(M + 2)
    load_rows(eng, X, first=1)
    eng.set_replicate_weights(W)
    G, Ga = eng.replicate_sums(1, M, want_abs=True)
    assert G.shape == (R, M) and eng.replicate_passes() == 1
    ex, exa = _fsum(W, X), _fsum(np.abs(W), np.abs(X))
    bound = P * 2.0 ** -53 * exa
    print(f"P {P} R {R} rows {M} {kind}: max |G - exact| / (P 2^-53 Gabs) "
          f"{(np.abs(G - ex) / np.maximum(bound, 1e-300)).max():.3g}, Gabs {(np.abs(Ga - exa) / np.maximum(bound, 1e-300)).max():.3g}")
    assert np.all(np.abs(G - ex) <= bound) and np.all(np.abs(Ga - exa) <= bound)
    assert np.array_equal(G, eng.replicate_sums(1, M))          # without Gabs: the same G
    for i in range(M):
        assert np.array_equal(eng.site_row_get(1 + i), X[i])
    assert not eng.site_row_get(0).any() and not eng.site_row_get(M + 1).any()


def test_huge_values_next_to_zero_weights():
    """+-1e300 where every replicate weighs 0: the products are 0, nothing overflows or turns NaN."""
    P, R, M = 4097, 16, 33
    rng = np.random.default_rng(5)
    W = _weights("counts", rng, R, P)
    X = -rng.gamma(2.0, 3.0, (M, P))
    huge = np.arange(3, P, 7)
    W[:, huge] = 0.0
    X[:, huge] = 1e300 * rng.choice([-1.0, 1.0], (M, len(huge)))
    assert np.all(W[:, huge - 1].sum(axis=0) > 0)              # live neighbours
    eng = bare_engine(P)
    eng.site_rows_reserve(M)
    load_rows(eng, X)
    eng.set_replicate_weights(W)
    G, Ga = eng.replicate_sums(0, M, want_abs=True)
    ex, exa = _fsum(W, X), _fsum(np.abs(W), np.abs(X))
    assert np.isfinite(G).all() and np.isfinite(Ga).all()
    assert np.all(np.abs(G - ex) <= P * 2.0 ** -53 * exa) and np.all(np.abs(Ga - exa) <= P * 2.0 ** -53 * exa)


# ---------------------------------------------------------------- 2. the summation rule, bitwise

def _rule_problem():
    P, R, M = 4097, 17, 17
    W, X = rule.exact_problem(P, R, M, seed=11)
    return P, R, M, W, X


def _sums(eng, W, X, want_abs=False):
    eng.site_rows_reserve(len(X))
    load_rows(eng, X)
    eng.set_replicate_weights(W)
    return eng.replicate_sums(0, len(X), want_abs=want_abs)


def test_rule_restatement_bitwise():
    P, R, M, W, X = _rule_problem()
    G, Ga = _sums(bare_engine(P), W, X, want_abs=True)
    assert np.array_equal(G, rule.rule_sums(W, X))
    assert np.array_equal(Ga, rule.rule_sums(np.abs(W), np.abs(X)))


def test_repeat_chunks_and_positions_bitwise(monkeypatch):
    P, R, M, W, X = _rule_problem()
    eng = bare_engine(P)
    G, Ga = _sums(eng, W, X, want_abs=True)
    again = eng.replicate_sums(0, M, want_abs=True)
    assert np.array_equal(G, again[0]) and np.array_equal(Ga, again[1])
    # two blocks: 16 B per element and block; 1 KiB holds 64 elements (32 with Gabs), so the 17
    # replicates go with 3 rows (with 1 row) at a time
    set_tune(monkeypatch, "RELL_CAP_KB", 1)
    c = eng.replicate_sums(0, M)
    assert eng.replicate_passes() == 6
    ca = eng.replicate_sums(0, M, want_abs=True)
    assert eng.replicate_passes() == 17
    monkeypatch.delenv("PLK_TUNE")
    assert np.array_equal(G, c) and np.array_equal(G, ca[0]) and np.array_equal(Ga, ca[1])
    # a sub-range of the rows, and replicates and rows at other positions
    assert np.array_equal(G[:, 5:9], eng.replicate_sums(5, 4))
    rp, mp = np.random.default_rng(3).permutation(R), np.random.default_rng(4).permutation(M)
    other = bare_engine(P)
    assert np.array_equal(G[rp][:, mp], _sums(other, W[rp], X[mp]))
    # fewer replicates: replicate 16 alone sits at another place of its tile
    other.set_replicate_weights(W[16:])
    assert np.array_equal(G[16:], other.replicate_sums(0, M)[:, np.argsort(mp)])


@pytest.mark.parametrize("devices", [[0, 0], pytest.param([0, 1], marks=pytest.mark.skipif(
    plk.device_count() < 2, reason="distinct-device handles need two GPUs"))])
def test_two_shards_bitwise(devices):
    P, R, M = 2 * 4096 + 5, 17, 17
    W, X = rule.exact_problem(P, R, M, seed=13)
    one = _sums(bare_engine(P), W, X, want_abs=True)
    eng = bare_engine(P, device=devices)
    assert eng.shard_count() == 2
    two = _sums(eng, W, X, want_abs=True)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert np.array_equal(one[0], rule.rule_sums(W, X, n_dev=2))
    assert all(np.array_equal(eng.site_row_get(i), X[i]) for i in (0, M - 1))


def test_replicate_errors():
    eng = bare_engine(100)
    assert _code(lambda: eng.replicate_sums(0, 1)) == STATE               # neither rows nor weights
    eng.site_rows_reserve(3)
    assert _code(lambda: eng.replicate_sums(0, 1)) == STATE               # no weights
    eng.set_replicate_weights(np.ones((2, 100)))
    assert eng.replicate_sums(0, 3).shape == (2, 3)
    for first, n in ((0, 4), (3, 1), (-1, 1), (0, 0)):
        assert _code(lambda: eng.replicate_sums(first, n)) == ARG, (first, n)
    assert _code(lambda: eng.site_row_set(3, np.zeros(100))) == ARG
    assert _code(lambda: eng.site_row_get(-1)) == ARG
    assert _code(lambda: eng.site_rows_reserve(-1)) == ARG
    eng.set_replicate_weights(None)
    assert _code(lambda: eng.replicate_sums(0, 1)) == STATE
    eng.set_replicate_weights(np.ones((2, 100)))
    eng.site_rows_reserve(0)
    assert _code(lambda: eng.replicate_sums(0, 1)) == STATE


# ---------------------------------------------------------------- 3. the root's site row

@pytest.mark.parametrize("S,C,tree,n_pat,mode", [(4, 4, "join12", 4097, "materialize"), (4, 4, "join12", 300, "lnl_only"),
                                                 (4, 2, "caterpillar7", 300, "levelwise"), (20, 4, "join12s20", 600, "materialize"),
                                                 (64, 1, "balanced8", 300, "materialize")])
def test_site_row_from_root_bitwise(S, C, tree, n_pat, mode):
    """Through the fused lnL-only tree4 path as well; the handle is left as it was."""
    pb = Problem(tree, S, C, n_pat, seed=7 + S + C, amb=S == 20)
    eng = pb.engine(GUARD | MODES[mode])
    root = pb.et.root
    before = (eng.root_loglik(root, want_sites=True, want_blocks=True), eng.kernel_path(), eng.root_underflow())
    if mode == "lnl_only":
        assert before[1] in ("jit_tree4", "tree4")          # the fused traversal reduced the root itself
    eng.site_rows_reserve(2)
    assert eng.site_row_from_root(root, 1) == 0
    row = eng.site_row_get(1)
    after = (eng.root_loglik(root, want_sites=True, want_blocks=True), eng.kernel_path(), eng.root_underflow())
    assert np.array_equal(row, before[0][1]) and not eng.site_row_get(0).any()
    assert before[0][0] == after[0][0] and all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert before[1:] == after[1:]
    # a fresh handle asked for the row first: the same values without an earlier reduction
    fresh = pb.engine(GUARD | MODES[mode])
    fresh.site_rows_reserve(1)
    fresh.site_row_from_root(root, 0)
    assert np.array_equal(fresh.site_row_get(0), row)
    assert fresh.root_loglik(root, want_sites=True)[0] == before[0][0]
    # the weighted sum of the row by one replicate of the pattern weights is the lnL (to rounding)
    eng.set_replicate_weights(pb.w[None, :])
    G, Ga = eng.replicate_sums(1, 1, want_abs=True)
    assert abs(G[0, 0] - before[0][0]) <= n_pat * 2.0 ** -52 * Ga[0, 0]


def test_site_row_from_root_rescaled_and_underflowed():
    """The deep caterpillar of test_gpu_nni.py with rescaling: scale counts included, bitwise.  The
    same tree unscaled underflows: those patterns are stored as 0.0 and counted."""
    et = phylo.engine_tree(_caterpillar(300, lo=0.1, hi=0.4))
    pb = Problem(None, 4, 4, 200, seed=5, et=et)
    eng = pb.engine(GUARD | plk.PLK_FLAG_SCALING)
    site = eng.root_loglik(et.root, want_sites=True)[1]
    eng.site_rows_reserve(1)
    assert eng.site_row_from_root(et.root, 0) == 0 and np.isfinite(site).all()
    assert np.array_equal(eng.site_row_get(0), site)
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(2, 0.5)
    et = phylo.engine_tree(_caterpillar(700, lo=0.3, hi=0.5))
    wl = workload.Workload("u", et, [m], None, rates, probs, m.pi, phylo.DNA, 64, False, True, 5)
    states = wl.simulate(0, 64).astype(np.int32)
    un = engine_for(et, 4, 2, 64, states, phylo.DNA.init_table, rates, probs, m.pi, [m], flags=plk.PLK_FLAG_LEVELWISE)
    un.update_pmatrices(np.array([n for n in range(et.n_nodes) if n != et.root], dtype=np.int32),
                        et.brlen[[n for n in range(et.n_nodes) if n != et.root]])
    un.update_partials(phylo.split_ops(et.ops))
    site = un.root_loglik(et.root, want_sites=True)[1]
    dead = ~np.isfinite(site)
    assert dead.any()
    flag = un.root_underflow()
    un.site_rows_reserve(1)
    assert un.site_row_from_root(et.root, 0) == dead.sum()
    row = un.site_row_get(0)
    assert np.all(row[dead] == 0.0) and np.array_equal(row[~dead], site[~dead])
    assert un.root_underflow() == flag


# ---------------------------------------------------------------- 4. log rho rows

def _swapped_sites(pb, eng, s, u, t):
    """Site lnL of the swapped tree with branch p at t: plain plk_evaluate-style traversal and
    root_loglik(want_sites=True) of a second handle, which is put back afterwards."""
    p = pb.par[s]
    ops = ref.postorder_ops(ref.swap_ops(pb.et.ops, s, u), pb.et.root)
    eng.update_pmatrices(np.array([p], dtype=np.int32), np.array([t]))
    eng.update_partials(phylo.split_ops(ops))
    site = eng.root_loglik(pb.et.root, want_sites=True)[1]
    eng.update_pmatrices(np.array([p], dtype=np.int32), pb.et.brlen[[p]])
    return site


@pytest.mark.parametrize("S,C,tree,n_pat", [(4, 1, "balanced8", 300), (4, 4, "join12", 4097), (4, 4, "trifurcating9", 300),
                                            (20, 4, "join12s20", 600), (20, 1, "join12s20", 65), (64, 1, "balanced8", 300),
                                            (64, 4, "caterpillar7", 70)])            # tip uncles on 64 states
def test_nni_site_rows(S, C, tree, n_pat):
    pb = Problem(tree, S, C, n_pat, seed=400 + S + C, amb=S == 20)
    nt = pb.et.n_tips
    sons = ref.sons_of(pb.et.ops)
    # a tip uncle, a tip sibling, an internal son, and every fourth move besides
    first = lambda cond: next((i for i, (s, u) in enumerate(pb.moves) if cond(s, u)), None)
    kinds = [first(lambda s, u: u < nt), first(lambda s, u: any(o < nt for o in sons[pb.par[s]] if o != s)),
             first(lambda s, u: s >= nt)]
    assert tree == "balanced8" or None not in kinds            # (a balanced tree has no tip uncle)
    pick = {i for i in kinds if i is not None} | set(range(0, len(pb.moves), 4))
    moves = [pb.moves[i] for i in sorted(pick)]
    son, uncle = pb.son_uncle(moves)
    t_cur = np.array([pb.et.brlen[pb.par[s]] for s, _ in moves])
    eng = pb.engine(GUARD | DR)
    plain = pb.engine(GUARD)                                   # the pre-existing path, no DR
    cur = plain.root_loglik(pb.et.root, want_sites=True)[1]
    n, wsum = len(moves), pb.w.sum()
    eng.site_rows_reserve(n + 1)
    eng.set_replicate_weights(pb.w[None, :])
    for t in (t_cur, np.full(n, 1e-6), np.full(n, 3.0)):
        eng.nni_site_rows(son, uncle, t, 1)
        rows = np.stack([eng.site_row_get(1 + i) for i in range(n)])
        delta = eng.nni_scores(son, uncle, t)["delta"]
        e_sum = np.abs(rows @ pb.w - delta).max() / wsum
        e_dev = np.abs(eng.replicate_sums(1, n)[0] - delta).max() / wsum
        e_pat = 0.0
        if t[0] != 1e-6:                                       # (the pruning difference cancels there)
            for i, (s, u) in enumerate(moves):
                e_pat = max(e_pat, np.abs(rows[i] - (_swapped_sites(pb, plain, s, u, t[i]) - cur)).max())
        print(f"t {t[0]:.3g}..: |sum w row - delta| / wsum {e_sum:.3g} (device sum {e_dev:.3g}), per pattern {e_pat:.3g}")
        assert np.isfinite(rows).all() and not eng.site_row_get(0).any()
        assert e_sum <= 1e-10 and e_dev <= 1e-10 and e_pat <= 1e-10


def test_nni_site_rows_chunks_shards_and_handle(monkeypatch):
    pb = Problem("join12", 4, 4, 9000, seed=52)
    son, uncle = pb.son_uncle()
    n = len(son)
    eng = pb.engine(GUARD | DR | plk.PLK_FLAG_LNL_ONLY)
    root = pb.et.root
    before = (eng.root_loglik(root, want_sites=True, want_blocks=True), eng.kernel_path(), eng.all_branch_derivatives())
    eng.site_rows_reserve(n)
    eng.nni_site_rows(son, uncle, pb.t_cur, 0)
    rows = np.stack([eng.site_row_get(i) for i in range(n)])
    after = (eng.root_loglik(root, want_sites=True, want_blocks=True), eng.kernel_path(), eng.all_branch_derivatives())
    assert before[0][0] == after[0][0] and all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert before[1] == after[1]
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
    set_tune(monkeypatch, "NNI_CAP_KB", 1)                     # one move per chunk
    eng.site_rows_reserve(n)
    eng.nni_site_rows(son, uncle, pb.t_cur, 0)
    monkeypatch.delenv("PLK_TUNE")
    assert all(np.array_equal(eng.site_row_get(i), rows[i]) for i in range(n))
    two = pb.engine(GUARD | DR | plk.PLK_FLAG_LNL_ONLY, device=[0, 0])
    assert two.shard_count() == 2
    two.site_rows_reserve(n)
    two.nni_site_rows(son, uncle, pb.t_cur, 0)
    assert all(np.array_equal(two.site_row_get(i), rows[i]) for i in range(n))


def test_nni_site_rows_errors():
    pb = Problem("trifurcating9", 4, 4, 100, seed=61)
    et, m = pb.et, pb.m
    son, uncle = pb.son_uncle()
    t0, n = pb.t_cur, len(son)
    mk = lambda flags: engine_for(et, 4, 4, 100, pb.states, pb.alph.init_table, pb.rates, pb.probs, m.pi, [m], flags=flags)
    eng = mk(GUARD | DR)
    eng.site_rows_reserve(n)
    assert _code(lambda: eng.nni_site_rows(son, uncle, t0, 0)) == STATE    # before a traversal
    eng.update_partials(phylo.split_ops(et.ops))
    assert _code(lambda: eng.nni_site_rows(son, uncle, t0, 0)) == STATE    # no dP / d2P
    _prepare(eng, et)
    eng.nni_site_rows(son, uncle, t0, 0)
    s0, u0 = pb.moves[0]
    for sn, un in (([et.root], [u0]), ([s0], [pb.par[s0]]), ([s0], [s0]), ([et.n_nodes], [u0]), ([s0], [-1])):
        assert _code(lambda: eng.nni_site_rows(sn, un, t0[:1], 0)) == ARG, (sn, un)
    assert _code(lambda: eng.nni_site_rows([], [], [], 0)) == ARG
    assert _code(lambda: eng.nni_site_rows(son, uncle, np.zeros(n), 0)) == ARG
    assert _code(lambda: eng.nni_site_rows(son, uncle, t0, 0, model=np.full(n, 3))) == ARG
    assert _code(lambda: eng.nni_site_rows(son, uncle, t0, 1)) == ARG      # the last row is not reserved
    e2 = mk(GUARD)
    _prepare(e2, et)
    e2.site_rows_reserve(n)
    assert _code(lambda: e2.nni_site_rows(son, uncle, t0, 0)) == STATE     # no PLK_FLAG_DOUBLE_RECURSIVE
    e3 = mk(GUARD | plk.PLK_FLAG_SUBTREE_PATTERNS)
    _prepare(e3, et)
    e3.site_rows_reserve(n)
    assert _code(lambda: e3.nni_site_rows(son, uncle, t0, 0)) == UNSUPPORTED
