"""NNI scoring on the device (plk_nni_scores): every nearest-neighbour interchange of a tree
with the length of the move's branch re-estimated -- the reference's
NNIHomogeneousTreeLikelihood::testNNI for every node of an NNITopologySearch round.

The reference is always plain pruning of the SWAPPED topology (test_nni_cpu.Pruning: the
oracle on the swapped son arrays), on the engine's own P(t) of the other branches and
V exp(lambda r t) Vinv for branch p, minus the same on the current tree.  The numpy restatement
of test_nni_cpu.py, which that module checks against the same pruning, serves as the Newton
reference and for d1 / d2.

Tolerances: the project's DR-versus-path figure on delta and on d1, absolute:
|x - ref| <= 1e-10 x the weight sum at every length, t = 1e-6 included (there |d1| reaches 31
weight sums on 20 states; measured 1.6e-13 weight sums); 1e-9 through the rescaled caterpillar.
d2 against the restatement's analytic d2, which test_nni_cpu.py checks to 1.9e-10 (t^2 d2 per
unit weight, the fourth-order central difference's own error): d2 carries (lambda r)^2 and the
square of rho'/rho where delta carries 1 and grows as 1 / t^2 at short lengths, so it is taken
relative, |x - ref| <= 1e-9 max(wsum, |ref|), ten times the figure of delta.
"""
import numpy as np
import pytest

import phylo
import plk
from conftest import set_tune

import test_nni_cpu as ref
from test_gpu_parity import MODES, _caterpillar, engine_for
from test_gpu_posteriors import _pmats, _prepare

pytestmark = pytest.mark.gpu

DR = plk.PLK_FLAG_DOUBLE_RECURSIVE
GUARD = plk.PLK_FLAG_NONNEG_GUARD
T_MIN, T_MAX = 1e-6, 100.0


# ---------------------------------------------------------------- problems

class Problem:
    def __init__(self, tree, S, C, n_pat, seed, amb=False, et=None):
        rng = np.random.default_rng(seed)
        self.et = et = ref.tree_by_name(tree) if et is None else et
        if S == 4:
            self.m, self.alph = phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5)), phylo.DNA
        elif S == 20:
            self.m, self.alph = phylo.lg08(), phylo.PROTEIN
        else:
            E = rng.uniform(0.1, 2.0, (S, S))
            pi = rng.dirichlet(np.ones(S) * 5)
            Q = phylo.reversible_generator(E + E.T, pi)
            self.m, self.alph = phylo.Model("rand", S, Q, pi, *phylo.reversible_eigen(Q, pi)), phylo.CODON
        self.S, self.C, self.n_pat = S, C, n_pat
        self.rates, self.probs = phylo.gamma_rates(C, 0.5)
        st = phylo.simulate(et, [self.m], None, self.rates, n_pat, seed=seed).astype(np.int32)
        if amb:
            mask = rng.random(st.shape) < 0.15
            st[mask] = rng.integers(S, self.alph.n_codes, size=mask.sum())
        self.states = st
        self.w = rng.integers(1, 9, n_pat).astype(np.float64)
        self.moves = ref.eligible_moves(et.ops, et.root)
        self.par = ref.parents_of(et.ops)
        self.t_cur = np.array([et.brlen[self.par[s]] for s, _ in self.moves])

    def engine(self, flags, device=0):
        et, m = self.et, self.m
        if device == 0:
            eng = engine_for(et, self.S, self.C, self.n_pat, self.states, self.alph.init_table, self.rates, self.probs,
                             m.pi, [m], flags=flags)
        else:
            eng = plk.Engine(device, self.S, self.C, self.n_pat, et.n_tips, et.n_internal, 1, flags)
            eng.set_code_table(self.alph.init_table)
            for i in range(et.n_tips):
                eng.set_tip_codes(i, self.states[i].astype(np.uint8))
            eng.set_category_rates(self.rates, self.probs)
            eng.set_root_frequencies(m.pi)
            eng.set_eigen(0, m.V, m.Vinv, m.lam)
        eng.set_pattern_weights(self.w)
        _prepare(eng, et)
        return eng

    def references(self, eng, scaling=False, restatement=True):
        P = _pmats(eng, self.et)
        et, m = self.et, self.m
        args = (self.states, self.alph.init_table, P, self.rates, self.probs, m.pi, m, self.w)
        pr = ref.Pruning(et.ops, et.root, et.n_nodes, et.n_tips, *args, scaling=scaling)
        rs = ref.Restatement(et.ops, et.root, et.n_tips, *args) if restatement else None
        return pr, rs

    def son_uncle(self, moves=None):
        mv = self.moves if moves is None else moves
        return np.array([s for s, _ in mv], dtype=np.int32), np.array([u for _, u in mv], dtype=np.int32)


def _check_fixed(pb, eng, pr, rs, t0, tol, moves=None):
    """max_iter = 0 at the lengths t0: delta against pruning, d1 / d2 against the restatement."""
    moves = pb.moves if moves is None else moves
    son, uncle = pb.son_uncle(moves)
    out = eng.nni_scores(son, uncle, t0)
    wsum = pb.w.sum()
    assert out["passes"] == 1 and np.array_equal(out["t_opt"], t0) and np.all(out["status"] == 0)
    rd = np.array([pr.delta(s, u, t) for (s, u), t in zip(moves, t0)])
    ed, e1, e2 = np.abs(out["delta"] - rd).max() / wsum, 0.0, 0.0
    if rs is not None:
        r = rs.scores(moves, t0)
        e1 = np.abs(out["d1"] - r["d1"]).max() / wsum
        e2 = (np.abs(out["d2"] - r["d2"]) / np.maximum(wsum, np.abs(r["d2"]))).max()
    tol2 = 10 * tol
    print(f"t0 {t0[0]:.3g}..: |delta - ref| / wsum {ed:.3g}, |d1 - ref| / wsum {e1:.3g} (tolerance {tol:g}), "
          f"d2 relative {e2:.3g} (tolerance {tol2:g}); max |d1| / wsum {np.abs(out['d1']).max() / wsum:.3g}")
    assert np.isfinite(out["delta"]).all() and np.isfinite(out["d1"]).all() and np.isfinite(out["d2"]).all()
    assert ed <= tol and e1 <= tol and e2 <= tol2
    return out


# ---------------------------------------------------------------- 1. fixed length, every move

S4_CASES = [
    # tree, C, patterns, ambiguity codes, mode
    ("balanced8", 1, 300, False, "materialize"),
    ("balanced8", 2, 1, True, "lnl_only"),
    ("caterpillar7", 2, 4097, True, "lnl_only"),        # a two-son root; a second block and tile
    ("caterpillar7", 4, 300, False, "levelwise"),
    ("trifurcating9", 4, 300, True, "materialize"),     # both uncles at the three-son root
    ("trifurcating9", 8, 1, False, "materialize"),      # C = 8: the levelwise preorder (U without pi), CT = 0
    ("join12", 4, 4097, False, "levelwise"),
    ("join12", 8, 300, True, "lnl_only"),
    ("join12", 1, 4097, True, "materialize"),
    ("balanced8", 8, 4097, False, "materialize"),
]


def _fixed_lengths(pb):
    return [pb.t_cur, 0.5 * pb.t_cur, np.full(len(pb.moves), 1e-6), np.full(len(pb.moves), 3.0)]


@pytest.mark.parametrize("tree,C,n_pat,amb,mode", S4_CASES)
def test_fixed_length_s4(tree, C, n_pat, amb, mode):
    pb = Problem(tree, 4, C, n_pat, seed=100 + C + n_pat % 7, amb=amb)
    par, nt, root = pb.par, pb.et.n_tips, pb.et.root
    assert any(par[par[s]] == root for s, _ in pb.moves) and any(par[par[par[s]]] == root for s, _ in pb.moves
                                                                  if par[par[s]] != root)
    assert any(s < nt for s, _ in pb.moves) and any(s >= nt for s, _ in pb.moves)
    eng = pb.engine(GUARD | MODES[mode] | DR)
    pr, rs = pb.references(eng)
    for t0 in _fixed_lengths(pb):
        _check_fixed(pb, eng, pr, rs, np.maximum(t0, T_MIN), 1e-10)


def test_tip_uncles_and_tip_siblings_are_among_the_moves():
    seen_u = seen_o = False
    for tree in ("balanced8", "caterpillar7", "trifurcating9", "join12"):
        et = ref.tree_by_name(tree)
        sons, par = ref.sons_of(et.ops), ref.parents_of(et.ops)
        for s, u in ref.eligible_moves(et.ops, et.root):
            seen_u |= u < et.n_tips
            seen_o |= any(o < et.n_tips for o in sons[par[s]] if o != s)
    assert seen_u and seen_o


@pytest.mark.parametrize("S,C,tree,n_pat", [(20, 4, "join12s20", 600), (64, 1, "balanced8", 300),
                                            (64, 2, "balanced8", 300)])
def test_fixed_length_mfma(S, C, tree, n_pat):
    pb = Problem(tree, S, C, n_pat, seed=S + C, amb=S == 20)
    eng = pb.engine(GUARD | DR)
    pr, rs = pb.references(eng)
    for t0 in _fixed_lengths(pb):
        _check_fixed(pb, eng, pr, rs, t0, 1e-10)


# ---------------------------------------------------------------- 2. scaling

def test_deep_caterpillar_rescaled():
    """300 taxa: L and U pass through rescaling and underflow doubles without it; the scale
    counts cancel in gamma / l_cur (while the product of the four to six stored vectors is a
    normal double: here every sibling and uncle is a tip; the coefficient build takes a power
    of two out of each vector for the other case, group G of test_gpu_xref_consumers.py).  Against the oracle with scaling on both topologies, t = 1e-6
    (the short-length form on rescaled L and U) included.  The restatement has no rescaling, so
    d1 and d2 are checked against fourth-order central differences of that oracle (h = 0.01 t,
    as t d1 and t^2 d2 per unit weight, bounds 1e-6 and 1e-5: test_nni_cpu.py's reasoning, the
    oracle's rounding through 300 levels, ~1e-12, divided by h and h^2 staying below them)."""
    et = phylo.engine_tree(_caterpillar(300, lo=0.1, hi=0.4))
    pb = Problem(None, 4, 4, 200, seed=5, et=et)
    eng = pb.engine(GUARD | plk.PLK_FLAG_SCALING | DR)
    pr, _ = pb.references(eng, scaling=True, restatement=False)
    # moves near the root, at the deepest node and in between, tips and internal sons
    step = max(1, len(pb.moves) // 7)
    moves = pb.moves[::step][:8] + pb.moves[-2:]
    assert len(moves) >= 8
    t_cur = np.array([et.brlen[pb.par[s]] for s, _ in moves])
    wsum, e1, e2 = pb.w.sum(), 0.0, 0.0
    for t0 in (t_cur, 0.5 * t_cur, np.full(len(moves), 1e-6), np.full(len(moves), 3.0)):
        out = _check_fixed(pb, eng, pr, None, t0, 1e-9, moves=moves)
        if t0[0] == 1e-6 or t0[0] == 3.0:
            continue
        for i, (s, u) in enumerate(moves):
            f1, f2 = ref._stencils(lambda x: pr.delta(s, u, x), t0[i], 0.01 * t0[i])
            e1 = max(e1, abs(out["d1"][i] - f1) * t0[i] / wsum)
            e2 = max(e2, abs(out["d2"][i] - f2) * t0[i] ** 2 / wsum)
    print(f"against central differences of the scaled oracle: t d1 {e1:.3g}, t^2 d2 {e2:.3g} per unit weight")
    assert e1 <= 1e-6 and e2 <= 1e-5


def test_scaled_and_unscaled_handles_agree():
    pb = Problem("join12", 4, 4, 300, seed=21)
    son, uncle = pb.son_uncle()
    a = pb.engine(GUARD | DR).nni_scores(son, uncle, pb.t_cur)
    b = pb.engine(GUARD | DR | plk.PLK_FLAG_SCALING).nni_scores(son, uncle, pb.t_cur)
    wsum = pb.w.sum()
    for k in ("delta", "d1", "d2"):
        assert np.abs(a[k] - b[k]).max() <= 1e-10 * max(wsum, np.abs(a[k]).max()), k


# ---------------------------------------------------------------- 3. optimisation

OPT_CASES = [(4, 1, "balanced8", 300), (4, 4, "trifurcating9", 300), (4, 8, "join12", 4097), (20, 4, "join12s20", 600)]


@pytest.mark.parametrize("S,C,tree,n_pat", OPT_CASES)
def test_optimised_lengths(S, C, tree, n_pat):
    pb = Problem(tree, S, C, n_pat, seed=300 + S + C, amb=S == 20)
    eng = pb.engine(GUARD | DR)
    pr, _ = pb.references(eng)
    son, uncle = pb.son_uncle()
    at0 = eng.nni_scores(son, uncle, pb.t_cur)
    out = eng.nni_scores(son, uncle, pb.t_cur, t_min=T_MIN, t_max=T_MAX, tol=1e-8, max_iter=40)
    wsum = pb.w.sum()
    tol = 1e-10 * wsum
    print(f"passes: {out['passes']}; t_opt in [{out['t_opt'].min():.3g}, {out['t_opt'].max():.3g}]")
    assert np.all(out["status"] == 0), np.flatnonzero(out["status"])
    assert np.all(out["delta"] >= at0["delta"])
    for i, (s, u) in enumerate(pb.moves):
        t = out["t_opt"][i]
        assert abs(out["delta"][i] - pr.delta(s, u, t)) <= tol, (s, u, t)
        if T_MIN < t < T_MAX:
            assert pr.delta(s, u, t * (1 + 1e-3)) <= out["delta"][i] + tol, (s, u, t)
            assert pr.delta(s, u, t * (1 - 1e-3)) <= out["delta"][i] + tol, (s, u, t)
        elif t == T_MIN:
            assert out["d1"][i] <= 0.0, (s, u)
        else:
            assert out["d1"][i] >= 0.0, (s, u)


@pytest.mark.parametrize("S,C,tree,n_pat", OPT_CASES)
def test_newton_path_equals_restatement(S, C, tree, n_pat):
    """t_opt (1e-6 relative: the sums differ in rounding) and the number of passes, side by side.

    Both sides decide F(t') >= F(t) on the change summed per pattern.  Decided on the difference
    of the two sums of logs, the last steps of a move (8e-10 in t, worth 1e-14 in F = -229.2 that
    carries 3e-14 of rounding) were accepted by one side and rejected by the other: on
    (4, 8, join12, 4097) the device then took 8 passes and the restatement 9."""
    pb = Problem(tree, S, C, n_pat, seed=300 + S + C, amb=S == 20)
    eng = pb.engine(GUARD | DR)
    _, rs = pb.references(eng)
    son, uncle = pb.son_uncle()
    out = eng.nni_scores(son, uncle, pb.t_cur, t_min=T_MIN, t_max=T_MAX, tol=1e-8, max_iter=40)
    cpu = rs.scores(pb.moves, pb.t_cur, t_min=T_MIN, t_max=T_MAX, tol=1e-8, max_iter=40)
    rel = np.abs(out["t_opt"] - cpu["t_opt"]) / cpu["t_opt"]
    print(f"t_opt vs restatement: {rel.max():.3g} relative; passes: device {out['passes']}, restatement {cpu['passes']}")
    assert rel.max() <= 1e-6
    assert out["passes"] == cpu["passes"]


def test_iteration_budget_is_reported():
    pb = Problem("join12", 4, 4, 300, seed=31)
    eng = pb.engine(GUARD | DR)
    son, uncle = pb.son_uncle()
    one = eng.nni_scores(son, uncle, pb.t_cur, max_iter=1, tol=1e-12)
    assert one["passes"] == 2 and np.any(one["status"] == 1)
    full = eng.nni_scores(son, uncle, pb.t_cur, max_iter=40, tol=1e-8)
    assert np.all(full["delta"] >= one["delta"] - 1e-10 * pb.w.sum())


# ---------------------------------------------------------------- 4. consistency with a real swap

def _apply(pb, eng, s, u, t):
    """The engine after the move: swapped ops, P(t) of branch p, a full traversal.  Returns lnL."""
    p = pb.par[s]
    ops = ref.postorder_ops(ref.swap_ops(pb.et.ops, s, u), pb.et.root)
    eng.update_pmatrices(np.array([p], dtype=np.int32), np.array([t]), deriv_mask=7)
    eng.update_partials(phylo.split_ops(ops))
    return eng.root_loglik(pb.et.root)[0]


@pytest.mark.parametrize("C,tree", [(4, "trifurcating9"), (8, "join12")])
def test_delta_is_the_change_of_lnl(C, tree):
    pb = Problem(tree, 4, C, 500, seed=41 + C, amb=True)
    son, uncle = pb.son_uncle()
    tol = 1e-10 * pb.w.sum()
    for i in range(0, len(pb.moves), 5):
        s, u = pb.moves[i]
        one = (son[i:i + 1], uncle[i:i + 1], pb.t_cur[i:i + 1])
        eng = pb.engine(GUARD | DR)
        lnl0 = eng.root_loglik(pb.et.root)[0]
        fwd = eng.nni_scores(*one, max_iter=40)
        at_old = eng.nni_scores(*one)
        lnl1 = _apply(pb, eng, s, u, fwd["t_opt"][0])
        assert abs((lnl1 - lnl0) - fwd["delta"][0]) <= tol, (s, u)
        # the inverse move from there, at the old length, leads back to the old tree
        back = eng.nni_scores([u], [s], pb.t_cur[i:i + 1])
        assert abs(back["delta"][0] + fwd["delta"][0]) <= tol, (s, u)
        # and with the forward move applied at the old length, it undoes delta at that length
        lnl2 = _apply(pb, eng, s, u, pb.t_cur[i])
        assert abs((lnl2 - lnl0) - at_old["delta"][0]) <= tol, (s, u)
        back = eng.nni_scores([u], [s], pb.t_cur[i:i + 1])
        assert abs(back["delta"][0] + at_old["delta"][0]) <= tol, (s, u)


# ---------------------------------------------------------------- 5. invariance

def _same(a, b, keys=("t_opt", "delta", "d1", "d2", "status")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def test_repeat_and_chunks_bitwise(monkeypatch):
    pb = Problem("join12", 4, 4, 4097, seed=51)
    eng = pb.engine(GUARD | DR)
    son, uncle = pb.son_uncle()
    for mi in (0, 40):
        a = eng.nni_scores(son, uncle, pb.t_cur, max_iter=mi)
        assert _same(a, eng.nni_scores(son, uncle, pb.t_cur, max_iter=mi))
        # 17 rows x 4352 padded patterns x 8 B = 578 KiB per move: three moves per chunk
        set_tune(monkeypatch, "NNI_CAP_KB", 1800)
        c = eng.nni_scores(son, uncle, pb.t_cur, max_iter=mi)
        set_tune(monkeypatch, "NNI_CAP_KB", 1)            # one move per chunk
        d = eng.nni_scores(son, uncle, pb.t_cur, max_iter=mi)
        monkeypatch.delenv("PLK_TUNE")
        assert c["passes"] > a["passes"] and d["passes"] >= len(pb.moves)
        assert _same(a, c) and _same(a, d)


def test_multi_device_bitwise():
    n = 9000                                                 # three 4096-blocks, a ragged tail
    pb = Problem("join12", 4, 4, n, seed=52)
    son, uncle = pb.son_uncle()
    outs = []
    for dev in (0, [0, 0]):
        eng = pb.engine(GUARD | DR, device=dev)
        if dev != 0:
            assert eng.shard_count() == 2
        outs.append([eng.nni_scores(son, uncle, pb.t_cur, max_iter=mi) for mi in (0, 40)])
    for a, b in zip(*outs):
        assert _same(a, b) and a["passes"] == b["passes"]


@pytest.mark.parametrize("C", [4, 8])
def test_call_leaves_the_handle_alone(C):
    pb = Problem("join12", 4, C, 500, seed=53 + C)
    eng = pb.engine(GUARD | DR | plk.PLK_FLAG_LNL_ONLY)
    root = pb.et.root
    before = (eng.root_loglik(root, want_sites=True, want_blocks=True), eng.kernel_path(), eng.all_branch_derivatives())
    son, uncle = pb.son_uncle()
    out = eng.nni_scores(son, uncle, pb.t_cur, max_iter=40)
    after = (eng.root_loglik(root, want_sites=True, want_blocks=True), eng.kernel_path(), eng.all_branch_derivatives())
    assert before[0][0] == after[0][0] and all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert before[1] == after[1]
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
    assert _same(out, eng.nni_scores(son, uncle, pb.t_cur, max_iter=40))


def test_repeated_call_is_one_build_and_follows_a_new_length():
    pb = Problem("join12", 4, 4, 1000, seed=55)
    et = pb.et
    eng = pb.engine(GUARD | DR)
    son, uncle = pb.son_uncle()
    stale = eng.nni_scores(son, uncle, pb.t_cur)
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_PARTIALS)
    again = eng.nni_scores(son, uncle, pb.t_cur)
    n = eng.get_timing()["launches"]
    eng.set_timing(False)
    assert n == 1 and _same(stale, again)                    # the coefficient build alone: U still holds
    # a new length on one branch, an incremental traversal: the preorder pass runs again
    b = 2
    et.brlen[b] *= 1.7
    eng.update_pmatrices(np.array([b], dtype=np.int32), et.brlen[[b]], deriv_mask=7)
    anc, v = set(), b
    while v in pb.par:
        v = pb.par[v]
        anc.add(v)
    eng.update_partials(phylo.split_ops([(p, ch) for p, ch in et.ops if p in anc]))
    new = eng.nni_scores(son, uncle, pb.t_cur)
    fresh = pb.engine(GUARD | DR).nni_scores(son, uncle, pb.t_cur)
    wsum = pb.w.sum()
    for k in ("delta", "d1", "d2"):
        assert np.abs(new[k] - fresh[k]).max() <= 1e-10 * max(wsum, np.abs(fresh[k]).max()), k
    assert np.abs(new["delta"] - stale["delta"]).max() > 1e-6


# ---------------------------------------------------------------- 6. errors

def _code(fn):
    with pytest.raises(plk.PlkError) as ei:
        fn()
    return ei.value.code


ARG, DEVICE, UNSUPPORTED, STATE = -1, -2, -4, -5


def test_errors(monkeypatch):
    pb = Problem("trifurcating9", 4, 4, 100, seed=61)
    et, m = pb.et, pb.m
    son, uncle = pb.son_uncle()
    t0 = pb.t_cur
    mk = lambda flags: engine_for(et, 4, 4, 100, pb.states, pb.alph.init_table, pb.rates, pb.probs, m.pi, [m], flags=flags)
    eng = mk(GUARD | DR)
    assert _code(lambda: eng.nni_scores(son, uncle, t0)) == STATE          # before a traversal
    eng.update_partials(phylo.split_ops(et.ops))
    assert _code(lambda: eng.nni_scores(son, uncle, t0)) == STATE          # no dP / d2P
    _prepare(eng, et)
    ok = eng.nni_scores(son, uncle, t0)
    assert ok["delta"].shape == (len(son),)
    sons, par = ref.sons_of(et.ops), pb.par
    rs = sons[et.root][0]
    s0, u0 = pb.moves[0]
    bad_moves = [([et.root], [u0]), ([rs], [u0]),                          # the root, a son of the root
                 ([s0], [par[s0]]), ([s0], [s0]),                          # the uncle is p; no son of g
                 ([et.n_nodes], [u0]), ([s0], [-1])]                       # out of range
    for sn, un in bad_moves:
        assert _code(lambda: eng.nni_scores(sn, un, t0[:1])) == ARG, (sn, un)
    assert _code(lambda: eng.nni_scores([], [], [])) == ARG                # n_moves <= 0
    assert _code(lambda: eng.nni_scores(son, uncle, t0, t_min=0.0)) == ARG
    assert _code(lambda: eng.nni_scores(son, uncle, t0, t_min=1.0, t_max=0.5)) == ARG
    assert _code(lambda: eng.nni_scores(son, uncle, np.full(len(son), 200.0))) == ARG
    assert _code(lambda: eng.nni_scores(son, uncle, np.full(len(son), 1e-9))) == ARG
    assert _code(lambda: eng.nni_scores(son, uncle, t0, model=np.full(len(son), 3))) == ARG
    # a node outside the current tree: a traversal of one cherry only
    # (topo_kids merges traversals, so use a fresh handle whose tree never held the other nodes)
    sub = next((p, ch) for p, ch in et.ops if all(c < et.n_tips for c in ch))
    e5 = mk(GUARD | DR)
    e5.update_partials(phylo.split_ops([sub]))
    s9, u9 = pb.moves[-1]
    assert s9 != sub[0] and s9 not in sub[1]
    assert _code(lambda: e5.nni_scores([s9], [u9], t0[-1:])) == ARG
    # no PLK_FLAG_DOUBLE_RECURSIVE
    e2 = mk(GUARD)
    _prepare(e2, et)
    assert _code(lambda: e2.nni_scores(son, uncle, t0)) == STATE
    # pattern compression
    e3 = mk(GUARD | plk.PLK_FLAG_SUBTREE_PATTERNS)
    _prepare(e3, et)
    assert _code(lambda: e3.nni_scores(son, uncle, t0)) == UNSUPPORTED
    # a model without an eigen system: P(t) given by the host
    e4 = plk.Engine(0, 4, 4, 100, et.n_tips, et.n_internal, 2, GUARD | DR)
    e4.set_code_table(pb.alph.init_table)
    for i in range(et.n_tips):
        e4.set_tip_codes(i, pb.states[i].astype(np.uint8))
    e4.set_category_rates(pb.rates, pb.probs)
    e4.set_root_frequencies(m.pi)
    e4.set_eigen(0, m.V, m.Vinv, m.lam)
    _prepare(e4, et)
    assert _code(lambda: e4.nni_scores(son, uncle, t0, model=np.ones(len(son), dtype=np.int32))) == STATE
    assert e4.nni_scores(son, uncle, t0, model=np.zeros(len(son), dtype=np.int32))["delta"].shape == (len(son),)
    # p or g of more than three sons
    t = phylo.Tree.from_newick("((a:0.1,b:0.2,c:0.05,d:0.3):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2);")
    pe = Problem(None, 4, 4, 100, seed=62, et=phylo.engine_tree(t))
    e6 = pe.engine(GUARD | DR)
    sons6, par6 = ref.sons_of(pe.et.ops), ref.parents_of(pe.et.ops)
    wide = next(p for p in sons6 if p != pe.et.root and len(sons6[p]) == 4)
    other = next(o for o in sons6[pe.et.root] if o != wide)
    assert _code(lambda: e6.nni_scores([sons6[wide][0]], [other], [0.1])) == UNSUPPORTED
