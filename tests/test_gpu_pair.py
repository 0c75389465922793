"""Pairwise ML distances on the device (plk_pair_counts, plk_pair_distances) against the numpy
restatement of test_pair_cpu.py, which that module checks against a per-pattern evaluation.

Counts: integer weights make every partial sum exact, so the tables are compared bitwise with
np.add.at on the caller's codes -- over a second pattern block (4097 patterns), more tips than a
pair group holds, 65 codes (one set of bins, weights read through L2), 33..64 codes (one set of
bins, weights staged) and few codes (a set of bins per wave), forced chunks, two calls, re-uploaded
codes and two shards.  Fractional weights: 4097 addends of like sign round to (4097 / 2) ulp at
the very worst, 5e-13 relative, and to ~sqrt(4097) / 2 ulp = 7e-15 as a random walk; the bound is
1e-13.

Fixed length: lnl and d1 within 1e-10 x the weight sum, d2 within 1e-9 max(weight sum, |ref|), the
bounds of test_gpu_nni.py for these quantities.  At t = 1e-6 an entry whose codes exclude each
other has l = O(t) and l'/l = 1 / t, so d1 = D / t with D the weight of those entries, and one ulp
of d1 is 1.1e-10 D: the bound is 0.9 (weight sum / D) ulp of the number it bounds.  For
sequences at distances 0.02 .. 2 (D up to 0.42 weight sums) that is two ulp, which no two
summation orders share: there the device measured 1.5e-10 weight sums against the restatement,
4e-16 of d1 = 3.9e5 weight sums.  The fixed-length problems are therefore close sequences, the
case the short-length form exists for: branch lengths 0.002 .. 0.02 and 3 % ambiguity codes keep
D under a tenth of the weight sum (asserted), so the bound leaves nine ulp of d1 or more.  Newton: t_opt within 10 tol max(t, t_min) of the
restatement's (each side's last step bounds its own error by tol max(t, t_min)), status and passes
equal.
"""
import numpy as np
import pytest

import phylo
import plk
from conftest import set_tune

import test_pair_cpu as ref

pytestmark = pytest.mark.gpu

T_MIN, T_MAX = ref.T_MIN, ref.T_MAX
GUARD = plk.PLK_FLAG_NONNEG_GUARD


def make_engine(pb, device=0, codes=None, eigen=True):
    """An engine for the pairwise calls: tips, code table, weights, rates, pi, eigen system; one
    internal node, no P(t), no traversal."""
    eng = plk.Engine(device, pb.S, pb.C, pb.n_pat, pb.n_tips, 1, 1, GUARD)
    eng.set_code_table(pb.alph.init_table)
    codes = pb.codes if codes is None else codes
    for i in range(pb.n_tips):
        eng.set_tip_codes(i, codes[i].astype(np.uint8))
    eng.set_pattern_weights(pb.w)
    eng.set_category_rates(pb.rates, pb.probs)
    eng.set_root_frequencies(pb.m.pi)
    if eigen:
        eng.set_eigen(0, pb.m.V, pb.m.Vinv, pb.m.lam)
    return eng


def ref_counts(pb, ta, tb, codes=None):
    codes = pb.codes if codes is None else codes
    return np.stack([ref.pair_table(codes[a], codes[b], pb.w, pb.alph.n_codes) for a, b in zip(ta, tb)])


def all_pairs(pb):
    ta, tb = zip(*pb.pairs)
    return np.array(ta, dtype=np.int32), np.array(tb, dtype=np.int32)


# ---------------------------------------------------------------- 1. counts

COUNT_CASES = [
    # S, C, tips, patterns, ambiguity codes
    (4, 1, 2, 1, False),
    (4, 4, 9, 300, False),
    (4, 4, 9, 4097, True),      # a second block
    (20, 2, 7, 300, True),
    (64, 1, 5, 4097, True),     # 65 codes
    (4, 8, 33, 300, True),      # 528 pairs: many pair groups
    (64, 1, 3, 300, False),     # 33..64 codes in use
]


@pytest.mark.parametrize("S,C,n_tips,n_pat,amb", COUNT_CASES)
def test_counts_bitwise(S, C, n_tips, n_pat, amb):
    pb = ref.Problem(S, C, n_tips, n_pat, amb, seed=200 + S + n_tips)
    used = len(np.unique(pb.codes))
    if S == 64:
        assert used == 65 if amb else 32 < used <= 64
    eng = make_engine(pb)
    ta, tb = all_pairs(pb)
    got = eng.pair_counts(ta, tb)
    assert got.shape == (len(ta), pb.alph.n_codes, pb.alph.n_codes)
    assert np.array_equal(got, ref_counts(pb, ta, tb))
    assert np.array_equal(eng.pair_counts(ta, tb), got)  # a second call


def test_counts_order_repeats_chunks_and_new_codes(monkeypatch):
    pb = ref.Problem(4, 4, 9, 4097, True, seed=31)
    eng = make_engine(pb)
    ta = np.array([0, 1, 0, 8, 3, 0, 5], dtype=np.int32)
    tb = np.array([1, 0, 1, 2, 4, 1, 3], dtype=np.int32)
    got = eng.pair_counts(ta, tb)
    assert np.array_equal(got, ref_counts(pb, ta, tb))
    assert np.array_equal(got[1], got[0].T) and np.array_equal(got[2], got[0]) and np.array_equal(got[5], got[0])
    # chunks: 15 table codes and two blocks of at most 15 codes in use are 5.4 KB per pair,
    # so 16 KB hold 3 of the 36 pairs
    ta, tb = all_pairs(pb)
    whole = eng.pair_counts(ta, tb)
    set_tune(monkeypatch, "PAIR_CAP_KB", 16)
    assert np.array_equal(eng.pair_counts(ta, tb), whole)
    d0 = eng.pair_distances(ta, tb, tol=1e-8, max_iter=40)
    monkeypatch.delenv("PLK_TUNE")
    d1 = eng.pair_distances(ta, tb, tol=1e-8, max_iter=40)
    for k in d0:
        assert np.array_equal(d0[k], d1[k]), k
    # new codes for one tip (a code the alignment had not used included)
    codes = pb.codes.copy()
    codes[2] = np.roll(codes[2], 7)
    codes[2, 5] = 13
    eng.set_tip_codes(2, codes[2].astype(np.uint8))
    assert np.array_equal(eng.pair_counts(ta, tb), ref_counts(pb, ta, tb, codes))


def test_counts_fractional_weights():
    pb = ref.Problem(4, 4, 9, 4097, True, seed=32, int_weights=False)
    eng = make_engine(pb)
    ta, tb = all_pairs(pb)
    got, want = eng.pair_counts(ta, tb), ref_counts(pb, ta, tb)
    assert np.array_equal(got == 0.0, want == 0.0)
    err = (np.abs(got - want) / np.where(want > 0, want, 1.0)).max()
    print(f"fractional weights: relative {err:.3g}")
    assert err <= 1e-13


# ---------------------------------------------------------------- 2. fixed length

FIXED_CASES = [(4, 1, 5, 300, False), (4, 4, 5, 300, True), (4, 8, 5, 4097, True), (20, 4, 4, 300, True),
               (64, 1, 3, 300, True)]


@pytest.mark.parametrize("S,C,n_tips,n_pat,amb", FIXED_CASES)
def test_fixed_length(S, C, n_tips, n_pat, amb):
    pb = ref.Problem(S, C, n_tips, n_pat, amb, seed=300 + S + C, brlen=(0.002, 0.02), amb_rate=0.03)
    eng, rs = make_engine(pb), pb.restatement()
    ta, tb = all_pairs(pb)
    ta, tb = np.concatenate([ta, tb[:2]]), np.concatenate([tb, ta[:2]])
    wsum = pb.w.sum()
    excl = rs.delta == 0.0  # codes that exclude each other
    assert max(rs.table(a, b)[excl].sum() for a, b in zip(ta, tb)) <= 0.1 * wsum
    start = np.array([rs.start(rs.table(a, b)) for a, b in zip(ta, tb)])
    worst = []
    for t0 in (np.full(len(ta), 1e-6), np.full(len(ta), 0.05), np.full(len(ta), 3.0), start, None):
        out = eng.pair_distances(ta, tb, t0)
        want = rs.distances(ta, tb, t0)
        assert out["passes"] == 1 and np.all(out["status"] == 0)
        assert np.array_equal(out["t_opt"], start if t0 is None else t0)
        e0 = np.abs(out["lnl"] - want["lnl"]).max() / wsum
        e1 = np.abs(out["d1"] - want["d1"]).max() / wsum
        e2 = (np.abs(out["d2"] - want["d2"]) / np.maximum(wsum, np.abs(want["d2"]))).max()
        print(f"S {S} C {C} t0 {'start' if t0 is None else format(t0[0], '.3g')}: |lnl - ref| / wsum {e0:.3g}, |d1 - ref| / wsum {e1:.3g} "
              f"(max |d1| / wsum {np.abs(want['d1']).max() / wsum:.3g}), d2 relative {e2:.3g}")
        assert np.isfinite(out["lnl"]).all() and np.isfinite(out["d1"]).all() and np.isfinite(out["d2"]).all()
        worst.append((e0, e1, e2))
    for e0, e1, e2 in worst:
        assert e0 <= 1e-10 and e1 <= 1e-10 and e2 <= 1e-9


# ---------------------------------------------------------------- 3. Newton

@pytest.mark.parametrize("S,C,n_tips,n_pat,amb", FIXED_CASES)
def test_newton(S, C, n_tips, n_pat, amb):
    pb = ref.Problem(S, C, n_tips, n_pat, amb, seed=300 + S + C)
    eng, rs = make_engine(pb), pb.restatement()
    ta, tb = all_pairs(pb)
    tol = 1e-8
    out = eng.pair_distances(ta, tb, tol=tol, max_iter=40)
    want = rs.distances(ta, tb, tol=tol, max_iter=40)
    err = (np.abs(out["t_opt"] - want["t_opt"]) / np.maximum(want["t_opt"], T_MIN)).max()
    print(f"S {S} C {C}: t_opt relative {err:.3g}, passes {out['passes']} (restatement {want['passes']})")
    assert err <= 10 * tol
    assert np.all(out["status"] == 0) and np.all(want["status"] == 0)
    assert out["passes"] == want["passes"]
    assert np.abs(out["lnl"] - want["lnl"]).max() <= 1e-10 * pb.w.sum()
    # a budget that runs out
    short = eng.pair_distances(ta, tb, tol=tol, max_iter=1)
    wshort = rs.distances(ta, tb, tol=tol, max_iter=1)
    assert np.array_equal(short["status"], wshort["status"]) and short["status"].any() and short["passes"] == 2


def test_newton_extremes():
    codes, alph, rates, probs, m, w = ref.extremes_problem()
    eng = plk.Engine(0, 4, 4, codes.shape[1], 3, 1, 1, GUARD)
    eng.set_code_table(alph.init_table)
    for i in range(3):
        eng.set_tip_codes(i, codes[i].astype(np.uint8))
    eng.set_pattern_weights(w)
    eng.set_category_rates(rates, probs)
    eng.set_root_frequencies(m.pi)
    eng.set_eigen(0, m.V, m.Vinv, m.lam)
    out = eng.pair_distances([0, 0], [1, 2], tol=1e-8, max_iter=40)
    assert out["t_opt"][0] == T_MIN and out["t_opt"][1] == T_MAX and np.all(out["status"] == 0)


def test_nonreversible_ordered_pairs():
    m = ref.nonreversible_model(np.random.default_rng(5))
    pb = ref.Problem(4, 4, 3, 300, True, 6, model=m)
    eng, pat = make_engine(pb), pb.patterns()
    ta, tb = np.array([0, 1, 0, 2], dtype=np.int32), np.array([1, 0, 2, 0], dtype=np.int32)
    wsum, tol = pb.w.sum(), 1e-8
    for t in (1e-6, 0.05, 3.0):
        out = eng.pair_distances(ta, tb, np.full(4, t))
        want = np.array([pat.F(a, b, t) for a, b in zip(ta, tb)])
        assert np.abs(out["lnl"] - want).max() <= 1e-10 * wsum
    out = eng.pair_distances(ta, tb, tol=tol, max_iter=40)
    assert np.all(out["status"] == 0)
    assert out["t_opt"][0] != out["t_opt"][1]
    for i, (a, b) in enumerate(zip(ta, tb)):
        root = pat.bisect_d1(a, b)
        assert root is not None and abs(out["t_opt"][i] - root) <= 10 * tol * max(root, T_MIN)


# ---------------------------------------------------------------- 4. two shards

def test_multi_device_bitwise():
    pb = ref.Problem(4, 4, 5, 8193, False, seed=41)
    # three blocks over two shards: 8192 patterns and 1.  Ambiguity codes in the first shard, and
    # one that only the second meets (the shards number their codes in use differently)
    pb.codes[:, 100:700][np.random.default_rng(42).random((5, 600)) < 0.3] = 14
    pb.codes[1, 5000:5100] = 5
    pb.codes[3, 8192] = 12
    one, two = make_engine(pb), make_engine(pb, device=[0, 0])
    assert two.shard_count() == 2
    ta, tb = all_pairs(pb)
    c1 = one.pair_counts(ta, tb)
    assert np.array_equal(c1, ref_counts(pb, ta, tb))
    assert np.array_equal(two.pair_counts(ta, tb), c1)
    for kw in ({}, {"t0": np.full(len(ta), 0.05)}, {"tol": 1e-8, "max_iter": 40}):
        a, b = one.pair_distances(ta, tb, **kw), two.pair_distances(ta, tb, **kw)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 5. errors, and what the call leaves alone

def _code(fn, *a, **kw):
    with pytest.raises(plk.PlkError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors():
    ARG, UNSUP, STATE = -1, -4, -5
    pb = ref.Problem(4, 2, 3, 50, False, seed=51)
    eng = make_engine(pb)
    for fn in (eng.pair_counts, eng.pair_distances):
        assert _code(fn, [0], [0]) == ARG
        assert _code(fn, [0], [3]) == ARG
        assert _code(fn, [-1], [1]) == ARG
        assert _code(fn, [], []) == ARG
    assert _code(eng.pair_distances, [0], [1], t_min=0.0) == ARG
    assert _code(eng.pair_distances, [0], [1], t_min=1.0, t_max=0.5) == ARG
    assert _code(eng.pair_distances, [0], [1], t0=[200.0]) == ARG
    assert _code(eng.pair_distances, [0], [1], t0=[1e-7]) == ARG
    assert _code(eng.pair_distances, [0], [1], model=1) == ARG
    # call order
    raw = plk.Engine(0, 4, 2, 50, 3, 1, 1, GUARD)
    assert _code(raw.pair_counts, [0], [1]) == STATE          # no code table
    raw.set_code_table(pb.alph.init_table)
    raw.set_tip_codes(0, pb.codes[0].astype(np.uint8))
    assert _code(raw.pair_counts, [0], [1]) == STATE          # tip 1 has no codes
    raw.set_tip_codes(1, pb.codes[1].astype(np.uint8))
    assert raw.pair_counts([0], [1]).sum() == 50
    assert _code(raw.pair_counts, [0], [2]) == STATE
    assert _code(raw.pair_distances, [0], [1]) == STATE       # no rates, no pi
    raw.set_category_rates(pb.rates, pb.probs)
    assert _code(raw.pair_distances, [0], [1]) == STATE
    raw.set_root_frequencies(pb.m.pi)
    assert _code(raw.pair_distances, [0], [1]) == STATE       # no eigen system
    raw.set_pmatrix(0, np.stack([pb.m.pij(0.1 * r) for r in pb.rates]))
    assert _code(raw.pair_distances, [0], [1]) == STATE       # (a P(t) alone is none)
    raw.set_eigen(0, pb.m.V, pb.m.Vinv, pb.m.lam)
    assert raw.pair_distances([0], [1])["passes"] == 1
    # more codes in use than the bins hold
    tab = np.eye(20)[np.arange(100) % 20]
    wide = plk.Engine(0, 20, 1, 100, 2, 1, 1, GUARD)
    wide.set_code_table(tab)
    for i in range(2):
        wide.set_tip_codes(i, np.arange(100, dtype=np.uint8))
    with pytest.raises(plk.PlkError) as e:
        wide.pair_counts([0], [1])
    assert e.value.code == UNSUP and "90" in str(e.value)


def test_under_a_communicator_unsupported():
    pb = ref.Problem(4, 2, 3, 50, False, seed=52)
    eng = make_engine(pb)
    eng.comm_init(1, 0, plk.comm_get_id())
    assert _code(eng.pair_counts, [0], [1]) == -4
    assert _code(eng.pair_distances, [0], [1]) == -4


def test_the_call_leaves_the_traversal_alone():
    newick = "((A:0.01, B:0.02):0.03,C:0.01,D:0.1);"
    et = phylo.engine_tree(phylo.Tree.from_newick(newick))
    rng = np.random.default_rng(61)
    m = phylo.t92(3.0, 0.5)
    rates, probs = phylo.gamma_rates(4, 1.0)
    codes = rng.integers(0, 4, (et.n_tips, 200))
    eng = plk.Engine(0, 4, 4, 200, et.n_tips, et.n_internal, 1, GUARD)
    eng.set_code_table(phylo.DNA.init_table)
    for i in range(et.n_tips):
        eng.set_tip_codes(i, codes[i].astype(np.uint8))
    eng.set_category_rates(rates, probs)
    eng.set_root_frequencies(m.pi)
    eng.set_eigen(0, m.V, m.Vinv, m.lam)
    br = np.array([n for n in range(et.n_nodes) if n != et.root], dtype=np.int32)
    eng.update_pmatrices(br, et.brlen[br])
    eng.update_partials(phylo.split_ops(et.ops))
    before, path = eng.root_loglik(et.root, want_sites=True), eng.kernel_path()
    pm, part = eng.get_pmatrix(0), eng.get_partials(et.root)
    eng.pair_counts([0, 1], [1, 2])
    eng.pair_distances([0, 1], [1, 2], tol=1e-8, max_iter=40)
    after = eng.root_loglik(et.root, want_sites=True)
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and eng.kernel_path() == path
    assert np.array_equal(eng.get_pmatrix(0), pm) and np.array_equal(eng.get_partials(et.root), part)
