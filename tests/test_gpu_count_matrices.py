"""Count matrices on the device (plk_set_count_types, plk_update_count_matrices,
plk_set_count_matrix, plk_get_count_matrix) against Van Loan's block exponential, at the
tolerance test_count_matrices_cpu.py works out: 10 x the floor between the two host
formulations, not below 1e-13 max(1, max |W|)."""
import numpy as np
import pytest

import phylo
import plk

from test_count_matrices_cpu import gtr_model, k80_like, van_loan, w_tolerance

pytestmark = pytest.mark.gpu

TS = np.array([1e-6, 0.013, 0.21, 1.0, 2.5, 0.0])     # one branch each; the last has t = 0


def _rand64(seed=7):
    rng = np.random.default_rng(seed)
    E = rng.uniform(0.1, 2.0, (64, 64))
    E = E + E.T
    pi = rng.dirichlet(np.ones(64) * 5)
    Q = phylo.reversible_generator(E, pi)
    V, Vinv, lam = phylo.reversible_eigen(Q, pi)
    return phylo.Model("rand64", 64, Q, pi, V, Vinv, lam)


def _engine(S, C, models, n_nodes=8):
    eng = plk.Engine(0, S, C, 64, n_nodes - 2, 2, len(models))
    rates, probs = phylo.gamma_rates(C, 0.5)
    eng.set_category_rates(rates, probs)
    for k, m in enumerate(models):
        eng.set_eigen(k, m.V, m.Vinv, m.lam)
    return eng, rates


def _check(eng, rates, branches, ts, models, Bs, mi=None):
    worst = 0.0
    for i, b in enumerate(branches):
        k = 0 if mi is None else int(mi[i])
        W = eng.get_count_matrix(int(b))
        assert W.shape == (Bs[k].shape[0], len(rates), models[k].S, models[k].S)
        ref = np.stack([van_loan(models[k].Q, Bs[k], ts[i] * r) for r in rates], axis=1)    # [T, C, S, S]
        tol = w_tolerance(ref)
        err = float(np.abs(W - ref).max())
        worst = max(worst, err / tol)
        assert err <= tol, (int(b), ts[i], err, tol)
        assert W.min() >= 0.0
        if ts[i] == 0.0:
            assert np.all(W == 0.0)
    print(f"worst error / tolerance: {worst:.3g}")


@pytest.mark.parametrize("S,C,T,model", [
    (4, 1, 1, gtr_model), (4, 4, 1, gtr_model), (4, 4, 12, gtr_model), (4, 1, 12, gtr_model),
    (4, 4, 1, k80_like), (4, 4, 12, k80_like),
    (20, 2, 1, phylo.lg08), (64, 1, 1, _rand64)])
def test_count_matrices_vs_van_loan(S, C, T, model):
    m = model()
    B = phylo.total_register(m.Q) if T == 1 else phylo.comprehensive_register(m.Q)
    eng, rates = _engine(S, C, [m])
    eng.set_count_types(0, B)
    br = np.arange(len(TS), dtype=np.int32)
    eng.update_count_matrices(br, TS)
    _check(eng, rates, br, TS, [m], [B])


def test_count_types_set_before_the_eigen_system_and_after_a_new_one():
    """G_k follows the eigen system: types given first, and an eigen system replaced later."""
    m, m2 = gtr_model(), k80_like()
    eng = plk.Engine(0, 4, 2, 64, 6, 2, 1)
    rates, probs = phylo.gamma_rates(2, 0.5)
    eng.set_category_rates(rates, probs)
    eng.set_count_types(0, phylo.total_register(m.Q))
    eng.set_eigen(0, m.V, m.Vinv, m.lam)
    br = np.arange(3, dtype=np.int32)
    eng.update_count_matrices(br, TS[1:4])
    _check(eng, rates, br, TS[1:4], [m], [phylo.total_register(m.Q)])
    eng.set_eigen(0, m2.V, m2.Vinv, m2.lam)
    eng.set_count_types(0, phylo.total_register(m2.Q))
    eng.update_count_matrices(br, TS[1:4])
    _check(eng, rates, br, TS[1:4], [m2], [phylo.total_register(m2.Q)])


def test_count_matrices_per_branch_models():
    """A per-branch model list (non-homogeneous): every branch from its own eigen system and types."""
    ms = [gtr_model(), k80_like(), phylo.gtr(0.7, 1.4, 0.9, 0.5, 1.1, 0.2, 0.3, 0.3, 0.2)]
    Bs = [phylo.comprehensive_register(m.Q) for m in ms]
    eng, rates = _engine(4, 4, ms)
    for k, B in enumerate(Bs):
        eng.set_count_types(k, B)
    br = np.array([5, 0, 3, 1, 4, 2], dtype=np.int32)
    mi = np.array([2, 0, 1, 1, 0, 2], dtype=np.int32)
    eng.update_count_matrices(br, TS, mi)
    _check(eng, rates, br, TS, ms, Bs, mi)


def test_set_get_round_trip():
    rng = np.random.default_rng(4)
    eng, _ = _engine(4, 4, [gtr_model()])
    W = rng.uniform(0.0, 2.0, (12, 4, 4, 4))
    eng.set_count_matrix(3, W)
    assert np.array_equal(eng.get_count_matrix(3), W)
    W2 = rng.uniform(0.0, 2.0, (12, 4, 4, 4))
    eng.set_count_matrix(7, W2)
    assert np.array_equal(eng.get_count_matrix(3), W) and np.array_equal(eng.get_count_matrix(7), W2)
    with pytest.raises(plk.PlkError) as ei:
        eng.get_count_matrix(2)                              # never set
    assert ei.value.code == -5


def test_count_matrix_errors():
    m = gtr_model()
    eng, _ = _engine(4, 4, [m])
    br = np.arange(2, dtype=np.int32)
    with pytest.raises(plk.PlkError) as ei:
        eng.update_count_matrices(br, TS[:2])                # before any types
    assert ei.value.code == -5
    eng.set_count_types(0, phylo.total_register(m.Q))
    with pytest.raises(plk.PlkError) as ei:
        eng.set_count_types(0, phylo.comprehensive_register(m.Q))    # another T on the same handle
    assert ei.value.code == -1
    with pytest.raises(plk.PlkError) as ei:
        eng.set_count_matrix(0, np.zeros((12, 4, 4, 4)))
    assert ei.value.code == -1
    with pytest.raises(plk.PlkError) as ei:
        eng.update_count_matrices(np.array([99], dtype=np.int32), TS[:1])
    assert ei.value.code == -1
    with pytest.raises(plk.PlkError) as ei:
        eng.update_count_matrices(br, np.array([0.1, -1.0]))
    assert ei.value.code == -1
    eng2, _ = _engine(4, 4, [m, m])
    eng2.set_count_types(0, phylo.total_register(m.Q))
    with pytest.raises(plk.PlkError) as ei:
        eng2.update_count_matrices(br, TS[:2], np.array([0, 1], dtype=np.int32))     # model 1 has no types
    assert ei.value.code == -5
