"""The reference count matrices of the substitution-mapping tests, checked on the CPU.

W^k(tau) = int_0^tau e^{Qs} B_k e^{Q(tau-s)} ds, the matrix plk_update_count_matrices forms
(W[x][y] = E[count of type k, end state y | start state x]).  Two independent formulations,
both numpy and both in this file:
  - Van Loan's block exponential (the reference of every test): expm([[Q, B_k], [0, Q]] tau)
    [:S, S:], with a small scaling-and-squaring Taylor expm (scipy may be absent);
  - the eigen formula V (J o (Vinv B_k V)) Vinv with
    J[i][j] = tau exp(max(l_i, l_j) tau) phi(-|l_i - l_j| tau), phi(z) = expm1(z) / z.
The largest difference between the two over the inputs below (GTR, a K80-like model whose
eigenvalues are an ulp apart, LG08; tau from 1e-6 to 10; the total and, for DNA, the
comprehensive register) is the reference's own floor.

Measured floor: 3.7e-14 (GTR 2.4e-14, K80-like 3.7e-14, LG08 1.5e-14, all at tau = 10 with
the total register, where max |W| is about 10; absolute).  The GPU tolerance for W is 10 x the
floor as reference_floor() measures it -- 3.7e-13 -- and not below 1e-13 * max(1, max |W|);
the 10 x is for the different summation order of the device's products.
"""
import functools

import numpy as np
import pytest

import phylo

TAUS = (1e-6, 1e-3, 0.1, 1.0, 10.0)


def _expm(A):
    """exp(A): scaling and squaring around a 24-term Taylor series (A may be a stack [..., n, n];
    the whole stack is scaled alike)."""
    A = np.asarray(A, dtype=np.float64)
    nrm = np.abs(A).sum(axis=-1).max()
    s = max(0, int(np.ceil(np.log2(nrm))) + 2) if nrm > 0 else 0
    X = A / 2.0 ** s
    E = np.broadcast_to(np.eye(A.shape[-1]), A.shape).copy()
    term = E.copy()
    for k in range(1, 25):
        term = term @ X / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def van_loan(Q, B, tau):
    """W^k(tau) for every type: [T, S, S]."""
    S = Q.shape[0]
    if tau == 0:
        return np.zeros((B.shape[0], S, S))
    A = np.zeros((B.shape[0], 2 * S, 2 * S))
    A[:, :S, :S] = Q
    A[:, S:, S:] = Q
    A[:, :S, S:] = B
    return _expm(A * tau)[:, :S, S:]


def eigen_counts(m, B, tau):
    """The same W from the eigen system, in the phi form."""
    lam = m.lam
    d = -np.abs(lam[:, None] - lam[None, :]) * tau
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(d == 0.0, 1.0, np.expm1(d) / np.where(d == 0.0, 1.0, d))
    J = tau * np.exp(np.maximum(lam[:, None], lam[None, :]) * tau) * phi
    return np.stack([m.V @ (J * (m.Vinv @ B[k] @ m.V)) @ m.Vinv for k in range(B.shape[0])])


def k80_like():
    """K80 through the numeric eigensolver, with the double eigenvalue split by exactly one
    ulp: what a solver may return, and fatal for (e_i - e_j) / (l_i - l_j) with an == 0 test."""
    m = phylo.gtr(1.0, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25)
    lam = m.lam.copy()
    order = np.argsort(lam)
    gaps = np.diff(lam[order])
    i = int(np.argmin(gaps))
    assert gaps[i] <= 1e-12 * abs(lam[order[i]])            # K80's double eigenvalue
    lam[order[i + 1]] = np.nextafter(lam[order[i]], 0.0)
    assert lam[order[i + 1]] != lam[order[i]]
    return phylo.Model("K80like", 4, m.Q, m.pi, m.V, m.Vinv, lam)


def gtr_model():
    return phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)


def _inputs():
    for m in (gtr_model(), k80_like()):
        yield m, phylo.total_register(m.Q)
        yield m, phylo.comprehensive_register(m.Q)
    m = phylo.lg08()
    yield m, phylo.total_register(m.Q)


@functools.lru_cache(maxsize=None)
def reference_floor():
    """max |Van Loan - eigen formula| over the inputs."""
    floor = 0.0
    for m, B in _inputs():
        for tau in TAUS:
            floor = max(floor, float(np.abs(van_loan(m.Q, B, tau) - eigen_counts(m, B, tau)).max()))
    return floor


def w_tolerance(W_ref):
    """The GPU tolerance for W: 10 x the reference's floor, not below 1e-13 max(1, max |W|)."""
    return max(10.0 * reference_floor(), 1e-13 * max(1.0, float(np.abs(W_ref).max())))


def test_van_loan_diagonal_blocks_are_P():
    for m, _ in _inputs():
        S = m.S
        for tau in TAUS:
            A = np.zeros((2 * S, 2 * S))
            A[:S, :S] = m.Q
            A[S:, S:] = m.Q
            A[:S, S:] = phylo.total_register(m.Q)[0]
            E = _expm(A * tau)
            P = (m.V * np.exp(m.lam * tau)) @ m.Vinv
            assert np.abs(E[:S, :S] - P).max() <= 1e-13
            assert np.abs(E[S:, S:] - P).max() <= 1e-13
            assert np.abs(E[S:, :S]).max() == 0.0


def test_expected_total_count_at_stationarity_is_tau():
    """pi^T W_total 1 = tau for a normalised reversible Q."""
    for m in (gtr_model(), k80_like(), phylo.lg08()):
        for tau in TAUS:
            W = van_loan(m.Q, phylo.total_register(m.Q), tau)[0]
            assert abs(m.pi @ W @ np.ones(m.S) - tau) <= 1e-13 * max(1.0, tau)


def test_two_formulations_agree():
    floor = reference_floor()
    print(f"reference floor (Van Loan vs eigen formula): {floor:.3g}")
    for m, B in _inputs():
        worst = max(np.abs(van_loan(m.Q, B, tau) - eigen_counts(m, B, tau)).max() for tau in TAUS)
        print(f"  {m.name} T={B.shape[0]}: {worst:.3g}")
    assert floor <= 1e-12          # two double-precision formulations of numbers <= ~10
    m = k80_like()
    W = eigen_counts(m, phylo.total_register(m.Q), 1.0)
    assert np.isfinite(W).all() and W.min() >= -1e-15


def test_count_matrices_are_nonnegative_and_zero_at_zero():
    for m, B in _inputs():
        assert np.all(van_loan(m.Q, B, 0.0) == 0.0)
        assert np.all(eigen_counts(m, B, 0.0) == 0.0)
        for tau in TAUS:
            assert van_loan(m.Q, B, tau).min() >= -1e-15


@pytest.mark.parametrize("model", [gtr_model, k80_like, phylo.lg08])
def test_register_helpers(model):
    m = model()
    tot = phylo.total_register(m.Q)
    assert tot.shape == (1, m.S, m.S) and np.all(np.diag(tot[0]) == 0.0)
    off = ~np.eye(m.S, dtype=bool)
    assert np.array_equal(tot[0][off], m.Q[off])
    comp = phylo.comprehensive_register(m.Q)
    assert comp.shape == (m.S * (m.S - 1), m.S, m.S)
    assert np.all((comp != 0).sum(axis=(1, 2)) <= 1)                  # one cell per type
    assert np.array_equal(comp.sum(axis=0), tot[0])                   # the types sum to the total B
    # numbered row by row: type k is the k-th ordered pair x != y
    pairs = [(x, y) for x in range(m.S) for y in range(m.S) if x != y]
    for k in (0, 1, len(pairs) - 1):
        assert comp[k][pairs[k]] == m.Q[pairs[k]]
