"""An extended-range reference of lnL and its branch derivatives: one plain up-down pass in
IEEE 80-bit numpy.longdouble (64-bit mantissa, exponents down to 1e-4932), with no
rescaling and no normalisation anywhere.

Every other check of rescaled results compares the engine's 2^256 scheme with a restatement
of the same scheme (the oracle's), or one GPU implementation with another.  The numbers
here were never rescaled, so an error in the scale-count accounting that both sides share
cannot cancel.  From one pass: the per-pattern likelihood, lnL, d lnL/dt and d2 lnL/dt2 of
every branch, and the directional derivatives of a pair of root sons
(plk_root_pair_derivatives).

The transition matrices come from the caller ([n_nodes][C][S][S], the engine's own P, r dP,
r^2 d2P cast up), as everywhere in the suite the pruning is checked on identical P(t).
Plain numpy: broadcasting and sum, no BLAS (which has no longdouble).  Imports neither the
oracle nor the engine.  Checked by tests/test_xref_cpu.py before tests/test_gpu_xref.py
relies on it.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

LD = np.longdouble
_fi = np.finfo(LD)
assert _fi.machep <= -63 and _fi.maxexp >= 16384, \
    f"numpy.longdouble is not an 80-bit extended type here (machep {_fi.machep}, maxexp {_fi.maxexp})"

RANGE_MIN = LD("1e-4000")   # the range condition: no pattern's likelihood comes near the format's floor


def _ld(a):
    return np.asarray(a, dtype=LD)


def _apply(M, L):
    """M [C][S][S] on L [n][C][S] -> [n][C][S]: out[i,c,x] = sum_y M[c,x,y] L[i,c,y]."""
    return (M[None, :, :, :] * L[:, :, None, :]).sum(axis=3)


def _apply_t(M, F):
    """out[i,c,y] = sum_x F[i,c,x] M[c,x,y] (the father side carried down a branch)."""
    return (F[:, :, :, None] * M[None, :, :, :]).sum(axis=2)


def _prod(vs, n, C, S):
    acc = np.ones((n, C, S), dtype=LD)
    for v in vs:
        acc = acc * v
    return acc


def _lower(et, states, init_table, P):
    """Lower partials L_v and products q_v = P_v L_v, [n][C][S] each, unnormalised."""
    init = _ld(init_table)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    L, q = {}, {}
    for t in range(et.n_tips):
        L[t] = np.broadcast_to(init[states[t]][:, None, :], (n, C, S))
    for p, ch in et.ops:
        for c in ch:
            q[c] = _apply(P[c], L[c])
        L[p] = _prod([q[c] for c in ch], n, C, S)
    return L, q


def _site(probs, v):
    """<probs, v>: sum over classes and states of probs_c v[i,c,x] -> [n]."""
    return (v.sum(axis=2) * probs[None, :]).sum(axis=1)


def updown(et, states, init_table, P, dP, d2P, probs, pi, weights=None):
    """One up-down pass.  P, dP, d2P: [n_nodes][C][S][S] (dP, d2P may be None: lnL only).

    Returns a namespace with, per pattern, l and logl; lnl = sum w logl; per node b (0 at the
    root) d1[b] = sum w g_b and d2[b] = sum w (h_b - g_b^2), where
    g_b = <probs, F_b * (dP_b L_b)> / l and h_b likewise with d2P_b, F_b being the father
    side of the branch: U_father * prod of the other sons' q (pi for U at the root); and
    abs1[b] = sum w |g_b|, abs2[b] = sum w |h_b - g_b^2|, the magnitudes that were summed
    (a miss of the order of eps * abs is cancellation, a larger one is a wrong term)."""
    P, probs, pi = _ld(P), _ld(probs), _ld(pi)
    states = np.asarray(states)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    w = np.ones(n, dtype=LD) if weights is None else _ld(weights)
    L, q = _lower(et, states, init_table, P)
    l = _site(probs, L[et.root] * pi[None, None, :])
    assert l.min() > RANGE_MIN, f"a pattern likelihood of {l.min()} is outside the reference's range"
    logl = np.log(l)
    out = SimpleNamespace(l=l, logl=logl, lnl=(w * logl).sum(), weights=w)
    if dP is None:
        return out
    dP, d2P = _ld(dP), _ld(d2P)
    n_nodes = et.n_nodes
    d1, d2, abs1, abs2 = (np.zeros(n_nodes, dtype=LD) for _ in range(4))
    U = {et.root: np.broadcast_to(pi[None, None, :], (n, C, S))}
    for p, ch in reversed(et.ops):
        for c in ch:
            F = U[p] * _prod([q[o] for o in ch if o != c], n, C, S)
            g = _site(probs, F * _apply(dP[c], L[c])) / l
            h = _site(probs, F * _apply(d2P[c], L[c])) / l
            d1[c], d2[c] = (w * g).sum(), (w * (h - g * g)).sum()
            abs1[c], abs2[c] = (w * np.abs(g)).sum(), (w * np.abs(h - g * g)).sum()
            if c >= et.n_tips:
                U[c] = _apply_t(P[c], F)
        del U[p]
    out.d1, out.d2, out.abs1, out.abs2 = d1, d2, abs1, abs2
    return out


def root_pair_terms(et, states, init_table, P, dP, d2P, probs, pi, a, b):
    """Per pattern (l, l_a/l, l_b/l, l_aa/l, l_bb/l, l_ab/l) for two sons a, b of the root: the
    root product with dP or d2P substituted on a and / or b."""
    P, dP, d2P, probs, pi = _ld(P), _ld(dP), _ld(d2P), _ld(probs), _ld(pi)
    states = np.asarray(states)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    L, q = _lower(et, states, init_table, P)
    kids = [c for p, ch in et.ops if p == et.root for c in ch]
    assert a in kids and b in kids and a != b
    rest = pi[None, None, :] * _prod([q[o] for o in kids if o != a and o != b], n, C, S)
    qa = [q[a], _apply(dP[a], L[a]), _apply(d2P[a], L[a])]
    qb = [q[b], _apply(dP[b], L[b]), _apply(d2P[b], L[b])]
    l = _site(probs, rest * qa[0] * qb[0])
    assert l.min() > RANGE_MIN, f"a pattern likelihood of {l.min()} is outside the reference's range"
    return (l, _site(probs, rest * qa[1] * qb[0]) / l, _site(probs, rest * qa[0] * qb[1]) / l,
            _site(probs, rest * qa[2] * qb[0]) / l, _site(probs, rest * qa[0] * qb[2]) / l,
            _site(probs, rest * qa[1] * qb[1]) / l)


def root_pair(et, states, init_table, P, dP, d2P, probs, pi, a, b, alpha, beta, weights=None, terms=None):
    """(d lnL/ds, d2 lnL/ds2) along t_a + alpha s, t_b + beta s for two sons a, b of the root:
    g1 = alpha l_a/l + beta l_b/l, g2 = alpha^2 l_aa/l + 2 alpha beta l_ab/l + beta^2 l_bb/l;
    the sums of w g1 and w (g2 - g1^2).  terms: root_pair_terms of the same inputs, to share
    one pass among several (alpha, beta)."""
    if terms is None:
        terms = root_pair_terms(et, states, init_table, P, dP, d2P, probs, pi, a, b)
    l, la, lb, laa, lbb, lab = terms
    w = np.ones(len(l), dtype=LD) if weights is None else _ld(weights)
    alpha, beta = LD(alpha), LD(beta)
    g1 = alpha * la + beta * lb
    g2 = alpha * alpha * laa + 2 * alpha * beta * lab + beta * beta * lbb
    return (w * g1).sum(), (w * (g2 - g1 * g1)).sum()


def eigen_matrices(V, Vinv, lam, t, r):
    """(P, r dP/dt, r^2 d2P/dt2) [S][S] at length t and class rate r from the eigen system, in
    longdouble: V diag(e) Vinv with e = exp(lam r t), (r lam) e, (r lam)^2 e.  For the CPU
    self-checks of this module only (the GPU tests take the engine's matrices)."""
    V, Vinv, lam = _ld(V), _ld(Vinv), _ld(lam)
    rl = lam * LD(r)
    e = np.exp(rl * LD(t))

    def mat(d):
        return (V[:, None, :] * d[None, None, :] * Vinv.T[None, :, :]).sum(axis=2)

    return mat(e), mat(rl * e), mat(rl * rl * e)
