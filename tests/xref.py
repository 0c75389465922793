"""An extended-range reference of lnL and its branch derivatives: one plain up-down pass in
IEEE 80-bit numpy.longdouble (64-bit mantissa, exponents down to 1e-4932), with no
rescaling and no normalisation anywhere.

Every other check of rescaled results compares the engine's 2^256 scheme with a restatement
of the same scheme (the oracle's), or one GPU implementation with another.  The numbers
here were never rescaled, so an error in the scale-count accounting that both sides share
cannot cancel.  From one pass: the per-pattern likelihood, lnL, d lnL/dt and d2 lnL/dt2 of
every branch, and the directional derivatives of a pair of root sons
(plk_root_pair_derivatives).  From the same lower partials and father sides, the three
consumers of the engine's stored L and U: node posteriors (posteriors: plk_node_posteriors),
expected substitution counts (branch_counts: plk_branch_counts) and NNI scores with their
per-pattern rows (nni: plk_nni_scores, plk_nni_site_rows), the last by a plain lower pass of
the swapped topology, with nothing of the engine's gamma / eigen formulation in it.

The transition matrices come from the caller ([n_nodes][C][S][S], the engine's own P, r dP,
r^2 d2P cast up; the count matrices W likewise), as everywhere in the suite the pruning is
checked on identical P(t); only the trial matrices of an NNI move's branch, which the engine
never stores, come from eigen_matrices.  Plain numpy: broadcasting and sum, no BLAS (which has
no longdouble).  Imports neither the oracle nor the engine.  Checked by tests/test_xref_cpu.py
before tests/test_gpu_xref.py (groups A to D) and tests/test_gpu_xref_consumers.py (groups E to
H) rely on it.
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


def eigen_matrices(V, Vinv, lam, t, r, unit=False):
    """(P, r dP/dt, r^2 d2P/dt2) [S][S] at length t and class rate r from the eigen system, in
    longdouble: V diag(e) Vinv with e = exp(lam r t), (r lam) e, (r lam)^2 e.  For the CPU
    self-checks of this module and for the trial matrices of an NNI move (the GPU tests take
    the engine's matrices for every stored branch).

    unit: P = I + V diag(expm1(lam r t)) Vinv, the form whose limit at t = 0 is the identity
    whatever V Vinv is.  An eigen system held in doubles has V Vinv = I + D with D of the order
    of 1e-15; V diag(e) Vinv carries D at every t.  Where the two sides of an NNI move
    disagree the likelihood at short t is a sum of large terms that cancel, and D, harmless in
    P itself, was measured at 7e-11 weight sums in d1 at t = 1e-6 on 64 states
    (tests/test_xref_cpu.py).  The engine's short-length form (csrc/plk_nni.hpp) is the unit
    form."""
    V, Vinv, lam = _ld(V), _ld(Vinv), _ld(lam)
    rl = lam * LD(r)
    e = np.exp(rl * LD(t))

    def mat(d):
        return (V[:, None, :] * d[None, None, :] * Vinv.T[None, :, :]).sum(axis=2)

    P = np.eye(len(lam), dtype=LD) + mat(np.expm1(rl * LD(t))) if unit else mat(e)
    return P, mat(rl * e), mat(rl * rl * e)


# ---------------------------------------------------------------- the consumers of L and U

def _father_sides(et, q, pi, P, n, C, S, want):
    """F_v = U_father * prod of the other sons' q for the non-root nodes v in `want`, and
    up_v = pi at the root, else F_v carried down P_v, for the internal nodes in `want`."""
    want = set(int(v) for v in want)
    F, up = {}, {}
    U = {et.root: np.broadcast_to(pi[None, None, :], (n, C, S))}
    if et.root in want:
        up[et.root] = U[et.root]
    for p, ch in reversed(et.ops):
        for c in ch:
            Fc = U[p] * _prod([q[o] for o in ch if o != c], n, C, S)
            if c in want:
                F[c] = Fc
            if c >= et.n_tips:
                U[c] = _apply_t(P[c], Fc)
                if c in want:
                    up[c] = U[c]
        del U[p]
    return F, up


def lower(et, states, init_table, P):
    """(L, q) of _lower on P cast up: hand it to posteriors, branch_counts and nni as lower=
    to share one lower pass among them (the same et, states, init_table and P)."""
    return _lower(et, np.asarray(states), init_table, _ld(P))


def posteriors(et, states, init_table, P, probs, pi, nodes, lower=None):
    """Marginal posteriors of the internal nodes `nodes`: joint [node][n][C][S] =
    p_c L_v[x] up_v[x] / l with up_v = pi at the root, otherwise the father side carried down
    P_v; states = its sum over classes, classes = its sum over states, best = the lowest index
    among the maxima of states.  Also l and logl per pattern."""
    P, probs, pi = _ld(P), _ld(probs), _ld(pi)
    states = np.asarray(states)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    L, q = _lower(et, states, init_table, P) if lower is None else lower
    l = _site(probs, L[et.root] * pi[None, None, :])
    assert l.min() > RANGE_MIN, f"a pattern likelihood of {l.min()} is outside the reference's range"
    _, up = _father_sides(et, q, pi, P, n, C, S, nodes)
    joint = np.stack([probs[None, :, None] * L[int(v)] * up[int(v)] / l[:, None, None] for v in nodes])
    st = joint.sum(axis=2)
    return SimpleNamespace(l=l, logl=np.log(l), joint=joint, states=st, classes=joint.sum(axis=3),
                           best=st.argmax(axis=2))


def branch_counts(et, states, init_table, P, W, probs, pi, branches, weights=None, lower=None):
    """Expected substitution counts: counts [branch][n][type] = n_k / l, n_k the root sum with
    W[v][k] [C][S][S] in the place of P_v (lnL is linear in one branch's matrix); totals
    [branch][type] their weighted sums.  W: indexable by node, each [T][C][S][S]."""
    P, probs, pi = _ld(P), _ld(probs), _ld(pi)
    states = np.asarray(states)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    w = np.ones(n, dtype=LD) if weights is None else _ld(weights)
    L, q = _lower(et, states, init_table, P) if lower is None else lower
    l = _site(probs, L[et.root] * pi[None, None, :])
    assert l.min() > RANGE_MIN, f"a pattern likelihood of {l.min()} is outside the reference's range"
    F, _ = _father_sides(et, q, pi, P, n, C, S, branches)
    out = []
    for v in branches:
        Wv = _ld(W[int(v)])
        out.append(np.stack([_site(probs, F[int(v)] * _apply(Wv[k], L[int(v)])) / l for k in range(Wv.shape[0])], axis=1))
    counts = np.stack(out)
    return SimpleNamespace(l=l, logl=np.log(l), counts=counts, totals=(w[None, :, None] * counts).sum(axis=1))


def trial_matrices(V, Vinv, lam, t, rates):
    """eigen_matrices at (t, r_c) for every class, P in the unit form: (P, r dP, r^2 d2P),
    [C][S][S] each."""
    m = [eigen_matrices(V, Vinv, lam, t, r, unit=True) for r in rates]
    return tuple(np.stack([x[k] for x in m]) for k in range(3))


def nni(et, states, init_table, P, probs, pi, moves, P_t, dP_t, d2P_t, weights=None, swap=None, lower=None):
    """NNI moves (son s, uncle u): p = father(s), g = father(p); s and u change places (each
    keeps its own branch) and branch p gets the trial matrices P_t[i] [C][S][S] of move i.
    Per move a plain lower pass of the swapped topology (the subtrees the move leaves alone
    keep their L; p and its ancestors are formed again from their new son lists), once with
    P_t, once with dP_t and once with d2P_t on branch p: l_sw, l_sw', l_sw''.  Returns per
    move and pattern log_rho = log l_sw - log l_cur, g = rho'/rho, h = rho''/rho, and per move
    delta = sum w log_rho, d1 = sum w g, d2 = sum w (h - g^2), abs0 / abs1 / abs2 the
    magnitudes that were summed.  swap: the son lists after a move, {father: sons} from
    (sons, par, s, u); the default swaps in both lists (a hook for planting errors)."""
    P, probs, pi = _ld(P), _ld(probs), _ld(pi)
    states = np.asarray(states)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    w = np.ones(n, dtype=LD) if weights is None else _ld(weights)
    L, q = _lower(et, states, init_table, P) if lower is None else lower
    l_cur = _site(probs, L[et.root] * pi[None, None, :])
    assert l_cur.min() > RANGE_MIN, f"a pattern likelihood of {l_cur.min()} is outside the reference's range"
    sons = {p: list(ch) for p, ch in et.ops}
    par = {c: p for p, ch in et.ops for c in ch}
    swap = _swapped_sons if swap is None else swap
    m = len(moves)
    log_rho, g, h = (np.zeros((m, n), dtype=LD) for _ in range(3))
    for i, (s, u) in enumerate(moves):
        s, u = int(s), int(u)
        p = par[s]
        assert p != et.root and u in sons[par[p]] and u != p
        new = swap(sons, par, s, u)

        def kids(f):
            return new.get(f, sons[f])

        Lp = _prod([q[o] for o in kids(p)], n, C, S)
        # the three passes side by side: [3 n][C][S], the untouched sons' q repeated
        v, qv = p, np.concatenate([_apply(_ld(M), Lp) for M in (P_t[i], dP_t[i], d2P_t[i])])
        while True:
            f = par[v]
            rest = _prod([q[o] for o in kids(f) if o != v], n, C, S)
            Lf = qv * np.concatenate([rest, rest, rest])
            if f == et.root:
                break
            v, qv = f, _apply(P[f], Lf)
        ls = _site(probs, Lf * pi[None, None, :]).reshape(3, n)
        assert ls[0].min() > RANGE_MIN, f"a swapped-tree likelihood of {ls[0].min()} is outside the reference's range"
        log_rho[i], g[i], h[i] = np.log(ls[0]) - np.log(l_cur), ls[1] / ls[0], ls[2] / ls[0]
    c2 = h - g * g
    return SimpleNamespace(l=l_cur, logl=np.log(l_cur), log_rho=log_rho, g=g, h=h,
                           delta=(w * log_rho).sum(axis=1), d1=(w * g).sum(axis=1), d2=(w * c2).sum(axis=1),
                           abs0=(w * np.abs(log_rho)).sum(axis=1), abs1=(w * np.abs(g)).sum(axis=1),
                           abs2=(w * np.abs(c2)).sum(axis=1))


def _swapped_sons(sons, par, s, u):
    p = par[s]
    g = par[p]
    return {p: [u if o == s else o for o in sons[p]], g: [s if o == u else o for o in sons[g]]}
