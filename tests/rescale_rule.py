"""The 2^256 rescaling rule of PLK_FLAG_SCALING restated in numpy, in fp64 like the engine, so
that it reports where a running product reaches a denormal number or 0.0 (the extended-range
reference of tests/xref.py never does, and cannot say).

Two rules, on the same walk over et.ops:

  stored_once  the rule up to now: at a check point the vector is multiplied by 2^256 once where
               its joint maximum over classes and states is positive and below 2^-256.
               fused=True checks once per node (the fused traversals: tree4, treeM and the
               generated kernels), fused=False after every three sons and at the node's end
               (the levelwise ACCUMULATE ops and the links kernels).
  stored_new   every check steps until the joint maximum is back in [2^-256, 1); the sons are
               taken three at a time, with a check after each group, at the node's end and, in
               every group but the first, after the group's second son (there the carried
               product is already one factor), so that at most three stored vectors enter a
               running product between two checks.

On nodes of up to three sons the two rules check at the same point, the node's end, and differ
in the step alone.  Every traversal path checks at stored_new's points (csrc/plk_tree4.hpp:
scale_check_after), so stored values and counts agree across them.

The stored U of a non-root node is the father side of its branch formed from the stored
vectors (pi in the place of U at the root), brought down its branch, checked once.  The fused
preorder (fathers of up to three sons) takes the exponents out of the factors first, so the
product is formed here in longdouble and then stored as a double: what is lost is lost in the
store.  A wider father goes through the levelwise ops; under the new rule they are checked
like the lower pass, and what they store is the product brought into range.

Checked by tests/test_xref_cpu.py before the GPU tests rely on it.
"""
from types import SimpleNamespace

import numpy as np

import xref

LD = np.longdouble
THR = 2.0 ** -256
UP = 2.0 ** 256
NORMAL_MIN = 2.0 ** -1022


def check_points(n_sons, new, fused=True):
    """The 1-based son indices after which the running product of a node is checked."""
    pts = {n_sons}
    if new or not fused:
        pts |= set(range(3, n_sons + 1, 3))
    if new:
        pts |= set(range(5, n_sons + 1, 3))
    return pts


def _check(run, cnt, new):
    """One check of run [n][C][S] (in place): once, or until in range."""
    while True:
        m = run.max(axis=(1, 2))
        r = (m > 0) & (m < THR)
        if not r.any():
            return
        run[r] *= UP
        cnt[r] += 1
        if not new:
            return


def _walk(et, states, init_table, P, pi, new, fused):
    P = np.asarray(P, dtype=np.float64)
    states = np.asarray(states)
    init = np.asarray(init_table, dtype=np.float64)
    n, C, S = states.shape[1], P.shape[1], P.shape[2]
    L = {t: np.broadcast_to(init[states[t]][:, None, :], (n, C, S)) for t in range(et.n_tips)}
    k = {t: np.zeros(n, dtype=np.int64) for t in range(et.n_tips)}
    q = {}
    low = np.full(n, np.inf)     # the smallest joint maximum a running product went through
    for p, ch in et.ops:
        run, cnt = np.ones((n, C, S)), np.zeros(n, dtype=np.int64)
        pts = check_points(len(ch), new, fused)
        for i, c in enumerate(ch, 1):
            q[c] = np.einsum("cxy,ncy->ncx", P[c], L[c])
            run = run * q[c]
            cnt = cnt + k[c]
            low = np.minimum(low, run.max(axis=(1, 2)))
            if i in pts:
                _check(run, cnt, new)
        L[p], k[p] = run, cnt
    # the upper pass
    piL = xref._ld(pi)
    U = {}
    for p, ch in reversed(et.ops):
        above = np.broadcast_to(piL[None, None, :], (n, C, S)) if p == et.root else xref._apply_t(xref._ld(P[p]), xref._ld(U[p]))
        for c in ch:
            if c < et.n_tips:
                continue
            F = above * xref._prod([xref._ld(q[o]) for o in ch if o != c], n, C, S)
            if new and len(ch) > 3:
                # a wider father goes through the levelwise ops, checked like the lower pass:
                # what they store is this product brought into range
                m = F.max(axis=(1, 2))
                while ((m > 0) & (m < THR)).any():
                    r = (m > 0) & (m < THR)
                    F[r] *= LD(UP)
                    m = F.max(axis=(1, 2))
            with np.errstate(under="ignore"):
                u = F.astype(np.float64)
            low = np.minimum(low, u.max(axis=(1, 2)))
            _check(u, np.zeros(n, dtype=np.int64), new)
            U[c] = u
    mx = lambda d: {v: a.max(axis=(1, 2)) for v, a in d.items()}
    return SimpleNamespace(L=L, k=k, U=U, low=low, Lmax=mx(L), Umax=mx(U), new=new, fused=fused)


def stored_once(et, states, init_table, P, pi, fused):
    """The vectors as the engine stored them up to now.  Returns L and U {node: [n][C][S]} in
    fp64, the scale counts k {node: [n]}, the joint maxima Lmax and Umax {node: [n]}, and low
    [n]: the smallest joint maximum that a running product (or a U at its store) went through."""
    return _walk(et, states, init_table, P, pi, False, fused)


def stored_new(et, states, init_table, P, pi):
    """The same under the rule "step until in range, at most three factors between checks"."""
    return _walk(et, states, init_table, P, pi, True, True)


def lost_lower(st, et):
    """Per pattern: the root partial is all zero."""
    return st.Lmax[et.root] == 0.0


def lost_upper(st):
    """Per pattern: the stored U of some node is all zero."""
    return np.any([m == 0.0 for m in st.Umax.values()], axis=0)


def in_range(st, et):
    """Every stored joint maximum of an internal node's L and U lies in [2^-256, 1]."""
    return all(np.all((m >= THR) & (m <= 1.0)) for v, m in list(st.Lmax.items()) + list(st.Umax.items())
               if v >= et.n_tips)


def scaled_reference(L_ref, k):
    """The reference's longdouble vector times 2^(256 k) per pattern (exact)."""
    return L_ref * (LD(2) ** (256 * k.astype(np.int64)).astype(LD))[:, None, None]
