"""NNI scoring, restated in numpy (no engine): the formulas and the Newton rule of
plk_nni_scores (include/plk.h), checked against plain pruning of the swapped tree.

A move is (son s, uncle u); p = father(s), g = father(p); s and u change places and branch p
gets the length t.  Per pattern and class, with q_v = P_v L_v,

    up_g = pi at the root, else (up_f prod_{siblings o of g} q_o) P_g        (state at g from above)
    A1 = up_g q_s prod_{o son of g, o not p, u} q_o      A2 = q_u prod_{o son of p, o not s} q_o
    B1 = up_g q_u prod_o q_o                             B2 = q_s prod_o q_o
    l_cur = sum_c p_c B1^T P_p B2
    gamma[c][k] = p_c (A1^T V)[k] (Vinv A2)[k] / l_cur
    rho(t) = sum_ck gamma[c][k] exp(lambda_k r_c t),   Delta(t) = sum_p w_p log rho(t)

and d1, d2 the derivatives of Delta in t.  While t max|lambda r| <= 1, rho is summed as
d + sum gamma expm1(lambda r t) with d = sum_c p_c A1 . A2 / l_cur (= sum gamma, formed without
a subtraction), as the engine does: where the two sides of a move disagree rho is small against
the gamma it is summed from, and the plain sum loses digits that d keeps.  The Newton rule's
F(t') >= F(t) is decided on F(t') - F(t) summed per pattern (evaluate), again as the engine does.
The reference is oracle.tree_loglik on the swapped son arrays with P_p = V exp(lambda r t) Vinv,
minus its value on the current tree: nothing of the restatement is in it.

Tolerances.  Delta: 1e-12 of the weight sum -- both sides are sums of w log(l) whose terms carry
a few ulps each (lnL per unit weight is O(10)), so the floor is ~1e-14; measured 2.9e-15 here.
d1, d2: against fourth-order central differences of the reference's Delta with the relative
step h = 0.01 t, compared as t d1 and t^2 d2 per unit weight; truncation ~h^4 = 1e-8 times a
moderate derivative ratio, rounding 1e-14 / h = 1e-12 (d1) and 1e-14 / h^2 = 1e-10 (d2): bounds
1e-6 and 1e-5.  Measured here: 1.8e-10 and 1.9e-10.

The GPU tests (test_gpu_nni.py) import this module as their Newton reference.
"""
import numpy as np
import pytest

import oracle
import phylo


# ---------------------------------------------------------------- trees and moves

def sons_of(ops):
    sons = {}
    for p, ch in ops:
        sons.setdefault(p, []).extend(ch)
    return sons


def parents_of(ops):
    return {c: p for p, ch in ops for c in ch}


def eligible_moves(ops, root):
    """Every (son, uncle) of the tree: the son's father is not the root; fathers and
    grandfathers of more than three sons are left out (the engine does not serve them)."""
    sons, par = sons_of(ops), parents_of(ops)
    out = []
    for s in sorted(par):
        p = par[s]
        if p == root:
            continue
        g = par[p]
        if len(sons[p]) > 3 or len(sons[g]) > 3:
            continue
        out += [(s, u) for u in sons[g] if u != p]
    return out


def reference_uncle(ops, root, s):
    """The uncle NNIHomogeneousTreeLikelihood::testNNI picks for the node s."""
    sons, par = sons_of(ops), parents_of(ops)
    p = par[s]
    g = par[p]
    pos = sons[g].index(p)
    return sons[g][0 if pos > 1 else 1 - pos]


def swap_ops(ops, s, u):
    """The op list of the tree after the move (s, u); fathers keep their place in the list."""
    par = parents_of(ops)
    p, g = par[s], par[par[s]]
    out = []
    for f, ch in ops:
        ch = list(ch)
        if f == p:
            ch[ch.index(s)] = u
        elif f == g:
            ch[ch.index(u)] = s
        out.append((f, tuple(ch)))
    return out


def postorder_ops(ops, root):
    """`ops` ordered so that every node follows its sons (a swap can break the order)."""
    sons = sons_of(ops)
    out = []

    def walk(n):
        if n in sons:
            for c in sons[n]:
                walk(c)
            out.append((n, tuple(sons[n])))
    walk(root)
    return out


def son_arrays(ops, n_nodes, n_tips):
    sons = sons_of(ops)
    start = np.zeros(n_nodes + 1, dtype=np.int32)
    for i in range(n_nodes):
        start[i + 1] = start[i] + len(sons.get(i, []))
    flat = np.array([c for i in range(n_nodes) for c in sons.get(i, [])], dtype=np.int32)
    leaf_row = np.array([i if i < n_tips else -1 for i in range(n_nodes)], dtype=np.int32)
    return start, flat, leaf_row


def caterpillar(n, seed=3, lo=0.02, hi=0.2):
    rng = np.random.default_rng(seed)
    s = "t0:%.4f" % rng.uniform(lo, hi)
    for i in range(1, n - 1):
        s = "(%s,t%d:%.4f):%.4f" % (s, i, rng.uniform(lo, hi), rng.uniform(lo, hi))
    return phylo.Tree.from_newick("(%s,t%d:%.4f);" % (s, n - 1, rng.uniform(lo, hi)))


def random_join(n, seed, lo=0.02, hi=0.4):
    """A random rooted binary tree: subtrees joined two at a time."""
    rng = np.random.default_rng(seed)
    parts = [f"t{i}" for i in range(n)]
    while len(parts) > 1:
        i, j = sorted(rng.choice(len(parts), size=2, replace=False), reverse=True)
        a, b = parts.pop(int(i)), parts.pop(int(j))
        parts.append("(%s:%.5f,%s:%.5f)" % (a, rng.uniform(lo, hi), b, rng.uniform(lo, hi)))
    return phylo.Tree.from_newick(parts[0] + ";")


TRIFURCATING9 = ("((a:0.11,b:0.07):0.05,((c:0.21,d:0.03):0.08,e:0.3):0.04,"
                 "((f:0.02,g:0.09):0.12,(h:0.15,i:0.06):0.07):0.1);")


def tree_by_name(name):
    """EngineTree of the test trees: balanced8 and join12 are unrooted by engine_tree (a
    three-son root), caterpillar7 keeps its two-son root, trifurcating9 is given unrooted."""
    if name == "balanced8":
        return phylo.engine_tree(phylo.balanced_tree(8, seed=8, lo=0.02, hi=0.3))
    if name == "caterpillar7":
        return phylo.engine_tree(caterpillar(7), unroot=False)
    if name == "trifurcating9":
        return phylo.engine_tree(phylo.Tree.from_newick(TRIFURCATING9))
    if name == "join12":
        return phylo.engine_tree(random_join(12, seed=12))
    if name == "join12s20":
        return phylo.engine_tree(random_join(12, seed=20))
    raise KeyError(name)


# ---------------------------------------------------------------- the restatement

def _q(P, L, v):
    return np.einsum("cxy,pcy->pcx", P[v], L[v])


def lower_partials(ops, n_tips, states, init_table, P):
    """Unnormalised L of every node, [pattern, class, state]."""
    C = P.shape[1]
    L = {i: np.repeat(init_table[states[i]][:, None, :], C, axis=1) for i in range(n_tips)}
    for f, ch in ops:
        acc = 1.0 if f not in L else L[f]
        for c in ch:
            acc = acc * _q(P, L, c)
        L[f] = acc
    return L


def up_vectors(ops, root, L, P, pi):
    """up_v[pattern, class, x] of every internal node: the state at v seen from above v."""
    sons = sons_of(ops)
    n_pat, C, S = L[root].shape
    up = {root: np.broadcast_to(pi[None, None, :], (n_pat, C, S))}
    order = []
    for f, _ in ops:
        if f not in order:
            order.append(f)
    for f in reversed(order):
        for c in sons[f]:
            if c not in sons:
                continue
            u = up[f]
            for o in sons[f]:
                if o != c:
                    u = u * _q(P, L, o)
            up[c] = np.einsum("pcy,cyx->pcx", u, P[c])
    return up


def move_coefficients(ops, L, up, P, probs, V, Vinv, s, u):
    """gamma[pattern, class, k] and d[pattern] = sum_c p_c A1 . A2 of the move (s, u), divided by
    l_cur; a pattern whose l_cur is not a positive finite number gets zeros."""
    sons, par = sons_of(ops), parents_of(ops)
    p = par[s]
    g = par[p]
    base1 = up[g]
    for o in sons[g]:
        if o not in (p, u):
            base1 = base1 * _q(P, L, o)
    base2 = 1.0
    for o in sons[p]:
        if o != s:
            base2 = base2 * _q(P, L, o)
    qs, qu = _q(P, L, s), _q(P, L, u)
    A1, A2, B1, B2 = base1 * qs, qu * base2, base1 * qu, qs * base2
    l_cur = np.einsum("c,pcx,cxy,pcy->p", probs, B1, P[p], B2)
    gam = probs[None, :, None] * np.einsum("pcx,xk->pck", A1, V) * np.einsum("ky,pcy->pck", Vinv, A2)
    ok = (l_cur > 0) & np.isfinite(l_cur)
    d = np.einsum("c,pcx,pcx->p", probs, A1, A2)
    inv = np.where(ok, 1.0 / np.where(ok, l_cur, 1.0), 0.0)
    return gam * inv[:, None, None], d * inv


def _rho(gam, d, mu, t):
    """sum gamma exp(mu t) per pattern, in the short-length form while t max|mu| <= 1."""
    if t * np.abs(mu).max() <= 1.0:
        return np.einsum("pck,ck->p", gam, np.expm1(mu * t)) + d
    return np.einsum("pck,ck->p", gam, np.exp(mu * t))


def evaluate(gam, d, lam, rates, w, t, t_acc=None):
    """(Delta, d1, d2) of one move at the length t, and Delta(t) - Delta(t_acc) summed per pattern
    as w log1p((rho(t) - rho(t_acc)) / rho(t_acc)) with rho(t) - rho(t_acc) =
    sum gamma exp(mu t_acc) expm1(mu (t - t_acc)): the Newton rule's F(t') >= F(t) is decided on
    it, since near the optimum the two sums of logs differ by less than their rounding."""
    mu = rates[:, None] * lam[None, :]
    e = np.exp(mu * t)
    d0 = d
    r0 = _rho(gam, d0, mu, t)
    r1 = np.einsum("pck,ck->p", gam, e * mu)
    r2 = np.einsum("pck,ck->p", gam, e * mu * mu)
    ok = (r0 > 0) & np.isfinite(r0)
    d = np.where(ok, r0, 1.0)
    g1, g2 = np.where(ok, r1 / d, 0.0), np.where(ok, r2 / d, 0.0)
    out = (float(np.sum(w * np.log(d))), float(np.sum(w * g1)), float(np.sum(w * (g2 - g1 * g1))))
    if t_acc is None:
        return out
    ra = _rho(gam, d0, mu, t_acc)
    dr = np.einsum("pck,ck->p", gam, np.exp(mu * t_acc) * np.expm1(mu * (t - t_acc)))
    ok_a = ok & (ra > 0) & np.isfinite(ra)
    q = np.where(ok_a, dr / np.where(ok_a, ra, 1.0), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        dl = np.where(q > -0.5, np.log1p(np.maximum(q, -0.5)), np.log(np.where(ok_a, r0 / np.where(ok_a, ra, 1.0), 1.0)))
    return out + (float(np.sum(w * np.where(ok_a, dl, 0.0))),)


def newton(evals, t0, t_min=1e-6, t_max=100.0, tol=1e-8, max_iter=0):
    """The safeguarded Newton ascent of plk_nni_scores over the moves in lockstep.
    evals[i](t) -> (F, d1, d2).  Returns a dict as Engine.nni_scores does."""
    n = len(evals)
    pt = np.array(t0, dtype=np.float64)
    val = [evals[i](pt[i])[:3] for i in range(n)]
    F, D1, D2 = (np.array([v[k] for v in val]) for k in range(3))
    trial, half, status = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int32)
    act, passes, it = list(range(n)), 1, 0
    while max_iter > 0:
        nxt = []
        for i in act:
            t = pt[i]
            if half[i]:
                tp = 0.5 * (t + trial[i])
            elif D2[i] < 0.0:
                tp = t - D1[i] / D2[i]
            else:
                tp = 2.0 * t if D1[i] > 0.0 else 0.5 * t
            tp = t if tp != tp else min(max(tp, t_min), t_max)
            if abs(tp - t) <= tol * max(t, t_min):
                continue
            trial[i] = tp
            nxt.append(i)
        act = nxt
        if not act:
            break
        if it == max_iter:
            status[act] = 1
            break
        passes += 1
        it += 1
        for i in act:
            _, a, b, dF = evals[i](trial[i], pt[i])
            if dF >= 0.0:          # F(t') >= F(t), on the change summed per pattern
                pt[i], F[i], D1[i], D2[i], half[i] = trial[i], F[i] + dF, a, b, False
            else:
                half[i] = True
    return {"t_opt": pt, "delta": F, "d1": D1, "d2": D2, "status": status, "passes": passes}


class Restatement:
    """All moves of one problem: P [n_nodes, C, S, S] (the root's entry is not read)."""

    def __init__(self, ops, root, n_tips, states, init_table, P, rates, probs, pi, model, weights=None):
        self.ops, self.root, self.P, self.rates, self.probs, self.model = ops, root, P, rates, probs, model
        self.w = np.ones(states.shape[1]) if weights is None else np.asarray(weights, dtype=np.float64)
        self.L = lower_partials(ops, n_tips, states, init_table, P)
        self.up = up_vectors(ops, root, self.L, P, pi)

    def coefficients(self, s, u):
        return move_coefficients(self.ops, self.L, self.up, self.P, self.probs, self.model.V, self.model.Vinv, s, u)

    def evaluator(self, s, u):
        gam, d = self.coefficients(s, u)
        return lambda t, t_acc=None: evaluate(gam, d, self.model.lam, self.rates, self.w, t, t_acc)

    def scores(self, moves, t0, **kw):
        return newton([self.evaluator(s, u) for s, u in moves], t0, **kw)


# ---------------------------------------------------------------- the reference: plain pruning

class Pruning:
    """lnL of the current and of any swapped tree from the oracle, on the given P."""

    def __init__(self, et_ops, root, n_nodes, n_tips, states, init_table, P, rates, probs, pi, model, weights=None,
                 scaling=False):
        self.ops, self.root, self.n_nodes, self.n_tips = et_ops, root, n_nodes, n_tips
        self.states, self.table, self.P, self.rates, self.probs, self.pi = states, init_table, P, rates, probs, pi
        self.model, self.scaling = model, scaling
        self.w = np.ones(states.shape[1]) if weights is None else np.asarray(weights, dtype=np.float64)
        self.cur = self.lnl(et_ops, P)

    def lnl(self, ops, P):
        ss, sons, lr = son_arrays(ops, self.n_nodes, self.n_tips)
        _, site, _, _ = oracle.tree_loglik(ss, sons, lr, self.root, self.states, self.table, P, self.probs, self.pi,
                                           use_patterns=False, scaling=self.scaling, want_sites=True)
        return float(np.sum(self.w * site))

    def delta(self, s, u, t):
        p = parents_of(self.ops)[s]
        P = self.P.copy()
        P[p] = np.stack([self.model.pij(r * t) for r in self.rates])
        return self.lnl(swap_ops(self.ops, s, u), P) - self.cur


# ---------------------------------------------------------------- the tests

def _problem(tree, C, n_pat, seed, weighted=True):
    et = tree_by_name(tree)
    rng = np.random.default_rng(seed)
    m = phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5))
    rates, probs = phylo.gamma_rates(C, 0.5)
    states = phylo.simulate(et, [m], None, rates, n_pat, seed=seed).astype(np.int32)
    w = rng.integers(1, 9, n_pat).astype(np.float64) if weighted else None
    P = np.zeros((et.n_nodes, C, 4, 4))
    for v in range(et.n_nodes):
        if v != et.root:
            P[v] = np.stack([m.pij(r * et.brlen[v]) for r in rates])
    P[et.root] = np.eye(4)[None]
    return et, m, rates, probs, states, w, P


CASES = [("balanced8", 1, 300, 1), ("caterpillar7", 2, 300, 2), ("trifurcating9", 4, 300, 3), ("join12", 4, 450, 4)]


def _stencils(f, t, h):
    v = [f(t + k * h) for k in (-2, -1, 0, 1, 2)]
    d1 = (v[0] - 8 * v[1] + 8 * v[3] - v[4]) / (12 * h)
    d2 = (-v[0] + 16 * v[1] - 30 * v[2] + 16 * v[3] - v[4]) / (12 * h * h)
    return d1, d2


@pytest.mark.parametrize("tree,C,n_pat,seed", CASES)
def test_restatement_vs_pruning(tree, C, n_pat, seed):
    et, m, rates, probs, states, w, P = _problem(tree, C, n_pat, seed)
    moves = eligible_moves(et.ops, et.root)
    par = parents_of(et.ops)
    assert len(moves) >= 2 * (et.n_tips - 3) - 2
    assert any(par[par[s]] == et.root for s, _ in moves) and any(par[par[s]] != et.root for s, _ in moves)
    assert any(s < et.n_tips for s, _ in moves) and any(s >= et.n_tips for s, _ in moves)
    rs = Restatement(et.ops, et.root, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
    ref = Pruning(et.ops, et.root, et.n_nodes, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
    wsum = w.sum()
    worst = e1 = e2 = 0.0
    for s, u in moves:
        f = rs.evaluator(s, u)
        t0 = et.brlen[par[s]]
        for t in (t0, 0.5 * t0, 1e-6, 3.0):
            worst = max(worst, abs(f(t)[0] - ref.delta(s, u, t)) / wsum)
        for t in (t0, 0.5 * t0):
            _, d1, d2 = f(t)
            r1, r2 = _stencils(lambda x: ref.delta(s, u, x), t, 0.01 * t)
            e1 = max(e1, abs(d1 - r1) * t / wsum)
            e2 = max(e2, abs(d2 - r2) * t * t / wsum)
    print(f"{tree}: {len(moves)} moves, |Delta - ref| / wsum {worst:.3g}, t d1 {e1:.3g}, t^2 d2 {e2:.3g}")
    assert worst <= 1e-12
    assert e1 <= 1e-6 and e2 <= 1e-5


def test_inverse_move_gives_minus_delta():
    """From the swapped tree, the inverse move (u, s) at the same length undoes the forward one."""
    et, m, rates, probs, states, w, P = _problem("join12", 4, 200, 9)
    rs = Restatement(et.ops, et.root, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
    par = parents_of(et.ops)
    for s, u in eligible_moves(et.ops, et.root)[::5]:
        t = et.brlen[par[s]]
        ops2 = postorder_ops(swap_ops(et.ops, s, u), et.root)
        rs2 = Restatement(ops2, et.root, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
        fwd, back = rs.evaluator(s, u)(t)[0], rs2.evaluator(u, s)(t)[0]
        assert abs(fwd + back) <= 1e-12 * w.sum()


@pytest.mark.parametrize("tree,C,n_pat,seed", CASES)
def test_newton_rule(tree, C, n_pat, seed):
    """Every move converges within 40 passes at tol 1e-8; delta never falls below Delta(t0) and is
    a local maximum of the reference (or sits at a bound with d1 pointing outward)."""
    et, m, rates, probs, states, w, P = _problem(tree, C, n_pat, seed)
    moves = eligible_moves(et.ops, et.root)
    par = parents_of(et.ops)
    rs = Restatement(et.ops, et.root, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
    ref = Pruning(et.ops, et.root, et.n_nodes, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
    t0 = np.array([et.brlen[par[s]] for s, _ in moves])
    at0 = rs.scores(moves, t0)
    out = rs.scores(moves, t0, max_iter=40)
    print(f"{tree}: {out['passes']} passes")
    assert at0["passes"] == 1 and np.array_equal(at0["t_opt"], t0)
    assert np.all(out["status"] == 0) and out["passes"] <= 41
    assert np.all(out["delta"] >= at0["delta"])
    tol = 1e-12 * w.sum()
    for i, (s, u) in enumerate(moves):
        t = out["t_opt"][i]
        assert abs(out["delta"][i] - ref.delta(s, u, t)) <= tol
        if 1e-6 < t < 100.0:
            assert ref.delta(s, u, t * (1 + 1e-3)) <= out["delta"][i] + tol
            assert ref.delta(s, u, t * (1 - 1e-3)) <= out["delta"][i] + tol
        else:
            assert out["d1"][i] <= 0.0 if t == 1e-6 else out["d1"][i] >= 0.0


def test_reference_uncle_choice():
    et = tree_by_name("trifurcating9")
    sons, par = sons_of(et.ops), parents_of(et.ops)
    for s in par:
        if par[s] == et.root:
            continue
        u = reference_uncle(et.ops, et.root, s)
        assert u in sons[par[par[s]]] and u != par[s]
