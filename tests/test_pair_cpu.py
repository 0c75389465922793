"""Pairwise ML distances (plk_pair_counts / plk_pair_distances), restated in numpy and checked
against an independent per-pattern evaluation.  The GPU tests (test_gpu_pair.py) use the
restatement as their reference.

The restatement follows include/plk.h: histogram N[a][b] of a pair's codes, the basis alpha, beta,
delta of the code table, l_ab(t) = sum_c p_c sum_k alpha beta exp(lambda_k r_c t) (in the
short-length form delta + sum alpha beta expm1(.) while t max|lambda r| <= 1),
F = sum N log l and its derivatives, and plk_nni_scores' Newton rule (test_nni_cpu.newton, the
same function the NNI restatement runs).

The independent evaluation knows no table: P_c(t) = V exp(lambda r_c t) Vinv and, pattern by
pattern, l(p) = sum_c p_c sum_xy pi_x init[code_a][x] P_c[x][y] init[code_b][y].  At t = 1e-6
that eigen form is itself the weaker side (an off-diagonal P of 1e-6 summed from O(1) terms
keeps ten digits), so there P_c comes from the Taylor series of exp(Q r_c t), whose off-diagonal
entries are sums of terms of falling size with nothing to cancel.

Tolerances are test_nni_cpu.py's for the same quantities: F to 1e-12 of the weight sum; d1 and
d2 against fourth-order central differences of the per-pattern F with step 0.01 t, as t d1 and
t^2 d2 per unit weight, 1e-6 and 1e-5.  t_opt: the last Newton step bounds its error by
tol max(t, t_min); a bisection of the per-pattern d1 to 1e-13 relative has its own error, and
10 tol max(t, t_min) covers both.
"""
import numpy as np
import pytest

import phylo

from test_nni_cpu import _stencils, newton

T_MIN, T_MAX = 1e-6, 100.0


# ---------------------------------------------------------------- the restatement

def pair_table(codes_a, codes_b, w, n_codes):
    N = np.zeros((n_codes, n_codes))
    np.add.at(N, (codes_a, codes_b), w)
    return N


class Restatement:
    def __init__(self, codes, init_table, rates, probs, model, w=None):
        """codes [tips, patterns] in the table's numbering."""
        self.codes = np.asarray(codes, dtype=np.int64)
        self.tab = np.asarray(init_table, dtype=np.float64)
        self.w = np.ones(self.codes.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
        self.rates, self.probs, self.m = np.asarray(rates), np.asarray(probs), model
        pi, V, Vi = model.pi, model.V, model.Vinv
        self.alpha = (self.tab * pi[None, :]) @ V           # [a][k]
        self.beta = Vi @ self.tab.T                         # [k][b]
        self.delta = (self.tab * pi[None, :]) @ self.tab.T  # [a][b]
        nz = self.tab != 0.0
        self.res = np.where(nz.sum(axis=1) == 1, nz.argmax(axis=1), -1)
        self.mu = self.rates[:, None] * model.lam[None, :]  # [c][k]
        self.cut = np.abs(model.lam).max() * np.abs(self.rates).max()

    def table(self, a, b):
        return pair_table(self.codes[a], self.codes[b], self.w, self.tab.shape[0])

    def start(self, N, t_min=T_MIN, t_max=T_MAX):
        r = self.res
        both = (r[:, None] >= 0) & (r[None, :] >= 0) & (N > 0)
        g = N[both].sum()
        d = N[both & (r[:, None] != r[None, :])].sum()
        return min(max(d / g, t_min), t_max) if g > 0 else t_min

    def _l(self, t):
        """l_ab(t) for all entries, in the short-length form while t max|mu| <= 1."""
        ab = self.alpha[:, :, None] * self.beta[None, :, :]  # [a][k][b]
        if t * self.cut <= 1.0:
            return self.delta + np.einsum("akb,k->ab", ab, self.probs @ np.expm1(self.mu * t))
        return np.einsum("akb,k->ab", ab, self.probs @ np.exp(self.mu * t))

    def evaluate(self, N, t, t_acc=None):
        """(F, d1, d2) at t, and with t_acc also F(t) - F(t_acc) summed per entry."""
        ab = self.alpha[:, :, None] * self.beta[None, :, :]
        e = np.exp(self.mu * t)
        l0 = self._l(t)
        l1 = np.einsum("akb,k->ab", ab, self.probs @ (self.mu * e))
        l2 = np.einsum("akb,k->ab", ab, self.probs @ (self.mu * self.mu * e))
        use = N > 0
        ok = use & (l0 > 0) & np.isfinite(l0)
        den = np.where(ok, l0, 1.0)
        g1, g2 = np.where(ok, l1 / den, 0.0), np.where(ok, l2 / den, 0.0)
        out = (float(np.sum(N * np.where(ok, np.log(den), 0.0))), float(np.sum(N * g1)), float(np.sum(N * (g2 - g1 * g1))))
        if t_acc is None:
            return out
        la = self._l(t_acc)
        dx = np.einsum("akb,k->ab", ab, self.probs @ (np.exp(self.mu * t_acc) * np.expm1(self.mu * (t - t_acc))))
        ok_a = ok & (la > 0) & np.isfinite(la)
        q = np.where(ok_a, dx / np.where(ok_a, la, 1.0), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            dl = np.where(q > -0.5, np.log1p(np.maximum(q, -0.5)), np.log(np.where(ok_a, l0 / np.where(ok_a, la, 1.0), 1.0)))
        return out + (float(np.sum(N * np.where(ok_a, dl, 0.0))),)

    def distances(self, tip_a, tip_b, t0=None, t_min=T_MIN, t_max=T_MAX, tol=1e-8, max_iter=0):
        """As Engine.pair_distances."""
        tabs = [self.table(a, b) for a, b in zip(tip_a, tip_b)]
        if t0 is None:
            t0 = [self.start(N, t_min, t_max) for N in tabs]
        evals = [lambda t, ta=None, N=N: self.evaluate(N, t, ta) for N in tabs]
        out = newton(evals, t0, t_min, t_max, tol, max_iter)
        out["lnl"] = out.pop("delta")
        return out


# ---------------------------------------------------------------- the per-pattern evaluation

def _pmat(m, x, order=0):
    """d^order/dt^order of exp(Q t) at t = x (x = r_c t; the chain rule's r_c^order is the caller's)."""
    if order == 0 and x * np.abs(m.lam).max() < 1e-3:
        P, term = np.eye(m.S), np.eye(m.S)
        for n in range(1, 12):
            term = term @ (m.Q * x) / n
            P = P + term
        return P
    return (m.V * (m.lam ** order * np.exp(m.lam * x))) @ m.Vinv


class Patterns:
    def __init__(self, codes, init_table, rates, probs, model, w):
        self.codes, self.tab, self.rates, self.probs, self.m, self.w = codes, init_table, rates, probs, model, w

    def _site(self, a, b, t, order=0):
        A, B = self.tab[self.codes[a]] * self.m.pi[None, :], self.tab[self.codes[b]]
        l = np.zeros(len(self.w))
        for r, p in zip(self.rates, self.probs):
            l += p * r ** order * np.einsum("px,xy,py->p", A, _pmat(self.m, r * t, order), B)
        return l

    def F(self, a, b, t):
        return float(np.sum(self.w * np.log(self._site(a, b, t))))

    def d1(self, a, b, t):
        return float(np.sum(self.w * self._site(a, b, t, 1) / self._site(a, b, t)))

    def bisect_d1(self, a, b, lo=T_MIN, hi=T_MAX):
        """The root of d1 in (lo, hi) to 1e-13 relative, or None when d1 keeps its sign."""
        flo, fhi = self.d1(a, b, lo), self.d1(a, b, hi)
        if not (flo > 0.0 > fhi):
            return None
        while hi - lo > 1e-13 * lo:
            mid = 0.5 * (lo + hi)
            if self.d1(a, b, mid) > 0.0:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)


# ---------------------------------------------------------------- problems (shared with the GPU tests)

def random_model(S, rng):
    if S == 4:
        return phylo.gtr(*rng.uniform(0.3, 2.0, 5), *rng.dirichlet(np.ones(4) * 5)), phylo.DNA
    if S == 20:
        return phylo.lg08(), phylo.PROTEIN
    E = rng.uniform(0.1, 2.0, (S, S))
    pi = rng.dirichlet(np.ones(S) * 5)
    Q = phylo.reversible_generator(E + E.T, pi)
    return phylo.Model("rand", S, Q, pi, *phylo.reversible_eigen(Q, pi)), phylo.CODON


def nonreversible_model(rng):
    """A 4-state generator without detailed balance and with a real spectrum: random rates whose
    lower triangle is perturbed by up to 15 % (distinct real eigenvalues stay real under a small
    perturbation; the draw is repeated until they are), scaled to one substitution per unit time."""
    while True:
        R = rng.uniform(0.2, 2.0, (4, 4))
        R[np.tril_indices(4, -1)] *= rng.uniform(0.85, 1.15, 6)
        np.fill_diagonal(R, 0.0)
        Q = R - np.diag(R.sum(axis=1))
        lam, V = np.linalg.eig(Q)
        if np.abs(lam.imag).max() > 0 or np.linalg.cond(V) > 1e3:
            continue
        lam, V = lam.real, V.real
        # stationary distribution: the left null vector
        wv, L = np.linalg.eig(Q.T)
        pi = np.abs(L[:, np.argmin(np.abs(wv))].real)
        pi /= pi.sum()
        Q = Q / -np.dot(np.diag(Q), pi)
        lam, V = np.linalg.eig(Q)
        lam, V = lam.real, V.real
        lam[np.argmin(np.abs(lam))] = 0.0
        if np.abs(Q * pi[:, None] - (Q * pi[:, None]).T).max() < 1e-3:
            continue  # (reversible after all)
        return phylo.Model("nonrev", 4, Q, pi, V, np.linalg.inv(V), lam)


class Problem:
    """Tips evolved from a common ancestor over branches of mixed lengths (star tree): pairs at
    distances from 0.02 to ~2 (brlen: other bounds of the tips' branch lengths).  Codes in the
    alphabet's table numbering, ambiguity codes at the share amb_rate of the characters on request."""

    def __init__(self, S, C, n_tips, n_pat, amb, seed, model=None, int_weights=True, brlen=(0.01, 1.0), amb_rate=0.15):
        rng = np.random.default_rng(seed)
        if model is None:
            self.m, self.alph = random_model(S, rng)
        else:
            self.m, self.alph = model, phylo.DNA
        self.S, self.C, self.n_tips, self.n_pat = S, C, n_tips, n_pat
        self.rates, self.probs = phylo.gamma_rates(C, 0.5)
        root = np.searchsorted(np.cumsum(self.m.pi), rng.random(n_pat), side="right").clip(0, S - 1)
        cls = rng.integers(0, C, n_pat)
        self.brlen = np.exp(rng.uniform(np.log(brlen[0]), np.log(brlen[1]), n_tips))
        codes = np.empty((n_tips, n_pat), dtype=np.int64)
        for i in range(n_tips):
            cum = np.cumsum(np.stack([self.m.pij(self.brlen[i] * r) for r in self.rates]), axis=2)
            codes[i] = (rng.random(n_pat)[:, None] > cum[cls, root]).sum(axis=1).clip(0, S - 1)
        if amb:
            mask = rng.random(codes.shape) < amb_rate
            codes[mask] = rng.integers(S, self.alph.n_codes, size=mask.sum())
        self.codes = codes
        self.w = rng.integers(1, 9, n_pat).astype(np.float64) if int_weights else rng.uniform(0.1, 3.0, n_pat)
        self.pairs = [(a, b) for a in range(n_tips) for b in range(a + 1, n_tips)]

    def restatement(self):
        return Restatement(self.codes, self.alph.init_table, self.rates, self.probs, self.m, self.w)

    def patterns(self):
        return Patterns(self.codes, self.alph.init_table, self.rates, self.probs, self.m, self.w)


# ---------------------------------------------------------------- the tests

CASES = [(4, 1, 4, 300, False, 1), (4, 4, 5, 300, True, 2), (20, 2, 4, 300, True, 3), (64, 1, 3, 200, True, 4)]


@pytest.mark.parametrize("S,C,n_tips,n_pat,amb,seed", CASES)
def test_restatement_vs_patterns(S, C, n_tips, n_pat, amb, seed):
    pb = Problem(S, C, n_tips, n_pat, amb, seed)
    rs, ref = pb.restatement(), pb.patterns()
    wsum = pb.w.sum()
    worst = e1 = e2 = 0.0
    for a, b in pb.pairs + [(b, a) for a, b in pb.pairs[:2]]:
        N = rs.table(a, b)
        assert N.sum() == wsum
        for t in (1e-6, 0.05, 0.4, 3.0):
            worst = max(worst, abs(rs.evaluate(N, t)[0] - ref.F(a, b, t)) / wsum)
        for t in (0.05, 0.4):
            _, d1, d2 = rs.evaluate(N, t)
            r1, r2 = _stencils(lambda x: ref.F(a, b, x), t, 0.01 * t)
            e1 = max(e1, abs(d1 - r1) * t / wsum)
            e2 = max(e2, abs(d2 - r2) * t * t / wsum)
    print(f"S {S} C {C}: |F - ref| / wsum {worst:.3g}, t d1 {e1:.3g}, t^2 d2 {e2:.3g}")
    assert worst <= 1e-12
    assert e1 <= 1e-6 and e2 <= 1e-5


@pytest.mark.parametrize("S,C,n_tips,n_pat,amb,seed", CASES)
def test_newton_reaches_the_per_pattern_optimum(S, C, n_tips, n_pat, amb, seed):
    pb = Problem(S, C, n_tips, n_pat, amb, seed)
    rs, ref = pb.restatement(), pb.patterns()
    ta, tb = zip(*pb.pairs)
    tol = 1e-8
    at0 = rs.distances(ta, tb)
    out = rs.distances(ta, tb, tol=tol, max_iter=40)
    assert at0["passes"] == 1 and np.all(at0["status"] == 0)
    assert np.all(out["status"] == 0) and out["passes"] <= 41
    assert np.all(out["lnl"] >= at0["lnl"])
    inner = 0
    for i, (a, b) in enumerate(pb.pairs):
        t = out["t_opt"][i]
        root = ref.bisect_d1(a, b)
        if root is None:
            assert t in (T_MIN, T_MAX)
            continue
        inner += 1
        assert abs(t - root) <= 10 * tol * max(t, T_MIN), (a, b, t, root)
        assert abs(out["lnl"][i] - ref.F(a, b, t)) <= 1e-12 * pb.w.sum()
    assert inner >= len(pb.pairs) - 1


def test_start_rule():
    """d / g over the resolved codes: an ambiguity code counts on neither side."""
    pb = Problem(4, 1, 3, 50, False, 7)
    pb.codes[0, :10] = 14  # N
    pb.codes[1, 5:15] = 5   # R
    rs = pb.restatement()
    N = rs.table(0, 1)
    keep = np.arange(15, 50)
    g = pb.w[keep].sum()
    d = pb.w[keep][pb.codes[0, keep] != pb.codes[1, keep]].sum()
    assert rs.start(N) == min(max(d / g, T_MIN), T_MAX)
    allamb = Restatement(np.full((2, 5), 14), pb.alph.init_table, pb.rates, pb.probs, pb.m)
    assert allamb.start(allamb.table(0, 1)) == T_MIN


def extremes_problem():
    """Tip 1 repeats tip 0; tip 2 is drawn from pi on its own.  Independent sequences agree at
    sum pi^2 of the sites only in expectation, and the sample decides whether d1 stays positive
    up to t_max: the seed is one (of five among the first eight) for which the restatement runs
    into t_max = 100."""
    rng = np.random.default_rng(4)
    m, alph = random_model(4, rng)
    rates, probs = phylo.gamma_rates(4, 0.5)
    codes = np.searchsorted(np.cumsum(m.pi), rng.random((3, 400)), side="right").clip(0, 3)
    codes[1] = codes[0]
    return codes, alph, rates, probs, m, rng.integers(1, 9, 400).astype(np.float64)


def test_identical_and_independent_sequences():
    """Identical sequences end at t_min, independent ones at t_max, both converged."""
    codes, alph, rates, probs, m, w = extremes_problem()
    rs = Restatement(codes, alph.init_table, rates, probs, m, w)
    out = rs.distances([0, 0], [1, 2], tol=1e-8, max_iter=40)
    assert out["t_opt"][0] == T_MIN and out["t_opt"][1] == T_MAX and np.all(out["status"] == 0)


def test_nonreversible_ordered_pairs():
    """Without detailed balance F of (a, b) and of (b, a) differ; each matches the per-pattern form."""
    rng = np.random.default_rng(5)
    m = nonreversible_model(rng)
    assert np.abs(m.Q.sum(axis=1)).max() < 1e-12 and np.abs(m.pi @ m.Q).max() < 1e-12
    assert np.abs(m.V @ np.diag(m.lam) @ m.Vinv - m.Q).max() < 1e-12
    pb = Problem(4, 4, 3, 300, True, 6, model=m)
    rs, ref = pb.restatement(), pb.patterns()
    wsum, seen = pb.w.sum(), 0.0
    for a, b in [(0, 1), (1, 0), (0, 2), (2, 0)]:
        N = rs.table(a, b)
        assert np.array_equal(N, rs.table(b, a).T)
        for t in (1e-6, 0.05, 3.0):
            assert abs(rs.evaluate(N, t)[0] - ref.F(a, b, t)) <= 1e-12 * wsum
        seen = max(seen, abs(ref.F(a, b, 0.4) - ref.F(b, a, 0.4)) / wsum)
    assert seen > 1e-6  # the order matters for this model
