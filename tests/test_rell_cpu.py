"""RELL resampling without a device: the declared interface, the summation rule of
plk_replicate_sums restated in numpy, and the site rows of plk_nni_site_rows against pruning.

The summation rule (include/plk.h, csrc/plk_rell.hpp).  Per 4096 patterns a partial starts from
+0.0 and takes the block's (padded) patterns by fused multiply-add: 32-pattern segments ascending,
inside a segment q = 0..7, inside q the patterns 32 seg + 8 k + q for k = 0..3.  The partials of an
element are then added in global block order, one chain from +0.0; a later shard continues the
chain of the one before it.  `rule_sums` restates that.  numpy has no fused multiply-add, so the
restatement is bitwise only where every product w * x is exact in fp64: `exact_problem` draws
integer counts below 2^10 and values of at most 24 significant bits (34-bit products) whose
exponents spread over 2^-40 .. 2^40, so that the sums do round.  On such data the result depends
on the ORDER of the additions alone, which is what the rule fixes.

The GPU tests (test_gpu_rell.py) import this module for the restatement.
"""
import os
import re

import numpy as np
import pytest

import phylo
import plk

import test_nni_cpu as nni

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, SEG = 4096, 32

NEW_SYMBOLS = ["plk_site_rows_reserve", "plk_site_row_set", "plk_site_row_get", "plk_site_row_from_root",
               "plk_nni_site_rows", "plk_set_replicate_weights", "plk_replicate_sums", "plk_replicate_passes"]
NEW_METHODS = ["site_rows_reserve", "site_row_set", "site_row_get", "site_row_from_root", "nni_site_rows",
               "set_replicate_weights", "replicate_sums", "replicate_passes"]


# ---------------------------------------------------------------- 1. the interface

def test_new_symbols_declared_and_abi_version_kept():
    hdr = open(os.path.join(ROOT, "include", "plk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(plk_[a-z_0-9]+)\s*\(", code))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in plk.EXPORTS, s
    for m in NEW_METHODS:
        assert callable(getattr(plk.Engine, m, None)), m
    assert re.search(r"#define\s+PLK_ABI_VERSION\s+2\b", hdr) and plk.ABI_VERSION == 2


# ---------------------------------------------------------------- 2. the summation rule

def n_pad(P):
    return (P + 255) // 256 * 256


def shard_starts(P, n_dev):
    """plk_create_multi's contiguous block-aligned ranges (the first shards take the extra blocks)."""
    nb = (P + BLOCK - 1) // BLOCK
    nd = min(n_dev, nb)
    per, extra = divmod(nb, nd)
    starts, b = [], 0
    for i in range(nd):
        starts.append(b * BLOCK)
        b += per + (1 if i < extra else 0)
    return starts + [P]


def _pad(A, P):
    out = np.zeros((A.shape[0], n_pad(P)))
    out[:, :P] = A
    return out


def block_partial(Wp, Xp, lo, hi):
    """Step 1 for the padded patterns [lo, hi) of one block: [R, M] accumulators from +0.0."""
    acc = np.zeros((Wp.shape[0], Xp.shape[0]))
    for seg in range(lo, hi, SEG):
        for q in range(8):
            for k in range(4):
                p = seg + 8 * k + q
                acc = acc + Wp[:, p, None] * Xp[None, :, p]
    return acc


def rule_sums(W, X, n_dev=1, r_chunk=None, m_chunk=None):
    """G [R, M] by the rule, over n_dev shards, replicates and rows in chunks of the given sizes."""
    R, P = W.shape
    M = X.shape[0]
    starts = shard_starts(P, n_dev)
    G = np.empty((R, M))
    r_chunk, m_chunk = r_chunk or R, m_chunk or M
    for r0 in range(0, R, r_chunk):
        for m0 in range(0, M, m_chunk):
            rs, ms = slice(r0, min(R, r0 + r_chunk)), slice(m0, min(M, m0 + m_chunk))
            g = np.zeros((rs.stop - rs.start, ms.stop - ms.start))
            for a, e in zip(starts[:-1], starts[1:]):              # shard after shard, seeded
                Wp, Xp = _pad(W[rs, a:e], e - a), _pad(X[ms, a:e], e - a)
                for lo in range(0, Wp.shape[1], BLOCK):             # the shard's blocks in order
                    g = g + block_partial(Wp, Xp, lo, min(lo + BLOCK, Wp.shape[1]))
            G[rs, ms] = g
    return G


def exact_problem(P, R, M, seed):
    """Counts below 2^10 and values of 24 significant bits: every product is exact in fp64."""
    rng = np.random.default_rng(seed)
    W = rng.multinomial(P, np.full(P, 1.0 / P), size=R).astype(np.float64)
    X = (-rng.gamma(2.0, 3.0, (M, P))).astype(np.float32).astype(np.float64)
    # (24-bit values of one magnitude would make every partial sum exact as well, and no order
    # would show: spread the exponents, which keeps the products exact and not the sums)
    X = X * 2.0 ** rng.integers(-40, 41, (M, P))
    assert W.max() < 1024
    return W, X


@pytest.mark.parametrize("P", [1, 4097, 2 * 4096 + 5])
@pytest.mark.parametrize("R,M", [(1, 1), (17, 1), (1, 17), (17, 17)])
def test_rule_is_the_same_sharded_and_chunked(P, R, M):
    W, X = exact_problem(P, R, M, seed=P + 31 * R + M)
    one = rule_sums(W, X)
    sharded = rule_sums(W, X, n_dev=2)
    chunked = rule_sums(W, X, r_chunk=5, m_chunk=3)
    assert len(shard_starts(P, 2)) == (3 if P > BLOCK else 2)
    assert np.array_equal(one, sharded) and np.array_equal(one, chunked)
    # and it is the sum: every order stays within P 2^-53 sum |w| |x|
    exact = W.astype(np.longdouble) @ X.astype(np.longdouble).T
    assert np.all(np.abs(one - exact) <= P * 2.0 ** -53 * (np.abs(W) @ np.abs(X).T))


def test_rule_order_matters_on_this_data():
    """The restatement is no tautology: another pattern order gives other bits on the same data."""
    W, X = exact_problem(4097, 17, 17, seed=7)
    plain = np.zeros((17, 17))
    for p in range(4097):
        plain = plain + W[:, p, None] * X[None, :, p]
    assert not np.array_equal(plain, rule_sums(W, X))


# ---------------------------------------------------------------- 3. log rho rows against pruning

def site_lnl(pr, ops, P):
    ss, sons, lr = nni.son_arrays(ops, pr.n_nodes, pr.n_tips)
    _, site, _, _ = nni.oracle.tree_loglik(ss, sons, lr, pr.root, pr.states, pr.table, P, pr.probs, pr.pi,
                                           use_patterns=False, scaling=pr.scaling, want_sites=True)
    return np.asarray(site)


def swapped_site_lnl(pr, s, u, t):
    """Per-pattern lnL of the tree with s and u swapped and branch p at length t (plain pruning)."""
    p = nni.parents_of(pr.ops)[s]
    P = pr.P.copy()
    P[p] = np.stack([pr.model.pij(r * t) for r in pr.rates])
    return site_lnl(pr, nni.swap_ops(pr.ops, s, u), P)


def log_rho_row(rs, s, u, t):
    """The row plk_nni_site_rows stores, from the restatement's coefficients."""
    gam, d = rs.coefficients(s, u)
    mu = rs.rates[:, None] * rs.model.lam[None, :]
    rho = nni._rho(gam, d, mu, t)
    ok = (rho > 0) & np.isfinite(rho)
    return np.where(ok, np.log(np.where(ok, rho, 1.0)), 0.0)


@pytest.mark.parametrize("tree,C,n_pat,seed", nni.CASES)
def test_log_rho_rows_vs_pruning(tree, C, n_pat, seed):
    """test_nni_cpu.py's bound for delta, 1e-12 of the weight sum, per unit weight: 1e-12 per
    pattern.  At t = 1e-6 the pruning difference is the one that cancels (two site lnL of O(10)
    subtracted), and 1e-12 still holds it: a few ulps of 10."""
    et, m, rates, probs, states, w, P = nni._problem(tree, C, n_pat, seed)
    args = (states, phylo.DNA.init_table, P, rates, probs, m.pi, m, w)
    rs = nni.Restatement(et.ops, et.root, et.n_tips, *args)
    pr = nni.Pruning(et.ops, et.root, et.n_nodes, et.n_tips, *args)
    cur = site_lnl(pr, et.ops, P)
    par = nni.parents_of(et.ops)
    worst = 0.0
    for s, u in nni.eligible_moves(et.ops, et.root):
        for t in (et.brlen[par[s]], 1e-6, 3.0):
            worst = max(worst, np.abs(log_rho_row(rs, s, u, t) - (swapped_site_lnl(pr, s, u, t) - cur)).max())
    print(f"{tree}: |log rho - (site lnL swapped - current)| per pattern {worst:.3g}")
    assert worst <= 1e-12


# ---------------------------------------------------------------- 4. the mirror's arithmetic

HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")


def local_bootstrap(G, rivals):
    """NNIHomogeneousTreeLikelihood::localBootstrapFromSums in numpy: G [replicate, rival rows]."""
    out, k0 = [], 0
    for k in rivals:
        g = G[:, k0:k0 + k]
        k0 += k
        share = np.where((g > 0).any(axis=1), 0.0, 1.0 / (1 + (g == 0).sum(axis=1)))
        out.append(share.mean())
    return np.array(out)


def expected_likelihood_weights(G):
    e = np.exp(G - G.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).mean(axis=0)


def test_numpy_resampling_arithmetic():
    G = np.array([[-1, -2, 0.5, -1], [0, -1, 0, 0], [1, 0, -3, -0.0], [-1e-300, -5, -1, -1]])
    assert np.allclose(local_bootstrap(G, [2, 2]), [2.5 / 4, (1 / 3 + 0.5 + 1) / 4], rtol=0, atol=1e-15)
    Y = np.array([[-10, -10 + np.log(3), -10], [-5, -1000, -5]])
    assert np.allclose(expected_likelihood_weights(Y), [0.35, 0.3, 0.35], rtol=0, atol=1e-12)


def test_cpp_resampling_arithmetic():
    """tests/cpp/test_rell_cpu.cpp: local bootstrap and expected likelihood weights from hand-made
    sums (ties included), bootstrap(n, s) summing to floor(n s + 0.5), the container."""
    import subprocess

    from conftest import run_make

    run_make("-s", "-j8", "-C", HOST, "bin/test_rell_cpu")
    r = subprocess.run([os.path.join(HOST, "bin", "test_rell_cpu")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout and "FAIL" not in r.stdout


def test_the_gpu_scenario_holds_on_the_cpu():
    """The two figures tests/cpp/test_rell_gpu.cpp rests on, from the alignment its `dump` mode
    prints (no device): on the true tree, with every rival interchange at its Newton-optimised
    length (the restatement of test_nni_cpu.py) and 1000 multinomial replicates, the branch of
    length 1e-3 gets a local bootstrap proportion below 0.95 and every other one at least 0.95."""
    import subprocess

    from conftest import run_make

    run_make("-s", "-j8", "-C", HOST, "bin/test_rell_gpu")
    r = subprocess.run([os.path.join(HOST, "bin", "test_rell_gpu"), "dump"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    newick, names, seqs = None, [], {}
    for line in r.stdout.splitlines():
        if line.startswith("NEWICK "):
            newick = line.split(" ", 1)[1]
        elif line.startswith("SEQ "):
            _, name, s = line.split(" ")
            seqs[name] = np.frombuffer(s.encode(), dtype=np.uint8) - ord("0")
    et = phylo.engine_tree(phylo.Tree.from_newick(newick))
    states = np.stack([seqs[n] for n in et.tip_names]).astype(np.int32)
    assert states.shape == (12, 2000) and states.max() <= 3
    m = phylo.gtr(1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2)
    rates, probs = phylo.gamma_rates(4, 0.6)
    P = np.zeros((et.n_nodes, 4, 4, 4))
    for v in range(et.n_nodes):
        P[v] = np.eye(4)[None] if v == et.root else np.stack([m.pij(r * et.brlen[v]) for r in rates])
    rs = nni.Restatement(et.ops, et.root, et.n_tips, states, phylo.DNA.init_table, P, rates, probs, m.pi, m)
    sons, par = nni.sons_of(et.ops), nni.parents_of(et.ops)
    branches = [p for p in sorted(sons) if p != et.root]
    rows, rivals = [], []
    for p in branches:
        mv = [(s, nni.reference_uncle(et.ops, et.root, s)) for s in sons[p]]
        t = rs.scores(mv, [et.brlen[p]] * len(mv), t_max=10000.0, tol=1e-8, max_iter=40)["t_opt"]
        rows += [log_rho_row(rs, s, u, ti) for (s, u), ti in zip(mv, t)]
        rivals.append(len(mv))
    assert len(branches) == 9 and sum(rivals) == 18
    W = np.random.default_rng(1).multinomial(2000, np.full(2000, 1 / 2000), size=1000).astype(np.float64)
    lbp = local_bootstrap(W @ np.stack(rows).T, rivals)
    short = [i for i, p in enumerate(branches) if et.brlen[p] < 0.01]
    print({p: (et.brlen[p], v) for p, v in zip(branches, lbp)})
    assert len(short) == 1 and lbp[short[0]] < 0.95
    assert all(v >= 0.95 for i, v in enumerate(lbp) if i != short[0])
