"""Substitution mapping on the device (plk_branch_counts): the posterior expected number of
substitutions of each type, on each branch, at each pattern -- the reference's
SubstitutionMappingTools::computeSubstitutionVectors over DecompositionSubstitutionCount.

Reference, numpy and in this file, on the engine's own P(t) and on Van Loan's W
(test_count_matrices_cpu.py): lnL is linear in one branch's P, so plain pruning with W^k_{v,c}
in the place of P_v gives n_k per pattern at the root, and pruning as it is gives l; the
counts are n_k / l.  Nothing of the engine's downward recursion is in it.  Through the deep
rescaled caterpillar, whose partials underflow doubles, a normalised up-down pass replaces
plain pruning (as in test_gpu_posteriors.py); it is checked against plain pruning on a small
case before it is relied on.

Tolerance: 1e-10 * max(1, |ref|) on counts and on totals divided by the weight sum (the
project's DR-vs-path figure, used by the posterior tests), 1e-9 through the caterpillar.
"""
import numpy as np
import pytest

import phylo
import plk
import workload

from test_count_matrices_cpu import van_loan
from test_gpu_parity import MODES, _caterpillar, _random_problem, engine_for
from test_gpu_posteriors import _all_outputs, _lower, _norm, _parents, _pmats, _prepare, _same, _six_nodes, _sons

pytestmark = pytest.mark.gpu

DR = plk.PLK_FLAG_DOUBLE_RECURSIVE
GUARD = plk.PLK_FLAG_NONNEG_GUARD


# ---------------------------------------------------------------- numpy references

def _branches(et):
    return [n for n in range(et.n_nodes) if n != et.root]


def _ref_W(et, models, Bs, rates, branches, mi=None):
    """Van Loan's W per branch: {v: [T, C, S, S]}."""
    out = {}
    for v in branches:
        k = 0 if mi is None else int(mi[v])
        out[v] = np.stack([van_loan(models[k].Q, Bs[k], et.brlen[v] * r) for r in rates], axis=1)
    return out


def _pruning_counts(et, L, P, W, probs, pi, v):
    """counts[pattern, type] of branch v: root sums with W^k_v, then P_v, in the place of P_v."""
    parents, sons = _parents(et), _sons(et)
    M = np.concatenate([P[v][None], W[v]])                                  # [1 + T, C, S, S]
    A = np.einsum("kcxy,pcy->kpcx", M, L[v])
    n = v
    while True:
        f = parents[n]
        for s in sons[f]:
            if s != n:
                A = A * np.einsum("cys,pcs->pcy", P[s], L[s])[None]
        if f not in parents:
            break
        A = np.einsum("cyx,kpcx->kpcy", P[f], A)
        n = f
    r = np.einsum("c,x,kpcx->kp", probs, pi, A)
    return (r[1:] / r[0]).T


def _updown_counts(et, states, init_table, P, W, probs, pi, branches):
    """The same counts from an up-down pass normalised per node and pattern (jointly over
    classes and states, so the factors cancel in n_k / l)."""
    C = P.shape[1]
    sons, parents = _sons(et), _parents(et)
    order = []
    for p, _ in et.ops:
        if p not in order:
            order.append(p)
    L = {i: np.repeat(init_table[states[i]][:, None, :], C, axis=1) for i in range(et.n_tips)}
    for p in order:
        acc = 1.0
        for c in sons[p]:
            acc = acc * np.einsum("cys,pcs->pcy", P[c], L[c])
        L[p], _ = _norm(acc)
    n_pat = states.shape[1]
    above = {et.root: np.broadcast_to(pi[None, None, :], (n_pat, C, len(pi)))}   # state at the node, from above
    U = {}                                                                       # state at the father
    for p in reversed(order):
        q = {c: np.einsum("cys,pcs->pcy", P[c], L[c]) for c in sons[p]}
        for c in sons[p]:
            u = above[p]
            for o in sons[p]:
                if o != c:
                    u = u * q[o]
            U[c], _ = _norm(u)
            if c >= et.n_tips:
                above[c], _ = _norm(np.einsum("pcy,cyx->pcx", U[c], P[c]))
    out = {}
    for v in branches:
        M = np.concatenate([P[v][None], W[v]])
        r = np.einsum("c,pcx,kcxy,pcy->kp", probs, U[v], M, L[v])
        out[v] = (r[1:] / r[0]).T
    return out


# ---------------------------------------------------------------- shared pieces

def _count_engine(et, S, C, n_pat, states, init_table, rates, probs, pi, models, Bs, flags, mi=None, weights=None,
                  device=0):
    if device == 0:
        eng = engine_for(et, S, C, n_pat, states, init_table, rates, probs, pi, models, model_of_node=mi, flags=flags)
    else:
        eng = plk.Engine(device, S, C, n_pat, et.n_tips, et.n_internal, len(models), flags)
        eng.set_code_table(init_table)
        for i in range(et.n_tips):
            eng.set_tip_codes(i, states[i].astype(np.uint8))
        eng.set_category_rates(rates, probs)
        eng.set_root_frequencies(pi)
        for k, m in enumerate(models):
            eng.set_eigen(k, m.V, m.Vinv, m.lam)
    if weights is not None:
        eng.set_pattern_weights(weights)
    _prepare(eng, et, mi)
    for k, B in enumerate(Bs):
        eng.set_count_types(k, B)
    br = np.array(_branches(et), dtype=np.int32)
    eng.update_count_matrices(br, et.brlen[br], None if mi is None else np.asarray(mi)[br].astype(np.int32))
    return eng


def _check_counts(out, ref, branches, weights, tol):
    refc = np.stack([ref[v] for v in branches])                                # [branch, pattern, type]
    c, t = out["counts"], out["totals"]
    assert c.shape == refc.shape and t.shape == (len(branches), refc.shape[2])
    err = np.abs(c - refc) / np.maximum(1.0, np.abs(refc))
    wsum = weights.sum()
    reft = np.einsum("p,bpk->bk", weights, refc) / wsum
    errt = np.abs(t / wsum - reft) / np.maximum(1.0, np.abs(reft))
    print(f"max error: counts {err.max():.3g} totals / weight sum {errt.max():.3g} (tolerance {tol:g})")
    assert err.max() <= tol and errt.max() <= tol
    assert c.min() >= 0.0 and t.min() >= 0.0


def _check_calls(eng, branches, out):
    """A second identical call is bitwise equal; each output alone equals the joint request."""
    assert _same(out, eng.branch_counts(branches))
    assert np.array_equal(eng.branch_counts(branches, totals=False)["counts"], out["counts"])
    assert np.array_equal(eng.branch_counts(branches, counts=False)["totals"], out["totals"])


def _registers(m, T):
    return phylo.total_register(m.Q) if T == 1 else phylo.comprehensive_register(m.Q)


def _check_comprehensive_sums_to_total(out, other):
    """DNA: the twelve comprehensive types sum to the total-register count (1e-12 relative)."""
    a, b = (out, other) if out["counts"].shape[2] == 12 else (other, out)
    s, t = a["counts"].sum(axis=2), b["counts"][:, :, 0]
    assert np.abs(s - t).max() <= 1e-12 * max(1.0, np.abs(t).max())
    st, tt = a["totals"].sum(axis=1), b["totals"][:, 0]
    assert np.abs(st - tt).max() <= 1e-12 * max(1.0, np.abs(tt).max())


# ---------------------------------------------------------------- the cases

CASES = [
    # S, C, mode, scaling, taxa, patterns, seed, ambiguity codes, T
    (4, 4, "materialize", False, 16, 300, 201, False, 12),
    (4, 4, "lnl_only", False, 16, 300, 202, True, 1),
    (4, 8, "materialize", False, 10, 300, 203, False, 12),       # C = 8: the levelwise preorder, CT = 0
    (4, 2, "levelwise", True, 12, 777, 204, False, 12),
    (20, 4, "lnl_only", False, 10, 130, 205, True, 1),
    (20, 2, "levelwise", True, 12, 200, 206, False, 1),
    (64, 2, "materialize", False, 6, 130, 207, False, 1),
    (4, 4, "materialize", False, 3, 1, 208, False, 12),          # every branch is a tip branch of the root
]


@pytest.mark.parametrize("S,C,mode,scaling,n_taxa,n_pat,seed,amb,T", CASES)
def test_counts_vs_pruning(S, C, mode, scaling, n_taxa, n_pat, seed, amb, T):
    et, m, alph, rates, probs, states = _random_problem(S, C, n_taxa, n_pat, seed=seed, amb=amb)
    flags = GUARD | MODES[mode] | DR | (plk.PLK_FLAG_SCALING if scaling else 0)
    B = _registers(m, T)
    eng = _count_engine(et, S, C, n_pat, states, alph.init_table, rates, probs, m.pi, [m], [B], flags)
    br = _branches(et)
    assert any(v < et.n_tips for v in br) and (n_taxa == 3 or any(v >= et.n_tips for v in br))
    out = eng.branch_counts(br)
    P = _pmats(eng, et)
    L = _lower(et, states, alph.init_table, P)
    W = _ref_W(et, [m], [B], rates, br)
    ref = {v: _pruning_counts(et, L, P, W, probs, m.pi, v) for v in br}
    ud = _updown_counts(et, states, alph.init_table, P, W, probs, m.pi, br)
    d = max(np.abs(ud[v] - ref[v]).max() for v in br)
    print(f"up-down vs pruning: {d:.3g}")
    assert d <= 1e-12
    _check_counts(out, ref, br, np.ones(n_pat), 1e-10)
    _check_calls(eng, br, out)
    if S == 4:
        other = _count_engine(et, S, C, n_pat, states, alph.init_table, rates, probs, m.pi, [m],
                              [_registers(m, 13 - T)], flags)
        _check_comprehensive_sums_to_total(out, other.branch_counts(br))


def _dna_case(et, n_pat, seed, C=4):
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(C, 0.5)
    wl = workload.Workload("m", et, [m], None, rates, probs, m.pi, phylo.DNA, n_pat, False, True, seed)
    return m, rates, probs, wl.simulate(0, n_pat).astype(np.int32)


def test_counts_polytomy():
    t = phylo.Tree.from_newick("((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2);")
    et = phylo.engine_tree(t)
    m, rates, probs, states = _dna_case(et, 300, 9)
    B = phylo.comprehensive_register(m.Q)
    eng = _count_engine(et, 4, 4, 300, states, phylo.DNA.init_table, rates, probs, m.pi, [m], [B], GUARD | DR)
    br = _branches(et)
    out = eng.branch_counts(br)
    P = _pmats(eng, et)
    L = _lower(et, states, phylo.DNA.init_table, P)
    W = _ref_W(et, [m], [B], rates, br)
    ref = {v: _pruning_counts(et, L, P, W, probs, m.pi, v) for v in br}
    _check_counts(out, ref, br, np.ones(300), 1e-10)
    _check_calls(eng, br, out)
    other = _count_engine(et, 4, 4, 300, states, phylo.DNA.init_table, rates, probs, m.pi, [m],
                          [phylo.total_register(m.Q)], GUARD | DR)
    _check_comprehensive_sums_to_total(out, other.branch_counts(br))


def test_counts_nonhomogeneous_rooted():
    """Per-branch models, a 2-son root, root frequencies that are not the model's."""
    wl = workload.make_workload("nh_gtr_g4_dna_2M_512", n_patterns=300)
    et = wl.et
    states = wl.simulate(0, 300).astype(np.int32)
    Bs = [phylo.comprehensive_register(m.Q) for m in wl.models]
    flags = plk.PLK_FLAG_SCALING | DR
    eng = _count_engine(et, 4, 4, 300, states, phylo.DNA.init_table, wl.rates, wl.probs, wl.root_freqs, wl.models, Bs,
                        flags, mi=wl.model_of_node)
    parents = _parents(et)
    sons = _sons(et)
    # every branch at the root and around the deepest node, tips included, and some in between
    pick = list(sons[et.root])
    for v in _six_nodes(et)[1:]:
        pick += [v] + list(sons[v])
    br = sorted(set(pick))
    assert any(v < et.n_tips for v in br) and all(v in parents for v in br)
    out = eng.branch_counts(br)
    P = _pmats(eng, et)
    W = _ref_W(et, wl.models, Bs, wl.rates, br, wl.model_of_node)
    ref = _updown_counts(et, states, phylo.DNA.init_table, P, W, wl.probs, wl.root_freqs, br)
    _check_counts(out, ref, br, np.ones(300), 1e-10)
    _check_calls(eng, br, out)
    tot = [phylo.total_register(m.Q) for m in wl.models]
    other = _count_engine(et, 4, 4, 300, states, phylo.DNA.init_table, wl.rates, wl.probs, wl.root_freqs, wl.models,
                          tot, flags, mi=wl.model_of_node)
    _check_comprehensive_sums_to_total(out, other.branch_counts(br))


def test_counts_deep_caterpillar_rescaled():
    """300 taxa: L and U pass through rescaling; the scale counts cancel in n_k / l.  (While the
    product of the stored vectors is a normal double: n_k multiplies two of them; group G of
    test_gpu_xref_consumers.py holds the products of four to six.)"""
    et = phylo.engine_tree(_caterpillar(300, lo=0.1, hi=0.4))
    m, rates, probs, states = _dna_case(et, 200, 5)
    B = phylo.comprehensive_register(m.Q)
    flags = GUARD | plk.PLK_FLAG_SCALING | DR
    eng = _count_engine(et, 4, 4, 200, states, phylo.DNA.init_table, rates, probs, m.pi, [m], [B], flags)
    sons = _sons(et)
    six = _six_nodes(et)                                     # the root, a son of it, the deepest node, three between
    deepest = six[2]
    tip = next(c for c in sons[deepest] if c < et.n_tips)
    br = [six[1], deepest, tip] + six[3:6]
    assert len(br) == 6 and len(set(br)) == 6
    out = eng.branch_counts(br)
    P = _pmats(eng, et)
    W = _ref_W(et, [m], [B], rates, br)
    ref = _updown_counts(et, states, phylo.DNA.init_table, P, W, probs, m.pi, br)
    _check_counts(out, ref, br, np.ones(200), 1e-9)
    _check_calls(eng, br, out)


# ---------------------------------------------------------------- weights, sharding

def _weighted_problem():
    n = 9000                                                 # three 4096-blocks, a ragged tail
    et, m, alph, rates, probs, states = _random_problem(4, 4, 12, n, seed=231)
    w = np.random.default_rng(7).integers(1, 9, n).astype(np.float64) + 0.25
    return n, et, m, alph, rates, probs, states, w


def test_weighted_totals():
    n, et, m, alph, rates, probs, states, w = _weighted_problem()
    B = phylo.comprehensive_register(m.Q)
    eng = _count_engine(et, 4, 4, n, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR, weights=w)
    br = _branches(et)
    out = eng.branch_counts(br)
    own = np.einsum("p,bpk->bk", w, out["counts"])
    assert np.abs(out["totals"] - own).max() <= 1e-12 * max(1.0, np.abs(own).max())
    P = _pmats(eng, et)
    L = _lower(et, states, alph.init_table, P)
    W = _ref_W(et, [m], [B], rates, br)
    ref = {v: _pruning_counts(et, L, P, W, probs, m.pi, v) for v in br}
    _check_counts(out, ref, br, w, 1e-10)
    _check_calls(eng, br, out)


def test_multi_device_counts_bitwise():
    n, et, m, alph, rates, probs, states, w = _weighted_problem()
    B = phylo.comprehensive_register(m.Q)
    br = _branches(et)
    outs = []
    for dev in (0, [0, 0]):
        eng = _count_engine(et, 4, 4, n, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR, weights=w,
                            device=dev)
        if dev != 0:
            assert eng.shard_count() == 2
        outs.append(eng.branch_counts(br))
        assert np.array_equal(eng.branch_counts(br, counts=False)["totals"], outs[-1]["totals"])
    assert _same(outs[0], outs[1])


# ---------------------------------------------------------------- no interference, freshness

@pytest.mark.parametrize("C", [4, 8])
def test_counts_leave_derivatives_and_posteriors_alone(C):
    """Both preorder forms (C = 4 fused, C = 8 levelwise): the upper vectors of tip branches
    formed for a mapping call change nothing the other two consumers return."""
    et, m, alph, rates, probs, states = _random_problem(4, C, 14, 500, seed=240 + C)
    B = phylo.total_register(m.Q)
    eng = _count_engine(et, 4, C, 500, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR)
    internal = [n for n in range(et.n_tips, et.n_nodes)]
    d_before = eng.all_branch_derivatives()
    p_before = _all_outputs(eng, internal)
    out = eng.branch_counts(_branches(et))
    p_after = _all_outputs(eng, internal)                     # (no preorder pass in between)
    d_after = eng.all_branch_derivatives()
    assert _same(p_before, p_after) and _same(p_before, _all_outputs(eng, internal))
    assert np.array_equal(d_before[0], d_after[0]) and np.array_equal(d_before[1], d_after[1])
    assert _same(out, eng.branch_counts(_branches(et)))       # and after a pass that the derivatives ran


def _timed_counts(eng, br, **kw):
    eng.reset_timing()
    eng.set_timing(plk.PLK_TIME_PARTIALS)
    out = eng.branch_counts(br, **kw)
    launches = eng.get_timing()["launches"]
    eng.set_timing(False)
    return out, launches


def test_repeated_request_issues_only_the_map_launch():
    et, m, alph, rates, probs, states = _random_problem(4, 4, 16, 1000, seed=251)
    B = phylo.total_register(m.Q)
    eng = _count_engine(et, 4, 4, 1000, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR)
    br = _branches(et)
    first, n_first = _timed_counts(eng, br)
    again, n_again = _timed_counts(eng, br)
    assert n_first > 1 and n_again == 1 and _same(first, again)
    # new count matrices are no input of U or L: still the map launch alone
    b = np.array(br, dtype=np.int32)
    eng.update_count_matrices(b, et.brlen[b] * 2.0)
    longer, n_longer = _timed_counts(eng, br)
    assert n_longer == 1
    assert np.all(longer["totals"] != first["totals"])
    eng.update_count_matrices(b, et.brlen[b])
    back, n_back = _timed_counts(eng, br)
    assert n_back == 1 and _same(first, back)


def test_counts_follow_an_incremental_traversal():
    et, m, alph, rates, probs, states = _random_problem(4, 4, 16, 800, seed=252)
    B = phylo.comprehensive_register(m.Q)
    eng = _count_engine(et, 4, 4, 800, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR)
    br = _branches(et)
    stale = eng.branch_counts(br)
    b = 2
    bl = et.brlen.copy()
    bl[b] *= 1.7
    eng.update_pmatrices(np.array([b], dtype=np.int32), bl[[b]], deriv_mask=7)
    eng.update_count_matrices(np.array([b], dtype=np.int32), bl[[b]])
    parents = _parents(et)
    anc, n = set(), b
    while n in parents:
        n = parents[n]
        anc.add(n)
    eng.update_partials(phylo.split_ops([(p, ch) for p, ch in et.ops if p in anc]))
    new = eng.branch_counts(br)
    et2 = phylo.EngineTree(et.n_tips, et.n_internal, et.root, et.tip_names, et.ops, bl, {}, [], [])
    eng2 = _count_engine(et2, 4, 4, 800, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR)
    fresh = eng2.branch_counts(br)
    for k in ("counts", "totals"):
        assert (np.abs(new[k] - fresh[k]) / np.maximum(1.0, np.abs(fresh[k]))).max() <= 1e-10
        assert np.abs(new[k] - stale[k]).max() > 1e-6


def test_host_supplied_count_matrices():
    """plk_set_count_matrix with Van Loan's W reproduces the device's own matrices' counts."""
    et, m, alph, rates, probs, states = _random_problem(4, 4, 10, 300, seed=253, amb=True)
    B = phylo.comprehensive_register(m.Q)
    eng = _count_engine(et, 4, 4, 300, states, alph.init_table, rates, probs, m.pi, [m], [B], GUARD | DR)
    br = _branches(et)
    dev = eng.branch_counts(br)
    eng2 = engine_for(et, 4, 4, 300, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    _prepare(eng2, et)
    W = _ref_W(et, [m], [B], rates, br)
    for v in br:
        eng2.set_count_matrix(v, W[v])
    host = eng2.branch_counts(br)
    for k in ("counts", "totals"):
        scale = 1.0 if k == "counts" else 300.0
        assert (np.abs(host[k] - dev[k]) / scale / np.maximum(1.0, np.abs(dev[k]) / scale)).max() <= 1e-10


# ---------------------------------------------------------------- underflow and errors

def test_unscaled_underflow_writes_zeros():
    et = phylo.engine_tree(_caterpillar(700, lo=0.3, hi=0.5))
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(2, 0.5)
    wl = workload.Workload("u", et, [m], None, rates, probs, m.pi, phylo.DNA, 64, False, True, 5)
    states = wl.simulate(0, 64).astype(np.int32)
    eng = engine_for(et, 4, 2, 64, states, phylo.DNA.init_table, rates, probs, m.pi, [m],
                     flags=DR | plk.PLK_FLAG_LEVELWISE)
    _, site, _ = _prepare(eng, et)
    dead = ~np.isfinite(site)
    assert dead.any()
    B = phylo.total_register(m.Q)
    eng.set_count_types(0, B)
    br = np.array(_sons(et)[et.root], dtype=np.int32)
    eng.update_count_matrices(br, et.brlen[br])
    out = eng.branch_counts(br)
    assert np.all(out["counts"][:, dead, :] == 0.0)
    assert np.isfinite(out["counts"]).all() and np.isfinite(out["totals"]).all()
    assert out["counts"].min() >= 0.0


def test_branch_count_errors():
    et, m, alph, rates, probs, states = _random_problem(4, 4, 6, 100, seed=3)
    B = phylo.total_register(m.Q)
    eng = engine_for(et, 4, 4, 100, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    br = np.array(_branches(et), dtype=np.int32)
    eng.set_count_types(0, B)
    eng.update_count_matrices(br, et.brlen[br])
    with pytest.raises(plk.PlkError) as ei:
        eng.branch_counts(br)                                 # before any traversal
    assert ei.value.code == -5
    _prepare(eng, et)
    for bad in ([et.root], [et.n_nodes], [-1], []):           # the root, out of range, an empty list
        with pytest.raises(plk.PlkError) as ei:
            eng.branch_counts(bad)
        assert ei.value.code == -1, bad
    with pytest.raises(plk.PlkError) as ei:
        eng.branch_counts(br, counts=False, totals=False)
    assert ei.value.code == -1
    assert eng.branch_counts(br)["counts"].shape == (len(br), 100, 1)
    # no PLK_FLAG_DOUBLE_RECURSIVE
    eng2 = engine_for(et, 4, 4, 100, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD)
    _prepare(eng2, et)
    eng2.set_count_types(0, B)
    eng2.update_count_matrices(br, et.brlen[br])
    with pytest.raises(plk.PlkError) as ei:
        eng2.branch_counts(br)
    assert ei.value.code == -5
    # a branch without a count matrix; no count matrices at all
    eng3 = engine_for(et, 4, 4, 100, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    _prepare(eng3, et)
    with pytest.raises(plk.PlkError) as ei:
        eng3.branch_counts(br)
    assert ei.value.code == -5
    eng3.set_count_types(0, B)
    eng3.update_count_matrices(br[1:], et.brlen[br[1:]])
    with pytest.raises(plk.PlkError) as ei:
        eng3.branch_counts(br)
    assert ei.value.code == -5
    assert eng3.branch_counts(br[1:], counts=False)["totals"].shape == (len(br) - 1, 1)
    # pattern compression
    eng4 = engine_for(et, 4, 4, 100, states, alph.init_table, rates, probs, m.pi, [m],
                      flags=GUARD | plk.PLK_FLAG_SUBTREE_PATTERNS)
    _prepare(eng4, et)
    eng4.set_count_types(0, B)
    eng4.update_count_matrices(br, et.brlen[br])
    with pytest.raises(plk.PlkError) as ei:
        eng4.branch_counts(br)
    assert ei.value.code == -4
