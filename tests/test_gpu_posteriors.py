"""Marginal posteriors of internal nodes on the device (plk_node_posteriors): ancestral
states and rate classes -- the reference's MarginalAncestralStateReconstruction,
DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate and
AbstractDiscreteRatesAcrossSitesTreeLikelihood::getPosteriorProbabilitiesOfEachRate.

References, both numpy and both in this file, on the engine's own transition matrices:
  - clamping (primary): for node v and state x, prune the tree with L_v zeroed except at x;
    the root sum of class c is J_v[c][x].  Nothing of the engine's downward recursion is in it.
  - an up-down pass (secondary), normalised per node and pattern jointly over classes and
    states with the logs carried, so that it also serves the trees that underflow doubles.
    It is checked against clamping on every small case before it is relied on.
On the seeded cases the two agree to better than 1e-15, far inside the tolerance.

Tolerances: absolute 1e-10 on joint, state_post and class_post (the project's DR-vs-path
figure), 1e-9 through the 300-taxon caterpillar's deep rescaling (as test_gpu_dr.py has it).
best_state must equal the reference's argmax wherever the reference's top two posteriors
differ by more than 1e-8; cells inside that gap are skipped, at most 1 % per case.
"""
import numpy as np
import pytest

import phylo
import plk
import workload
from conftest import set_tune

from test_gpu_parity import MODES, _caterpillar, _random_problem, engine_for, engine_pmats, run_engine

pytestmark = pytest.mark.gpu

DR = plk.PLK_FLAG_DOUBLE_RECURSIVE
GUARD = plk.PLK_FLAG_NONNEG_GUARD


# ---------------------------------------------------------------- numpy references

def _sons(et):
    sons = {}
    for p, ch in et.ops:
        sons.setdefault(p, []).extend(ch)
    return sons


def _parents(et):
    return {c: p for p, ch in et.ops for c in ch}


def _lower(et, states, init_table, P):
    """Unnormalised lower partials of every node, [pattern, class, state]."""
    C = P.shape[1]
    L = {i: np.repeat(init_table[states[i]][:, None, :], C, axis=1) for i in range(et.n_tips)}
    done = set(range(et.n_tips))
    sons = _sons(et)
    for p, _ in et.ops:
        if p in done:
            continue
        acc = 1.0
        for c in sons[p]:
            acc = acc * np.einsum("cys,pcs->pcy", P[c], L[c])
        L[p] = acc
        done.add(p)
    return L


def _clamp_joint(et, L, P, probs, pi, v):
    """J_v[pattern, class, x]: the root sum with L_v zeroed except at x, for every x at once."""
    S = P.shape[2]
    parents, sons = _parents(et), _sons(et)
    A = L[v][:, :, None, :] * np.eye(S)[None, None]          # [p, c, x, s]
    n = v
    while n in parents:
        f = parents[n]
        A = np.einsum("cys,pcxs->pcxy", P[n], A)
        for s in sons[f]:
            if s != n:
                A = A * np.einsum("cys,pcs->pcy", P[s], L[s])[:, :, None, :]
        n = f
    return probs[None, :, None] * np.einsum("y,pcxy->pcx", pi, A)


def _norm(a):
    m = a.max(axis=(1, 2))
    m = np.where(m > 0, m, 1.0)
    return a / m[:, None, None], np.log(m)


def _updown(et, states, init_table, P, probs, pi, nodes):
    """Up-down pass, normalised per node and pattern: {v: joint[pattern, class, state]} and
    the per-pattern log-likelihood seen from each requested node."""
    C = P.shape[1]
    sons = _sons(et)
    order = []
    for p, _ in et.ops:
        if p not in order:
            order.append(p)
    L = {i: np.repeat(init_table[states[i]][:, None, :], C, axis=1) for i in range(et.n_tips)}
    lg = {i: 0.0 for i in range(et.n_tips)}
    for p in order:
        acc, s = 1.0, 0.0
        for c in sons[p]:
            acc = acc * np.einsum("cys,pcs->pcy", P[c], L[c])
            s = s + lg[c]
        L[p], m = _norm(acc)
        lg[p] = s + m
    n_pat = states.shape[1]
    B = {et.root: np.broadcast_to(pi[None, None, :], (n_pat, C, len(pi)))}   # state at the node, from above
    bl = {et.root: 0.0}
    for p in reversed(order):
        q = {c: np.einsum("cys,pcs->pcy", P[c], L[c]) for c in sons[p]}
        for c in sons[p]:
            if c < et.n_tips:
                continue
            U, s = B[p], bl[p]
            for o in sons[p]:
                if o != c:
                    U = U * q[o]
                    s = s + lg[o]
            B[c], m = _norm(np.einsum("pcy,cyx->pcx", U, P[c]))
            bl[c] = s + m
    joint, site = {}, {}
    for v in nodes:
        J = probs[None, :, None] * B[v] * L[v]
        l = J.sum(axis=(1, 2))
        joint[v] = J / l[:, None, None]
        site[v] = np.log(l) + bl[v] + lg[v]
    return joint, site


def _pmats(eng, et):
    P = engine_pmats(eng, et)
    P[et.root] = np.eye(eng.S)[None]
    return P


# ---------------------------------------------------------------- shared checks

def _check_outputs(out, ref_joint, nodes, root_cls, S, tol):
    """Engine outputs of `nodes` against the reference joints, plus the properties every
    case must have."""
    ref = np.stack([ref_joint[v] for v in nodes])             # [node, pattern, class, state]
    j, sp, cp, best = out["joint"], out["states"], out["classes"], out["best"]
    ej, es, ec = np.abs(j - ref).max(), np.abs(sp - ref.sum(axis=2)).max(), np.abs(cp - ref.sum(axis=3)).max()
    print(f"max abs error: joint {ej:.3g} state_post {es:.3g} class_post {ec:.3g}")
    assert ej <= tol and es <= tol and ec <= tol, (ej, es, ec)
    assert np.abs(sp.sum(axis=2) - 1.0).max() <= 1e-12
    assert np.abs(cp.sum(axis=2) - 1.0).max() <= 1e-12
    assert np.abs(sp - j.sum(axis=2)).max() <= 1e-14
    assert np.abs(cp - j.sum(axis=3)).max() <= 1e-14
    assert np.abs(cp - root_cls[None]).max() <= 1e-10
    for a in (j, sp, cp):
        assert a.min() >= 0.0 and a.max() <= 1.0
    assert best.max() < S
    rs = ref.sum(axis=2)
    top = np.sort(rs, axis=2)
    clear = top[:, :, -1] - top[:, :, -2] > 1e-8
    skipped = 1.0 - clear.mean()
    print(f"best_state: {clear.size - clear.sum()} of {clear.size} cells inside the 1e-8 gap")
    assert skipped <= 0.01, skipped
    assert np.array_equal(best[clear], rs.argmax(axis=2)[clear])


def _all_outputs(eng, nodes):
    return eng.node_posteriors(nodes, joint=True, states=True, classes=True, best=True)


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _prepare(eng, et, mi=None):
    br = np.array([n for n in range(et.n_nodes) if n != et.root], dtype=np.int32)
    eng.update_pmatrices(br, et.brlen[br], None if mi is None else np.asarray(mi)[br].astype(np.int32), deriv_mask=7)
    return run_engine(eng, et)


def _internal(et):
    return [n for n in range(et.n_tips, et.n_nodes)]


def _six_nodes(et):
    """The root, one of its internal sons, the deepest internal node and three in between."""
    parents, sons = _parents(et), _sons(et)
    depth = {}
    for v in _internal(et):
        d, n = 0, v
        while n in parents:
            n = parents[n]
            d += 1
        depth[v] = d
    deepest = max(depth, key=lambda v: (depth[v], -v))
    son = next(c for c in sons[et.root] if c >= et.n_tips)
    path, n = [], deepest
    while n in parents:
        path.append(n)
        n = parents[n]
    mid = [path[len(path) * k // 4] for k in (1, 2, 3)]
    out = []
    for v in [et.root, son, deepest] + mid:
        if v not in out:
            out.append(v)
    return out


# ---------------------------------------------------------------- the cases

CASES = [
    # S, C, mode, scaling, taxa, patterns, seed, ambiguity codes
    (4, 4, "materialize", False, 16, 300, 101, False),
    (4, 4, "lnl_only", False, 16, 300, 102, True),
    (20, 4, "lnl_only", False, 10, 130, 103, True),
    (64, 2, "materialize", False, 6, 130, 104, False),
    (4, 1, "lnl_only", False, 9, 700, 105, False),
    (4, 2, "levelwise", True, 12, 777, 106, False),
    (4, 8, "materialize", False, 10, 300, 107, False),      # C = 8: the levelwise preorder
    (20, 2, "levelwise", True, 12, 200, 108, False),
    (64, 1, "lnl_only", False, 8, 130, 109, False),
    (4, 4, "lnl_only", False, 3, 1, 110, False),            # the root is the only internal node
]


@pytest.mark.parametrize("S,C,mode,scaling,n_taxa,n_pat,seed,amb", CASES)
def test_posteriors_vs_clamping(S, C, mode, scaling, n_taxa, n_pat, seed, amb):
    _run_case(S, C, mode, scaling, n_taxa, n_pat, seed, amb)


@pytest.mark.parametrize("S,C,mode,scaling,n_taxa,n_pat,seed,amb", [c for c in CASES if c[0] > 4])
def test_posteriors_valu_form_vs_clamping(S, C, mode, scaling, n_taxa, n_pat, seed, amb, monkeypatch):
    """PLK_TUNE POST_VALU=1: the LDS-staged VALU form of the 20- / 64-state kernel (the A/B
    partner of the MFMA default), held to the same checks."""
    set_tune(monkeypatch, "POST_VALU", 1)
    _run_case(S, C, mode, scaling, n_taxa, n_pat, seed, amb)


def _run_case(S, C, mode, scaling, n_taxa, n_pat, seed, amb):
    et, m, alph, rates, probs, states = _random_problem(S, C, n_taxa, n_pat, seed=seed, amb=amb)
    flags = GUARD | MODES[mode] | DR | (plk.PLK_FLAG_SCALING if scaling else 0)
    eng = engine_for(et, S, C, n_pat, states, alph.init_table, rates, probs, m.pi, [m], flags=flags)
    _, site, _ = _prepare(eng, et)
    nodes = _internal(et)
    out = _all_outputs(eng, nodes)
    P = _pmats(eng, et)
    L = _lower(et, states, alph.init_table, P)
    clamp = {}
    for v in nodes:
        J = _clamp_joint(et, L, P, probs, m.pi, v)
        l = J.sum(axis=(1, 2))
        assert np.allclose(np.log(l), site, rtol=1e-10, atol=0)     # the same normaliser at every node
        clamp[v] = J / l[:, None, None]
    ud, ud_site = _updown(et, states, alph.init_table, P, probs, m.pi, nodes)
    d = max(np.abs(ud[v] - clamp[v]).max() for v in nodes)
    print(f"up-down vs clamping: {d:.3g}")
    assert d <= 1e-13
    for v in nodes:
        assert np.allclose(ud_site[v], site, rtol=1e-10, atol=0)
    _check_outputs(out, clamp, nodes, clamp[et.root].sum(axis=2), S, 1e-10)
    # a second call with nothing changed: bitwise, and each output alone as in the full request
    assert _same(out, _all_outputs(eng, nodes))
    assert np.array_equal(eng.node_posteriors(nodes, states=False)["best"], out["best"])
    two = eng.node_posteriors(nodes, states=True, classes=True, best=False)
    assert np.array_equal(two["states"], out["states"]) and np.array_equal(two["classes"], out["classes"])


def test_posteriors_polytomy():
    t = phylo.Tree.from_newick("((a:0.1,b:0.2,c:0.05,d:0.3,e:0.12):0.1,(f:0.2,g:0.1):0.05,h:0.3,i:0.2);")
    et = phylo.engine_tree(t)
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(4, 0.5)
    wl = workload.Workload("p", et, [m], None, rates, probs, m.pi, phylo.DNA, 300, False, True, 9)
    states = wl.simulate(0, 300).astype(np.int32)
    eng = engine_for(et, 4, 4, 300, states, phylo.DNA.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    _prepare(eng, et)
    nodes = _internal(et)
    out = _all_outputs(eng, nodes)
    P = _pmats(eng, et)
    L = _lower(et, states, phylo.DNA.init_table, P)
    clamp = {}
    for v in nodes:
        J = _clamp_joint(et, L, P, probs, m.pi, v)
        clamp[v] = J / J.sum(axis=(1, 2))[:, None, None]
    ud, _ = _updown(et, states, phylo.DNA.init_table, P, probs, m.pi, nodes)
    assert max(np.abs(ud[v] - clamp[v]).max() for v in nodes) <= 1e-13
    _check_outputs(out, clamp, nodes, clamp[et.root].sum(axis=2), 4, 1e-10)
    assert _same(out, _all_outputs(eng, nodes))


def test_posteriors_deep_caterpillar_rescaled():
    """300 taxa: lower partials and upper vectors pass through rescaling; the scale counts
    cancel in J / l and are never read.  (That holds while the product of the stored vectors
    is a normal double: J multiplies two of them, each above 2^-512, so it does here; where
    four to six meet -- branch terms, NNI -- see group G of test_gpu_xref_consumers.py.)"""
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(4, 0.5)
    et = phylo.engine_tree(_caterpillar(300, lo=0.1, hi=0.4))
    wl = workload.Workload("c", et, [m], None, rates, probs, m.pi, phylo.DNA, 200, False, True, 5)
    states = wl.simulate(0, 200).astype(np.int32)
    eng = engine_for(et, 4, 4, 200, states, phylo.DNA.init_table, rates, probs, m.pi, [m],
                     flags=GUARD | plk.PLK_FLAG_SCALING | DR)
    _, site, _ = _prepare(eng, et)
    assert site.min() < -256 * np.log(2)
    nodes = _six_nodes(et)
    assert len(nodes) == 6
    out = _all_outputs(eng, nodes)
    P = _pmats(eng, et)
    ud, ud_site = _updown(et, states, phylo.DNA.init_table, P, probs, m.pi, nodes)
    for v in nodes:
        assert np.allclose(ud_site[v], site, rtol=1e-10, atol=0)
    _check_outputs(out, ud, nodes, ud[et.root].sum(axis=2), 4, 1e-9)
    assert _same(out, _all_outputs(eng, nodes))


def test_posteriors_nonhomogeneous_rooted():
    """Per-branch models, a 2-son root, root frequencies that are not the model's."""
    wl = workload.make_workload("nh_gtr_g4_dna_2M_512", n_patterns=300)
    et = wl.et
    states = wl.simulate(0, 300).astype(np.int32)
    eng = engine_for(et, 4, 4, 300, states, phylo.DNA.init_table, wl.rates, wl.probs, wl.root_freqs, wl.models,
                     model_of_node=wl.model_of_node, flags=plk.PLK_FLAG_SCALING | DR)
    _, site, _ = _prepare(eng, et, wl.model_of_node)
    nodes = _six_nodes(et)
    assert len(nodes) == 6
    out = _all_outputs(eng, nodes)
    P = _pmats(eng, et)
    ud, ud_site = _updown(et, states, phylo.DNA.init_table, P, wl.probs, wl.root_freqs, nodes)
    for v in nodes:
        assert np.allclose(ud_site[v], site, rtol=1e-10, atol=0)
    _check_outputs(out, ud, nodes, ud[et.root].sum(axis=2), 4, 1e-10)
    assert _same(out, _all_outputs(eng, nodes))


# ---------------------------------------------------------------- staleness

def test_posteriors_follow_an_incremental_traversal():
    et, m, alph, rates, probs, states = _random_problem(4, 4, 16, 800, seed=91)
    eng = engine_for(et, 4, 4, 800, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    _prepare(eng, et)
    nodes = _internal(et)
    stale = _all_outputs(eng, nodes)
    b = 2
    bl = et.brlen.copy()
    bl[b] *= 1.7
    eng.update_pmatrices(np.array([b], dtype=np.int32), bl[[b]], deriv_mask=7)
    parents = _parents(et)
    anc, n = set(), b
    while n in parents:
        n = parents[n]
        anc.add(n)
    eng.update_partials(phylo.split_ops([(p, ch) for p, ch in et.ops if p in anc]))
    new = _all_outputs(eng, nodes)
    et2 = phylo.EngineTree(et.n_tips, et.n_internal, et.root, et.tip_names, et.ops, bl, {}, [], [])
    eng2 = engine_for(et2, 4, 4, 800, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    _prepare(eng2, et2)
    fresh = _all_outputs(eng2, nodes)
    for k in ("joint", "states", "classes"):
        assert np.abs(new[k] - fresh[k]).max() <= 1e-10
        assert np.abs(new[k] - stale[k]).max() > 1e-6


def test_repeated_request_does_not_rerun_the_preorder():
    """U stays current until a P(t), partial, tip code, pi or rate changes.  The timed kernels
    (HIP events) of a repeated request are the posterior launch alone; after new class
    probabilities they are the preorder pass as well, which moves three times the bytes."""
    n = 50000
    et, m, alph, rates, probs, states = _random_problem(4, 4, 64, n, seed=92)
    eng = engine_for(et, 4, 4, n, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    _prepare(eng, et)
    nodes = _internal(et)

    def timed(**kw):
        eng.reset_timing()
        eng.set_timing(plk.PLK_TIME_PARTIALS)
        out = eng.node_posteriors(nodes, states=False, best=True, **kw)
        t = eng.get_timing()
        eng.set_timing(False)
        return out, t["partials_ms"], t["launches"]

    first, _, _ = timed()
    again, ms_again, launches = timed()
    assert launches == 1 and np.array_equal(first["best"], again["best"])
    eng.all_branch_derivatives()                                  # the pass itself leaves U current
    _, ms_after_dr, _ = timed()
    p2 = probs[::-1].copy() * np.array([0.4, 0.8, 1.2, 1.6])     # other class probabilities
    eng.set_category_rates(rates, p2)
    moved, ms_rerun, _ = timed(classes=True)
    _, ms_settled, _ = timed(classes=True)
    print(f"kernel ms: repeated {ms_again:.4f}, after the DR pass {ms_after_dr:.4f}, "
          f"after new rates {ms_rerun:.4f}, then {ms_settled:.4f}")
    assert ms_rerun > 2.0 * ms_again and ms_rerun > 2.0 * ms_after_dr and ms_rerun > 1.5 * ms_settled
    ref = eng.node_posteriors([et.root], states=False, classes=True, best=False)["classes"]
    assert np.abs(moved["classes"] - ref).max() <= 1e-10          # every node's class posterior is the root's


# ---------------------------------------------------------------- root-only requests

@pytest.mark.parametrize("S,mode,scaling", [(4, mo, sc) for mo in MODES for sc in (False, True)] +
                         [(20, "lnl_only", False)])
def test_root_only_on_plain_handles(S, mode, scaling):
    """No PLK_FLAG_DOUBLE_RECURSIVE, no dP / d2P: the root's posterior rate classes, and the
    handle left as found."""
    C, n_pat = 4, 300
    et, m, alph, rates, probs, states = _random_problem(S, C, 12, n_pat, seed=120 + S)
    flags = GUARD | MODES[mode] | (plk.PLK_FLAG_SCALING if scaling else 0)
    eng = engine_for(et, S, C, n_pat, states, alph.init_table, rates, probs, m.pi, [m], flags=flags)
    r0 = run_engine(eng, et)
    path = eng.kernel_path()
    out = _all_outputs(eng, [et.root])
    assert eng.kernel_path() == path
    r1 = eng.root_loglik(et.root, want_sites=True, want_blocks=True)
    assert r0[0] == r1[0] and np.array_equal(r0[1], r1[1]) and np.array_equal(r0[2], r1[2])
    P = _pmats(eng, et)
    ud, ud_site = _updown(et, states, alph.init_table, P, probs, m.pi, [et.root])
    assert np.allclose(ud_site[et.root], r0[1], rtol=1e-10, atol=0)
    _check_outputs(out, ud, [et.root], ud[et.root].sum(axis=2), S, 1e-10)
    assert _same(out, _all_outputs(eng, [et.root]))
    # the partials: those of a handle that was never asked for posteriors
    eng2 = engine_for(et, S, C, n_pat, states, alph.init_table, rates, probs, m.pi, [m], flags=flags)
    run_engine(eng2, et)
    mid = et.ops[len(et.ops) // 2][0]
    assert np.array_equal(eng.get_partials(mid), eng2.get_partials(mid))
    assert np.array_equal(eng.get_partials(et.root), eng2.get_partials(et.root))
    other = next(v for v in _internal(et) if v != et.root)
    with pytest.raises(plk.PlkError) as ei:
        eng.node_posteriors([et.root, other])
    assert ei.value.code == -5


# ---------------------------------------------------------------- multi-device handle

def test_multi_device_posteriors_bitwise():
    n = 9000                                                # more than one 4096-aligned range
    et, m, alph, rates, probs, states = _random_problem(4, 4, 12, n, seed=131)
    outs = []
    for dev in (0, [0, 0]):
        eng = plk.Engine(dev, 4, 4, n, et.n_tips, et.n_internal, 1, GUARD | DR)
        eng.set_code_table(alph.init_table)
        for i in range(et.n_tips):
            eng.set_tip_codes(i, states[i].astype(np.uint8))
        eng.set_category_rates(rates, probs)
        eng.set_root_frequencies(m.pi)
        eng.set_eigen(0, m.V, m.Vinv, m.lam)
        _prepare(eng, et)
        nodes = [et.root, _internal(et)[0], _internal(et)[len(_internal(et)) // 2]]
        outs.append(_all_outputs(eng, nodes))
        if dev != 0:
            assert eng.shard_count() == 2
    assert _same(outs[0], outs[1])


# ---------------------------------------------------------------- underflow and errors

def test_unscaled_underflow_writes_zeros_and_255():
    """An unscaled handle on a tree whose site likelihoods underflow doubles: probabilities 0
    and best_state 255 for those patterns, no error."""
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.3, 0.2, 0.25, 0.25)
    rates, probs = phylo.gamma_rates(2, 0.5)
    et = phylo.engine_tree(_caterpillar(700, lo=0.3, hi=0.5))
    wl = workload.Workload("u", et, [m], None, rates, probs, m.pi, phylo.DNA, 64, False, True, 5)
    states = wl.simulate(0, 64).astype(np.int32)
    eng = engine_for(et, 4, 2, 64, states, phylo.DNA.init_table, rates, probs, m.pi, [m],
                     flags=DR | plk.PLK_FLAG_LEVELWISE)
    _, site, _ = _prepare(eng, et)
    dead = ~np.isfinite(site)
    assert dead.any()
    out = _all_outputs(eng, [et.root])
    assert np.all(out["best"][0][dead] == 255)
    for k in ("joint", "states", "classes"):
        assert np.all(out[k][0][dead] == 0.0)
    assert np.all(out["best"][0][~dead] < 4)
    assert np.abs(out["states"][0][~dead].sum(axis=1) - 1.0).max(initial=0.0) <= 1e-12


def test_posterior_errors():
    et, m, alph, rates, probs, states = _random_problem(4, 4, 6, 100, seed=3)
    eng = engine_for(et, 4, 4, 100, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    with pytest.raises(plk.PlkError) as ei:
        eng.node_posteriors([et.root])                      # before any traversal
    assert ei.value.code == -5
    _prepare(eng, et)
    for bad in ([0], [et.n_nodes], [-1], []):               # a tip, out of range, an empty list
        with pytest.raises(plk.PlkError) as ei:
            eng.node_posteriors(bad)
        assert ei.value.code == -1, bad
    with pytest.raises(plk.PlkError) as ei:
        eng.node_posteriors([et.root], joint=False, states=False, classes=False, best=False)
    assert ei.value.code == -1
    eng2 = engine_for(et, 4, 4, 100, states, alph.init_table, rates, probs, m.pi, [m], flags=GUARD | DR)
    run_engine(eng2, et)
    other = next(v for v in _internal(et) if v != et.root)
    with pytest.raises(plk.PlkError) as ei:
        eng2.node_posteriors([other])                       # dP / d2P missing
    assert ei.value.code == -5
    assert eng2.node_posteriors([et.root])["best"].shape == (1, 100)
