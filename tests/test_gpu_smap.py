"""GPU tests of plk_smap_sample (csrc/plk_smap.hpp) against the numpy restatement of its draws in
tests/smap_rule.py, fed P from plk_get_pmatrix, L from plk_get_partials (a tip: its code's row) and
the tables from plk_smap_get_tables.  Classes, states, n_jumps and counts are integers and every
draw is a pure function of (seed, replicate, site, node): they are compared with ==.  Dwelling times
are compared at rtol 1e-12 (the device's log differs from libm's by a few ulp over at most 129
terms), the tables at rtol 1e-13 against numpy (Poisson terms below the normal range, which carry
fewer than 53 bits, at 1e-305 absolute).

  A  against the rule: 4, 20 and 64 states, roots of two and three sons, a five-son node, node
     numbers out of preorder, per-branch models, several workgroups, rescaled partials, two shards.
  B  invariants: resolved tips, the flow of the counted changes, dwell summing to t, batching of
     replicates, site0, streams apart from plk_simulate's.
  C  convergence of 2048 kept replicates to plk_node_posteriors, plk_branch_counts and expected
     rewards, 6 standard errors each (tests/test_smap_cpu.py holds the rule alone to the same).
     Largest |z| observed on the MI355X: see test_c_sample_means_converge.
  D  errors and n_bad."""
import numpy as np
import pytest

import phylo
import plk
import sim_rule as sr
import smap_check as sc
import smap_rule as sm
from conftest import set_tune

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OOM, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -4, -5
GUARD = plk.PLK_FLAG_NONNEG_GUARD
DR = plk.PLK_FLAG_DOUBLE_RECURSIVE
DNA_MODEL = phylo.t92(3.0, 0.4)
G4 = phylo.gamma_rates(4, 0.7)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


def test_error_codes_are_the_header_s():
    hdr = open(plk.os.path.join(plk.os.path.dirname(plk._HERE), "include", "plk.h")).read()
    for name, code in (("PLK_ERR_ARG", ERR_ARG), ("PLK_ERR_OOM", ERR_OOM), ("PLK_ERR_UNSUPPORTED", ERR_UNSUPPORTED),
                       ("PLK_ERR_STATE", ERR_STATE)):
        assert f"{name} = {code}" in hdr, name


def make_engine(tree, models, rates, probs, codes, table, t, type_of, T, flags=GUARD, device=0, mon=None,
                identity=(), traverse=True, generators=True):
    ops, root, nt = tree
    nn = len(t)
    n = codes.shape[1]
    eng = plk.Engine(device, models[0].S, len(rates), n, nt, nn - nt, len(models), flags)
    eng.set_code_table(table)
    for tip in range(nt):
        eng.set_tip_codes(tip, codes[tip])
    eng.set_category_rates(rates, probs)
    eng.set_root_frequencies(models[0].pi)
    for k, m in enumerate(models):
        eng.set_eigen(k, m.V, m.Vinv, m.lam)
        if generators:
            eng.smap_set_generator(k, m.Q)
    br = np.array([v for v in range(nn) if v != root], dtype=np.int32)
    eng.mon = None if mon is None else np.asarray(mon, dtype=np.int32)
    eng.update_pmatrices(br, t[br], None if mon is None else eng.mon[br], deriv_mask=7 if flags & DR else 1)
    for v in identity:
        eng.set_pmatrix(v, np.broadcast_to(np.eye(models[0].S), (len(rates),) + (models[0].S,) * 2))
    if type_of is not None:
        eng.smap_set_types(T, type_of)
    eng.n_nodes, eng.root, eng.ops, eng.br, eng.t, eng.codes, eng.table, eng.models = nn, root, ops, br, t, codes, table, models
    if traverse:
        eng.update_partials(ops)
    return eng


def sample(eng, seed, replicate0=0, n_replicates=1, **kw):
    eng.smap_sample(eng.root, eng.br, eng.t[eng.br], seed, replicate0, n_replicates,
                    models=None if eng.mon is None else eng.mon[eng.br], **kw)


def np_tables(eng, v):
    m = 0 if eng.mon is None else int(eng.mon[v])
    return sm.tables(eng.models[m].Q, eng.rates_, eng.t[v])


def rule_for(eng, rates, probs, seed, replicates, site0=0, check_tables=True, paths=None):
    """The rule's draws from the engine's own P, L and tables (the tables checked against numpy);
    paths: the branches whose tables are read and whose paths are drawn (None: all)."""
    eng.rates_ = rates
    P = {int(v): eng.get_pmatrix(int(v)) for v in eng.br}
    nt, C, S = eng.n_tips, eng.C, eng.S
    L = {}
    for v in range(eng.n_nodes):
        L[v] = np.broadcast_to(eng.table[eng.codes[v]][:, None, :], (eng.P, C, S)) if v < nt else eng.get_partials(v)
    tabs = {}
    for v in eng.br if paths is None else paths:
        v = int(v)
        tabs[v] = eng.smap_tables(0 if eng.mon is None else int(eng.mon[v]), v)
        if check_tables:
            ref = np_tables(eng, v)
            for key in ("R", "Rpow", "pois"):
                assert np.allclose(tabs[v][key], ref[key], rtol=1e-13, atol=1e-305), (key, v)
    order = sr.preorder(sr.kids_of_ops(eng.ops), eng.root)
    return sm.sample(order, eng.root, P, L, probs, eng.models[0].pi, tabs, {int(v): eng.t[v] for v in eng.br},
                     eng.type_of_, eng.smap_T, seed, np.asarray(replicates), np.arange(site0, site0 + eng.P), paths)


def kept(eng, replicates, paths=None):
    """The kept rows of the replicates in the rule's layout (paths: of these branches only)."""
    out = {"classes": np.stack([eng.smap_classes(r) for r in replicates]).astype(np.int64), "states": {}, "jumps": {},
           "counts": {}, "dwell": {}}
    for v in range(eng.n_nodes):
        out["states"][v] = np.stack([eng.smap_states(r, v) for r in replicates]).astype(np.int64)
    for v in eng.br if paths is None else paths:
        v = int(v)
        out["jumps"][v] = np.stack([eng.smap_jumps(r, v) for r in replicates]).astype(np.int64)
        out["counts"][v] = np.stack([eng.smap_counts(r, v) for r in replicates]).astype(np.int64)
        out["dwell"][v] = np.stack([eng.smap_dwell(r, v) for r in replicates])
    return out


def assert_equal_rule(got, ref, nodes, br):
    assert np.array_equal(got["classes"], ref["classes"]), "classes"
    for v in nodes:
        assert np.array_equal(got["states"][v], ref["states"][v]), ("states", v)
    for v in br:
        v = int(v)
        assert np.array_equal(got["jumps"][v], ref["jumps"][v]), ("jumps", v)
        assert np.array_equal(got["counts"][v], ref["counts"][v]), ("counts", v)
        assert np.allclose(got["dwell"][v], ref["dwell"][v], rtol=1e-12, atol=0), ("dwell", v)


def check_against_rule(eng, rates, probs, seed, replicates, site0=0, weights=None):
    """Kept rows against the rule; the sums, tallies and totals against the kept rows."""
    ref = rule_for(eng, rates, probs, seed, replicates, site0)
    got = kept(eng, replicates)
    assert_equal_rule(got, ref, range(eng.n_nodes), eng.br)
    assert eng.smap_bad() == ref["n_bad"]
    sums, tal = eng.smap_sums(eng.br), eng.smap_tallies(np.arange(eng.n_nodes))
    good = ~ref["bad"]
    for i, v in enumerate(eng.br):
        v = int(v)
        assert np.array_equal(sums["counts"][i], got["counts"][v].sum(axis=0)), ("count_sum", v)
        assert np.allclose(sums["dwell"][i], got["dwell"][v].sum(axis=0), rtol=1e-12, atol=0), ("dwell_sum", v)
        assert np.allclose(got["dwell"][v].sum(axis=2)[:, good], eng.t[v], rtol=1e-12, atol=0), ("dwell = t", v)
    for v in range(eng.n_nodes):
        want = (got["states"][v][:, :, None] == np.arange(eng.S)).sum(axis=0)
        assert np.array_equal(tal["states"][v], want), ("state_tally", v)
    assert np.array_equal(tal["classes"], (got["classes"][:, :, None] == np.arange(eng.C)).sum(axis=0))
    w = np.ones(eng.P) if weights is None else weights
    assert np.allclose(eng.smap_totals(eng.br), np.einsum("p,bpk->bk", w, sums["counts"].astype(np.float64)), rtol=1e-12)
    return ref, got


# A. against the rule

def _case(name):
    """(tree, models, mon, rates, probs, table, type_of, T, n, ambiguous cells, identity branches)."""
    g4r, g4p = G4
    dna, tot4 = phylo.DNA.init_table, sc.ts_tv_types()
    if name == "dna_root3_300" or name == "dna_root3_1100":
        n = 300 if name.endswith("300") else 1100
        return sc.TREE5, [DNA_MODEL], None, g4r, g4p, dna, tot4, 2, n, ((0, 4, 14), (3, 17, 5), (4, 250, 14)), (5,)
    if name == "protein_130":
        return (sc.TREE7, [phylo.lg08()], None, np.array([0.4, 1.9]), np.array([0.6, 0.4]), phylo.PROTEIN.init_table,
                sc.total_types(20), 1, 130, ((1, 9, 23),), ())
    if name == "codon_70":
        return sc.TREE6, [phylo.yn98(2.0, 0.3)], None, np.ones(1), np.ones(1), phylo.CODON.init_table, sc.total_types(64), 1, 70, (), ()
    if name == "per_branch_models":
        ms = [phylo.gtr(a=1.2, b=0.4, c=0.6, d=0.8, e=0.5, piA=0.30, piC=0.20, piG=0.25, piT=0.25),
              phylo.gtr(a=0.7, b=1.4, c=0.9, d=0.3, e=1.5, piA=0.20, piC=0.30, piG=0.30, piT=0.20)]
        return sc.ROOT2, ms, [0, 1, 1, 0, 1, 0, 0], g4r, g4p, dna, tot4, 2, 200, ((2, 5, 14),), ()
    tree = {"five_sons": sc.STAR5, "scrambled": sc.SCRAMBLED}[name]
    return tree, [DNA_MODEL], None, g4r, g4p, dna, tot4, 2, 300, ((1, 8, 14),), ()


def _engine_of(name, flags=GUARD, device=0, t_seed=7):
    tree, models, mon, rates, probs, table, type_of, T, n, amb, ident = _case(name)
    nn = max(p for p, _, _ in tree[0]) + 1
    t = sc.branch_lengths(nn, tree[1], t_seed)
    for v in ident:
        t[v] = 0.0
    codes = sc.tip_codes(tree, models[0], rates, probs, t, n, seed=21, ambiguous=amb)
    eng = make_engine(tree, models, rates, probs, codes, table, t, type_of, T, flags, device, mon, ident)
    eng.type_of_ = type_of
    return eng, rates, probs


@pytest.mark.parametrize("name", ["dna_root3_300", "protein_130", "codon_70", "five_sons", "scrambled", "per_branch_models",
                                  "dna_root3_1100", "dna_root3_300_global"])
def test_a_draws_equal_the_rule(name, monkeypatch):
    """The 4-state tables are staged in LDS (SMAP_LDS=0: read from global memory); 1100 sites are
    five workgroups; branch 5 of the DNA tree has length 0 and P = I: the son is the father, no jump."""
    if name.endswith("_global"):
        set_tune(monkeypatch, "SMAP_LDS", "0")
        name = name[:-7]
    eng, rates, probs = _engine_of(name)
    reps = [5, 6, 7] if name == "dna_root3_300" else [0, 1]
    sample(eng, 4242, reps[0], len(reps), keep=True)
    assert eng.smap_launches() <= 3
    ref, got = check_against_rule(eng, rates, probs, 4242, reps)
    assert ref["n_bad"] == 0
    assert len(np.unique(got["classes"])) == len(rates)
    assert max(int(got["jumps"][int(v)].max()) for v in eng.br) >= 2
    assert any((got["counts"][int(v)].sum(axis=2) < got["jumps"][int(v)]).any() for v in eng.br)  # virtual jumps occur
    if name == "dna_root3_300":
        assert np.array_equal(got["states"][5], got["states"][7]) and not got["jumps"][5].any()
        assert np.all(got["states"][0][:, 4] < 4) and np.all(got["states"][4][:, 250] < 4)  # the N cells get a state
    eng.close()


def test_a_rescaled_partials():
    """A PLK_FLAG_SCALING handle whose stored partials carry scale counts (the 300-taxon caterpillar
    of test_gpu_xref's group BC4: per-pattern lnL below -256 ln 2): the draws read them as stored."""
    from test_gpu_xref import RESCALED, SC, _case_deep
    case = _case_deep(4)
    eng, site, _ = case.engine("materialize", SC)
    assert site.min() < RESCALED, site.min()
    m = case.models[0]
    eng.smap_set_generator(0, m.Q)
    eng.smap_set_types(2, sc.ts_tv_types())
    et = case.et
    eng.n_nodes, eng.root, eng.ops, eng.br, eng.t = et.n_nodes, et.root, phylo.split_ops(et.ops), case.br, et.brlen
    eng.codes, eng.table, eng.models, eng.mon, eng.type_of_ = case.states.astype(np.int64), case.alph.init_table, [m], None, sc.ts_tv_types()
    # the stored root partial against the never-rescaled reference: an exact power of 2^256 on every pattern, not the zeroth on some
    import xref
    from test_gpu_parity import engine_pmats
    low = xref.lower(et, case.states, case.alph.init_table, engine_pmats(eng, et))
    lifted = np.log2(eng.get_partials(et.root).max(axis=(1, 2)) / low[0][et.root].max(axis=(1, 2))).astype(np.float64)
    assert np.allclose(lifted, 256 * np.round(lifted / 256), atol=1e-6) and (lifted > 255).any(), lifted
    sample(eng, 99, 3, 1, keep=True)
    # the states of every node; the paths of the branches next to the root and of every 37th
    paths = [int(v) for v in eng.br if v >= et.n_nodes - 12 or v % 37 == 0]
    ref = rule_for(eng, case.rates, case.probs, 99, [3], check_tables=False, paths=paths)
    assert_equal_rule(kept(eng, [3], paths), ref, range(eng.n_nodes), paths)
    assert ref["n_bad"] == 0 and eng.smap_bad() == 0
    eng.close()


def test_a_two_shards_equal_one_device_bitwise():
    n = 2 * 4096 + 77
    tree, rates, probs = sc.TREE5, *G4
    t = sc.branch_lengths(8, 7, 7)
    codes = sc.tip_codes(tree, DNA_MODEL, rates, probs, t, n, seed=21, ambiguous=((0, 4, 14), (2, 5000, 5)))
    w = np.random.default_rng(1).integers(1, 5, n).astype(np.float64)
    out = []
    for device in (0, [0, 0]):
        eng = make_engine(tree, [DNA_MODEL], rates, probs, codes, phylo.DNA.init_table, t, sc.ts_tv_types(), 2, device=device)
        eng.set_pattern_weights(w)
        sample(eng, 77, 1, 2, keep=True)
        got = kept(eng, [1, 2])
        out.append((got, eng.smap_sums(eng.br), eng.smap_tallies(np.arange(8)), eng.smap_totals(eng.br), eng.smap_bad()))
        if device != 0:
            assert eng.shard_count() == 2
        eng.close()
    (g1, s1, t1, tot1, b1), (g2, s2, t2, tot2, b2) = out
    for key in ("states", "jumps", "counts", "dwell"):
        for v in g1[key]:
            assert np.array_equal(g1[key][v], g2[key][v]), (key, v)
    assert np.array_equal(g1["classes"], g2["classes"])
    assert all(np.array_equal(s1[k], s2[k]) for k in s1) and all(np.array_equal(t1[k], t2[k]) for k in t1)
    assert np.array_equal(tot1, tot2) and b1 == b2 == 0
    assert np.allclose(tot1, np.einsum("p,bpk->bk", w, s1["counts"].astype(np.float64)), rtol=1e-12)
    # the sites of the second shard against the rule
    sub = slice(4096, 4096 + 300)
    eng = make_engine(tree, [DNA_MODEL], rates, probs, codes[:, sub], phylo.DNA.init_table, t, sc.ts_tv_types(), 2)
    eng.type_of_ = sc.ts_tv_types()
    sample(eng, 77, 1, 2, site0=4096, keep=True)
    ref = rule_for(eng, rates, probs, 77, [1, 2], site0=4096)
    for key in ("states", "jumps", "counts"):
        for v in ref[key]:
            assert np.array_equal(g2[key][v][:, sub], ref[key][v]), (key, v)
    eng.close()


# B. invariants

def _comprehensive_types():
    ty = np.zeros((4, 4), dtype=np.uint8)
    pairs = [(x, y) for x in range(4) for y in range(4) if x != y]
    for k, (x, y) in enumerate(pairs):
        ty[x, y] = k + 1
    return ty, pairs


def _engine_b(n=300, sub=slice(None), **kw):
    tree, rates, probs = sc.TREE5, *G4
    t = sc.branch_lengths(8, 7, 7)
    codes = sc.tip_codes(tree, DNA_MODEL, rates, probs, t, 300, seed=21, ambiguous=((0, 4, 14), (3, 117, 5)))[:, sub]
    ty, _ = _comprehensive_types()
    eng = make_engine(tree, [DNA_MODEL], rates, probs, codes, phylo.DNA.init_table, t, ty, 12, **kw)
    eng.type_of_ = ty
    return eng


def test_b_tips_flow_and_dwell():
    """Resolved tips keep their state; per branch and state the counted changes out of it minus
    those into it are [state = a] - [state = b] (the comprehensive register counts every change of
    the chain by its ordered pair); dwell sums to t and is positive in both end states."""
    eng = _engine_b()
    _, pairs = _comprehensive_types()
    sample(eng, 31, 0, 3, keep=True)
    got = kept(eng, [0, 1, 2])
    for tip in range(5):
        res = eng.codes[tip] < 4
        assert np.all(got["states"][tip][:, res] == eng.codes[tip][res])
    assert set(np.unique(got["states"][3][:, 117])) <= {0, 2}
    par = {c: p for p, ch, _ in eng.ops for c in ch}
    for v in eng.br:
        v = int(v)
        a, b, cnt, dw = got["states"][par[v]], got["states"][v], got["counts"][v], got["dwell"][v]
        flow = np.zeros(a.shape + (4,), dtype=np.int64)
        for k, (x, y) in enumerate(pairs):
            flow[..., x] += cnt[..., k]
            flow[..., y] -= cnt[..., k]
        assert np.array_equal(flow, (a[..., None] == np.arange(4)).astype(np.int64) - (b[..., None] == np.arange(4))), v
        assert np.all(cnt.sum(axis=2) <= got["jumps"][v])
        assert np.allclose(dw.sum(axis=2), eng.t[v], rtol=1e-12, atol=0)
        assert np.all(np.take_along_axis(dw, a[..., None], 2) > 0) and np.all(np.take_along_axis(dw, b[..., None], 2) > 0)
        visited = (a[..., None] == np.arange(4)) | (b[..., None] == np.arange(4))
        for k, (x, y) in enumerate(pairs):
            visited[..., x] |= cnt[..., k] > 0
            visited[..., y] |= cnt[..., k] > 0
        assert np.array_equal(dw > 0, visited), v
    eng.close()


def test_b_batches_of_replicates_accumulate_bitwise():
    whole, parts = _engine_b(), _engine_b()
    sample(whole, 8, 0, 4, keep=True)
    rows_w = kept(whole, [0, 1, 2, 3])
    sample(parts, 8, 0, 2, keep=True)
    first = kept(parts, [0, 1])
    with pytest.raises(plk.PlkError) as ei:
        parts.smap_states(2, 0)
    assert ei.value.code == ERR_ARG
    sample(parts, 8, 2, 2, keep=True, accumulate=True)
    second = kept(parts, [2, 3])
    for key in ("states", "jumps", "counts", "dwell"):
        for v in rows_w[key]:
            assert np.array_equal(rows_w[key][v], np.concatenate([first[key][v], second[key][v]])), (key, v)
    assert np.array_equal(rows_w["classes"], np.concatenate([first["classes"], second["classes"]]))
    sw, sp = whole.smap_sums(whole.br), parts.smap_sums(parts.br)
    tw, tp = whole.smap_tallies(np.arange(8)), parts.smap_tallies(np.arange(8))
    assert all(np.array_equal(sw[k], sp[k]) for k in sw) and all(np.array_equal(tw[k], tp[k]) for k in tw)
    assert np.array_equal(whole.smap_totals(whole.br), parts.smap_totals(parts.br))
    assert sw["counts"].sum() > 0 and tw["classes"].sum() == 4 * 300
    # without ACCUMULATE the sums start again
    sample(parts, 8, 2, 2)
    assert parts.smap_tallies([7])["classes"].sum() == 2 * 300
    whole.close()
    parts.close()


def test_b_site0_is_the_global_site():
    whole, part = _engine_b(), _engine_b(sub=slice(100, 300))
    sample(whole, 8, 1, 2, keep=True)
    sample(part, 8, 1, 2, site0=100, keep=True)
    a, b = kept(whole, [1, 2]), kept(part, [1, 2])
    for key in ("states", "jumps", "counts", "dwell"):
        for v in a[key]:
            assert np.array_equal(a[key][v][:, 100:], b[key][v]), (key, v)
    assert np.array_equal(a["classes"][:, 100:], b["classes"])
    whole.close()
    part.close()


def test_b_streams_apart_from_plk_simulate():
    """c3 = 1 against plk_simulate's 0: the same seed, replicate and draw index give other uniforms.
    The simulated root follows pi, so it agrees with the sampled one at 30 % of the sites at most."""
    eng = _engine_b()
    sample(eng, 8, 0, 1, keep=True)
    eng.simulate(eng.ops, eng.root, seed=8, replicate=0, set_tips=False)
    assert (eng.sim_states(7) != eng.smap_states(0, 7)).sum() > 300 // 4
    site = np.arange(300, dtype=np.uint64)
    assert not np.any(sm.uniform(8, site * 0, site, 1, 1) == sr.uniform(8, 0, site, 1))
    eng.close()


# C. convergence

def test_c_sample_means_converge():
    """DNA + Gamma4, 7 tips, 64 sites, 2048 kept replicates at seed 20260, pooled over sites, 6
    standard errors each: state and class tallies against plk_node_posteriors (variance
    R sum_p q (1 - q)), count sums against R plk_branch_counts and dwell sums against the expected
    rewards (block-expm reward matrices through plk_set_count_matrix on a second handle with T = 4),
    both with the sample's own standard error.

    Largest |z| on the MI355X: states 1.45, classes 1.68, counts 2.35, dwell 1.92 -- the rule's own
    figures (tests/test_smap_cpu.py), as the draws are the rule's."""
    case = sc.case_c()
    m, R = case.model, sc.C_REPLICATES
    br = np.array(case.br, dtype=np.int32)
    eng = make_engine(case.tree, [m], case.rates, case.probs, case.codes, phylo.DNA.init_table, case.t, case.type_of,
                      case.T, flags=GUARD | DR)
    sample(eng, sc.C_SEED, 0, R, keep=True)
    assert eng.smap_bad() == 0
    tal, sums = eng.smap_tallies(case.internal), eng.smap_sums(br)
    post = eng.node_posteriors(case.internal, states=True, classes=True, best=False)
    eng.set_count_types(0, sc.register_B(m.Q, case.type_of, case.T))
    eng.update_count_matrices(br, case.t[br])
    want_counts = eng.branch_counts(br, totals=False)["counts"]
    rew = make_engine(case.tree, [m], case.rates, case.probs, case.codes, phylo.DNA.init_table, case.t, None, 0,
                      flags=GUARD | DR, generators=False)
    for v in br:
        rew.set_count_matrix(int(v), sc.reward_matrices(m.Q, case.rates, case.t[v]))
    want_dwell = rew.branch_counts(br, totals=False)["counts"]
    assert np.allclose(want_dwell.sum(axis=2), case.t[br][:, None], rtol=1e-9)
    per_rep_counts = np.stack([np.stack([eng.smap_counts(r, int(v)).sum(axis=0, dtype=np.int64) for v in br]) for r in range(R)])
    per_rep_dwell = np.stack([np.stack([eng.smap_dwell(r, int(v)).sum(axis=0) for v in br]) for r in range(R)])
    assert np.array_equal(per_rep_counts.sum(axis=0), sums["counts"].sum(axis=1, dtype=np.int64))
    assert np.allclose(per_rep_dwell.sum(axis=0), sums["dwell"].sum(axis=1), rtol=1e-10)
    z_state = sc.z_tally(tal["states"], post["states"], R)
    z_class = sc.z_tally(tal["classes"], post["classes"][0], R)
    z_count = sc.z_mean(per_rep_counts, want_counts.sum(axis=1))
    z_dwell = sc.z_mean(per_rep_dwell, want_dwell.sum(axis=1))
    print(f"smap C: z states {z_state:.2f} classes {z_class:.2f} counts {z_count:.2f} dwell {z_dwell:.2f}")
    assert max(z_state, z_class, z_count, z_dwell) <= sc.Z_BOUND
    eng.close()
    rew.close()


# D. errors and n_bad

def _code(call, *a, **kw):
    with pytest.raises(plk.PlkError) as ei:
        call(*a, **kw)
    return ei.value.code


def test_d_error_codes():
    tree, rates, probs = sc.TREE5, *G4
    t = sc.branch_lengths(8, 7, 7)
    codes = sc.tip_codes(tree, DNA_MODEL, rates, probs, t, 100, seed=21)
    args = (tree, [DNA_MODEL], rates, probs, codes, phylo.DNA.init_table, t)
    ty = sc.ts_tv_types()
    # PLK_ERR_STATE: before a traversal, without a generator, without types, without root frequencies, without
    # category rates (every P(t) uploaded).  A branch of the traversed tree without P(t) cannot be reached: the
    # traversal itself refuses it (asserted below), so that check of plk_smap_sample is a second line only.
    # PLK_ERR_OOM of PLK_SMAP_KEEP is not exercised: it would take a device allocation to fail.
    eng = make_engine(*args, ty, 2, traverse=False)
    assert _code(sample, eng, 1) == ERR_STATE
    assert _code(eng.smap_sums, eng.br) == ERR_STATE and _code(eng.smap_bad) == ERR_STATE
    eng.update_partials(eng.ops)
    sample(eng, 1)
    eng.close()
    eng = make_engine(*args, ty, 2, generators=False)
    assert _code(sample, eng, 1) == ERR_STATE
    eng.close()
    eng = make_engine(*args, None, 0)
    assert _code(sample, eng, 1) == ERR_STATE
    eng.close()
    eng = plk.Engine(0, 4, 4, 100, 5, 3, 1, GUARD)
    eng.set_code_table(phylo.DNA.init_table)
    for tip in range(5):
        eng.set_tip_codes(tip, codes[tip])
    eng.set_category_rates(rates, probs)
    eng.set_eigen(0, DNA_MODEL.V, DNA_MODEL.Vinv, DNA_MODEL.lam)
    eng.smap_set_generator(0, DNA_MODEL.Q)
    eng.smap_set_types(2, ty)
    br = np.arange(7, dtype=np.int32)
    eng.update_pmatrices(br[:6], t[:6])
    eng.root, eng.br, eng.t, eng.mon = 7, br, t, None
    eng.set_pmatrix(6, np.broadcast_to(np.eye(4), (4, 4, 4)))
    eng.update_partials(tree[0])
    assert _code(sample, eng, 1) == ERR_STATE  # no root frequencies
    eng.close()
    eng = plk.Engine(0, 4, 4, 100, 5, 3, 1, GUARD)
    eng.set_code_table(phylo.DNA.init_table)
    for tip in range(5):
        eng.set_tip_codes(tip, codes[tip])
    eng.set_root_frequencies(DNA_MODEL.pi)
    eng.smap_set_generator(0, DNA_MODEL.Q)
    eng.smap_set_types(2, ty)
    eng.root, eng.br, eng.t, eng.mon = 7, br, t, None
    for v in range(6):
        eng.set_pmatrix(v, np.stack([DNA_MODEL.pij(t[v] * r) for r in rates]))
    assert _code(eng.update_partials, tree[0]) == ERR_STATE  # branch 6 has no P(t): no traversal, so no sample
    assert _code(sample, eng, 1) == ERR_STATE
    eng.set_pmatrix(6, np.stack([DNA_MODEL.pij(t[6] * r) for r in rates]))
    eng.update_partials(tree[0])
    assert _code(sample, eng, 1) == ERR_STATE  # no category rates
    eng.set_category_rates(rates, probs)
    sample(eng, 1)
    eng.close()
    # PLK_ERR_UNSUPPORTED: handles that do not keep every partial at full length; mu r t beyond 32
    for flag in (plk.PLK_FLAG_LNL_ONLY, plk.PLK_FLAG_SUBTREE_PATTERNS):
        eng = make_engine(*args, ty, 2, flags=GUARD | flag)
        assert _code(sample, eng, 1) == ERR_UNSUPPORTED
        eng.close()
    eng = make_engine(*args, ty, 2)
    long_t = t.copy()
    long_t[2] = 33.0 / (np.max(-np.diag(DNA_MODEL.Q)) * rates.max())
    assert _code(eng.smap_sample, 7, eng.br, long_t[eng.br], 1) == ERR_UNSUPPORTED
    # PLK_ERR_ARG
    assert _code(eng.smap_sample, 7, eng.br[1:], t[eng.br[1:]], 1) == ERR_ARG            # a branch is missing
    assert _code(eng.smap_sample, 7, np.arange(8), t, 1) == ERR_ARG                      # the root is no branch
    assert _code(eng.smap_sample, 7, np.r_[eng.br[:-1], 8], t[eng.br], 1) == ERR_ARG     # outside the handle
    assert _code(eng.smap_sample, 7, np.r_[eng.br, 0], np.r_[t[eng.br], 0.1], 1) == ERR_ARG  # twice
    assert _code(eng.smap_sample, 6, eng.br, t[eng.br], 1) == ERR_ARG                    # not the root
    assert _code(sample, eng, 1, 0, 0) == ERR_ARG and _code(sample, eng, 1, 0, -3) == ERR_ARG
    Q = DNA_MODEL.Q.copy()
    Q[1, 2] = -1e-3
    assert _code(eng.smap_set_generator, 0, Q) == ERR_ARG
    assert _code(eng.smap_set_generator, 1, DNA_MODEL.Q) == ERR_ARG
    assert _code(eng.smap_set_types, 17, ty) == ERR_ARG and _code(eng.smap_set_types, 1, ty) == ERR_ARG
    sample(eng, 1, 4, 2)
    assert _code(eng.smap_states, 4, 0) == ERR_ARG                                       # nothing kept
    sample(eng, 1, 4, 2, keep=True)
    eng.smap_states(5, 0)
    assert _code(eng.smap_states, 6, 0) == ERR_ARG and _code(eng.smap_dwell, 3, 0) == ERR_ARG
    assert _code(eng.smap_jumps, 4, 7) == ERR_ARG                                        # the root has no branch
    eng.close()


def test_d_a_site_without_likelihood_is_bad():
    """A tip code whose row is all zero: the site's class total is 0.  States 255, counts and
    dwelling times 0, n_bad one per replicate, no error; every other site is the rule's."""
    tree, rates, probs = sc.TREE5, *G4
    t = sc.branch_lengths(8, 7, 7)
    codes = sc.tip_codes(tree, DNA_MODEL, rates, probs, t, 150, seed=21)
    codes[1, 77] = 15
    table = np.vstack([phylo.DNA.init_table, np.zeros((1, 4))])
    eng = make_engine(tree, [DNA_MODEL], rates, probs, codes, table, t, sc.ts_tv_types(), 2)
    eng.type_of_ = sc.ts_tv_types()
    sample(eng, 5, 0, 3, keep=True)
    assert eng.smap_bad() == 3
    ref, got = check_against_rule(eng, rates, probs, 5, [0, 1, 2])
    assert ref["bad"].sum() == 1 and ref["bad"][77]
    assert np.all(got["classes"][:, 77] == 255) and all(np.all(got["states"][v][:, 77] == 255) for v in range(8))
    sums, tal = eng.smap_sums(eng.br), eng.smap_tallies(np.arange(8))
    assert not sums["counts"][:, 77].any() and not sums["dwell"][:, 77].any()
    assert not tal["states"][:, 77].any() and not tal["classes"][77].any()
    for v in eng.br:
        assert not got["dwell"][int(v)][:, 77].any() and not got["jumps"][int(v)][:, 77].any()
    eng.close()
