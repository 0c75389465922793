"""GPU tests of the plk_pars_* calls (csrc/plk_pars.hpp) against the numpy restatement of
tests/test_pars_cpu.py.  Integer arithmetic throughout: every quantity -- the score, the site
scores, every lower and upper pair, every NNI delta -- is compared with ==.

Shapes: pattern counts 1, 5, 257 and 1000 (no multiple of 4, 64 or 256; below and above one
workgroup), parsimony state counts 5 (1-byte sets, four patterns per lane), 21 (4-byte sets), 33
and 64 (8-byte sets), and five topologies (2-son and 3-son roots, an internal node of three sons,
an 8-taxon caterpillar, a random 12-taxon tree)."""
import numpy as np
import pytest

import phylo
import plk
import test_pars_cpu as pc

pytestmark = pytest.mark.gpu


def topology(name, rng):
    if name == "root2":
        return pc.random_tree(rng, 6, root_sons=2) + (6,)
    if name == "root3":
        return pc.random_tree(rng, 6, root_sons=3) + (6,)
    if name == "tri":
        return pc.random_tree(rng, 9, root_sons=2, tri_internal=True) + (9,)
    if name == "caterpillar8":
        return pc.caterpillar(8) + (8,)
    return pc.random_tree(rng, 12, root_sons=3) + (12,)


def make_engine(n_patterns, n_tips, n_internal, n_codes, codes, weights=None, masks=None, n_states_pars=None):
    eng = plk.Engine(0, 5, 1, n_patterns, n_tips, n_internal, 1, plk.PLK_FLAG_NONNEG_GUARD)
    eng.set_code_table(np.ones((n_codes, 5)))
    for t in range(n_tips):
        eng.set_tip_codes(t, codes[t])
    if weights is not None:
        eng.set_pattern_weights(np.asarray(weights, dtype=np.float64))
    if masks is not None:
        eng.pars_set_code_masks(n_states_pars, masks)
    return eng


def check_all(eng, rs):
    assert eng.pars_launches() == 1
    score, sites = eng.pars_score(want_sites=True)
    assert score == rs.score
    assert np.array_equal(sites.astype(np.int64), rs.site_scores)
    for v in range(rs.nt):
        s, c = eng.pars_get_edge(v)
        assert np.array_equal(s, rs.low(v)[0]) and not c.any()
    for v in rs.kids:
        s, c = eng.pars_get_edge(v)
        assert np.array_equal(s, rs.low(v)[0]), ("low set", v)
        assert np.array_equal(c.astype(np.int64), rs.low(v)[1]), ("low score", v)
        if v != rs.root:
            s, c = eng.pars_get_edge(v, upper=True)
            assert np.array_equal(s, rs.up(v)[0]), ("up set", v)
            assert np.array_equal(c.astype(np.int64), rs.up(v)[1]), ("up score", v)
    moves = rs.moves()
    if moves:
        son, uncle = zip(*moves)
        delta = eng.pars_nni_scores(son, uncle)
        assert eng.pars_launches() == 1
        assert delta.tolist() == [rs.delta(s, u) for s, u in moves]
    assert eng.pars_score() == rs.score


@pytest.mark.parametrize("topo", ["root2", "root3", "tri", "caterpillar8", "random12"])
@pytest.mark.parametrize("n_states", [5, 21, 33, 64])
@pytest.mark.parametrize("n_patterns", [1, 5, 257, 1000])
def test_pairs_scores_and_deltas_equal_the_restatement(n_patterns, n_states, topo):
    rng = np.random.default_rng([n_patterns, n_states, len(topo)])
    kids, root, n = topology(topo, rng)
    masks = pc.mask_table(rng, n_states)
    codes = pc.random_codes(rng, n, n_patterns, n_states, len(masks))
    w = pc.random_weights(rng, n_patterns)
    rs = pc.Restatement(kids, root, n, masks[codes], w)
    eng = make_engine(n_patterns, n, max(kids) - n + 1, len(masks), codes, w, masks, n_states)
    eng.pars_update(rs.ops())
    check_all(eng, rs)
    eng.close()


def test_golden_alignment_scores_nine():
    rs, codes, masks = pc.golden_case()
    eng = make_engine(codes.shape[1], rs.nt, len(rs.kids), len(masks), codes.astype(np.uint8), None, masks, 5)
    eng.pars_update(rs.ops())
    assert eng.pars_score() == 9
    check_all(eng, rs)
    eng.close()


def test_masks_default_to_the_code_table():
    rng = np.random.default_rng(3)
    kids, root = pc.random_tree(rng, 7, root_sons=3)
    dna = np.array([sum(1 << phylo.NUC.index(a) for a in phylo._DNA_ALIAS[c]) for c in phylo.DNA_CHARS], dtype=np.uint64)
    codes = pc.random_codes(rng, 7, 130, 4, 15)
    rs = pc.Restatement(kids, root, 7, dna[codes], np.ones(130, dtype=np.int64))
    eng = plk.Engine(0, 4, 1, 130, 7, len(kids), 1, plk.PLK_FLAG_NONNEG_GUARD)
    eng.set_code_table(phylo.DNA.init_table)
    for t in range(7):
        eng.set_tip_codes(t, codes[t])
    eng.pars_update(rs.ops())
    check_all(eng, rs)
    eng.close()


def test_scores_above_255_on_a_300_tip_caterpillar():
    """The states cycle along the tips, so almost every fold misses.  Two alternating states give
    only one change per two tips (150 here: after a union the next tip always meets it); a cycle
    of eight states gives seven changes per eight tips, 262, past what 8 bits hold -- and eight
    states still take the 1-byte sets with their packed 16-bit score adds."""
    n, P = 300, 64
    kids, root = pc.caterpillar(n)
    codes = ((np.arange(n)[:, None] + np.arange(P)[None, :]) % 8).astype(np.uint8)
    masks = np.uint64(1) << np.arange(8, dtype=np.uint64)
    rs = pc.Restatement(kids, root, n, masks[codes], np.ones(P, dtype=np.int64))
    assert rs.site_scores.min() > 255
    eng = make_engine(P, n, n - 1, 8, codes, None, masks, 8)
    eng.pars_update(rs.ops())
    score, sites = eng.pars_score(want_sites=True)
    assert score == rs.score and np.array_equal(sites.astype(np.int64), rs.site_scores)
    for v in (root, root - 1, n + 150):
        s, c = eng.pars_get_edge(v)
        assert np.array_equal(s, rs.low(v)[0]) and np.array_equal(c.astype(np.int64), rs.low(v)[1])
    s, c = eng.pars_get_edge(n + 1, upper=True)
    assert np.array_equal(s, rs.up(n + 1)[0]) and np.array_equal(c.astype(np.int64), rs.up(n + 1)[1])
    assert c.min() > 255
    moves = rs.moves()[::37]
    delta = eng.pars_nni_scores(*zip(*moves))
    assert delta.tolist() == [rs.delta(s, u) for s, u in moves]
    eng.close()


def test_likelihood_results_are_bitwise_unchanged_by_parsimony_calls():
    newick = "((A:0.01, B:0.02):0.03,(C:0.01,E:0.2):0.05,D:0.1);"
    et = phylo.engine_tree(phylo.Tree.from_newick(newick))
    rng = np.random.default_rng(5)
    P = 300
    states = rng.integers(0, 15, size=(et.n_tips, P)).astype(np.uint8)
    m = phylo.t92(3.0, 0.5)
    rates, probs = phylo.gamma_rates(4, 1.0)
    eng = plk.Engine(0, 4, 4, P, et.n_tips, et.n_internal, 1, plk.PLK_FLAG_NONNEG_GUARD)
    eng.set_code_table(phylo.DNA.init_table)
    for i in range(et.n_tips):
        eng.set_tip_codes(i, states[i])
    eng.set_category_rates(rates, probs)
    eng.set_root_frequencies(m.pi)
    eng.set_eigen(0, m.V, m.Vinv, m.lam)
    br = np.array([n for n in range(et.n_nodes) if n != et.root], dtype=np.int32)
    eng.update_pmatrices(br, et.brlen[br])
    ops = phylo.split_ops(et.ops)
    eng.update_partials(ops)
    lnl0, site0, _ = eng.root_loglik(et.root, want_sites=True)
    part0 = eng.get_partials(et.root)
    path0 = eng.kernel_path()
    eng.pars_update(ops)
    son, uncle = 0, [c for c in et.ops[-1][1] if c != et.ops[0][0]][0]
    assert et.ops[0][1][0] == 0 and et.ops[0][0] in et.ops[-1][1]
    eng.pars_nni_scores([son], [uncle])
    eng.pars_score(want_sites=True)
    assert eng.kernel_path() == path0
    lnl1, site1, _ = eng.root_loglik(et.root, want_sites=True)
    assert lnl1 == lnl0 and np.array_equal(site1, site0)
    assert np.array_equal(eng.get_partials(et.root), part0)
    eng.update_partials(ops)
    lnl2, site2, _ = eng.root_loglik(et.root, want_sites=True)
    assert lnl2 == lnl0 and np.array_equal(site2, site0)
    eng.close()


def code(fn, *args):
    with pytest.raises(plk.PlkError) as e:
        fn(*args)
    return e.value.code


ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5


def test_error_codes():
    kids, root = pc.caterpillar(5)
    rs = pc.Restatement(kids, root, 5, np.ones((5, 3), dtype=np.uint64), [1, 1, 1])
    codes = np.zeros((5, 3), dtype=np.uint8)
    eng = make_engine(3, 5, 4, 2, codes)
    assert code(eng.pars_set_code_masks, 65, [1, 2]) == ERR_UNSUPPORTED
    assert code(eng.pars_set_code_masks, 2, [1, 0]) == ERR_ARG
    assert code(eng.pars_set_code_masks, 2, [1, 4]) == ERR_ARG
    assert code(eng.pars_set_code_masks, 2, np.ones(257)) == ERR_ARG
    # before plk_pars_update
    assert code(eng.pars_score) == ERR_STATE
    assert code(eng.pars_get_edge, root) == ERR_STATE
    assert code(eng.pars_nni_scores, [0], [2]) == ERR_STATE
    # a non-integer weight, a negative one, one of 2^32
    for bad in (1.5, -1.0, 4294967296.0):
        eng.set_pattern_weights(np.array([1.0, bad, 1.0]))
        assert code(eng.pars_update, rs.ops()) == ERR_STATE
    eng.set_pattern_weights(np.array([1.0, 4294967295.0, 0.0]))
    eng.pars_update(rs.ops())
    assert eng.pars_score() == 0
    assert code(eng.pars_get_edge, root, True) == ERR_ARG       # up of the root
    assert code(eng.pars_get_edge, 0, True) == ERR_ARG          # up of a tip
    assert code(eng.pars_get_edge, 9) == ERR_ARG
    # caterpillar(5): 5 = (0, 1), 6 = (5, 2), 7 = (6, 3), root 8 = (7, 4)
    assert code(eng.pars_nni_scores, [root], [4]) == ERR_ARG    # a move at the root
    assert code(eng.pars_nni_scores, [7], [4]) == ERR_ARG       # a son of the root
    assert code(eng.pars_nni_scores, [0], [3]) == ERR_ARG       # 3 is no son of g = 6
    assert code(eng.pars_nni_scores, [0], [5]) == ERR_ARG       # u = p
    assert code(eng.pars_nni_scores, [0], [12]) == ERR_ARG
    assert code(eng.pars_nni_scores, [], []) == ERR_ARG
    assert eng.pars_nni_scores([0], [2]).tolist() == [0]
    # new weights, codes or masks drop the pairs
    eng.set_pattern_weights(np.ones(3))
    assert code(eng.pars_score) == ERR_STATE
    eng.pars_update(rs.ops())
    eng.set_tip_codes(0, codes[0])
    assert code(eng.pars_nni_scores, [0], [2]) == ERR_STATE
    eng.pars_update(rs.ops())
    eng.pars_set_code_masks(2, [1, 2])
    assert code(eng.pars_get_edge, root) == ERR_STATE
    # a tip without codes
    eng2 = plk.Engine(0, 5, 1, 3, 5, 4, 1, plk.PLK_FLAG_NONNEG_GUARD)
    eng2.set_code_table(np.ones((2, 5)))
    for t in range(4):
        eng2.set_tip_codes(t, codes[t])
    assert code(eng2.pars_update, rs.ops()) == ERR_STATE
    eng2.close()
    eng3 = plk.Engine(0, 5, 1, 3, 5, 4, 1, plk.PLK_FLAG_NONNEG_GUARD | plk.PLK_FLAG_SUBTREE_PATTERNS)
    assert code(eng3.pars_update, rs.ops()) == ERR_UNSUPPORTED
    eng3.close()
    # a multi-device handle (one device listed twice)
    eng4 = plk.Engine([0, 0], 5, 1, 8199, 5, 4, 1, plk.PLK_FLAG_NONNEG_GUARD)
    assert code(eng4.pars_set_code_masks, 2, [1, 2]) == ERR_UNSUPPORTED
    assert code(eng4.pars_update, rs.ops()) == ERR_UNSUPPORTED
    assert code(eng4.pars_score) == ERR_UNSUPPORTED
    eng4.close()
    eng.close()
