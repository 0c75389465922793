"""GPU tests of plk_simulate (csrc/plk_sim.hpp) against the numpy restatement of the draw in
tests/sim_rule.py.  States and classes are integers and the draw is a pure function of
(seed, replicate, site, node): every comparison with the restatement is ==, with P read back
from the device through plk_get_pmatrix.

Shapes: 300, 130 and 70 sites (no multiple of 64, 128 or 256; one and two workgroups of 256), 1100
and 1300 sites (two workgroups of 1024), 4, 20 and 64 states, 1 to 4 classes, roots of two and
three sons, a node of five sons, node numbers out of preorder, 4-state trees whose tables fit LDS
(the default path), one whose tables do not (158 nodes) and one kept out of LDS by its tuning
switch; 2 x 4096 + 77 sites over two shards."""
import numpy as np
import pytest

import phylo
import plk
import sim_rule as sr
from conftest import set_tune

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -5
GUARD = plk.PLK_FLAG_NONNEG_GUARD

# (ops, root, tips)
TREE5 = ([(5, (0, 1), 0), (6, (2, 3), 0), (7, (5, 6, 4), 0)], 7, 5)            # the root has three sons
TREE7 = ([(7, (0, 1), 0), (8, (2, 3), 0), (9, (7, 8), 0), (10, (4, 5), 0), (11, (9, 10, 6), 0)], 11, 7)
TREE6 = ([(6, (0, 1), 0), (7, (2, 3), 0), (8, (6, 7), 0), (9, (8, 4, 5), 0)], 9, 6)
STAR5 = ([(6, (0, 1), 0), (7, (6, 2, 3), 0), (7, (4, 5), plk.PLK_OP_ACCUMULATE)], 7, 6)  # five sons at node 7
SCRAMBLED = ([(6, (0, 1), 0), (5, (2, 3), 0), (4, (6, 5), 0)], 4, 4)            # the root is the lowest internal node


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


def branch_lengths(n_nodes, root, seed):
    t = np.random.default_rng(seed).uniform(0.05, 0.6, size=n_nodes)
    t[root] = 0.0
    return t


def make_engine(tree, model, rates, probs, n, flags=GUARD, device=0, table=None, t_seed=7):
    ops, root, nt = tree
    nn = max(p for p, _, _ in ops) + 1
    eng = plk.Engine(device, model.S, len(rates), n, nt, nn - nt, 1, flags)
    if table is not None:
        eng.set_code_table(table)
    eng.set_category_rates(rates, probs)
    eng.set_root_frequencies(model.pi)
    eng.set_eigen(0, model.V, model.Vinv, model.lam)
    br = np.array([v for v in range(nn) if v != root], dtype=np.int32)
    eng.update_pmatrices(br, branch_lengths(nn, root, t_seed)[br])
    eng.n_nodes, eng.root, eng.ops, eng.br = nn, root, ops, br
    return eng


def device_P(eng):
    return {int(v): eng.get_pmatrix(int(v)) for v in eng.br}


def check_against_rule(eng, probs, pi, seed, replicate=0, site0=0, P=None):
    """Every node's states and the classes equal the restatement's; returns the latter."""
    cls, states = sr.simulate(eng.ops, eng.root, P or device_P(eng), probs, pi, seed, replicate, site0, eng.P)
    assert np.array_equal(eng.sim_classes(), cls), "classes"
    assert set(states) == set(range(eng.n_nodes))
    for v in range(eng.n_nodes):
        assert np.array_equal(eng.sim_states(v), states[v]), ("states", v)
    return cls, states


DNA_MODEL = phylo.t92(3.0, 0.4)
G4 = phylo.gamma_rates(4, 0.7)


# A. bitwise against the rule

def _balanced(n_taxa):
    et = phylo.engine_tree(phylo.balanced_tree(n_taxa, seed=3))
    return (phylo.split_ops(et.ops), et.root, et.n_tips)


@pytest.mark.parametrize("name", ["dna_root3_300", "protein_130", "codon_70", "five_sons", "scrambled", "dna_158_nodes",
                                  "dna_root3_1100_global"])
def test_states_and_classes_equal_the_rule(name, monkeypatch):
    """4 states stage the tables in LDS while they fit (workgroups of 1024 lanes: 1100 sites are two);
    158 nodes x 4 classes do not fit, and SIM_LDS=0 keeps a small tree in global memory."""
    if name == "dna_root3_1100_global":
        set_tune(monkeypatch, "SIM_LDS", "0")
    if name == "dna_158_nodes":
        tree, m, (rates, probs), n = _balanced(80), DNA_MODEL, G4, 300
        assert (tree[1] + 1) * 4 * 4 * 36 > 80 * 1024
    elif name == "protein_130":
        tree, m, rates, probs, n = TREE7, phylo.lg08(), np.array([0.4, 1.9]), np.array([0.6, 0.4]), 130
    elif name == "codon_70":
        tree, m, rates, probs, n = TREE6, phylo.yn98(2.0, 0.3), np.ones(1), np.ones(1), 70
    else:
        tree = {"dna_root3_300": TREE5, "five_sons": STAR5, "scrambled": SCRAMBLED, "dna_root3_1100_global": TREE5}[name]
        m, (rates, probs), n = DNA_MODEL, G4, 1100 if name.endswith("global") else 300
    eng = make_engine(tree, m, rates, probs, n)
    eng.simulate(eng.ops, eng.root, seed=12345, replicate=3, set_tips=False)
    assert eng.sim_launches() == 2
    cls, states = check_against_rule(eng, probs, m.pi, 12345, 3)
    assert len(np.unique(cls)) == len(rates)
    for v in range(eng.n_nodes):  # no degenerate sample: several states at every node
        assert len(np.unique(states[v])) >= 3
    eng.close()


# B. uploaded matrices

def test_identity_branch_copies_the_father():
    eng = make_engine(TREE5, DNA_MODEL, *G4, 300)
    eng.set_pmatrix(5, np.broadcast_to(np.eye(4), (4, 4, 4)))
    eng.simulate(eng.ops, eng.root, seed=9, set_tips=False)
    _, states = check_against_rule(eng, G4[1], DNA_MODEL.pi, 9)
    assert np.array_equal(eng.sim_states(5), eng.sim_states(7))
    assert len(np.unique(states[5])) == 4
    eng.close()


def test_rows_summing_to_a_half_take_the_fallback_index():
    eng = make_engine(TREE5, DNA_MODEL, *G4, 300)
    row = np.array([0.2, 0.2, 0.1, 0.0])  # trailing zero: the fallback is index 2, not the last
    eng.set_pmatrix(2, np.broadcast_to(row, (4, 4, 4)))
    eng.simulate(eng.ops, eng.root, seed=10, set_tips=False)
    check_against_rule(eng, G4[1], DNA_MODEL.pi, 10)
    u = sr.uniform(10, 0, np.arange(300, dtype=np.uint64), 2 + 2)
    fell = u >= sr.cumulative(row)[-1]
    assert fell.sum() >= 300 // 4
    got = eng.sim_states(2)
    assert (got[fell] == 2).all() and got.max() == 2
    eng.close()


# C. keys

def test_seed_replicate_and_site0_are_the_whole_key():
    n = 300
    eng = make_engine(TREE5, DNA_MODEL, *G4, n)
    ops, root = eng.ops, eng.root

    def run(e, **kw):
        e.simulate(ops, root, set_tips=False, **kw)
        return np.stack([e.sim_states(v) for v in range(e.n_nodes)] + [e.sim_classes()])

    a = run(eng, seed=5, replicate=2)
    assert np.array_equal(run(eng, seed=5, replicate=2), a)
    for other in (run(eng, seed=5, replicate=3), run(eng, seed=6, replicate=2)):
        for tip in range(5):
            assert (other[tip] != a[tip]).sum() > n // 4, tip
    shifted = run(eng, seed=5, replicate=2, site0=1000)
    big = make_engine(TREE5, DNA_MODEL, *G4, 1300)
    whole = run(big, seed=5, replicate=2)
    assert np.array_equal(shifted, whole[:, 1000:1300])
    assert np.array_equal(a, whole[:, :300])
    big.close()
    eng.close()


# D. shards

def test_two_shards_equal_one_device_bitwise():
    n = 2 * 4096 + 77
    br_t = None
    out = []
    for device in (0, [0, 0]):
        eng = make_engine(TREE5, DNA_MODEL, *G4, n, flags=GUARD | plk.PLK_FLAG_LNL_ONLY, device=device,
                          table=phylo.DNA.init_table)
        eng.simulate(eng.ops, eng.root, seed=77, replicate=1)
        st = np.stack([eng.sim_states(v) for v in range(eng.n_nodes)] + [eng.sim_classes()])
        br_t = branch_lengths(eng.n_nodes, eng.root, 7)[eng.br]
        lnl, blocks = eng.evaluate(eng.br, br_t, eng.ops, eng.root)
        _, site, _ = eng.root_loglik(eng.root, want_sites=True)
        out.append((st, lnl, blocks, site))
        if device != 0:
            assert eng.shard_count() == 2
            check_against_rule(eng, G4[1], DNA_MODEL.pi, 77, 1)
        eng.close()
    one, two = out
    assert np.array_equal(one[0], two[0])
    assert one[1] == two[1] and np.array_equal(one[2], two[2]) and np.array_equal(one[3], two[3])
    assert np.isfinite(one[1])


# E. the tip codes land where the traversals read them

def _site_lnl(eng):
    eng.update_partials(eng.ops)
    lnl, site, _ = eng.root_loglik(eng.root, want_sites=True)
    assert np.isfinite(site).all()
    return site


@pytest.mark.parametrize("kind", ["jit_tree4", "jit_treeM", "subtree_patterns"])
def test_traversals_read_the_simulated_tips(kind):
    if kind == "jit_treeM":
        m, rates, probs, table = phylo.lg08(), np.array([0.4, 1.9]), np.array([0.5, 0.5]), phylo.PROTEIN.init_table
    else:
        m, (rates, probs), table = DNA_MODEL, G4, phylo.DNA.init_table
    flags = GUARD | (plk.PLK_FLAG_SUBTREE_PATTERNS if kind == "subtree_patterns" else plk.PLK_FLAG_LNL_ONLY)
    n = 700
    tree = _balanced(16)
    nt = tree[2]
    eng = make_engine(tree, m, rates, probs, n, flags=flags, table=table)
    fresh = make_engine(tree, m, rates, probs, n, flags=flags, table=table)
    first = np.random.default_rng(1).integers(0, m.S, size=(nt, n)).astype(np.uint8)
    for t in range(nt):
        eng.set_tip_codes(t, first[t])
    site_first = _site_lnl(eng)
    assert eng.kernel_path() == kind
    seen = [site_first]
    for replicate in (0, 1):
        eng.simulate(eng.ops, eng.root, seed=31, replicate=replicate, set_tips=True)
        got = _site_lnl(eng)
        assert eng.kernel_path() == kind
        for t in range(nt):
            fresh.set_tip_codes(t, eng.sim_states(t))
        want = _site_lnl(fresh)
        assert np.allclose(got, want, rtol=1e-12, atol=0), replicate
        for earlier in seen:  # the data did change: a stale cache would repeat an earlier answer
            assert (np.abs(got - earlier) > 1e-9 * np.abs(got)).sum() > n // 2
        seen.append(got)
    eng.close()
    fresh.close()


def test_parsimony_pairs_are_dropped_by_a_simulation():
    eng = make_engine(TREE5, DNA_MODEL, *G4, 300, table=phylo.DNA.init_table)
    eng.simulate(eng.ops, eng.root, seed=1)
    eng.pars_update(eng.ops)
    before = eng.pars_score()
    eng.simulate(eng.ops, eng.root, seed=1, set_tips=False)  # nothing of the handle changes
    assert eng.pars_score() == before
    eng.simulate(eng.ops, eng.root, seed=2)
    with pytest.raises(plk.PlkError) as e:
        eng.pars_score()
    assert e.value.code == ERR_STATE
    eng.pars_update(eng.ops)
    assert eng.pars_score() > 0
    eng.close()


def test_state_code_permutation_into_a_table_of_six_codes():
    """Codes 0..3 of the table are T, G, C, A (state 3 - code); 4 and 5 are ambiguity rows that the
    simulation never writes."""
    table = np.vstack([np.eye(4)[::-1], [[1, 1, 0, 0], [1, 1, 1, 1]]]).astype(np.float64)
    perm = np.array([3, 2, 1, 0], dtype=np.uint8)
    n = 300
    eng = make_engine(TREE5, DNA_MODEL, *G4, n, table=table)
    eng.simulate(eng.ops, eng.root, seed=4, state_code=perm)
    check_against_rule(eng, G4[1], DNA_MODEL.pi, 4)
    got = _site_lnl(eng)
    fresh = make_engine(TREE5, DNA_MODEL, *G4, n, table=table)
    for t in range(5):
        fresh.set_tip_codes(t, perm[eng.sim_states(t)])
    assert np.allclose(got, _site_lnl(fresh), rtol=1e-12, atol=0)
    ident = make_engine(TREE5, DNA_MODEL, *G4, n, table=np.eye(4))
    for t in range(5):
        ident.set_tip_codes(t, eng.sim_states(t))
    assert np.allclose(got, _site_lnl(ident), rtol=1e-12, atol=0)
    for e in (eng, fresh, ident):
        e.close()


# F. errors

def code(fn, *args, **kw):
    with pytest.raises(plk.PlkError) as e:
        fn(*args, **kw)
    return e.value.code


def test_error_codes():
    ops, root, nt = TREE5
    m, (rates, probs) = DNA_MODEL, G4
    eng = plk.Engine(0, 4, 4, 300, 5, 3, 1, GUARD)
    # getters before any simulation
    assert code(eng.sim_states, 0) == ERR_STATE
    assert code(eng.sim_classes) == ERR_STATE
    # no P(t), then no rates, then no root frequencies
    assert code(eng.simulate, ops, root, 1, set_tips=False) == ERR_STATE
    P = np.stack([m.pij(0.1 * r) for r in rates])
    for b in range(6):
        eng.set_pmatrix(b, P)
    eng.set_category_rates(rates, probs)
    eng.set_root_frequencies(m.pi)
    assert code(eng.simulate, ops, root, 1, set_tips=False) == ERR_STATE  # branch 6 has no P(t)
    eng.set_pmatrix(6, P)
    eng2 = plk.Engine(0, 4, 4, 300, 5, 3, 1, GUARD)
    for b in range(7):
        eng2.set_pmatrix(b, P)
    assert code(eng2.simulate, ops, root, 1, set_tips=False) == ERR_STATE  # rates
    eng2.set_category_rates(rates, probs)
    assert code(eng2.simulate, ops, root, 1, set_tips=False) == ERR_STATE  # root frequencies
    eng2.close()
    # SET_TIPS before the code table; without it the call goes through
    assert code(eng.simulate, ops, root, 1, set_tips=True) == ERR_STATE
    eng.simulate(ops, root, 1, set_tips=False)
    eng.set_code_table(np.eye(4))
    assert code(eng.simulate, ops, root, 1, state_code=[0, 1, 2, 4]) == ERR_ARG
    eng.simulate(ops, root, 1, state_code=[0, 1, 2, 3])
    # the op rules
    assert code(eng.simulate, ops, 6, 1) == ERR_ARG                                  # root is not the last op's parent
    assert code(eng.simulate, ops[::-1], 5, 1) == ERR_ARG                           # not in postorder
    assert code(eng.simulate, [(5, (0, 1), 0), (7, (5, 0, 4), 0)], 7, 1) == ERR_ARG  # tip 0 has two fathers
    assert code(eng.simulate, [(5, (0, 9), 0)], 5, 1) == ERR_ARG                     # a node outside the handle
    assert code(eng.simulate, [], 7, 1) == ERR_ARG
    # getters on nodes outside the last simulated tree
    eng.simulate([(5, (0, 1), 0)], 5, 1, set_tips=False)
    assert eng.sim_states(5).shape == (300,)
    assert code(eng.sim_states, 2) == ERR_ARG
    assert code(eng.sim_states, 7) == ERR_ARG
    assert code(eng.sim_states, 8) == ERR_ARG
    assert code(eng.sim_states, -1) == ERR_ARG
    eng.close()


# G. launches

def test_two_launches_per_call():
    eng = make_engine(TREE7, DNA_MODEL, *G4, 130, table=phylo.DNA.init_table)
    for set_tips in (False, True):
        eng.simulate(eng.ops, eng.root, seed=3, set_tips=set_tips)
        assert eng.sim_launches() == 2
    eng.close()
