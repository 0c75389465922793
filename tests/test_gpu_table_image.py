"""The table image of the one-class-per-workgroup tree4 kernel on the MI355X (plk_jit.hpp
JitShape::img): the traversal's tables are built once per class by the builder kernel that stands
in for pmat4_kernel's launch (plk_update_pmatrices), and a traversal workgroup's prologue copies
its fragment's and class's image into LDS.

No operation or its order changes, so every comparison is BITWISE (== on float64,
np.array_equal) and against a handle that never sees the code under test: the interpreter
(PLK_TUNE JIT=0), whose P(t) and tip tables come from pmat4_kernel and whose tables are built by
nobody.  What is compared: lnL, block sums, per-pattern lnL, and pmats of every branch.

Which path served is read from the table-launch counter (PLK_TIME_TABLES): a stale image costs
one builder launch in front of the traversal, a request that went through the builder costs none.

Trees: the 7-tip tree of tests/jit/jit_emit_wp.cpp (a quad, a cherry and a tip under the root), a
16-tip balanced tree (4 quads) and the 64-tip balanced tree (16 quads).  Patterns 130, 257 and
4 097: ragged tasks, the last one crosses a 4 096-pattern block.  ACGT data, lnL only, unscaled.
"""
import numpy as np
import pytest

import phylo
import plk
import workload
from conftest import set_tune
from test_gpu_parity import engine_for, run_engine
from test_gpu_weights import Problem

pytestmark = pytest.mark.gpu
LNL = plk.PLK_FLAG_LNL_ONLY | plk.PLK_FLAG_NONNEG_GUARD

T7 = "(((t0:0.11,t1:0.23):0.07,(t2:0.31,t3:0.05):0.19):0.13,(t4:0.17,t5:0.29):0.09,t6:0.21);"
RATES = {1: np.ones(1), 2: np.array([0.25, 1.5]), 4: np.array([0.1, 0.45, 1.1, 2.6])}
PROBS = {1: np.ones(1), 2: np.array([0.3, 0.7]), 4: np.array([0.1, 0.2, 0.3, 0.4])}
M1 = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.30, 0.20, 0.25, 0.25)
M2 = phylo.gtr(0.7, 1.3, 0.9, 0.5, 1.1, 0.22, 0.28, 0.31, 0.19)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


_PROBLEMS = {}


def _problem(tree, C, n):
    """Seeded problem, made once per (tree, C, n) and never changed."""
    key = (tree, C, n)
    if key not in _PROBLEMS:
        t = phylo.Tree.from_newick(T7) if tree == "t7" else phylo.balanced_tree(int(tree[1:]), seed=7, lo=0.05, hi=0.4)
        et = phylo.engine_tree(t)
        wl = workload.Workload("m", et, [M1], None, RATES[C], PROBS[C], M1.pi, phylo.DNA, n, False, True, 5)
        states = wl.simulate(0, n).astype(np.int32)
        assert states.max() < 4                                  # ACGT only: four codes in use
        _PROBLEMS[key] = Problem.of(et, M1, phylo.DNA, RATES[C], PROBS[C], states)
    return _PROBLEMS[key]


def _engine(p, models=None, model_of_node=None):
    """A handle on the problem with P(t) of every branch requested once (before any plan exists).
    Whether it becomes the reference is decided where it traverses (_run: PLK_TUNE JIT=0 is read
    when the program is cut), so a reference handle never compiles a kernel and its requests
    always go to pmat4_kernel."""
    eng = engine_for(p.et, 4, p.C, p.n, p.states, p.alph.init_table, p.rates, p.probs, p.pi, models or [p.m],
                     model_of_node=model_of_node, flags=LNL)
    eng.set_timing(plk.PLK_TIME_PARTIALS | plk.PLK_TIME_TABLES)
    return eng


def _run(eng, p, monkeypatch, interp):
    with monkeypatch.context() as mp:
        if interp:
            set_tune(mp, "JIT", "0")
        res = run_engine(eng, p.et)
        assert eng.kernel_path() == ("tree4" if interp else "jit_tree4")
        if not interp:
            assert eng.traversal_work()["table_nodes"] > 0
    return res


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), (what, np.flatnonzero(a[1] != b[1])[:8])
    assert np.array_equal(a[2], b[2]), what


def _same_pmats(eng, ref, p, what):
    for b in p.br:
        assert np.array_equal(eng.get_pmatrix(int(b)), ref.get_pmatrix(int(b))), (what, int(b))


def _tables(eng):
    return eng.get_timing()["table_launches"]


def _lengths(p, k):
    """The k-th set of branch lengths (k = 0: the tree's own)."""
    return p.et.brlen[p.br] * (1.0 + 0.25 * k) + 0.01 * k


SHAPES = [(t, C, n) for t in ("t7", "t16", "t64") for C in (1, 2, 4) for n in (130, 257, 4097)]


@pytest.mark.parametrize("tree,C,n", SHAPES)
def test_first_and_later_evaluations_equal_the_interpreter(tree, C, n, monkeypatch):
    """The first evaluation (no plan at P(t) time: pmat4_kernel, then one builder launch from
    memory), then two more with other lengths on the same handle (the builder serves the request:
    no table launch) -- each equal to the interpreter, so no row of an earlier image survives."""
    p = _problem(tree, C, n)
    eng, ref = _engine(p), _engine(p)
    first = _run(eng, p, monkeypatch, False)
    assert _tables(eng) == 1                                     # the stale image, rebuilt from pmats / tipP
    _same(first, _run(ref, p, monkeypatch, True), "first")
    assert len(first[1]) == n
    for k in (1, 2):
        eng.update_pmatrices(p.br, _lengths(p, k))
        ref.update_pmatrices(p.br, _lengths(p, k))
        res = _run(eng, p, monkeypatch, False)
        assert _tables(eng) == 1                                 # built with the request
        _same(res, _run(ref, p, monkeypatch, True), f"lengths {k}")
        assert res[0] != first[0]
        _same_pmats(eng, ref, p, f"lengths {k}")
    assert _tables(ref) == 0
    eng.close()
    ref.close()


@pytest.mark.parametrize("tree", ["t7", "t16"])
def test_two_models_and_zero_length_branches(tree, monkeypatch):
    """Two models on one handle, and t == 0 (the identity rule) on a third of the branches in
    turn, tips, cherries and quads among them: pmats of every branch and the results equal the
    pmat4_kernel / interpreter handle's."""
    p = _problem(tree, 4, 257)
    mon = np.arange(p.et.n_nodes) % 2
    mi = mon[p.br].astype(np.int32)
    eng = _engine(p, [M1, M2], mon)
    ref = _engine(p, [M1, M2], mon)
    _same(_run(eng, p, monkeypatch, False), _run(ref, p, monkeypatch, True), "first")
    for r in range(3):
        t = _lengths(p, 1).copy()
        t[r::3] = 0.0
        eng.update_pmatrices(p.br, t, mi)
        ref.update_pmatrices(p.br, t, mi)
        _same_pmats(eng, ref, p, f"zero {r}")
        _same(_run(eng, p, monkeypatch, False), _run(ref, p, monkeypatch, True), f"zero {r}")
        for b in p.br[r::3]:
            assert np.array_equal(eng.get_pmatrix(int(b)), np.broadcast_to(np.eye(4), (4, 4, 4)))
    assert _tables(eng) == 1
    eng.close()
    ref.close()


@pytest.mark.parametrize("tree,C", [("t7", 4), ("t16", 4), ("t16", 2), ("t64", 4)])
def test_subset_requests_on_a_live_handle(tree, C, monkeypatch):
    """After a full evaluation, one branch changes at a time -- every branch of the tree in turn
    (for t64 every fifth): a tip inside a quad, a cherry, a quad's own branch, a branch above the
    quads.  The builder computes that branch's rows itself and reads the others as stored; each
    result equals a fresh interpreter handle that evaluates all branches with the same lengths."""
    p = _problem(tree, C, 257)
    eng = _engine(p)
    _run(eng, p, monkeypatch, False)
    t = _lengths(p, 1).copy()
    eng.update_pmatrices(p.br, t)
    _run(eng, p, monkeypatch, False)
    base = _tables(eng)
    for i in range(0, len(p.br), 5 if tree == "t64" else 1):
        t[i] = t[i] * 1.7 + 0.03
        eng.update_pmatrices(p.br[i:i + 1], t[i:i + 1])
        res = _run(eng, p, monkeypatch, False)
        fresh = _engine(p)
        fresh.update_pmatrices(p.br, t)
        _same(res, _run(fresh, p, monkeypatch, True), f"branch {int(p.br[i])}")
        _same_pmats(eng, fresh, p, f"branch {int(p.br[i])}")
        fresh.close()
    assert _tables(eng) == base                                  # every subset request went through the builder
    eng.close()


def test_stale_image_is_rebuilt(monkeypatch):
    """P(t) by another route -- plk_set_pmatrix on every branch in turn (a quad's among them), and a
    request with derivative masks -- leaves the image behind: the next traversal rebuilds it from
    memory (one table launch) and equals the interpreter."""
    p = _problem("t7", 4, 257)
    eng, ref = _engine(p), _engine(p)
    _run(eng, p, monkeypatch, False)
    _run(ref, p, monkeypatch, True)
    eng.update_pmatrices(p.br, _lengths(p, 1))
    ref.update_pmatrices(p.br, _lengths(p, 1))
    _same(_run(eng, p, monkeypatch, False), _run(ref, p, monkeypatch, True), "live")
    n = _tables(eng)
    other = _engine(p)
    other.update_pmatrices(p.br, _lengths(p, 3))
    for b in p.br:
        P = other.get_pmatrix(int(b))
        eng.set_pmatrix(int(b), P)
        ref.set_pmatrix(int(b), P)
        _same(_run(eng, p, monkeypatch, False), _run(ref, p, monkeypatch, True), f"set_pmatrix {int(b)}")
        n += 1
        assert _tables(eng) == n
    other.close()
    mask = plk.PLK_DERIV_P | plk.PLK_DERIV_DP | plk.PLK_DERIV_D2P
    eng.update_pmatrices(p.br, _lengths(p, 2), deriv_mask=mask)
    ref.update_pmatrices(p.br, _lengths(p, 2), deriv_mask=mask)
    _same(_run(eng, p, monkeypatch, False), _run(ref, p, monkeypatch, True), "derivative masks")
    assert _tables(eng) == n + 1
    # ... and the builder takes over again with the next plain request
    eng.update_pmatrices(p.br, _lengths(p, 1))
    ref.update_pmatrices(p.br, _lengths(p, 1))
    _same(_run(eng, p, monkeypatch, False), _run(ref, p, monkeypatch, True), "live again")
    assert _tables(eng) == n + 1
    eng.close()
    ref.close()


@pytest.mark.parametrize("tree", ["t7", "t16"])
def test_separate_calls_equal_evaluate(tree, monkeypatch):
    """plk_update_pmatrices + plk_update_partials + the root reduction against plk_evaluate, on
    the first evaluation of a handle and on later ones, and both against the interpreter."""
    p = _problem(tree, 4, 4097)
    a, b, ref = _engine(p), _engine(p), _engine(p)
    for k in (1, 2, 3):
        a.update_pmatrices(p.br, _lengths(p, k))
        ra = _run(a, p, monkeypatch, False)
        lnl, blocks = b.evaluate(p.br, _lengths(p, k), p.ops, p.et.root)
        assert b.kernel_path() == "jit_tree4"
        assert lnl == ra[0] and np.array_equal(blocks, ra[2]), k
        ref.update_pmatrices(p.br, _lengths(p, k))
        _same(ra, _run(ref, p, monkeypatch, True), f"interpreter {k}")
        _same_pmats(b, ref, p, f"evaluate {k}")
    assert _tables(a) == 1 and _tables(b) == 1
    for e in (a, b, ref):
        e.close()
