"""The task tail of the one-class-per-workgroup tree4 kernel on the MI355X (plk_jit.hpp
reduce_root_cls): pi[0..3] and the class probability are read once per launch into wave-uniform
registers in front of the task loop, and the rotation of the prefetched codes stands in front of a
task's root-term stores instead of at the top of the next task.

Neither changes an operation or its order, so every case compares lnL, per-pattern lnL and block
sums BITWISE across four engines -- the default (wave tasks from the pool), JIT_WP=0 (static
stride), JIT_WT=0 (super-blocks, which keep the rotation at the top) and JIT=0 (the interpreter,
which reads pi and the probabilities from memory).  Every engine evaluates twice on one handle,
the second time with another pi, other class probabilities and other branch lengths and no
recompile: the constants are per launch, not part of the program, so the second result must
differ from the first and both must match the oracle at the suite's 1e-12 per pattern (on the
engine's own P(t)).

The tree is the 7-taxon shape of tests/jit/jit_emit_wp.cpp's tree4q program: a quad, a cherry and
a tip under the root, ACGT data, lnL only, unscaled -- the generated kernel is plk_jit_tree4c
(kernel_path "jit_tree4" with a quad unit among its tables).  Pattern counts 1, 129 and 2 053 are
1, 2 and 17 tasks with a ragged last one; the 2 053 case runs on one workgroup of four waves
(JIT_WGS=1, JIT_G=4), so that every wave walks at least three tasks and the hoisted values and the
rotated codes are carried across iterations.
"""
import numpy as np
import pytest

import phylo
import plk
import workload
from conftest import set_tune
from test_gpu_parity import check, run_engine
from test_gpu_weights import Problem

pytestmark = pytest.mark.gpu
REL = 1e-12
LNL = plk.PLK_FLAG_LNL_ONLY
GUARD = plk.PLK_FLAG_NONNEG_GUARD

SCHEDULES = (("default", {}), ("wp0", {"JIT_WP": "0"}), ("wt0", {"JIT_WT": "0"}), ("interp", {"JIT": "0"}))
NEWICK = "(((t0:0.11,t1:0.23):0.07,(t2:0.31,t3:0.05):0.19):0.13,(t4:0.17,t5:0.29):0.09,t6:0.21);"
RATES = {1: np.ones(1), 2: np.array([0.25, 1.5]), 4: np.array([0.1, 0.45, 1.1, 2.6])}
PROBS = {1: (np.ones(1), np.ones(1)),
         2: (np.array([0.3, 0.7]), np.array([0.65, 0.35])),
         4: (np.array([0.1, 0.2, 0.3, 0.4]), np.array([0.37, 0.13, 0.28, 0.22]))}
PIS = {"skewed": (np.array([0.4, 0.1, 0.15, 0.35]), np.array([0.05, 0.45, 0.3, 0.2])),
       "zero": (np.array([0.45, 0.0, 0.2, 0.35]), np.array([0.3, 0.25, 0.45, 0.0]))}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


def _problem(C, n, pi):
    et = phylo.engine_tree(phylo.Tree.from_newick(NEWICK))
    m = phylo.gtr(1.2, 0.4, 0.6, 0.8, 0.5, 0.30, 0.20, 0.25, 0.25)
    wl = workload.Workload("m", et, [m], None, RATES[C], PROBS[C][0], m.pi, phylo.DNA, n, False, True, 5)
    states = wl.simulate(0, n).astype(np.int32)
    assert states.max() < 4                                  # ACGT only: four codes in use
    p = Problem.of(et, m, phylo.DNA, RATES[C], PROBS[C][0], states)
    p.pi = pi
    return p


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), (what, np.flatnonzero(a[1] != b[1])[:8])
    assert np.array_equal(a[2], b[2]), what


def _case(monkeypatch, C, n, pis, flags, tune):
    for k, v in tune.items():
        set_tune(monkeypatch, k, v)
    pi1, pi2 = PIS[pis]
    probs1, probs2 = PROBS[C]
    p = _problem(C, n, pi1)
    t2 = p.et.brlen[p.br] * 1.25 + 0.01
    ref = None
    for name, keys in SCHEDULES:
        with monkeypatch.context() as mp:
            for k, v in keys.items():
                set_tune(mp, k, v)
            eng = p.engine(flags)
            first = run_engine(eng, p.et)
            o1 = p.oracle(eng, probs=probs1, pi=pi1) if ref is None else None
            # another pi, other probabilities, other branch lengths: same handle, same program
            eng.set_root_frequencies(pi2)
            eng.set_category_rates(RATES[C], probs2)
            eng.update_pmatrices(p.br, t2)
            second = run_engine(eng, p.et)
            assert eng.kernel_path() == ("jit_tree4" if name != "interp" else "tree4"), name
            if name != "interp":
                assert eng.traversal_work()["table_nodes"] > 0, name
        assert first[0] != second[0] and not np.array_equal(first[1], second[1]), name
        assert len(first[1]) == n and len(second[1]) == n
        if ref is None:
            o2 = p.oracle(eng, probs=probs2, pi=pi2)
            eng.close()
            print(f"C {C} n {n} {pis}: lnL {first[0]!r} -> {second[0]!r}; oracle {o1[0]!r} -> {o2[0]!r}")
            check(first[0], first[1], o1[0], o1[1], REL)
            check(second[0], second[1], o2[0], o2[1], REL)
            ref = (first, second)
            continue
        eng.close()
        _same(first, ref[0], name + " first")
        _same(second, ref[1], name + " second")


# one workgroup of four waves for the 17 tasks of 2 053 patterns: 5, 4, 4, 4 tasks per wave under
# the static stride, at least three per wave from the pool
MANY = {"JIT_WGS": "1", "JIT_G": "4"}


@pytest.mark.parametrize("n", [1, 129, 2053])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_tail_bitwise_across_schedules(C, n, monkeypatch):
    _case(monkeypatch, C, n, "skewed", LNL | GUARD, MANY if n == 2053 else {})


@pytest.mark.parametrize("guard", [True, False], ids=["guard", "clamp"])
@pytest.mark.parametrize("n", [129, 2053])
def test_zero_frequency_under_both_root_rules(n, guard, monkeypatch):
    """A pi with an entry equal to 0 (another entry in the second evaluation): its root terms are
    <= 0 and dropped under the guard, and added as zeros under the clamp rule."""
    _case(monkeypatch, 4, n, "zero", LNL | (GUARD if guard else 0), MANY if n == 2053 else {})


def test_clamp_rule_skewed_pi(monkeypatch):
    _case(monkeypatch, 2, 2053, "skewed", LNL, MANY)


def test_the_shape_has_a_quad_unit(monkeypatch):
    """The cases above run the one-class-per-workgroup kernel: with quad units switched off
    (JIT_QUAD_KB=0) the same problem builds fewer table nodes."""
    p = _problem(4, 129, PIS["skewed"][0])
    tn = []
    for kb in (None, "0"):
        with monkeypatch.context() as mp:
            if kb is not None:
                set_tune(mp, "JIT_QUAD_KB", kb)
            eng = p.engine(LNL | GUARD)
            run_engine(eng, p.et)
            tn.append(eng.traversal_work()["table_nodes"])
            eng.close()
    assert tn[0] > tn[1] > 0, tn
