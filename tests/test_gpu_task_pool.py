"""The workgroup task pool on the MI355X (plk_jit.hpp JitShape::wp; PLK_TUNE JIT_WP): workgroup x
of a (fragment, class) owns the tasks x, x + gridDim.x, ... and its waves draw them from one LDS
counter, whichever wave is free next.

Which wave computes a task changes no operation and no order, so every case compares lnL,
per-pattern lnL and block sums BITWISE across four engines -- JIT_WP=1 (the pool), JIT_WP=0 (wave
tasks on the static stride), JIT_WT=0 (super-blocks) and JIT=0 (the interpreter).  Every engine
evaluates twice, the second time with other branch lengths: a task that the pool skipped the
second time would leave the first evaluation's class terms, and they would show.  Both
evaluations are compared across the engines, and the pool engine's second one against the oracle
at 1e-12 on the engine's own P(t) (the first one's P(t) are gone by then; it is tied to the
other three engines bitwise).  The pool changes neither the program nor its flops:
kernel_path() and plk_traversal_work are those of the static stride.

Unless a case says otherwise: the 64-taxon balanced tree, ACGT data, PLK_FLAG_LNL_ONLY, C = 4.
"""
import numpy as np
import pytest

import plk
import workload
from conftest import set_tune
from test_gpu_configs import _engine_pmats, _oracle
from test_gpu_parity import check, run_engine
from test_gpu_weights import Problem

pytestmark = pytest.mark.gpu
REL = 1e-12
LNL = plk.PLK_FLAG_LNL_ONLY
GUARD = plk.PLK_FLAG_NONNEG_GUARD

# (JIT_WT=1 is spelled out: the every-class-in-the-wave kernel keeps super-blocks by default)
SCHEDULES = (("wp1", {"JIT_WT": "1", "JIT_WP": "1"}), ("wp0", {"JIT_WT": "1", "JIT_WP": "0"}),
             ("wt0", {"JIT_WT": "0"}), ("interp", {"JIT": "0"}))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), (what, np.flatnonzero(a[1] != b[1])[:8])
    assert np.array_equal(a[2], b[2]), what


def _four(monkeypatch, tune, make, evaluate, path="jit_tree4"):
    """Under each schedule: an engine from `make`, evaluate(eng, 0) then evaluate(eng, 1) (other
    branch lengths).  Both results bitwise equal across the four engines.  Returns the pool engine
    (open) and its second result."""
    for k, v in tune.items():
        set_tune(monkeypatch, k, v)
    keep, ref, work = None, None, None
    for name, keys in SCHEDULES:
        with monkeypatch.context() as mp:
            for k, v in keys.items():
                set_tune(mp, k, v)
            eng = make()
            res = [evaluate(eng, 0), evaluate(eng, 1)]
            assert eng.kernel_path() == (path if name != "interp" else "tree4"), name
            if name in ("wp1", "wp0"):   # the pool: same program, same flops
                w = (eng.kernel_path(), eng.traversal_work())
                assert work is None or w == work, (w, work)
                work = w
        assert res[0][0] != res[1][0], name                   # the branch lengths did change
        if ref is None:
            keep, ref = eng, res
            continue
        _same(res[0], ref[0], name + " first")
        _same(res[1], ref[1], name + " second")
        eng.close()
    return keep, ref[1]


def _problem_case(monkeypatch, p, tune, flags=LNL | GUARD):
    t2 = p.et.brlen[p.br] * 1.25 + 0.01

    def evaluate(eng, k):
        if k:
            eng.update_pmatrices(p.br, t2)
        return run_engine(eng, p.et)

    eng, (lnl, site, _) = _four(monkeypatch, tune, lambda: p.engine(flags), evaluate)
    lo, so = p.oracle(eng)                                    # on the second evaluation's P(t)
    eng.close()
    assert len(site) == p.n
    check(lnl, site, lo, so, REL)


@pytest.mark.parametrize("n", [1, 129, 2049, 5000])
def test_ragged_sizes(n, monkeypatch):
    """1 pattern: one task; 129: a second task with one valid pattern; 2049: 17 tasks on the 16
    waves of one workgroup, so exactly one wave draws a task from the pool; 5000: 40 tasks."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", n), {})


@pytest.mark.parametrize("wgs", [1, 2])
def test_many_draws_per_wave(wgs, monkeypatch):
    """JIT_WGS caps the workgroups per (fragment, class): 20 000 patterns are 157 tasks over 16
    (32) waves, about ten (five) draws per wave; with two workgroups one owns 79 tasks and the
    other 78."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 20000), {"JIT_WGS": str(wgs)})


def test_fewer_tasks_than_waves(monkeypatch):
    """JIT_G=16 with 300 patterns: 3 tasks, 13 waves skip the loop, and the first ticket drawn
    from the pool (16) is already past the end."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 300), {"JIT_G": "16"})


@pytest.mark.parametrize("C", [1, 2])
def test_class_counts(C, monkeypatch):
    _problem_case(monkeypatch, Problem(4, C, "balanced64", 700), {})


def test_one_pattern_per_lane(monkeypatch):
    """JIT_PW=1: tasks of 64 patterns, two per 128-pattern tile."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 700), {"JIT_PW": "1"})


def test_retune_on_a_live_handle(monkeypatch):
    """PLK_TUNE is read again at every call, so a handle that has evaluated must follow a tune that
    changes afterwards: one engine evaluates under the default tunes, JIT_PW=1, JIT_PW=2, JIT_WP=0
    and JIT_G=16 in turn, each time bitwise equal to a fresh engine under the same tunes.  700
    patterns pad to six 128-pattern tasks at PW = 2 and twelve 64-pattern tasks at PW = 1: a kernel
    compiled for one and launched with the other's task count cannot give the per-pattern values."""
    p = Problem(4, 4, "balanced64", 700)
    live = p.engine(LNL | GUARD)
    for tune in ({}, {"JIT_PW": "1"}, {"JIT_PW": "2"}, {"JIT_WP": "0"}, {"JIT_G": "16"}):
        with monkeypatch.context() as mp:
            for k, v in tune.items():
                set_tune(mp, k, v)
            res = run_engine(live, p.et)
            assert live.kernel_path() == "jit_tree4", tune
            fresh = p.engine(LNL | GUARD)
            ref = run_engine(fresh, p.et)
            fresh.close()
        assert len(res[1]) == p.n
        _same(res, ref, str(tune))
    live.close()


@pytest.mark.parametrize("guard", [True, False], ids=["guard", "noguard"])
def test_root_rules(guard, monkeypatch):
    """Both root rules: terms <= 0 dropped per state and class | every term added and the site
    sum clamped."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 600), {}, flags=LNL | (GUARD if guard else 0))


def test_clock_waves_show_the_deal_and_add_up(monkeypatch):
    """PLK_DEBUG_CLOCK=3, per-wave records (Engine.clock_waves): 5 000 patterns are 40 tasks per
    class over 3 workgroups of 16 waves -- the pool deals 14, 13, 13 where the static stride
    deals 16, 16, 8 -- and the stamps of an evaluation split over two plk_update_partials calls
    add up into one record instead of the second call's overwriting the first's."""
    monkeypatch.setenv("PLK_DEBUG_CLOCK", "3")
    p = Problem(4, 4, "balanced64", 5000)
    n_tasks = (p.n + 127) // 128
    deals = {}
    for wp in ("1", "0"):
        with monkeypatch.context() as mp:
            set_tune(mp, "JIT_WP", wp)
            eng = p.engine(LNL | GUARD)
            res = run_engine(eng, p.et, sites=False)
            rec1 = eng.clock_records()
            waves1, gx = eng.clock_waves()
            eng.update_partials(p.ops)
            eng.update_partials(p.ops)
            res2 = eng.root_loglik(p.et.root, want_sites=False, want_blocks=True)
            rec2 = eng.clock_records()
            waves2, _ = eng.clock_waves()
            eng.close()
        assert res2[0] == res[0]
        assert rec1.shape == (1, 5) and rec2.shape == (1, 5)             # the record keeps its width
        assert gx == 3 and waves1.shape == (p.C * gx, 16, 2)
        assert waves1[:, :, 1].sum() == p.C * n_tasks and rec1[0, 4] == (waves1[:, :, 1] > 0).sum()
        assert np.all((waves1[:, :, 0] > 0) == (waves1[:, :, 1] > 0))
        assert waves2.shape == (2 * p.C * gx, 16, 2) and waves2[:, :, 1].sum() == 2 * p.C * n_tasks
        assert rec2[0, 4] == 2 * rec1[0, 4]
        deals[wp] = waves1[:, :, 1].sum(axis=1).reshape(p.C, gx)
    assert np.all(deals["1"] == [14, 13, 13]), deals["1"]
    assert np.all(deals["0"] == [16, 16, 8]), deals["0"]


def test_multi_tier_512_taxa_rescaled(monkeypatch):
    """The 512-taxon rooted non-homogeneous tree with rescaling: the every-class-in-the-wave
    direct-code kernel (JIT_DC_CIW=1) with wave tasks and the pool -- several tiers, stored
    fragment roots and scale counts."""
    n = 6000
    wl = workload.make_workload("nh_gtr_g4_dna_2M_512", n_patterns=n)
    states = wl.simulate(0, n).astype(np.int32)
    brlen2 = wl.et.brlen * 1.1

    class Ev(workload.Evaluator):   # (the engine's queries on the evaluator, for _four)
        def kernel_path(self):
            return self.eng.kernel_path()

        def traversal_work(self):
            return self.eng.traversal_work()

        def close(self):
            self.eng.close()

    def evaluate(ev, k):
        lnl, _, blocks = ev.step(brlen2 if k else None)
        lnl_r, site, _ = ev.eng.root_loglik(wl.et.root, want_sites=True)
        assert lnl_r == lnl
        return lnl, site, blocks

    ev, (lnl, site, _) = _four(monkeypatch, {"JIT_DC_CIW": "1"},
                               lambda: Ev(wl, 0, 0, n, states=states, extra_flags=LNL), evaluate)
    lo, so = _oracle(wl, states, pmats=_engine_pmats(ev.eng, wl.et), use_patterns=True)
    ev.close()
    assert np.all(np.isfinite(site)) and site.min() < -256 * np.log(2)     # rescaled
    assert abs(lnl - lo) <= REL * abs(lo), (lnl, lo)
    assert np.allclose(site, so, rtol=REL, atol=0)
