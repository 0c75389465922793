"""Wave tasks on the MI355X (plk_jit.hpp JitShape::wt; PLK_TUNE JIT_WT, default 1 where the
direct-code kernel has one wave per pattern group): every wave walks its own 64 * PW-pattern
tasks, static stride or one ticket per task, and the loop has no barrier.

Which wave computes a pattern changes no operation and no order, so every case compares lnL,
per-pattern lnL and block sums BITWISE across three engines -- JIT_WT=1, JIT_WT=0 (the
super-block schedule) and JIT=0 (the interpreter) -- and the wave-task engine against the
oracle at 1e-12 on the engine's own P(t).  Every engine evaluates twice and must return the
same doubles: the second evaluation starts from the counters the first one's exit ticket left.

Unless a case says otherwise: the 64-taxon balanced tree (the smallest with the 16 quads of a
fragment), ACGT data, PLK_FLAG_LNL_ONLY, C = 4.
"""
import numpy as np
import pytest

import negroot
import plk
import workload
from conftest import set_tune
from test_gpu_configs import _engine_pmats, _oracle
from test_gpu_parity import check, engine_for, engine_pmats, oracle_for, run_engine
from test_gpu_root_rules import _engine as negroot_engine
from test_gpu_weights import Problem

pytestmark = pytest.mark.gpu
REL = 1e-12
LNL = plk.PLK_FLAG_LNL_ONLY
GUARD = plk.PLK_FLAG_NONNEG_GUARD

SCHEDULES = (("wt1", {"JIT_WT": "1"}), ("wt0", {"JIT_WT": "0"}), ("interp", {"JIT": "0"}))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


def _three(monkeypatch, tune, make, evaluate, path="jit_tree4", quads=True):
    """Run `evaluate` twice on an engine from `make` under each schedule; the results of the
    three engines bitwise equal.  Returns the wave-task engine (open) and its result."""
    for k, v in tune.items():
        set_tune(monkeypatch, k, v)
    keep, ref = None, None
    for name, keys in SCHEDULES:
        with monkeypatch.context() as mp:
            for k, v in keys.items():
                set_tune(mp, k, v)
            eng = make()
            res = evaluate(eng)
            again = evaluate(eng)
            assert eng.kernel_path() == (path if name != "interp" else "tree4"), name
            if name == "wt1" and quads:
                assert eng.traversal_work()["table_nodes"] > 0
        lnl, site, blocks = res
        assert lnl == again[0] and np.array_equal(site, again[1]) and np.array_equal(blocks, again[2]), name
        if ref is None:
            keep, ref = eng, res
            continue
        assert lnl == ref[0], (name, lnl, ref[0])
        assert np.array_equal(site, ref[1]), (name, np.flatnonzero(site != ref[1])[:8])
        assert np.array_equal(blocks, ref[2]), name
        eng.close()
    return keep, ref


def _problem_case(monkeypatch, p, tune, flags=LNL | GUARD, **kw):
    eng, (lnl, site, _) = _three(monkeypatch, tune, lambda: p.engine(flags), lambda e: run_engine(e, p.et), **kw)
    lo, so = p.oracle(eng)
    eng.close()
    assert len(site) == p.n
    check(lnl, site, lo, so, REL)


# ---------------------------------------------------------------- ragged and tiny sizes

@pytest.mark.parametrize("n", [1, 7, 129, 2049, 5000])
def test_ragged_sizes(n, monkeypatch):
    """1 and 7 patterns: one task, mostly padding; 129: a second task with one valid pattern;
    2049: one task past a 2048-pattern super-block of the parent schedule; 5000."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", n), {})


# ---------------------------------------------------------------- root rules

@pytest.mark.parametrize("guard", [True, False], ids=["guard", "noguard"])
@pytest.mark.parametrize("negative", [False, True], ids=["plain", "negterms"])
def test_root_rules(guard, negative, monkeypatch):
    """Both root rules (terms <= 0 dropped per state and class | every term added and the site
    sum clamped), on ordinary matrices and on matrices with a negative shift (tests/negroot.py),
    where the two rules give different site likelihoods."""
    n = 600
    flags = LNL | (GUARD if guard else 0)
    if not negative:
        _problem_case(monkeypatch, Problem(4, 4, "balanced64", n), {}, flags=flags)
        return
    et, m, init, states, rates, probs, pi, pm = negroot.problem(4, 4, 64, n, seed=172)
    _, pm2, census = negroot.choose(et, states, init, pm, pi, probs, "mixed")
    assert census["neg_terms"] > 0
    eng, (lnl, site, _) = _three(monkeypatch, {},
                                 lambda: negroot_engine(et, 4, 4, n, init, states, rates, probs, pi, pm2, flags),
                                 lambda e: run_engine(e, et))
    eng.close()
    lo, so = negroot.oracle_sites(et, states, init, pm2, probs, pi, False, nh_root=not guard)
    negroot.same_sites(site, so, REL)
    assert abs(lnl - lo) <= REL * abs(lo), (lnl, lo)


# ---------------------------------------------------------------- class counts

@pytest.mark.parametrize("C", [1, 2])
def test_class_counts(C, monkeypatch):
    _problem_case(monkeypatch, Problem(4, C, "balanced64", 700), {})


# ---------------------------------------------------------------- dynamic tasks at small size

@pytest.mark.parametrize("dyn", [True, False], ids=["dyn", "static"])
@pytest.mark.parametrize("wgs", [1, 2])
def test_many_tasks_per_wave(wgs, dyn, monkeypatch):
    """JIT_WGS caps the persistent workgroups per (fragment, class): 20 000 patterns are 157
    tasks of 128 patterns over at most 16 (32) waves, >= 3 per wave, so the tasks after the
    first come from the counter with JIT_DYN=1 (wave tasks take tickets only when asked to; the
    super-block schedule does by default) and from the static stride with JIT_DYN=0."""
    tune = {"JIT_WGS": str(wgs), "JIT_DYN": "1" if dyn else "0"}
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 20000), tune)


# ---------------------------------------------------------------- fewer tasks than waves

def test_fewer_tasks_than_waves(monkeypatch):
    """JIT_G=16 asks for 16 waves per workgroup; 300 patterns are 3 tasks: the other waves of
    the one workgroup skip the loop."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 300), {"JIT_G": "16"})


# ---------------------------------------------------------------- fewer codes

@pytest.mark.parametrize("U", [3, 2])
def test_fewer_codes(U, monkeypatch):
    """A code table of 3 / 2 rows: quad tables of U^4 rows in plain order (no row rotation)."""
    p = Problem(4, 4, "balanced64", 900)
    init = np.array(p.alph.init_table[:U], dtype=np.float64, copy=True)
    states = (p.states % U).astype(np.int32)
    assert len(np.unique(states)) == U

    def make():
        return engine_for(p.et, 4, 4, p.n, states, init, p.rates, p.probs, p.pi, [p.m], flags=LNL | GUARD)

    eng, (lnl, site, _) = _three(monkeypatch, {}, make, lambda e: run_engine(e, p.et))
    lo, so = oracle_for(p.et, states, init, p.rates, p.probs, p.pi, [p.m], pmats=engine_pmats(eng, p.et))
    eng.close()
    check(lnl, site, lo, so, REL)


# ---------------------------------------------------------------- one pattern per lane

def test_one_pattern_per_lane(monkeypatch):
    """JIT_PW=1: tasks of 64 patterns, two per 128-pattern tile."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced64", 700), {"JIT_PW": "1"})


# ---------------------------------------------------------------- multi-tier

def test_multi_tier_300_taxa(monkeypatch):
    """The 300-taxon balanced tree: several tiers of fragments, stored fragment roots loaded
    by the tiers above."""
    _problem_case(monkeypatch, Problem(4, 4, "balanced300", 2000), {})


def test_multi_tier_512_taxa_rescaled(monkeypatch):
    """The 512-taxon rooted non-homogeneous tree with rescaling: the every-class-in-the-wave
    direct-code kernel (JIT_DC_CIW=1) with stored fragment roots and scale counts."""
    n = 30000
    wl = workload.make_workload("nh_gtr_g4_dna_2M_512", n_patterns=n)
    states = wl.simulate(0, n).astype(np.int32)

    def evaluate(eng_ev):
        lnl, _, blocks = eng_ev.step()
        lnl_r, site, _ = eng_ev.eng.root_loglik(wl.et.root, want_sites=True)
        assert lnl_r == lnl
        return lnl, site, blocks

    class Ev(workload.Evaluator):   # (the engine's queries on the evaluator, for _three)
        def kernel_path(self):
            return self.eng.kernel_path()

        def traversal_work(self):
            return self.eng.traversal_work()

        def close(self):
            self.eng.close()

    ev, (lnl, site, _) = _three(monkeypatch, {"JIT_DC_CIW": "1"},
                                lambda: Ev(wl, 0, 0, n, states=states, extra_flags=LNL), evaluate, quads=False)
    lo, so = _oracle(wl, states, pmats=_engine_pmats(ev.eng, wl.et), use_patterns=True)
    ev.close()
    assert np.all(np.isfinite(site)) and site.min() < -256 * np.log(2)     # rescaled
    assert abs(lnl - lo) <= REL * abs(lo), (lnl, lo)
    assert np.allclose(site, so, rtol=REL, atol=0)
