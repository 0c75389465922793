"""Chains of rescaled vectors in the lower and upper pass under PLK_FLAG_SCALING, against the
extended-range reference (tests/xref.py: 80-bit longdouble, never rescaled) on the engine's own
matrices, on every traversal path that serves the state count.

The rule (tests/rescale_rule.py restates both forms in fp64; tests/test_xref_cpu.py proves the
regime of every case here on the CPU): a check multiplies a vector by 2^256 until its joint
maximum over classes and states is back in [2^-256, 1).  Up to now a check stepped once: an op
of three sons near 2^-256 stored its result near 2^-512, below the range the rule promises, and
a father of three such nodes multiplied to about 2^-1536, which is 0.0 in a double.

  I  "tri-chain": an unrooted three-son root; each root son a three-son node whose sons are
     clades of three tips that carry a code of 2^-84 in every state (test_gpu_xref_consumers
     group G: exact, it costs the reference no rounding; a clade sits at 2^-252), and one level
     more of three-son nodes below the first root son.  Every product of three takes two steps.
     45 tips; 4 states with 1, 4 and 8 classes, 20 states with 2, 64 states with 1.
  J  "wide": nodes of five and of nine sons, all of them such clades.  J5 / J9: the wide node is
     the root; Js: a nine-son and a five-son node beside an ordinary tip under a three-son
     root, so that the upper pass meets them.  (J5 dies only where the node is checked once at
     its end; a check after every three sons, stepping once, kept five sons alive.)
  K  "star", natural data, no tiny code: branch lengths in [2, 3), 64 patterns, 576 tips on 4
     states (GTR; one class, and four), 352 on 20 (LG08): the smallest multiples of 32 at which
     every pattern of the one-class cases is 0.0 in fp64 when the node is checked once at its
     end (tests/test_xref_cpu.py).  K runs on the interpreters (JIT=0, JITM=0), the levelwise
     and the per-subtree-compressed traversal: a generated kernel for a node of several hundred
     sons is a straight line of as many table reads and its tables do not fit in LDS.

Per case and path: kernel_path(); per-pattern and total lnL against xref.updown at
test_gpu_xref's REL; the stored partial of every internal node equals the reference's L times an
exact 2^(256 k), k >= 0 an integer equal to the restated rule's count, to 1e-12 relative, no
cell zero where the reference is not, the joint maximum in [2^-256, 1].  With
PLK_FLAG_DOUBLE_RECURSIVE, on the fused, the interpreter and the levelwise path: all-branch and
path derivatives finite and at group G's tolerance, node posteriors and branch counts (I and Js)
through check_posteriors and check_counts, which pin the stored U.  Across paths: per-pattern
lnL bitwise equal between the levelwise and the per-subtree-compressed handle on 4 states
(test_gpu_parity.test_subtree_patterns_wide_polytomy_rescale asks the same of ordinary trees);
stored partials and per-pattern lnL between tree4 and jit_tree4, and between tree4 and
levelwise, at 1e-13 relative: no existing test promises those bitwise for ordinary trees, so
bitwise is not asserted here (it was observed: see below).

Measured on the MI355X (worst over the cases and paths of a group; 115 cases in 21 s):
  I  lnL per pattern 2.2e-16; stored partials against the reference 9.3e-15; derivatives
     all-branch 5.9e-14, path 2.8e-14; posteriors 1.6e-15; counts 1.1e-15; largest scale count 14
  J  lnL 2.2e-16; partials 5.8e-15; derivatives 4.3e-14, path 2.1e-14; posteriors 1.9e-15; counts
     7.2e-16; largest scale count 13
  K  lnL 1.8e-16; partials 3.6e-15; derivatives 1.1e-15, path 2.8e-15; largest scale count 5; 375
     cells of K-C4 below 2^-766 of their pattern's maximum (check_partials)
  every scale count equal to the restated rule's; across the paths (tree4, jit_tree4, levelwise,
  subtree_patterns) every compared partial and per-pattern lnL bitwise equal on all seven cases
  -- observed, not promised: the assertion stays at 1e-13
With the kernels as they were (the parent's library under this file): 104 of the 115 cases
failed.  I: all 22 lnL cases, on every path alike, with per-pattern lnL that were not finite,
all 12 derivative cases NaN for every branch; the two cross-path cases passed, the paths being
wrong alike.  J: 40 of 46 lnL cases not finite; the six J5 cases on the levelwise and the
per-subtree-compressed path kept the product alive but stored the root partial at 6.8e-226,
below the range; derivatives NaN in 12 of 14 cases (the two fused J5 cases passed); all four
cross-path cases failed, the fused paths at 0.0 where levelwise was not.  K: every lnL case on
tree4 and treeM not finite, every levelwise and subtree_patterns case right (a check after
every three sons, stepping once, is enough for tips); K-S20's path derivatives NaN; the
cross-path case failed.
"""
import functools

import numpy as np
import pytest

import plk
import rescale_rule
import xref
from conftest import set_tune

import phylo
from test_gpu_xref import DR, SC, Case, _check_lnl, _close_err, _model, _path_branches
from test_gpu_xref_consumers import _clade, _loose, _shared, _tiny_case, check_counts, check_posteriors

pytestmark = pytest.mark.gpu

LD = np.longdouble
CL = (0.1, 0.12, 0.08, 0.05, 0.06)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


def _three(names, lengths=(0.1, 0.12, 0.07)):
    """A three-son node whose sons are tiny clades."""
    return "(" + ",".join(f"{_clade(nm, CL)}:{t}" for nm, t in zip(names, lengths)) + ")"


def tree_i():
    deep = f"({_three('abc')}:0.1,{_three('def')}:0.08,{_three('ghi')}:0.12)"
    return f"({deep}:0.1,{_three('jkl')}:0.09,{_three('mno')}:0.11);"


def _wide(names):
    """A node whose sons are tiny clades, one per letter."""
    ts = (0.1, 0.12, 0.07, 0.09, 0.11, 0.08, 0.1, 0.13, 0.06)
    return "(" + ",".join(f"{_clade(nm, CL)}:{t}" for nm, t in zip(names, ts)) + ")"


def tree_j(kind):
    """root5 / root9: the wide node is the root.  son: a nine-son and a five-son node beside an
    ordinary tip under a three-son root, so that the upper pass meets them too."""
    if kind == "son":
        return f"({_wide('abcdefghi')}:0.1,{_wide('jklmn')}:0.12,xd:0.2);"
    return _wide("abcdefghi" if kind == "root9" else "abcde") + ";"


def tree_k(n_tips, seed):
    """A star, branch lengths uniform in [2, 3)."""
    t = np.random.default_rng(seed).uniform(2.0, 3.0, n_tips)
    return "(" + ",".join(f"t{i}:{t[i]:.6f}" for i in range(n_tips)) + ");"


# tips of the K stars: the smallest multiples of 32 at which every pattern's product of the tips'
# vectors is 0.0 in fp64 when it is checked once at the node's end (tests/test_xref_cpu.py)
K_TIPS = {4: 576, 20: 352}

# tree, S, C, patterns, seed, share of patterns on which every tiny tip carries the tiny code (elsewhere
# 70 % of the cells do).  I on 64 states: none, the codon frequencies of YN98 are equal and the posteriors of
# such a pattern are ties, which best_state cannot be compared on.
CASES = {
    "I-C1": ("i", 4, 1, 160, 21, 0.3), "I-C4": ("i", 4, 4, 160, 22, 0.3), "I-C8": ("i", 4, 8, 160, 23, 0.3),
    "I-S20": ("i", 20, 2, 100, 24, 0.3), "I-S64": ("i", 64, 1, 64, 25, 0.0),
    "J5-C1": ("root5", 4, 1, 130, 31, 0.3), "J5-C4": ("root5", 4, 4, 130, 32, 0.3), "J5-S20": ("root5", 20, 2, 100, 33, 0.3),
    "J5-S64": ("root5", 64, 1, 64, 34, 0.3),
    "J9-C4": ("root9", 4, 4, 130, 35, 0.3), "J9-C8": ("root9", 4, 8, 130, 36, 0.3), "J9-S20": ("root9", 20, 2, 100, 37, 0.3),
    "Js-C4": ("son", 4, 4, 130, 38, 0.3), "Js-C8": ("son", 4, 8, 130, 39, 0.3), "Js-S20": ("son", 20, 2, 100, 40, 0.3),
    "K-C1": ("star", 4, 1, 64, 43, None), "K-C4": ("star", 4, 4, 64, 41, None), "K-S20": ("star", 20, 1, 64, 42, None),
}


@functools.lru_cache(maxsize=None)
def case_of(name):
    tree, S, C, n, seed, whole = CASES[name]
    if tree == "star":   # natural data, no tiny code
        et = phylo.engine_tree(phylo.Tree.from_newick(tree_k(K_TIPS[S], seed)))
        m, alph = _model(S)
        return Case(et, [m], None, alph, C, n, seed=seed)
    return _tiny_case(tree_i() if tree == "i" else tree_j(tree), True, S, C, n, seed, whole, 0.7)


# path name: (traversal mode, tuning knob to clear, kernel_path by state count)
PATHS = {
    "fused": ("materialize", None, {4: "jit_tree4", 20: "jit_treeM", 64: "treeM"}),
    "fused-lnl": ("lnl_only", None, {4: "jit_tree4", 20: "jit_treeM", 64: "treeM"}),
    "interp": ("materialize", {4: "JIT", 20: "JITM"}, {4: "tree4", 20: "treeM"}),
    "interp-lnl": ("lnl_only", {4: "JIT", 20: "JITM"}, {4: "tree4", 20: "treeM"}),
    "levelwise": ("levelwise", None, {4: "levelwise", 20: "levelwise", 64: "levelwise"}),
    "subtree": ("subtree", None, {4: "subtree_patterns"}),
}


def paths_of(name):
    tree, S, C = CASES[name][:3]
    if S == 4 and C == 8:   # off the fused kernels: the levelwise traversal, whatever the mode
        return ["levelwise", "subtree"]
    paths = [p for p, (_, _, kp) in PATHS.items() if S in kp]
    if tree == "star":      # the interpreters only: see the module docstring
        paths = [p for p in paths if not p.startswith("fused")]
    return paths


def engine_on(monkeypatch, case, path, extra=0):
    mode, knob, kp = PATHS[path]
    if knob is not None:
        set_tune(monkeypatch, knob[case.S], 0)
    return case.engine(mode, SC | extra, expect=kp[case.S])


def rule_of(case, eng):
    """(P, the reference's lower pass, the restated rule on the engine's P), shared per case."""
    sh = _shared(case)
    P, low = sh.lower(case, eng)
    st = sh.get("rule", lambda: rescale_rule.stored_new(case.et, case.states, case.alph.init_table, P, case.pi))
    return P, low, st


def check_partials(group, case, eng):
    """Assertion 2 of the module docstring.  The joint maximum of a stored vector is at least
    2^-256, so a cell of at least 2^-766 of its pattern's maximum is a normal double: it must be
    nonzero and right to 1e-12.  A smaller cell (another rate class of a star pattern) may be
    a denormal number or 0.0 beside a maximum near 2^-256, in any arithmetic that scales a
    pattern jointly; it must only not be larger than that."""
    _, (L, _), st = rule_of(case, eng)
    worst, small = 0.0, 0
    for v in range(case.et.n_tips, case.et.n_nodes):
        got, ref = eng.get_partials(v), L[v]
        assert np.isfinite(got).all(), v
        gm, rm = got.max(axis=(1, 2)), ref.max(axis=(1, 2))
        assert np.all(rm > 0)
        assert np.all((gm >= 2.0 ** -256) & (gm <= 1.0)), (v, float(gm.min()), float(gm.max()))
        kf = np.log2(LD(1) * gm / rm) / 256
        k = np.rint(kf).astype(np.int64)
        assert np.all(np.abs(kf - k) < 1e-9) and np.all(k >= 0), v
        want = rescale_rule.scaled_reference(ref, k)
        big = np.asarray(ref >= rm[:, None, None] * LD(2) ** -766)
        small += int((~big & np.asarray(ref != 0)).sum())
        assert np.all(got[big] != 0.0), (v, int((got[big] == 0.0).sum()))
        assert np.all(got[~big] <= 2.0 ** -765 * np.broadcast_to(gm[:, None, None], got.shape)[~big]), v
        assert np.array_equal(got[np.asarray(ref == 0)], np.zeros(int(np.asarray(ref == 0).sum()))), v
        worst = max(worst, float((np.abs(got[big] - want[big]) / want[big]).max()))
        assert np.array_equal(k, st.k[v]), (v, k[:8], st.k[v][:8])
    print(f"xref {group} stored partials: {worst:.3g} against the reference times 2^(256 k), largest k "
          f"{max(int(st.k[v].max()) for v in range(case.et.n_tips, case.et.n_nodes))}; cells below 2^-766 of "
          f"their pattern's maximum {small}")
    assert worst <= 1e-12, worst


ALL = [(name, path) for name in CASES for path in paths_of(name)]


@pytest.mark.parametrize("name,path", ALL)
def test_lnl_and_partials(monkeypatch, name, path):
    case = case_of(name)
    eng, site, lnl = engine_on(monkeypatch, case, path)
    _, x = case.reference(eng)   # (with derivatives: the case's tests share it)
    assert x.l.min() > xref.RANGE_MIN
    _check_lnl(f"{name} {path}", site, lnl, x)
    assert site.min() < -3 * 256 * np.log(2)   # (several steps per pattern)
    check_partials(f"{name} {path}", case, eng)


def _dr_paths(name):
    """The materialising paths PLK_FLAG_DOUBLE_RECURSIVE runs on (not the per-subtree compression);
    all of them on the I cases and on the J cases whose wide nodes are root sons, the first
    elsewhere."""
    paths = [p for p in paths_of(name) if p in ("fused", "interp", "levelwise")]
    return paths if CASES[name][0] in ("i", "son") else paths[:1]


@pytest.mark.parametrize("name,path", [(name, path) for name in sorted(CASES) for path in _dr_paths(name)])
def test_derivatives_posteriors_counts(monkeypatch, name, path):
    """With PLK_FLAG_DOUBLE_RECURSIVE: every branch through plk_all_branch_derivatives, every
    branch (twelve on trees above 40 taxa) through plk_branch_derivatives; posteriors of every
    internal node and counts of every branch on the I cases and the J cases whose wide nodes
    are root sons."""
    case = case_of(name)
    eng, site, lnl = engine_on(monkeypatch, case, path, DR)
    _, x = case.reference(eng)
    d1, d2 = eng.all_branch_derivatives()
    tol = 1e-10 * _loose(site)
    assert np.isfinite(d1).all() and np.isfinite(d2).all(), (d1, d2)
    worst = max(max(_close_err(d1[b], x.d1[b]), _close_err(d2[b], x.d2[b])) for b in case.br)
    if CASES[name][0] == "star":   # (every branch is a tip's: twelve spread evenly)
        pick = sorted(set(int(i) for i in np.linspace(0, case.et.n_tips - 1, 12)))
    else:
        pick = _path_branches(case.et)
    path = [eng.branch_derivatives(int(b)) for b in pick]
    assert np.isfinite(path).all(), path
    worst_p = max(max(_close_err(p1, x.d1[b]), _close_err(p2, x.d2[b])) for b, (p1, p2) in zip(pick, path))
    print(f"xref {name} {path} derivatives: all-branch {worst:.3g} over {len(case.br)} branches, path {worst_p:.3g} over "
          f"{len(pick)} (tolerance {tol:g})")
    assert worst <= tol and worst_p <= tol, (worst, worst_p)
    if CASES[name][0] in ("i", "son"):
        et = case.et
        check_posteriors(f"{name} {path}", case, eng, site, list(range(et.n_tips, et.n_nodes)))
        check_counts(f"{name} {path}", case, eng, site, [int(v) for v in case.br])


def _rel(a, b):
    nz = b != 0
    assert np.array_equal(a == 0, b == 0)
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


@pytest.mark.parametrize("name", ["I-C1", "I-C4", "J5-C1", "J5-C4", "J9-C4", "Js-C4", "K-C1"])
def test_across_paths(monkeypatch, name):
    case = case_of(name)
    nodes = range(case.et.n_tips, case.et.n_nodes)
    res = {}
    for path in ("fused", "levelwise", "subtree", "interp"):   # (interp last: it sets the knob)
        if path in paths_of(name):
            eng, site, lnl = engine_on(monkeypatch, case, path)
            res[path] = (site, lnl, {v: eng.get_partials(v) for v in nodes})
    assert np.array_equal(res["levelwise"][0], res["subtree"][0]) and res["levelwise"][1] == res["subtree"][1]
    err = {"partials levelwise / subtree_patterns": max(_rel(res["levelwise"][2][v], res["subtree"][2][v]) for v in nodes),
           "partials tree4 / levelwise": max(_rel(res["interp"][2][v], res["levelwise"][2][v]) for v in nodes),
           "per-pattern lnL tree4 / levelwise": _rel(res["interp"][0], res["levelwise"][0])}
    if "fused" in res:
        err["partials tree4 / jit_tree4"] = max(_rel(res["interp"][2][v], res["fused"][2][v]) for v in nodes)
        err["per-pattern lnL tree4 / jit_tree4"] = _rel(res["interp"][0], res["fused"][0])
    print(f"xref {name} across paths: " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()))
    assert max(err.values()) <= 1e-13, err
