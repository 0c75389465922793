"""The three consumers of the stored lower partials L and upper vectors U -- node posteriors
(plk_node_posteriors), substitution counts (plk_branch_counts), NNI scores and their site rows
(plk_nni_scores, plk_nni_site_rows) -- against the extended-range reference (tests/xref.py:
80-bit longdouble, never rescaled, checked on the CPU by tests/test_xref_cpu.py), on the
engine's own P, r dP, r^2 d2P and count matrices W; only the trial matrices of a move's branch,
which the engine never stores, come from the eigen system (xref.trial_matrices).

  E  per-pattern lnL below -1022 ln 2 (the 600-taxon caterpillar of test_gpu_xref's BC10).
  F  20 and 64 states with rescaling that fires (120 / 150 taxa): the MFMA forms post_mfma,
     map_mfma_kernel, nni_coef_mfma_kernel, and POST_VALU=1.
  G  many rescaled vectors in one product.  "The scale counts cancel and are never read" holds
     while the product of the stored vectors is a normal double; the traversal's rule (x 2^256
     until the joint maximum is back above 2^-256) leaves every stored vector anywhere in
     [2^-256, 1), and an NNI coefficient build multiplies four of them on a binary tree, six at
     trifurcations, a branch term of the preorder pass four at a three-son node.  A tip code
     whose init vector is 2^-84 in every state (exact: it costs the reference no rounding; the
     tri cases' 2^-85.3 and their second code are plain doubles, no powers of two: a uniform
     vector still goes through P as v times a row sum) stands in for a deep subtree; three such tips make
     a clade at 2^-252.  Each case proves from the reference's vectors, reduced by the
     traversal's rule (_stored; confirmed against plk_get_partials), that on a quarter of the
     patterns the fp64 product of the factors' joint maxima is below 2^-1022.
  H  per-branch models (three GTR over the rooted 20-taxon tree of BC1): per-model count
     matrices, model= per NNI move; flat and under PLK_FLAG_SCALING.

Tolerances are the project's: posteriors 1e-10 absolute on joint, state and class posteriors;
counts 1e-10 max(1, |ref|); NNI delta and d1 1e-10 weight sums, d2 1e-9 max(wsum, |ref|), site
rows 1e-10 per pattern; each ten times looser where the case's smallest per-pattern lnL is
below -256 ln 2.  best_state equals the reference's argmax wherever its top two differ by more
than 1e-8, at most 1 % of cells skipped.  Every test prints its worst difference
("xref <group> ..."): a record, not a tolerance.

What group G found (E, F and H found nothing).  With the kernels as they were, the tri cases
on 4 states with 4 classes and on 20 states had NaN all-branch derivatives (dr_pre_s4_kernel
<4, true> and dr_pre_m20_kernel<.., true>: l = l' = l'' = 0 at the three-son nodes), and all
three tri cases had NNI scores with dropped patterns: delta off by 5.1e-3 (C = 4), 1.9e-3
(C = 8) and 4.3e-2 (20 states) weight sums, d2 by 0.33, 0.12 and 0.49 relative, 245, 194 and
183 site rows an exact 0.0 against a nonzero reference, status 0 throughout; on the poly case
every path derivative was NaN (deriv_kernel multiplied the five sons of the polytomy before its
one rescale).  C = 8 took the levelwise preorder, which was right.  The binary cases were right
as they stood: four vectors just above 2^-256 multiply to a number below 2^-1022 but above
2^-1075, a denormal that still carries the digits needed here.  Now nni_coef_*_kernel and
dr_pre_{s4,m20}_kernel<.., true> take an exact power of two out of every vector first, and
deriv_kernel rescales after every son; results elsewhere are bitwise what they were (compared
on the MI355X between the two builds: NNI scores, Newton runs and site rows on 4, 20 and 64
states, all-branch and path derivatives and posteriors on flat and rescaled handles).

A note on the lower pass.  When group G was written a check stepped by 2^256 once, and the fused
traversals checked once per node: a three-son op of sons near 2^-256 stored its result near
2^-512, and a chain of such ops left the double range in the lower pass itself.  The cases
stayed clear of that (the tri root kept a cherry and an ordinary clade, the poly case ran
PLK_FLAG_LEVELWISE only).  Now every check steps until the vector is in range and every path
checks inside a wide node (tests/test_gpu_xref_rescale.py pins that): the tri root's other
sons are tiny as well, the poly case also runs on the fused path, and with every stored vector
in [2^-256, 1) the tri cases reach their regime by vectors that sit within a bit of 2^-256
(_tree_tri); test_xref_cpu.test_gpu_cases_best_state_and_regime holds the regimes on the CPU.

Measured on the MI355X (worst over the cases of a group):
  E  posteriors 8.3e-16; counts 5.7e-16; NNI delta 4.1e-17, d1 1.6e-17 weight sums, d2 2.7e-16, site rows 7.8e-16;
     Newton delta at t_opt 7.4e-16
  F  posteriors 6.7e-16 (POST_VALU=1 included); counts 9.0e-16; NNI delta 1.7e-16, d1 1.4e-15 weight sums, d2 4.0e-15, site rows 1.5e-15
  G  derivatives 3.1e-14; posteriors 1.0e-15; counts 3.7e-16; NNI delta 2.8e-16, d1 5.5e-16 weight
     sums, d2 7.8e-15, site rows 2.4e-15; stored partials against the rule 3.4e-15
  H  posteriors 6.3e-16; counts 4.5e-16; NNI delta 5.3e-16, d1 2.8e-16 weight sums, d2 1.4e-15, site
     rows 5.6e-14; Newton delta at t_opt 5.9e-16
"""
import functools

import numpy as np
import pytest

import phylo
import plk
import rescale_rule
import xref
from conftest import set_tune

import test_nni_cpu as nni_ref
from test_gpu_posteriors import _six_nodes
from test_gpu_xref import DR, RESCALED, SC, Case, _case_bc1, _case_deep, _case_very_deep, _close_err, _path_branches

pytestmark = pytest.mark.gpu

LD = np.longdouble
T_SHORT = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if plk.device_count() < 1:
        pytest.fail("no GPU visible: gpu-marked tests must run on the MI355X box")


# ---------------------------------------------------------------- helpers

def _loose(site):
    """Ten times looser below -256 ln 2 (test_gpu_xref._tol)."""
    return 10.0 if site.min() < RESCALED else 1.0


def _model_of(case, v):
    return case.models[0 if case.mon is None else int(case.mon[v])]


def _registers(case):
    """DNA: the twelve comprehensive types; 20 and 64 states: the total register."""
    return [phylo.comprehensive_register(m.Q) if m.S == 4 else phylo.total_register(m.Q) for m in case.models]


def _moves_by_depth(et, k):
    """About k eligible moves spread from the root to the deepest node, tips and internal sons."""
    moves = nni_ref.eligible_moves(et.ops, et.root)
    par = nni_ref.parents_of(et.ops)

    def depth(v):
        d = 0
        while v in par:
            v, d = par[v], d + 1
        return d

    moves = sorted(moves, key=lambda mv: (depth(mv[0]), mv))
    if len(moves) <= k:
        return moves
    pick = sorted(set(int(i) for i in np.linspace(0, len(moves) - 1, k)))
    return [moves[i] for i in pick]


class Shared:
    """What the tests of one case share: the engine's matrices and the reference's lower pass,
    formed once while the engines of the case hold bitwise the same matrices."""

    def __init__(self):
        self.P, self.low, self.memo = None, None, {}

    def lower(self, case, eng):
        P = case.matrices(eng)[0]
        if self.P is None or not np.array_equal(P, self.P):
            self.P, self.memo = P, {}
            self.low = xref.lower(case.et, case.states, case.alph.init_table, P)
        return self.P, self.low

    def get(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]


def _shared(case):
    if not hasattr(case, "_shared"):
        case._shared = Shared()
    return case._shared


def _args(case, P):
    return (case.et, case.states, case.alph.init_table, P, case.probs, case.pi)


def check_posteriors(group, case, eng, site, nodes):
    sh = _shared(case)
    P, low = sh.lower(case, eng)
    x = sh.get(("post", tuple(nodes)), lambda: xref.posteriors(*_args(case, P), nodes, lower=low))
    assert x.l.min() > xref.RANGE_MIN
    out = eng.node_posteriors(nodes, joint=True, states=True, classes=True, best=True)
    for k in ("joint", "states", "classes"):
        assert np.isfinite(out[k]).all(), k
    tol = 1e-10 * _loose(site)
    ej = float(np.abs(out["joint"] - x.joint).max())
    es = float(np.abs(out["states"] - x.states).max())
    ec = float(np.abs(out["classes"] - x.classes).max())
    top = np.sort(x.states, axis=2)
    clear = np.asarray(top[:, :, -1] - top[:, :, -2] > 1e-8)
    skipped = 1.0 - clear.mean()
    print(f"xref {group} posteriors: joint {ej:.3g} state {es:.3g} class {ec:.3g} (tolerance {tol:g}) over "
          f"{len(nodes)} nodes; best_state: {clear.size - clear.sum()} of {clear.size} cells inside the 1e-8 gap")
    assert ej <= tol and es <= tol and ec <= tol, (ej, es, ec)
    assert skipped <= 0.01, skipped
    assert np.array_equal(out["best"][clear], x.best[clear])
    return out


def count_matrices(case, eng, branches):
    """The engine's own W of the branches (plk_update_count_matrices from the eigen systems)."""
    for k, B in enumerate(_registers(case)):
        eng.set_count_types(k, B)
    br = np.asarray(branches, dtype=np.int32)
    eng.update_count_matrices(br, case.et.brlen[br], None if case.mon is None else case.mon[br])
    return {int(v): eng.get_count_matrix(int(v)) for v in br}


def check_counts(group, case, eng, site, branches):
    sh = _shared(case)
    P, low = sh.lower(case, eng)
    W = count_matrices(case, eng, branches)
    x = sh.get(("counts", tuple(branches)),
               lambda: xref.branch_counts(*_args(case, P)[:4], W, case.probs, case.pi, branches, weights=case.w, lower=low))
    out = eng.branch_counts(branches)
    assert np.isfinite(out["counts"]).all() and np.isfinite(out["totals"]).all()
    tol = 1e-10 * _loose(site)
    ref = x.counts.astype(np.float64)
    wsum = float(case.n if case.w is None else case.w.sum())
    reft = (x.totals / LD(wsum)).astype(np.float64)
    ec = float((np.abs(out["counts"] - x.counts) / np.maximum(1.0, np.abs(ref))).max())
    et_ = float((np.abs(out["totals"] / wsum - reft) / np.maximum(1.0, np.abs(reft))).max())
    print(f"xref {group} counts: per pattern {ec:.3g}, totals / weight sum {et_:.3g} (tolerance {tol:g}) over "
          f"{len(branches)} branches, largest count {ref.max():.3g}")
    assert ec <= tol and et_ <= tol, (ec, et_)
    assert out["counts"].min() >= 0.0
    return out


def _trial(case, moves, t):
    par = nni_ref.parents_of(case.et.ops)
    mats = []
    for (s, _), ti in zip(moves, t):
        m = _model_of(case, par[s])
        mats.append(xref.trial_matrices(m.V, m.Vinv, m.lam, ti, case.rates))
    return tuple([mm[k] for mm in mats] for k in range(3))


def nni_reference(case, eng, moves, t, key=None):
    sh = _shared(case)
    P, low = sh.lower(case, eng)
    make = lambda: xref.nni(*_args(case, P), moves, *_trial(case, moves, t), weights=case.w, lower=low)
    return make() if key is None else sh.get(("nni", tuple(moves), key), make)


def _move_models(case, moves):
    if case.mon is None:
        return None
    par = nni_ref.parents_of(case.et.ops)
    return np.array([case.mon[par[s]] for s, _ in moves], dtype=np.int32)


def check_nni(group, case, eng, site, moves, newton=False):
    """Fixed-length scores at t_cur and at 1e-6 and the site rows at both; with newton, one
    Newton run whose delta is compared with the reference at the returned t_opt."""
    et = case.et
    par = nni_ref.parents_of(et.ops)
    son = np.array([s for s, _ in moves], dtype=np.int32)
    uncle = np.array([u for _, u in moves], dtype=np.int32)
    model = _move_models(case, moves)
    t_cur = np.array([et.brlen[par[s]] for s, _ in moves])
    w = np.ones(case.n) if case.w is None else case.w
    wsum = float(w.sum())
    loose = _loose(site)
    tol, tol2 = 1e-10 * loose, 1e-9 * loose
    eng.site_rows_reserve(len(moves))
    for name, t in (("t_cur", t_cur), ("1e-6", np.full(len(moves), T_SHORT))):
        x = nni_reference(case, eng, moves, t, key=name)
        out = eng.nni_scores(son, uncle, t, model=model)
        for k in ("delta", "d1", "d2"):
            assert np.isfinite(out[k]).all(), (k, out[k])
        assert np.all(out["status"] == 0) and np.array_equal(out["t_opt"], t)
        ed = float(np.abs(out["delta"] - x.delta).max()) / wsum
        e1 = float(np.abs(out["d1"] - x.d1).max()) / wsum
        e2 = float((np.abs(out["d2"] - x.d2) / np.maximum(wsum, np.abs(x.d2))).max())
        eng.nni_site_rows(son, uncle, t, 0, model=model)
        rows = np.stack([eng.site_row_get(i) for i in range(len(moves))])
        assert np.isfinite(rows).all()
        er = float(np.abs(rows - x.log_rho).max())
        # a pattern that counts never contributes an exact 0.0 unless the reference's log rho is 0
        dropped = (rows == 0.0) & (w[None, :] > 0) & (np.abs(x.log_rho) > tol)
        print(f"xref {group} NNI at {name}: delta {ed:.3g} d1 {e1:.3g} weight sums (tolerance {tol:g}), d2 relative "
              f"{e2:.3g} (tolerance {tol2:g}), site rows {er:.3g}, exact-zero rows against a nonzero reference "
              f"{int(dropped.sum())}; {len(moves)} moves, max |d1| / wsum {np.abs(out['d1']).max() / wsum:.3g}")
        assert not dropped.any(), (np.argwhere(dropped)[:8], x.log_rho[dropped][:8])
        assert ed <= tol and e1 <= tol and e2 <= tol2 and er <= tol, (ed, e1, e2, er)
    if newton:
        out = eng.nni_scores(son, uncle, t_cur, t_min=T_SHORT, t_max=100.0, tol=1e-8, max_iter=40, model=model)
        assert np.isfinite(out["delta"]).all() and np.isfinite(out["t_opt"]).all()
        x = nni_reference(case, eng, moves, out["t_opt"])
        ed = float(np.abs(out["delta"] - x.delta).max()) / wsum
        print(f"xref {group} NNI Newton: delta at t_opt {ed:.3g} weight sums (tolerance {tol:g}), {out['passes']} passes, "
              f"t_opt in [{out['t_opt'].min():.3g}, {out['t_opt'].max():.3g}], budget spent on "
              f"{int((out['status'] == 1).sum())} moves")
        assert ed <= tol, ed


# ---------------------------------------------------------------- E. below the double range

@functools.lru_cache(maxsize=None)
def _engine_e(C):
    case = _case_very_deep(4, C)
    eng, site, _ = case.engine("lnl_only", SC | DR)
    assert site.min() < -1022 * np.log(2), site.min()
    return case, eng, site


@pytest.mark.parametrize("C", [3, 8])
def test_e_posteriors(C):
    case, eng, site = _engine_e(C)
    nodes = _six_nodes(case.et)
    assert len(nodes) == 6
    check_posteriors(f"E C={C}", case, eng, site, nodes)


@pytest.mark.parametrize("C", [3, 8])
def test_e_counts(C):
    case, eng, site = _engine_e(C)
    br = _path_branches(case.et)
    assert len(br) == 12
    check_counts(f"E C={C}", case, eng, site, br)


@pytest.mark.parametrize("C", [3, 8])
def test_e_nni(C):
    case, eng, site = _engine_e(C)
    moves = _moves_by_depth(case.et, 10)
    assert len(moves) == 10
    check_nni(f"E C={C}", case, eng, site, moves, newton=True)


# ---------------------------------------------------------------- F. 20 and 64 states, rescaling that fires

@functools.lru_cache(maxsize=None)
def _engine_f(S):
    case = _case_deep(S)
    eng, site, _ = case.engine("lnl_only", SC | DR)   # (Case.engine asserts the kernel path)
    assert site.min() < RESCALED, site.min()
    return case, eng, site


@pytest.mark.parametrize("S", [20, 64])
def test_f_posteriors(S):
    case, eng, site = _engine_f(S)
    check_posteriors(f"F S={S}", case, eng, site, _six_nodes(case.et))


def test_f_posteriors_valu_form(monkeypatch):
    """PLK_TUNE POST_VALU=1: the LDS-staged VALU form of the 20-state kernel; bitwise is not
    asked, the same tolerance is."""
    set_tune(monkeypatch, "POST_VALU", 1)
    case, eng, site = _engine_f(20)
    check_posteriors("F S=20 POST_VALU", case, eng, site, _six_nodes(case.et))


@pytest.mark.parametrize("S", [20, 64])
def test_f_counts(S):
    case, eng, site = _engine_f(S)
    check_counts(f"F S={S}", case, eng, site, _path_branches(case.et))


@pytest.mark.parametrize("S,k", [(20, 8), (64, 4)])
def test_f_nni(S, k):
    """(64 states: four moves, the reference's swapped passes cost 64 x 64 longdouble products
    per node of the path to the root)"""
    case, eng, site = _engine_f(S)
    check_nni(f"F S={S}", case, eng, site, _moves_by_depth(case.et, k), newton=S == 20)


# ---------------------------------------------------------------- H. per-branch models

@functools.lru_cache(maxsize=None)
def _engine_h(scaling):
    case = _case_bc1(scaling)
    eng, site, _ = case.engine("lnl_only", (SC if scaling else 0) | DR)
    return case, eng, site


@pytest.mark.parametrize("scaling", [False, True])
def test_h_per_branch_models(scaling):
    case, eng, site = _engine_h(scaling)
    et = case.et
    group = f"H {'scaled' if scaling else 'flat'}"
    assert len(set(case.mon[case.br])) == 3
    check_posteriors(group, case, eng, site, list(range(et.n_tips, et.n_nodes)))
    check_counts(group, case, eng, site, [int(v) for v in case.br])
    moves = nni_ref.eligible_moves(et.ops, et.root)
    assert len(set(_move_models(case, moves))) == 3
    check_nni(group, case, eng, site, moves, newton=True)


# ---------------------------------------------------------------- G. many rescaled vectors in one product

TINY = 2.0 ** -84
THR = LD(2) ** -256
UP = LD(2) ** 256


def _tiny_alphabet(alph, tiny=TINY, shim=None):
    """A copy of the alphabet whose last code is 2^-84 (or tiny) in every state; with shim, the
    code before it is shim in every state."""
    tab = np.array(alph.init_table, dtype=np.float64, copy=True)
    tab[-1] = tiny
    if shim is not None:
        assert tab.shape[0] - 2 >= alph.n_states
        tab[-2] = shim
    return phylo.Alphabet(alph.name + "-tiny", alph.n_states, alph.chars, tab), tab.shape[0] - 1


def _clade(name, lengths, long_pair=None, single=None):
    """Three tips that carry the tiny code, a:b first, then c; with long_pair a cherry of two
    ordinary tips on branches of that length beside them, with single one ordinary tip."""
    a, b, c, ab, abc = lengths
    s = f"(({name}a:{a},{name}b:{b}):{ab},{name}c:{c})"
    if long_pair is not None:
        s = f"({s}:{abc},({name}d:{long_pair},{name}e:{long_pair}):{abc})"
    if single is not None:
        s = f"({s}:{abc},{name}d:{single})"
    return s


def _tree_binary():
    """s, its sibling o and the uncle u are clades of three tiny tips and a cherry of two
    ordinary tips on branches of length 3: under a model close to Jukes-Cantor the cherry's
    vector is P[x][a] P[x][b], between 0.0625 and 0.08 at its largest, so the clade's joint
    maximum is 2^-252 x 2^-3.7 to 2^-252 x 2^-4, a little above 2^-256.  The part above g is the
    other root son r, three tiny tips and one ordinary tip on a branch of 1.7: U_g = pi (*) q_r
    is about 2^-252 x 0.25 x 0.33.  The four multiply to about 2^-1023.4."""
    cl = lambda n: _clade(n, (0.1, 0.12, 0.08, 0.05, 0.06), long_pair=3.0)
    r = _clade("r", (0.1, 0.12, 0.08, 0.05, 0.06), single=1.7)
    return f"((({cl('s')}:0.1,{cl('o')}:0.12):0.1,{cl('u')}:0.09):0.1,{r}:0.11);"


TINY_TRI = 2.0 ** -85.3


def _tree_tri():
    """p = (s, o, q) and g = (p, u, v) of three sons each, g a son of the three-son root, whose
    other sons are a cherry r of two tiny tips and a tip zz.  Every stored vector is in
    [2^-256, 1) now, so four of them multiply to less than 2^-1022 only where each is within a
    bit of 2^-256: the tiny code of these cases is 2^-85.3, a clade of three is at 2^-255.9,
    L_p = 2^-767.7 is stored at 2^-255.7, and zz carries a second code, 2^-85.3 / max(pi), on the
    patterns whose tips are all tiny, so that U_g = pi (*) q_r (*) q_zz is at 2^-255.9 as well
    and U_p, three such factors, at 2^-255.7.  The branch terms at g and at p then multiply
    four vectors to about 2^-1023."""
    cl = lambda n, t: _clade(n, (0.1, 0.12, 0.08, 0.05, 0.06)) + f":{t}"
    return (f"((({cl('s', 0.1)},{cl('o', 0.12)},{cl('q', 0.07)}):0.1,{cl('u', 0.09)},{cl('v', 0.11)}):0.1,"
            f"(ra:0.1,rb:0.12):0.11,zz:0.08);")


def _tree_poly():
    """POLY with the five sons of its polytomy grown into clades."""
    cl = lambda n, t: _clade(n, (0.1, 0.12, 0.08, 0.05, 0.06)) + f":{t}"
    return (f"(({cl('a', 0.1)},{cl('b', 0.2)},{cl('c', 0.05)},{cl('d', 0.3)},{cl('e', 0.12)}):0.1,"
            f"(f:0.2,g:0.1):0.05,h:0.3,i:0.2);")


G_CASES = {
    # tree, unroot, S, C, patterns, seed, share of patterns whose tiny tips are all tiny, cell share elsewhere, mode
    "binary-C4": (_tree_binary, False, 4, 4, 256, 11, 0.9, 0.5, "materialize"),
    "binary-C8": (_tree_binary, False, 4, 8, 256, 12, 0.9, 0.5, "materialize"),
    "tri-C4": (_tree_tri, True, 4, 4, 300, 13, 0.6, 0.7, "materialize"),
    "tri-C8": (_tree_tri, True, 4, 8, 200, 14, 0.6, 0.7, "materialize"),
    "tri-S20": (_tree_tri, True, 20, 2, 200, 15, 0.6, 0.7, "materialize"),
    "poly-C4": (_tree_poly, True, 4, 4, 300, 16, 0.6, 0.7, "levelwise"),
    "poly-C4-fused": (_tree_poly, True, 4, 4, 300, 16, 0.6, 0.7, "materialize"),
}


def _tiny_case(newick, unroot, S, C, n, seed, whole, cells, alpha=0.6, tiny=TINY, shim=False):
    """A case whose tips named by one lower-case letter and a, b or c (_clade) carry the tiny
    code: on a share `whole` of the patterns all of them, elsewhere a share `cells` of the cells.
    shim: the tip zz carries the code before it, tiny / max(pi) in every state, on the patterns
    of the first kind."""
    et = phylo.engine_tree(phylo.Tree.from_newick(newick), unroot=unroot)
    if S == 4:   # close to Jukes-Cantor (distinct eigenvalues): see _tree_binary
        m, alph = phylo.gtr(1.02, 0.98, 1.0, 1.01, 0.99, 0.2505, 0.2495, 0.25, 0.25), phylo.DNA
    elif S == 20:
        m, alph = phylo.lg08(), phylo.PROTEIN
    else:
        m, alph = phylo.yn98(2.0, 0.3), phylo.CODON
    alph, code = _tiny_alphabet(alph, tiny, tiny / m.pi.max() if shim else None)
    case = Case(et, [m], None, alph, C, n, seed=seed, alpha=alpha)
    rng = np.random.default_rng(seed)
    tiny_tips = [i for i, nm in enumerate(et.tip_names) if len(nm) == 2 and nm[0].islower() and nm[1] in "abc"]
    assert len(tiny_tips) >= 12
    mask = np.zeros(case.states.shape, dtype=bool)
    all_tiny = rng.random(n) < whole
    mask[np.ix_(tiny_tips, np.flatnonzero(all_tiny))] = True
    rest = np.flatnonzero(~all_tiny)
    mask[np.ix_(tiny_tips, rest)] = rng.random((len(tiny_tips), len(rest))) < cells
    case.states[mask] = code
    if shim:
        case.states[et.tip_names.index("zz"), all_tiny] = code - 1
    case.w = rng.integers(1, 9, n).astype(np.float64)
    return case


@functools.lru_cache(maxsize=None)
def _case_g(name):
    tree, unroot, S, C, n, seed, whole, cells, _ = G_CASES[name]
    tri = tree is _tree_tri
    return _tiny_case(tree(), unroot, S, C, n, seed, whole, cells, alpha=200.0 if tree is _tree_binary else 0.6,
                      tiny=TINY_TRI if tri else TINY, shim=tri)


def _stored(case, P, low):
    """The vectors as the engine stores them under PLK_FLAG_SCALING (tests/rescale_rule.py:
    stored_new, every check stepping by 2^256 until the joint maximum over classes and states is
    back in [2^-256, 1)): the scale counts come from the fp64 walk, the vectors are the
    reference's own times 2^(256 k).  Returns the joint maxima per pattern, {v: [n]} for L and
    for the stored U of the internal nodes, and the stored L themselves."""
    et = case.et
    st = rescale_rule.stored_new(et, case.states, case.alph.init_table, P, case.pi)
    L, _ = low
    Ls = {v: rescale_rule.scaled_reference(L[v], st.k[v]) for v in range(et.n_nodes)}
    Lmax = {v: a.max(axis=(1, 2)).astype(np.float64) for v, a in Ls.items()}
    return Lmax, st.Umax, Ls


def _regime(case, Lmax, Umax):
    """Per pattern, the fp64 product of the joint maxima of the stored vectors that meet (a) in
    the coefficient build of each eligible NNI move: U_g, L_s, L_u, the third son of g, the other
    sons of p; (b) in the branch terms at each father f: U_f and every son's L.  Returns the
    largest share of patterns below 2^-1022 over the moves and over the fathers."""
    et = case.et
    sons, par = nni_ref.sons_of(et.ops), nni_ref.parents_of(et.ops)
    floor = 2.0 ** -1022
    one = np.ones(case.n)

    def share(vs):
        prod = one.copy()
        for v in vs:
            prod = prod * v
        return float((prod < floor).mean())

    best_move, best_f = (0.0, None), (0.0, None)
    for s, u in nni_ref.eligible_moves(et.ops, et.root):
        p = par[s]
        g = par[p]
        vs = [Lmax[o] for o in sons[g] if o != p] + [Lmax[o] for o in sons[p]] + ([] if g == et.root else [Umax[g]])
        best_move = max(best_move, (share(vs), (s, u)), key=lambda z: z[0])
    for f, ch in et.ops:
        vs = [Lmax[o] for o in ch] + ([] if f == et.root else [Umax[f]])
        best_f = max(best_f, (share(vs), f), key=lambda z: z[0])
    return best_move, best_f


@functools.lru_cache(maxsize=None)
def _engine_g(name):
    case = _case_g(name)
    eng, site, _ = case.engine(G_CASES[name][-1], SC | DR)
    return case, eng, site


def _prove_regime(name, case, eng):
    sh = _shared(case)
    P, low = sh.lower(case, eng)

    def make():
        Lmax, Umax, Ls = _stored(case, P, low)
        # the rule, once against the engine: the stored partial of every internal node
        worst = 0.0
        for v in range(case.et.n_tips, case.et.n_nodes):
            got, want = eng.get_partials(v), Ls[v].astype(np.float64)
            assert np.array_equal(got == 0.0, want == 0.0), v
            nz = want != 0.0
            worst = max(worst, float((np.abs(got[nz] - want[nz]) / want[nz]).max()))
        return _regime(case, Lmax, Umax), worst

    ((mv_share, mv), (f_share, f)), worst = sh.get("regime", make)
    l_min = low[0][case.et.root]
    l_min = xref._site(xref._ld(case.probs), l_min * xref._ld(case.pi)[None, None, :]).min()
    print(f"xref G {name} regime: product of the stored maxima below 2^-1022 on {mv_share:.0%} of the patterns at the "
          f"move {mv}, on {f_share:.0%} at the father {f}; stored partials against the rule {worst:.3g}; smallest "
          f"reference likelihood 2^{float(np.log2(l_min)):.0f}")
    assert worst <= 1e-12
    assert l_min > xref.RANGE_MIN
    if name.startswith("binary"):
        assert mv_share >= 0.25, mv_share          # (three vectors meet at a two-son node: no branch term)
    elif name.startswith("tri"):
        assert mv_share >= 0.25 and f_share >= 0.25, (mv_share, f_share)
    else:
        assert f_share >= 0.25, f_share


@pytest.mark.parametrize("name", sorted(G_CASES))
def test_g_regime_and_derivatives(name):
    """The regime condition, then all-branch and path derivatives of every branch."""
    case, eng, site = _engine_g(name)
    _prove_regime(name, case, eng)
    _, x = case.reference(eng)
    d1, d2 = eng.all_branch_derivatives()
    tol = 1e-10 * _loose(site)
    assert np.isfinite(d1).all() and np.isfinite(d2).all(), (d1, d2)
    worst = max(max(_close_err(d1[b], x.d1[b]), _close_err(d2[b], x.d2[b])) for b in case.br)
    path = [eng.branch_derivatives(int(b)) for b in case.br]
    assert np.isfinite(path).all(), path
    worst_p = max(max(_close_err(p1, x.d1[b]), _close_err(p2, x.d2[b])) for b, (p1, p2) in zip(case.br, path))
    print(f"xref G {name} derivatives: all-branch {worst:.3g}, path {worst_p:.3g} (tolerance {tol:g}) over "
          f"{len(case.br)} branches")
    assert worst <= tol and worst_p <= tol, (worst, worst_p)


@pytest.mark.parametrize("name", sorted(G_CASES))
def test_g_posteriors_and_counts(name):
    case, eng, site = _engine_g(name)
    _prove_regime(name, case, eng)
    et = case.et
    check_posteriors(f"G {name}", case, eng, site, list(range(et.n_tips, et.n_nodes)))
    check_counts(f"G {name}", case, eng, site, [int(v) for v in case.br])


@pytest.mark.parametrize("name", sorted(G_CASES))
def test_g_nni(name):
    case, eng, site = _engine_g(name)
    _prove_regime(name, case, eng)
    moves = nni_ref.eligible_moves(case.et.ops, case.et.root)
    assert moves
    check_nni(f"G {name}", case, eng, site, moves)
