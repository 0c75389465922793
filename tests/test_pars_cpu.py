"""Fitch parsimony as include/plk.h states it (the plk_pars_* block), restated in numpy: the
arbiter of the GPU tests (tests/test_gpu_pars.py imports this module).  Everything is integer
arithmetic, so every comparison is an equality.

A pair is (set, score), sets are uint64 bit masks, one entry per pattern.  F is the sequential
fold: start from the first pair; for each further pair add its score and intersect the sets; where
the intersection is empty take the union and add 1.  The order of the inputs is part of the
definition (the score of F does not depend on it, the set does)."""
import os

import numpy as np

import phylo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fold(pairs):
    s, c = pairs[0][0].copy(), pairs[0][1].copy()
    for t, d in pairs[1:]:
        c = c + d
        i = s & t
        empty = i == 0
        s = np.where(empty, s | t, i)
        c = c + empty
    return s, c


class Restatement:
    """kids: {internal node: sons in order}; tip_sets: uint64 [n_tips, n_patterns]; weights: ints."""

    def __init__(self, kids, root, n_tips, tip_sets, weights):
        self.kids, self.root, self.nt = {v: list(k) for v, k in kids.items()}, root, n_tips
        self.tip_sets = np.asarray(tip_sets, dtype=np.uint64)
        self.w = np.asarray(weights, dtype=np.int64)
        self.parent = {c: v for v, k in self.kids.items() for c in k}
        self.low_, self.up_ = {}, {}
        zero = np.zeros(self.tip_sets.shape[1], dtype=np.int64)
        for t in range(n_tips):
            self.low_[t] = (self.tip_sets[t], zero)
        for v in self.postorder():
            self.low_[v] = fold([self.low_[c] for c in self.kids[v]])
        for v in self.preorder():
            if v == root:
                continue
            f = self.parent[v]
            self.up_[v] = fold(([] if f == root else [self.up_[f]]) + [self.low_[c] for c in self.kids[f] if c != v])
        self.site_scores = self.low_[root][1]
        self.score = int(np.dot(self.w, self.site_scores))

    def postorder(self):
        out = []

        def rec(v):
            for c in self.kids.get(v, []):
                rec(c)
            if v in self.kids:
                out.append(v)
        rec(self.root)
        return out

    def preorder(self):
        out = []

        def rec(v):
            if v in self.kids:
                out.append(v)
                for c in self.kids[v]:
                    rec(c)
        rec(self.root)
        return out

    def low(self, v):
        return self.low_[v]

    def up(self, v):
        return self.up_[v]

    def moves(self):
        """Every eligible (son, uncle)."""
        out = []
        for s, p in sorted(self.parent.items()):
            if p == self.root:
                continue
            g = self.parent[p]
            out += [(s, u) for u in self.kids[g] if u != p]
        return out

    def delta(self, s, u):
        p = self.parent[s]
        g = self.parent[p]
        gf = fold(([] if g == self.root else [self.up_[g]]) + [self.low_[o] for o in self.kids[g] if o not in (p, u)]
                  + [self.low_[s]])
        pp = fold([self.low_[o] for o in self.kids[p] if o != s] + [self.low_[u], gf])
        return int(np.dot(self.w, pp[1])) - self.score

    def swapped(self, s, u):
        """The tree after the interchange: s and u change fathers, each appended to its new father's sons."""
        p = self.parent[s]
        g = self.parent[p]
        kids = {v: list(k) for v, k in self.kids.items()}
        kids[p].remove(s)
        kids[g].remove(u)
        kids[p].append(u)
        kids[g].append(s)
        return Restatement(kids, self.root, self.nt, self.tip_sets, self.w)

    def ops(self):
        """Postorder plk ops, at most three sons each (later chunks accumulate)."""
        return phylo.split_ops([(v, tuple(self.kids[v])) for v in self.postorder()])


# ---------------------------------------------------------------- trees and data

def caterpillar(n):
    """((((0,1),2),3),...,n-1): internal nodes n, n+1, ...; the root has two sons."""
    kids, cur = {}, 0
    for i in range(1, n):
        kids[n + i - 1] = [cur, i]
        cur = n + i - 1
    return kids, cur


def random_tree(rng, n_tips, root_sons=2, tri_internal=False):
    """Random joins of tips; with tri_internal one internal node gets three sons."""
    act = list(range(n_tips))
    kids, nxt = {}, n_tips
    tri_at = rng.integers(4, n_tips - 1) if tri_internal else -1
    while len(act) > root_sons:
        k = 3 if len(act) == tri_at and len(act) - 2 >= root_sons else 2
        pick = [act.pop(int(rng.integers(len(act)))) for _ in range(k)]
        kids[nxt] = pick
        act.append(nxt)
        nxt += 1
    kids[nxt] = act
    return kids, nxt


def mask_table(rng, n_states, n_ambiguous=12):
    """Codes 0 .. n_states-1: the single states; then n_ambiguous random sets of two or more states."""
    m = [1 << s for s in range(n_states)]
    for _ in range(n_ambiguous):
        k = int(rng.integers(2, min(n_states, 6) + 1))
        m.append(sum(1 << int(s) for s in rng.choice(n_states, size=k, replace=False)))
    return np.array(m, dtype=np.uint64)


def random_codes(rng, n_tips, n_patterns, n_states, n_codes, ambiguous=0.15):
    """A few states per pattern (so that sets meet and miss), 15 % ambiguity codes."""
    base = rng.integers(0, n_states, size=(3, n_patterns))
    codes = base[rng.integers(0, 3, size=(n_tips, n_patterns)), np.arange(n_patterns)]
    amb = rng.random((n_tips, n_patterns)) < ambiguous
    codes = np.where(amb, rng.integers(n_states, n_codes, size=(n_tips, n_patterns)), codes)
    return codes.astype(np.uint8)


def random_weights(rng, n_patterns):
    w = rng.integers(1, 9, size=n_patterns)
    w[rng.random(n_patterns) < 0.1] = 0
    return w.astype(np.int64)


def golden_case():
    """tests/golden/example1.ph on example1.mp.dnd, the gap a fifth state: (Restatement, tip names)."""
    with open(os.path.join(GOLDEN, "example1.mp.dnd")) as f:
        et = phylo.engine_tree(phylo.Tree.from_newick(f.read().replace("\n", "")), unroot=False)
    with open(os.path.join(GOLDEN, "example1.ph")) as f:
        lines = f.read().split("\n")
    n, length = (int(x) for x in lines[0].split())
    seqs = dict(l.split() for l in lines[1:1 + n])
    masks = np.array([sum(1 << phylo.NUC.index(a) for a in phylo._DNA_ALIAS[c]) for c in phylo.DNA_CHARS] + [1 << 4],
                     dtype=np.uint64)
    codes = np.array([[15 if ch == "-" else phylo.DNA_CHARS.index(ch) for ch in seqs[name]] for name in et.tip_names])
    assert codes.shape == (n, length)
    kids = {}
    for p, ch in et.ops:
        kids.setdefault(p, []).extend(ch)
    return Restatement(kids, et.root, et.n_tips, masks[codes], np.ones(length, dtype=np.int64)), codes, masks


# ---------------------------------------------------------------- the tests

def test_golden_alignment_scores_nine_with_the_gap_as_a_state():
    rs, codes, _ = golden_case()
    assert len(rs.kids[rs.root]) == 3 and codes.shape == (5, 10)
    assert rs.score == 9
    # without the gap state the gap column costs nothing
    rs4 = Restatement(rs.kids, rs.root, rs.nt, np.where(rs.tip_sets == 16, 15, rs.tip_sets), rs.w)
    assert rs4.score == 8


def test_binary_caterpillar_scores_three():
    kids, root = caterpillar(8)
    states = np.array([0, 1, 0, 1, 1, 1, 0, 0])
    rs = Restatement(kids, root, 8, (np.uint64(1) << states.astype(np.uint64))[:, None], [1])
    assert rs.score == 3


def test_fold_score_is_order_free_and_the_set_is_not():
    one = np.zeros(1, dtype=np.int64)
    diff = 0
    for a in range(1, 16):
        for b in range(1, 16):
            for c in range(1, 16):
                x = [(np.array([m], dtype=np.uint64), one) for m in (a, b, c)]
                f1, f2 = fold(x), fold([x[2], x[0], x[1]])
                assert f1[1][0] == f2[1][0]
                diff += int(f1[0][0] != f2[0][0])
    assert diff > 0


def test_delta_is_the_swapped_tree_minus_the_current_tree():
    """Holds where every internal node but the root has two sons (the root: two or three).  The
    fold is not associative, so around an internal node of three sons the value of a move -- the
    reference's testNNI value, folded at p -- need not be the difference of two scores folded at
    the root; there delta is defined by the fold alone."""
    rng = np.random.default_rng(7)
    n_moves = 0
    for trial in range(40):
        n = int(rng.integers(5, 13))
        kids, root = random_tree(rng, n, root_sons=2 + trial % 2)
        masks = mask_table(rng, 4, 8)
        codes = random_codes(rng, n, 37, 4, len(masks))
        rs = Restatement(kids, root, n, masks[codes], random_weights(rng, 37))
        for s, u in rs.moves():
            assert rs.delta(s, u) == rs.swapped(s, u).score - rs.score, (trial, s, u)
            n_moves += 1
    assert n_moves > 500
