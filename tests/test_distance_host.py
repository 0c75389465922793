"""NJ and BioNJ of the Bio++ mirror (tests/cpp/test_distance_cpu.cpp) against numpy versions
written here from the papers: Saitou & Nei 1987 with the Studier-Keppler criterion
Q_ij = (r - 2) d_ij - S_i - S_j, and Gascuel 1997 (lambda per join clamped to [0, 1], the
variance matrix updated alongside).  The program checks both methods on the additive matrix of
a fixed 9-leaf tree itself (bipartitions, every length to 1e-12, rooted and unrooted) and prints
their trees for that matrix plus 0.01 sin(3 i + 5 j), symmetrised, and for a 5-taxon matrix that
yields a negative length; this test recomputes the matrices and compares bipartitions and
lengths to 1e-12."""
import os
import subprocess

import numpy as np

import phylo
from conftest import run_make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")

TREE9 = ("(((A:0.11,B:0.23):0.07,(C:0.31,D:0.05):0.13):0.09,((E:0.17,F:0.19):0.21,G:0.29):0.03,"
         "(H:0.37,I:0.02):0.15);")
# B sits next to A but is far closer to everything else than A is: A's branch takes more than d_AB
NEG5 = np.array([[0.0, 0.1, 5.0, 5.2, 4.9],
                 [0.1, 0.0, 1.0, 1.3, 0.8],
                 [5.0, 1.0, 0.0, 0.6, 1.1],
                 [5.2, 1.3, 0.6, 0.0, 1.2],
                 [4.9, 0.8, 1.1, 1.2, 0.0]])


# ---------------------------------------------------------------- numpy NJ and BioNJ

def agglomerate(D, names, bionj=False, rooted=False, positive=False):
    """Returns {frozenset of leaf names on the side without names[0]: branch length}."""
    d = np.array(D, dtype=np.float64)
    v = d.copy()
    act = list(range(len(names)))
    below = {i: frozenset([names[i]]) for i in act}
    splits = {}
    everyone = frozenset(names)

    def emit(leaves, length):
        if positive and length < 0:
            length = 0.0
        key = leaves if names[0] not in leaves else everyone - leaves
        splits[key] = splits.get(key, 0.0) + length

    while len(act) > (2 if rooted else 3):
        r = len(act)
        S = {a: sum(d[a, b] for b in act if b != a) for a in act}
        best, qbest = None, np.inf
        for i in range(r):
            for j in range(i + 1, r):
                q = (r - 2) * d[act[i], act[j]] - S[act[i]] - S[act[j]]
                if q < qbest:
                    best, qbest = (i, j), q
        a, b = act[best[0]], act[best[1]]
        ba = 0.5 * d[a, b] + (S[a] - S[b]) / (2.0 * (r - 2))
        bb = d[a, b] - ba
        lam = 0.5
        if bionj and v[a, b] != 0:
            lam = 0.5 + sum(v[b, k] - v[a, k] for k in act if k not in (a, b)) / (2.0 * (r - 2) * v[a, b])
            lam = min(max(lam, 0.0), 1.0)
        for k in act:
            if k in (a, b):
                continue
            if bionj:
                d[a, k] = d[k, a] = lam * (d[a, k] - ba) + (1 - lam) * (d[b, k] - bb)
                v[a, k] = v[k, a] = lam * v[a, k] + (1 - lam) * v[b, k] - lam * (1 - lam) * v[a, b]
            else:
                d[a, k] = d[k, a] = 0.5 * (d[a, k] + d[b, k] - d[a, b])
        emit(below[a], ba)
        emit(below[b], bb)
        below[a] = below[a] | below[b]
        act.remove(b)
    if len(act) == 3:
        a, b, c = act
        emit(below[a], 0.5 * (d[a, b] + d[a, c] - d[b, c]))
        emit(below[b], 0.5 * (d[a, b] + d[b, c] - d[a, c]))
        emit(below[c], 0.5 * (d[a, c] + d[b, c] - d[a, b]))
    else:
        a, b = act
        emit(below[a], 0.5 * d[a, b])
        emit(below[b], 0.5 * d[a, b])
    return splits


def tree_splits(newick):
    """The same map for a Newick string, and its leaf names in order."""
    t = phylo.Tree.from_newick(newick)
    names = sorted(t.leaf_names())
    everyone = frozenset(names)
    below, splits = {}, {}
    for n in t.nodes():
        below[id(n)] = frozenset([n.name]) if n.is_leaf() else frozenset().union(*(below[id(s)] for s in n.sons))
        if n.father is not None:
            key = below[id(n)] if names[0] not in below[id(n)] else everyone - below[id(n)]
            splits[key] = splits.get(key, 0.0) + n.dist
    return splits, names


def additive_matrix(newick):
    t = phylo.Tree.from_newick(newick)
    leaves = sorted(t.leaves(), key=lambda n: n.name)

    def path(n):
        out = {}
        acc = 0.0
        while n is not None:
            out[id(n)] = acc
            acc += n.dist or 0.0
            n = n.father
        return out

    paths = [path(l) for l in leaves]
    n = len(leaves)
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = min(paths[i][k] + paths[j][k] for k in paths[i] if k in paths[j])
    return D, [l.name for l in leaves]


def perturbed(D):
    n = len(D)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return D + np.where(i == j, 0.0, 0.01 * np.sin(3.0 * lo + 5.0 * hi))


def same(a, b, tol=1e-12):
    return a.keys() == b.keys() and all(abs(a[k] - b[k]) <= tol for k in a)


# ---------------------------------------------------------------- the tests

def test_numpy_methods_are_exact_on_an_additive_matrix_and_differ_on_a_perturbed_one():
    D, names = additive_matrix(TREE9)
    want, _ = tree_splits(TREE9)
    for bionj in (False, True):
        for rooted in (False, True):
            assert same(agglomerate(D, names, bionj, rooted), want)
    P = perturbed(D)
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0)
    nj, bio = agglomerate(P, names), agglomerate(P, names, bionj=True)
    # the BioNJ path is exercised only where its reduction gives other numbers than NJ's
    assert nj.keys() != bio.keys() or max(abs(nj[k] - bio[k]) for k in nj) > 1e-6
    assert min(agglomerate(NEG5, list("ABCDE")).values()) < -0.1


def test_cpp_distance_methods():
    run_make("-s", "-j8", "-C", HOST, "bin/test_distance_cpu")
    r = subprocess.run([os.path.join(HOST, "bin", "test_distance_cpu")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
    trees = {}
    for line in r.stdout.splitlines():
        if line.startswith("TREE "):
            _, case, method, shape, newick = line.split(" ", 4)
            trees[(case, method, shape)] = newick
    D, names = additive_matrix(TREE9)
    P = perturbed(D)
    assert len(trees) == 16
    for (case, method, shape), newick in trees.items():
        got, got_names = tree_splits(newick)
        bionj, rooted = method == "BioNJ", shape == "rooted"
        assert len(phylo.Tree.from_newick(newick).root.sons) == (2 if rooted else 3)
        if case in ("additive", "perturbed"):
            assert got_names == names
            assert same(got, agglomerate(D if case == "additive" else P, names, bionj, rooted)), (case, method, shape)
        else:
            assert got_names == list("ABCDE")
            assert same(got, agglomerate(NEG5, got_names, bionj, rooted, positive=case == "positive")), (case, method, shape)
            assert (min(got.values()) == 0.0) if case == "positive" else (min(got.values()) < -0.1)


def test_the_gpu_scenario_recovers_its_tree_on_the_cpu():
    """The condition tests/cpp/test_distance_gpu.cpp rests on: from the alignment it simulates
    (its `dump` mode touches no device), the numpy restatement's ML distances and the numpy BioNJ
    return the true tree's bipartitions."""
    import test_pair_cpu as pair

    run_make("-s", "-j8", "-C", HOST, "bin/test_distance_gpu")
    r = subprocess.run([os.path.join(HOST, "bin", "test_distance_gpu"), "dump"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    newick, names, seqs = None, [], []
    for line in r.stdout.splitlines():
        if line.startswith("NEWICK "):
            newick = line.split(" ", 1)[1]
        elif line.startswith("SEQ "):
            _, name, s = line.split(" ")
            names.append(name)
            seqs.append(np.frombuffer(s.encode(), dtype=np.uint8) - ord("0"))
    codes = np.stack(seqs).astype(np.int64)
    assert codes.shape == (12, 3000) and codes.max() <= 3
    m = phylo.gtr(1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2)
    rates, probs = phylo.gamma_rates(4, 0.6)
    rs = pair.Restatement(codes, phylo.DNA.init_table, rates, probs, m)
    n = len(names)
    ta, tb = zip(*[(a, b) for a in range(n) for b in range(a + 1, n)])
    out = rs.distances(ta, tb, t_max=10000.0, tol=1e-8, max_iter=40)
    assert np.all(out["status"] == 0)
    D = np.zeros((n, n))
    D[ta, tb] = D[tb, ta] = out["t_opt"]
    want, _ = tree_splits(newick)
    inner = lambda s: {k for k in s if 1 < len(k) < n - 1}
    # (tree_splits and agglomerate put the side without the alphabetically first name; the
    # alignment's first sequence is that one)
    assert names[0] == min(names)
    assert inner(agglomerate(D, names, bionj=True)) == inner(want) and len(inner(want)) == 9
