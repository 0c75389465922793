"""The Bio++ mirror's Newick and Phylip readers (tests/cpp/test_readers_cpu.cpp, no device) on the
two parsimony fixtures of tests/golden: the tree's names, shape and lengths -- the two zero lengths
included -- and the 5 x 10 alignment with its gap column, against a reading of the files made
here."""
import os
import subprocess

import phylo
from conftest import run_make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bpp-phyl_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_cpp_readers_on_the_parsimony_fixtures():
    run_make("-s", "-j8", "-C", HOST, "bin/test_readers_cpu")
    r = subprocess.run([os.path.join(HOST, "bin", "test_readers_cpu"), GOLDEN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
    nodes, seqs, aln, newick = {}, [], None, None
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "NODE":
            nodes[int(f[1])] = (f[2], int(f[3]), int(f[4]), None if f[5] == "none" else float(f[5]))
        elif f[0] == "ALN":
            aln = (int(f[1]), int(f[2]))
        elif f[0] == "SEQ":
            seqs.append((f[1], f[2], [int(x) for x in f[3:]]))
        elif f[0] == "NEWICK":
            newick = line.split(" ", 1)[1]

    # the tree: (((s05:0.1,s04:0):0.3,s03:0):0.26667,s02:0.06667,s01:0.16667); ids in postorder
    want = {0: ("s05", 2, 0, 0.1), 1: ("s04", 2, 0, 0.0), 2: ("-", 4, 2, 0.3), 3: ("s03", 4, 0, 0.0),
            4: ("-", 7, 2, 0.26667), 5: ("s02", 7, 0, 0.06667), 6: ("s01", 7, 0, 0.16667), 7: ("-", -1, 3, None)}
    assert nodes == want
    assert nodes[1][3] == 0.0 and nodes[3][3] == 0.0   # zero lengths are lengths, not missing ones
    with open(os.path.join(GOLDEN, "example1.mp.dnd")) as f:
        src = phylo.Tree.from_newick(f.read().replace("\n", ""))
    back = phylo.Tree.from_newick(newick)
    assert [(n.name, n.dist, len(n.sons)) for n in back.nodes()] == [(n.name, n.dist, len(n.sons)) for n in src.nodes()]

    # the alignment
    with open(os.path.join(GOLDEN, "example1.ph")) as f:
        lines = f.read().split("\n")
    assert aln == (5, 10) == tuple(int(x) for x in lines[0].split())
    assert [(n, s) for n, s, _ in seqs] == [tuple(l.split()) for l in lines[1:6]]
    codes = {c: i for i, c in enumerate(phylo.DNA_CHARS)}
    codes["-"] = -1
    for name, s, values in seqs:
        assert values == [codes[ch] for ch in s]
    column = [v[4] for _, _, v in seqs]
    assert column == [codes["G"], -1, -1, -1, -1]
