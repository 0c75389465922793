"""CPU tests of the draw's restatement (tests/sim_rule.py): Philox4x64-10 against its known answer
and numpy's own Philox, the uniform numbers, the inverse-CDF rule on hand-written rows, and a
goodness-of-fit check that the walk samples the model it is given."""
import itertools
import math

import numpy as np
import pytest

import phylo
import sim_rule as sr


def test_philox_known_answer():
    w = sr.philox((0, 0, 0, 0), (0, 0))
    assert [f"{int(x):016x}" for x in w] == ["16554d9eca36314c", "db20fe9d672d0fdc", "d7e772cee186176b",
                                             "7e68b68aec7ba23b"]


PAIRS = [((0, 0, 0, 0), (0, 0)),
         ((2**64 - 2, 5, 7, 9), (0x0123456789ABCDEF, 0xFEDCBA9876543210)),
         ((123456789, 2**63, 2**64 - 1, 42), (2**64 - 1, 1))]


def _counter_plus_one(c):
    v = sum(int(x) << (64 * i) for i, x in enumerate(c)) + 1
    return tuple((v >> (64 * i)) & (2**64 - 1) for i in range(4))


@pytest.mark.parametrize("counter,key", PAIRS)
def test_philox_equals_numpy(counter, key):
    """numpy increments the counter before its first block."""
    bg = np.random.Philox(counter=np.array(counter, dtype=np.uint64), key=np.array(key, dtype=np.uint64))
    raw = bg.random_raw(8)
    c1 = _counter_plus_one(counter)
    c2 = _counter_plus_one(c1)
    assert [int(x) for x in sr.philox(c1, key)] == [int(x) for x in raw[:4]]
    assert [int(x) for x in sr.philox(c2, key)] == [int(x) for x in raw[4:]]


def test_philox_is_vectorised():
    sites = np.array([0, 1, 2**40 + 3, 2**64 - 1], dtype=np.uint64)
    blocks = sr.philox((sites, 3, 7, 0), (11, 0))
    for i, s in enumerate(sites):
        one = sr.philox((int(s), 3, 7, 0), (11, 0))
        assert [int(b[i]) for b in blocks] == [int(x) for x in one]


@pytest.mark.parametrize("counter,key", PAIRS)
def test_uniform_equals_numpy_generator(counter, key):
    g = np.random.Generator(np.random.Philox(counter=np.array(counter, dtype=np.uint64),
                                             key=np.array(key, dtype=np.uint64)))
    u = sr.to_unit(np.array([int(x) for x in sr.philox(_counter_plus_one(counter), key)], dtype=np.uint64))
    assert np.array_equal(u, g.random(4))


def test_uniform_range_and_indexing():
    sites = np.arange(5000, dtype=np.uint64)
    for k in (0, 1, 2, 3, 4, 9, 130):
        u = sr.uniform(5, 2, sites, k)
        assert u.min() >= 0.0 and u.max() < 1.0
        blk = sr.philox((sites, k >> 2, 2, 0), (5, 0))
        assert np.array_equal(u, sr.to_unit(blk[k & 3]))
    assert sr.to_unit(2**64 - 1) == 1.0 - 2.0**-53 and sr.to_unit(0) == 0.0 and sr.to_unit(2047) == 0.0


def test_inverse_cdf_rule():
    inv = lambda p, u: sr.inv_cdf(np.array(p), np.array(u)).tolist()
    # zeros at the front, in the middle and at the end: a zero entry is never drawn
    assert inv([0.0, 0.5, 0.5], [0.0, 0.49, 0.5, 0.99]) == [1, 1, 2, 2]
    assert inv([0.5, 0.0, 0.5], [0.0, 0.49, 0.5, 0.99]) == [0, 0, 2, 2]
    assert inv([0.5, 0.5, 0.0], [0.0, 0.49, 0.5, 1.0 - 2.0**-53]) == [0, 0, 1, 1]
    # a row that sums to 0.5: above it the largest index with p > 0
    assert inv([0.25, 0.25, 0.0], [0.49, 0.5, 0.51, 0.99]) == [1, 1, 1, 1]
    assert inv([0.25, 0.0, 0.25, 0.0], [0.24, 0.25, 0.49, 0.5, 0.75]) == [0, 2, 2, 2, 2]
    # u exactly a cumulative value belongs to the next index (u < cum is strict)
    assert inv([0.25, 0.25, 0.25, 0.25], [0.25, 0.5, 0.75]) == [1, 2, 3]
    assert inv([0.25, 0.25, 0.25, 0.25], [np.nextafter(0.25, 0), np.nextafter(0.5, 0)]) == [0, 1]
    # rounding: 0.1 * 10 sums to less than 1 in sequential fp64
    p = [0.1] * 10
    assert sr.cumulative(np.array(p))[-1] < 1.0
    assert inv(p, [1.0 - 2.0**-53]) == [9]
    # one row per u
    rows = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    assert sr.inv_cdf(rows, np.array([0.3, 0.3, 0.3])).tolist() == [0, 1, 0]


def chi2_quantile(df, upper_tail=1e-6):
    try:
        from scipy.stats import chi2
        return float(chi2.isf(upper_tail, df))
    except ImportError:
        z = 4.753424308822899  # the normal quantile of 1 - 1e-6
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3  # Wilson-Hilferty


def pearson(counts, expected):
    """Pearson's statistic and its cells after merging cells of expected count below 5."""
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    small = expected < 5.0
    if small.any():
        counts = np.append(counts[~small], counts[small].sum())
        expected = np.append(expected[~small], expected[small].sum())
    return float(((counts - expected) ** 2 / expected).sum()), len(counts)


N_SITES = 2**18
OPS = [(4, (0, 1), 0), (5, (2, 3), 0), (6, (4, 5), 0)]
ROOT = 6


@pytest.fixture(scope="module")
def sample():
    m = phylo.t92(3.0, 0.3)
    rates = np.array([0.3, 2.4])
    probs = np.array([2.0 / 3.0, 1.0 / 3.0])
    t = {0: 0.1, 1: 0.3, 2: 0.05, 3: 0.6, 4: 0.2, 5: 0.15}
    P = {v: np.stack([(m.V * np.exp(m.lam * r * tv)) @ m.Vinv for r in rates]) for v, tv in t.items()}
    cls, states = sr.simulate(OPS, ROOT, P, probs, m.pi, seed=1, n_sites=N_SITES)
    return m, probs, P, cls, states


def pattern_probabilities(P, probs, pi):
    """Exact probability of each of the 256 tip patterns by pruning over the tree OPS."""
    pat = np.array(list(itertools.product(range(4), repeat=4)))  # [256, tip]
    total = np.zeros(len(pat))
    for c, pc in enumerate(probs):
        L = {t: np.eye(4)[pat[:, t]] for t in range(4)}  # [256, state]
        for p, ch, _ in OPS:
            L[p] = np.prod([L[s] @ P[s][c].T for s in ch], axis=0)
        total += pc * (L[ROOT] @ pi)
    return total


def test_walk_samples_the_tip_patterns(sample):
    m, probs, P, _, states = sample
    prob = pattern_probabilities(P, probs, m.pi)
    assert abs(prob.sum() - 1.0) < 1e-12
    idx = ((states[0] * 4 + states[1]) * 4 + states[2]) * 4 + states[3]
    stat, cells = pearson(np.bincount(idx, minlength=256), N_SITES * prob)
    assert cells > 100
    assert stat < chi2_quantile(cells - 1), (stat, cells)


def test_walk_samples_root_states_and_classes(sample):
    m, probs, _, cls, states = sample
    stat, cells = pearson(np.bincount(states[ROOT], minlength=4), N_SITES * m.pi)
    assert cells == 4 and stat < chi2_quantile(3), stat
    stat, cells = pearson(np.bincount(cls, minlength=2), N_SITES * probs)
    assert cells == 2 and stat < chi2_quantile(1), stat
