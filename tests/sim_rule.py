"""The draw of plk_simulate (include/plk.h), restated in numpy: Philox4x64-10, the uniform of a
(seed, replicate, site, draw index), the inverse-CDF rule and the walk down a preorder list.

Everything here is the definition, not an approximation of it: the GPU tests compare states and
classes with ==.  No GPU, no libplk."""
import numpy as np

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157  # multipliers
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B  # key increments
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mulhilo(a, b):
    """(hi, lo) of the 128-bit product of the constant a and the uint64 array b."""
    b = _u64(b)
    al, ah = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    bl, bh = b & _M32, b >> _S32
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    hi = hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)
    return hi, np.uint64(a) * b


def philox(counter, key):
    """Philox4x64-10 of counter (c0, c1, c2, c3) and key (k0, k1); every entry a Python int or a
    uint64 array (broadcast against each other).  Returns the block's four words."""
    with np.errstate(over="ignore"):
        c = [_u64(x) for x in np.broadcast_arrays(*[_u64(x) for x in counter])]
        k0, k1 = int(key[0]), int(key[1])
        for _ in range(10):
            hi0, lo0 = mulhilo(M0, c[0])
            hi1, lo1 = mulhilo(M1, c[2])
            c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
            k0, k1 = (k0 + W0) & (2**64 - 1), (k1 + W1) & (2**64 - 1)
    return c


def to_unit(word):
    """A word's uniform number in [0, 1): its upper 53 bits times 2^-53."""
    return (_u64(word) >> np.uint64(11)).astype(np.float64) * 2.0**-53


def uniform(seed, replicate, site, k):
    """u(site, k): word k & 3 of Philox(counter = (site, k >> 2, replicate, 0), key = (seed, 0))."""
    return to_unit(philox((site, k >> 2, replicate, 0), (seed, 0))[k & 3])


def cumulative(p):
    """Sequential fp64 sums along the last axis: cum[0] = p[0], cum[y] = cum[y - 1] + p[y]."""
    p = np.asarray(p, dtype=np.float64)
    cum = np.empty_like(p)
    cum[..., 0] = p[..., 0]
    for y in range(1, p.shape[-1]):
        cum[..., y] = cum[..., y - 1] + p[..., y]
    return cum


def fallback(p):
    """The largest y with p[y] > 0 along the last axis (0 for a row without one)."""
    p = np.asarray(p, dtype=np.float64)
    n = p.shape[-1]
    pos = p > 0
    return np.where(pos.any(axis=-1), n - 1 - np.argmax(pos[..., ::-1], axis=-1), 0)


def inv_cdf(p, u):
    """Per row of p [N, n] (or one row for every u) the first y with u < cum[y], else fallback."""
    p = np.asarray(p, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    if p.ndim == 1:
        p = np.broadcast_to(p, (len(u), p.shape[0]))
    below = u[:, None] < cumulative(p)
    return np.where(below.any(axis=1), np.argmax(below, axis=1), fallback(p)).astype(np.int64)


def preorder(kids, root):
    """[(node, father)] for every non-root node, fathers first, sons in list order."""
    out, st = [], [root]
    while st:
        v = st.pop()
        for c in kids.get(v, ()):
            out.append((c, v))
        st.extend(reversed(list(kids.get(v, ()))))
    return out


def kids_of_ops(ops):
    """Sons per node from an op list (ACCUMULATE ops append to their father's list)."""
    kids = {}
    for p, ch, _ in ops:
        kids.setdefault(p, []).extend(ch)
    return kids


def walk(order, root, P, probs, pi, seed, replicate, sites):
    """classes [N] and {node: states [N]} of the sites (global indices): k = 0 the class, 1 the root
    state, 2 + v node v from row P[v][class][state of v's father]."""
    sites = _u64(sites)
    cls = inv_cdf(np.asarray(probs, dtype=np.float64), uniform(seed, replicate, sites, 0))
    states = {root: inv_cdf(np.asarray(pi, dtype=np.float64), uniform(seed, replicate, sites, 1))}
    for v, f in order:
        states[v] = inv_cdf(np.asarray(P[v])[cls, states[f]], uniform(seed, replicate, sites, 2 + v))
    return cls, states


def simulate(ops, root, P, probs, pi, seed, replicate=0, site0=0, n_sites=1):
    """walk() over the tree of an op list for the sites site0 .. site0 + n_sites."""
    return walk(preorder(kids_of_ops(ops), root), root, P, probs, pi, seed, replicate,
                np.arange(site0, site0 + n_sites, dtype=np.uint64))
