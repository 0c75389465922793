"""The draws of plk_smap_sample (include/plk.h), restated in numpy and vectorised over sites and
replicates: the weighted draw, the ancestral states down the tree, and per branch the number of
jumps, the chain of states and the spacings of the uniformised path.

Everything here is the definition, not an approximation of it: fed the device's P, L and tables,
classes, states, n_jumps and counts are compared with ==, dwelling times at 1e-12 (the device's log
is not libm's).  Philox and the sequential sums come from sim_rule.py.  No GPU, no libplk."""
import numpy as np

import sim_rule as sr

N_MAX = 128  # PLK_SMAP_MAX_JUMPS


def uniform(seed, replicate, site, k, c3):
    """u(site, k) of stream c3: word k & 3 of Philox(counter = (site, k >> 2, replicate, c3), key =
    (seed, 0)); site and replicate uint64 arrays of one shape, k an int or an array of that shape."""
    k = np.broadcast_to(np.asarray(k, dtype=np.uint64), np.shape(site))
    w = sr.philox((site, k >> np.uint64(2), replicate, c3), (seed, 0))
    return sr.to_unit(np.choose((k & np.uint64(3)).astype(np.int64), w))


def tables(Q, rates=None, t=None):
    """mu, R = I + Q / mu, Rpow [N_MAX + 1][S][S] and, with rates and t, pois [C][N_MAX + 1]."""
    Q = np.asarray(Q, dtype=np.float64)
    S = Q.shape[0]
    mu = float(np.max(-np.diag(Q)))
    R = Q / mu
    R[np.arange(S), np.arange(S)] = 1.0 + np.diag(Q) / mu
    Rpow = np.empty((N_MAX + 1, S, S))
    Rpow[0] = np.eye(S)
    for n in range(1, N_MAX + 1):
        Rpow[n] = Rpow[n - 1] @ R
    out = {"mu": mu, "R": R, "Rpow": Rpow}
    if rates is not None:
        lam = mu * np.asarray(rates, dtype=np.float64) * t
        pois = np.empty((len(lam), N_MAX + 1))
        pois[:, 0] = np.exp(-lam)
        for n in range(1, N_MAX + 1):
            pois[:, n] = pois[:, n - 1] * lam / n
        out["pois"] = pois
    return out


def weighted_draw(w, u, thr=None):
    """Per row of w [N, n]: weights not > 0 count as 0, cum the sequential sum, thr = u cum[-1]; the
    first y with thr < cum[y], else the largest y with w[y] > 0 (0 for a row without one)."""
    w = np.asarray(w, dtype=np.float64)
    w = np.where(w > 0, w, 0.0)
    cum = sr.cumulative(w)
    if thr is None:
        thr = u * cum[:, -1]
    below = thr[:, None] < cum
    return np.where(below.any(axis=1), np.argmax(below, axis=1), sr.fallback(w)).astype(np.int64)


def class_weights(L_root, probs, pi):
    """w [N, C] = p_c * (sum_x pi_x * L_root[c][x]), the inner sum sequential in x."""
    L_root = np.asarray(L_root, dtype=np.float64)
    s = np.zeros(L_root.shape[:2])
    for x in range(L_root.shape[2]):
        s = s + pi[x] * L_root[:, :, x]
    return np.asarray(probs, dtype=np.float64)[None, :] * s


def draw_path(a, b, cls, P, tab, t, type_of, T, seed, rep, site, v):
    """The path on branch v for the flat samples (a, b, cls, rep, site): (n_jumps [N], counts [N, T],
    dwell [N, S], forced [N]).  P [C][S][S]; tab: R, Rpow of the branch's model and pois [C][N_MAX + 1]
    of the branch."""
    N, S = len(a), P.shape[1]
    R, Rpow, pois = tab["R"], tab["Rpow"], tab["pois"]
    c3 = 2 + v
    # number of jumps: scan upward until every sample has stopped
    thr = uniform(seed, rep, site, 0, c3) * P[cls, a, b]
    cum = np.zeros(N)
    last = np.full(N, -1)
    n = np.full(N, -1)
    for j in range(N_MAX + 1):
        open_ = n < 0
        if not open_.any():
            break
        w = pois[cls, j] * Rpow[j, a, b]
        pos = open_ & (w > 0)
        cum = np.where(pos, cum + w, cum)
        last = np.where(pos, j, last)
        n = np.where(pos & (thr < cum), j, n)
    n = np.where(n < 0, last, n)
    forced = (n < 0) & (a != b)
    n = np.where(n < 0, np.where(a == b, 0, 1), n)
    counts = np.zeros((N, T), dtype=np.int64)
    dwell = np.zeros((N, S))
    idx = np.arange(N)
    stay = n == 0
    dwell[idx[stay], a[stay]] = t
    nmax = int(n.max())
    if nmax == 0:
        return n, counts, dwell, forced
    e = np.zeros((nmax + 1, N))
    se = np.zeros(N)
    for j in range(nmax + 1):
        act = (n > 0) & (j <= n)
        e[j] = -np.log(1.0 - uniform(seed, rep, site, 2 * j + 2, c3))
        se = np.where(act, se + e[j], se)
    x = a.copy()
    for j in range(nmax + 1):
        act = (n > 0) & (j <= n)
        if j > 0:
            xn = np.where(act, b, x)
            inner = act & (j < n)
            if inner.any():
                ii = idx[inner]
                w = R[x[ii]] * Rpow[n[ii] - j, :, b[ii]]
                xn[ii] = weighted_draw(w, uniform(seed, rep[ii], site[ii], 2 * j - 1, c3))
            ty = np.where(act & (xn != x), type_of[x, xn], 0)
            ev = ty > 0
            np.add.at(counts, (idx[ev], ty[ev] - 1), 1)
            x = xn
        ia = idx[act]
        dwell[ia, x[ia]] += (t * e[j, ia]) / se[ia]
    return n, counts, dwell, forced


def sample(order, root, P, L, probs, pi, tabs, t, type_of, T, seed, replicates, sites, paths=None):
    """Every draw of plk_smap_sample for the replicates x sites (global site indices); paths: the
    branches whose paths are drawn (None: all; the states of every node are drawn either way).

    order: [(node, father)] fathers first; P: {v: [C][S][S]}; L: {node: [n_sites][C][S]} (a tip: its
    code's row for every class); tabs: {v: tables of v's model with v's pois}; t: {v: length}.
    Returns a dict: "classes" [R, n], "states" {node: [R, n]}, "jumps" {v: [R, n]}, "counts"
    {v: [R, n, T]}, "dwell" {v: [R, n, S]}, "bad" [n] and "n_bad".  Bad sites: 255, zeros."""
    sites = np.asarray(sites, dtype=np.uint64)
    reps = np.asarray(replicates, dtype=np.uint64)
    nR, n = len(reps), len(sites)
    probs, pi = np.asarray(probs, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    type_of = np.asarray(type_of, dtype=np.int64)
    wc = class_weights(L[root], probs, pi)
    wc = np.where(wc > 0, wc, 0.0)
    tot = sr.cumulative(wc)[:, -1]
    bad = ~((tot > 0) & np.isfinite(tot))
    good = np.where(~bad)[0]
    # the flat samples: replicate-major over the good sites
    rep = np.repeat(reps, len(good))
    pat = np.tile(good, nR)
    site = sites[pat]
    cls = weighted_draw(wc[pat], uniform(seed, rep, site, 0, 1))
    flat = {root: weighted_draw(pi[None, :] * L[root][pat, cls], uniform(seed, rep, site, 1, 1))}
    S = len(pi)

    def full(x, fill, dtype):
        out = np.full((nR, n) + x.shape[1:], fill, dtype=dtype)
        out[:, good] = x.reshape((nR, len(good)) + x.shape[1:])
        return out

    out = {"classes": full(cls, 255, np.int64), "states": {}, "jumps": {}, "counts": {}, "dwell": {}, "bad": bad}
    n_bad = int(bad.sum()) * nR
    for v, f in order:
        a = flat[f]
        b = weighted_draw(P[v][cls, a] * L[v][pat, cls], uniform(seed, rep, site, 2 + v, 1))
        flat[v] = b
        if paths is not None and v not in paths:
            continue
        nj, cnt, dw, forced = draw_path(a, b, cls, P[v], tabs[v], t[v], type_of, T, seed, rep, site, v)
        n_bad += int(forced.sum())
        out["jumps"][v] = full(nj, 0, np.int64)
        out["counts"][v] = full(cnt, 0, np.int64)
        out["dwell"][v] = full(dw, 0.0, np.float64)
    for v, x in flat.items():
        out["states"][v] = full(x, 255, np.int64)
    out["n_bad"] = n_bad
    return out
