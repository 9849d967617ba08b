"""NumPy float64 restatement of the part-appearance index (include/upsparts_hip.h "part-appearance index", csrc/partindex.hip,
upsparts_amd/partindex.py): the distance as a loop over the channel, the neighbours by np.lexsort, one k-means step, the seeding and
the Lloyd loop.  The kernels and PartIndex are held to these with equal bits."""
import math

import numpy as np


def distance(x, y):
    """d[..] = sum_a (double(x[.., a]) - double(y[.., a]))^2, accumulated in ascending a from 0.0 (x, y broadcast against each other):
    one rounded subtraction, multiplication and addition per step."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    acc = np.zeros(np.broadcast(x[..., 0], y[..., 0]).shape, dtype=np.float64)
    for a in range(x.shape[-1]):
        d = x[..., a] - y[..., a]
        acc = acc + d * d
    return acc


def normalize(feat, valid):
    """Every code divided by its float64 L2 norm (sqrt of the ascending-channel sum of squares), rounded to float32; a code of norm 0
    becomes invalid (and stays as it is)."""
    f = np.asarray(feat, dtype=np.float64)
    norm = np.sqrt(distance(f, np.zeros_like(f)))
    ok = norm > 0
    out = (f / np.where(ok, norm, 1.0)[..., None]).astype(np.float32)
    return out, (np.asarray(valid) != 0) & ok


def knn(q, qvalid, g, gvalid, K, exclude_same_index):
    """idx [Nq,P,K] int32, dist [Nq,P,K] float64: the K eligible gallery items smallest in (d, g), padded with -1 / +inf."""
    Nq, P, _ = q.shape
    Ng = g.shape[0]
    idx = np.full((Nq, P, K), -1, dtype=np.int32)
    dist = np.full((Nq, P, K), np.inf, dtype=np.float64)
    gi = np.arange(Ng)
    for p in range(P):
        d = distance(q[:, None, p, :], g[None, :, p, :])                  # [Nq, Ng]
        for n in range(Nq):
            if not qvalid[n, p]:
                continue
            ok = gvalid[:, p] != 0
            if exclude_same_index:
                ok = ok & (gi != n)
            cand = gi[ok]
            order = np.lexsort((cand, d[n, cand]))[:K]
            idx[n, p, :len(order)] = cand[order]
            dist[n, p, :len(order)] = d[n, cand[order]]
    return idx, dist


def kmeans_step(feat, valid, cent, prev_label=None):
    """One step on centroids cent [P,k,A] float64 -> dict(label [N,P] int32, mind [N,P], counts [P,k] int32, sums [P,k,A], inertia [P],
    changed, sum_terms [P,k,A], inertia_terms [P]).  label is the first minimal j (-1 where invalid), mind +inf where invalid; the
    float sums are added in index order.  *_terms are the sums of the absolute terms (for the reordered-sum bound)."""
    N, P, A = feat.shape
    k = cent.shape[1]
    valid = np.asarray(valid) != 0
    label = np.full((N, P), -1, dtype=np.int32)
    mind = np.full((N, P), np.inf, dtype=np.float64)
    counts = np.zeros((P, k), dtype=np.int32)
    sums = np.zeros((P, k, A), dtype=np.float64)
    inertia = np.zeros(P, dtype=np.float64)
    f64 = feat.astype(np.float64)
    for p in range(P):
        d = distance(feat[:, None, p, :], cent[p][None, :, :])            # [N, k]
        j = d.argmin(axis=1)                                              # the first minimal index
        v = valid[:, p]
        label[v, p] = j[v]
        mind[v, p] = d[np.arange(N), j][v]
        counts[p] = np.bincount(j[v], minlength=k)
        for n in np.flatnonzero(v):
            sums[p, j[n]] = sums[p, j[n]] + f64[n, p]
            inertia[p] = inertia[p] + mind[n, p]
    changed = int((label != prev_label).sum()) if prev_label is not None else 0
    sum_terms = np.zeros((P, k, A))
    for p in range(P):
        for jj in range(k):
            sum_terms[p, jj] = np.abs(f64[label[:, p] == jj, p]).sum(axis=0)
    inertia_terms = np.where(valid, mind, 0.0).sum(axis=0)
    return {"label": label, "mind": mind, "counts": counts, "sums": sums, "inertia": inertia, "changed": changed,
            "sum_terms": sum_terms, "inertia_terms": inertia_terms}


def reordered_sum_bound(n, terms):
    """(n - 1) 2^-53 sum|term|: the bound on a float64 sum of n terms added in another order."""
    return max(n - 1, 0) * 2.0 ** -53 * terms


def update_centroids(cent, sums, counts):
    """sums / counts in float64; an empty cluster keeps its centroid."""
    new = cent.copy()
    has = counts > 0
    new[has] = sums[has] / counts[has][:, None].astype(np.float64)
    return new


def seed_centres(feat, valid, k, seed, init="kmeans++", assign=None):
    """Initial centroids [P,k,A] float64.  Per part p a np.random.RandomState(seed * 1000 + p).  "kmeans++": the first centre is a
    uniform draw among the valid items; centre j is the valid item at searchsorted(cumsum(mind over the valid items in index order),
    u * total, side="right"), clamped, u = random_sample(), mind from an assignment on the j centres so far.  "random": the first k of
    a permutation of the valid items.  A part with fewer than k valid items raises ValueError naming it.
    `assign(cent [P,j,A]) -> mind [N,P]` (default: this module's kmeans_step) lets PartIndex run the same host logic on the kernel."""
    N, P, A = feat.shape
    valid = np.asarray(valid) != 0
    if init not in ("kmeans++", "random"):
        raise ValueError("init: 'kmeans++' or 'random' (got {!r})".format(init))
    if assign is None:
        def assign(c):
            return kmeans_step(feat, valid, c)["mind"]
    items = [np.flatnonzero(valid[:, p]) for p in range(P)]
    for p in range(P):
        if len(items[p]) < k:
            raise ValueError("k-means: part {} has {} valid items, fewer than k = {}".format(p, len(items[p]), k))
    rngs = [np.random.RandomState(seed * 1000 + p) for p in range(P)]
    f64 = feat.astype(np.float64)
    cent = np.zeros((P, k, A), dtype=np.float64)
    if init == "random":
        for p in range(P):
            cent[p] = f64[items[p][rngs[p].permutation(len(items[p]))[:k]], p]
        return cent
    for p in range(P):
        cent[p, 0] = f64[items[p][rngs[p].randint(len(items[p]))], p]
    for j in range(1, k):
        mind = assign(cent[:, :j].copy())
        for p in range(P):
            cum = np.cumsum(mind[items[p], p])
            u = rngs[p].random_sample()
            at = min(int(np.searchsorted(cum, u * cum[-1], side="right")), len(items[p]) - 1)
            cent[p, j] = f64[items[p][at], p]
    return cent


def lloyd(feat, valid, k, seed=1, init="kmeans++", max_iter=100):
    """Seed, then iterate (step, new centroids) until no label changes or max_iter steps.  Returns the PartIndex.kmeans dict plus
    "inertia_trace" (per iteration, [P]) and "min_gap" (the smallest relative gap between the best and the second-best centroid of a
    valid item over all iterations; inf at k = 1)."""
    N, P, A = feat.shape
    cent = seed_centres(feat, valid, k, seed, init)
    prev = np.full((N, P), -2, dtype=np.int32)
    trace, gap, it = [], np.inf, 0
    v = np.asarray(valid) != 0
    while it < max_iter:
        r = kmeans_step(feat, valid, cent, prev)
        it += 1
        trace.append(r["inertia"].copy())
        if k > 1:
            for p in range(P):
                d = np.sort(distance(feat[:, None, p, :], cent[p][None]), axis=1)[v[:, p]]
                if len(d):
                    gap = min(gap, float(((d[:, 1] - d[:, 0]) / np.maximum(d[:, 1], 1e-300)).min()))
        if r["changed"] == 0:
            break
        cent = update_centroids(cent, r["sums"], r["counts"])
        prev = r["label"]
    return {"clusters": cent, "labels": np.ascontiguousarray(r["label"].T), "counts": r["counts"], "inertia": r["inertia"],
            "iterations": it, "inertia_trace": trace, "min_gap": gap}


# ---------------------------------------------------------------------------------------------- generators
def _valid(rng, N, P):
    v = (rng.uniform(size=(N, P)) >= 0.2).astype(np.uint8)
    return v


def lattice_bank(rng, N, P, A, blobs):
    """feat [N,P,A] float32 = a blob centre (randint(-4, 5) * 8) + an offset (randint(-16, 17) / 16), valid [N,P] uint8 with about
    20 % zeros: every float64 sum of such values (and of their squared differences) is exact in any order."""
    centres = rng.randint(-4, 5, size=(P, blobs, A)) * 8.0
    which = rng.randint(0, blobs, size=(N, P))
    feat = centres[np.arange(P)[None, :], which] + rng.randint(-16, 17, size=(N, P, A)) / 16.0
    return feat.astype(np.float32), _valid(rng, N, P)


def float_bank(rng, N, P, A):
    return rng.standard_normal((N, P, A)).astype(np.float32), _valid(rng, N, P)


def part_area_threshold(min_part_area, S):
    return int(math.ceil(min_part_area * S * S))
