"""NumPy float64 restatement of the landmark regression kernels (include/upsparts_hip.h "landmark regression evaluation",
csrc/landmarks.hip): ups_part_moments, ups_landmark_gram, ups_landmark_solve, ups_landmark_predict, with the kernels' orders of
summation.  The loops run over chunk items, Cholesky columns and substitution chains; inside them every step is ONE element-wise array
operation, so every multiplication, addition, division and square root is rounded once, as in the kernels.  No BLAS, no np.sum, no
einsum on anything whose bits are compared."""
import numpy as np

MOMENTS_CHUNK = 256             # = ups_part_moments_chunk()
LANDMARK_CHUNK = 64             # = ups_landmark_chunk()
EPS = 2.0 ** -53


def reordered_sum_bound(n, abs_terms):
    """(n - 1) 2^-53 sum|term|: the first-order bound on the error of a float64 sum of n terms in ANY order (each of the n - 1
    additions errs by at most 2^-53 of a partial sum, which sum|term| bounds).  The tests hold a sum in the kernels' order to it
    against a sum of the same terms in another order."""
    return max(n - 1, 0) * EPS * abs_terms


def pow2_at_least(P):
    Pp = 1
    while Pp < P:
        Pp *= 2
    return Pp


def pixel_units(h, w):
    """(u_x [h*w], u_y [h*w], ix, iy): u_x = double(2x + 1 - w) / double(w) for the flat pixel index y * w + x."""
    idx = np.arange(h * w)
    x, y = idx % w, idx // w
    ix, iy = 2 * x + 1 - w, 2 * y + 1 - h
    return ix.astype(np.float64) / np.float64(w), iy.astype(np.float64) / np.float64(h), ix, iy


def part_moments(soft, pred=None, min_mass=0.0, chunk=MOMENTS_CHUNK):
    """soft [N,h,w,P] float32, pred [N,h,w] int64 or None -> {"mass" [N,P], "centre" [N,P,2], "valid" [N,P] uint8, "hard" [N,P,3]
    int32 | None, "invalid" int, "terms" [N,P,3]: sum |term| of the three float sums (for the tests' bounds)}."""
    soft = np.asarray(soft)
    assert soft.dtype == np.float32 and soft.ndim == 4
    N, h, w, P = soft.shape
    HW = h * w
    Pp = pow2_at_least(P)
    G, chunks = chunk // Pp, -(-HW // chunk)
    s = np.zeros((N, chunks * chunk, P), dtype=np.float64)
    s[:, :HW] = soft.reshape(N, HW, P).astype(np.float64)
    ux, uy = np.zeros(chunks * chunk), np.zeros(chunks * chunk)
    ux[:HW], uy[:HW], ix, iy = pixel_units(h, w)
    s = s.reshape(N, chunks, G, Pp, P)
    ux, uy = ux.reshape(1, chunks, G, Pp, 1), uy.reshape(1, chunks, G, Pp, 1)
    m = np.zeros((N, chunks, G, P))
    sx, sy = m.copy(), m.copy()
    with np.errstate(all="ignore"):
        for i in range(Pp):                                  # group g: its Pp pixels in ascending order from 0.0
            v = s[:, :, :, i, :]
            m = m + v
            sx = sx + v * ux[:, :, :, i, :]
            sy = sy + v * uy[:, :, :, i, :]
        g = G
        while g > 1:                                         # t[g] += t[g + s], s = G/2 .. 1
            g //= 2
            m, sx, sy = m[:, :, :g] + m[:, :, g:2 * g], sx[:, :, :g] + sx[:, :, g:2 * g], sy[:, :, :g] + sy[:, :, g:2 * g]
        tm, tx, ty = np.zeros((N, P)), np.zeros((N, P)), np.zeros((N, P))
        for c in range(chunks):                              # the second launch: block order from 0.0
            tm, tx, ty = tm + m[:, c, 0], tx + sx[:, c, 0], ty + sy[:, c, 0]
        ok = np.isfinite(tm) & (tm > 0.0) & (tm >= min_mass)
        den = np.where(ok, tm, 1.0)
        centre = np.stack([np.where(ok, tx / den, 0.0), np.where(ok, ty / den, 0.0)], axis=-1)
        flat = np.abs(soft.reshape(N, HW, P).astype(np.float64))
        fux, fuy = np.abs(ux.reshape(-1)[:HW]), np.abs(uy.reshape(-1)[:HW])
        terms = np.stack([flat.sum(1), (flat * fux[None, :, None]).sum(1), (flat * fuy[None, :, None]).sum(1)], axis=-1)
    out = {"mass": tm, "centre": centre, "valid": ok.astype(np.uint8), "hard": None, "invalid": 0, "terms": terms,
           "sums": np.stack([tm, tx, ty], axis=-1)}
    if pred is not None:
        pred = np.asarray(pred).reshape(N, HW)
        hard = np.zeros((N, P, 3), dtype=np.int64)
        inside = (pred >= 0) & (pred < P)
        for n in range(N):
            pv = pred[n][inside[n]]
            hard[n, :, 0] = np.bincount(pv, minlength=P)
            hard[n, :, 1] = np.bincount(pv, weights=ix[inside[n]], minlength=P).astype(np.int64)      # (|sums| < 2^31: exact in float64)
            hard[n, :, 2] = np.bincount(pv, weights=iy[inside[n]], minlength=P).astype(np.int64)
        out["hard"], out["invalid"] = hard.astype(np.int32), int((~inside).sum())
    return out


def hard_centres(hard, h, w, min_count):
    """centre [N,P,2] = sum(2x + 1 - w) / (w count) in float64 (one multiplication, one division), mass = count, valid = count >=
    min_count and count > 0: what TrainModel.part_centres(source="hard") computes from the integer sums."""
    cnt = hard[..., 0].astype(np.float64)
    ok = (cnt > 0) & (cnt >= min_count)
    den = np.where(ok, cnt, 1.0)
    cx = np.where(ok, hard[..., 1].astype(np.float64) / (np.float64(w) * den), 0.0)
    cy = np.where(ok, hard[..., 2].astype(np.float64) / (np.float64(h) * den), 0.0)
    return np.stack([cx, cy], axis=-1), cnt, ok.astype(np.uint8)


def features(centre, valid):
    """feat [N,2P] float64 = the centres flattened (x_0, y_0, x_1, ..), an invalid part's as (0, 0)."""
    centre = np.asarray(centre, dtype=np.float64)
    keep = (np.asarray(valid) != 0)[..., None]
    return np.ascontiguousarray(np.where(keep, centre, 0.0).reshape(centre.shape[0], -1))


def with_one(feat):
    return np.concatenate([feat, np.ones((feat.shape[0], 1))], axis=1)


def gram(feat, target, vis, chunk=LANDMARK_CHUNK):
    """feat [N,D-1], target [N,K,2], vis [N,K] -> (G [K,D,D], R [K,D,2], cnt [K] int32)."""
    f = with_one(np.asarray(feat, dtype=np.float64))
    N, D = f.shape
    K = vis.shape[1]
    see = np.asarray(vis) != 0
    tgt = np.where(see[..., None], np.asarray(target, dtype=np.float64), 0.0)          # (an invisible target is never read)
    G, R = np.zeros((K, D, D)), np.zeros((K, D, 2))
    for n0 in range(0, N, chunk):
        g, r = np.zeros((K, D, D)), np.zeros((K, D, 2))
        for n in range(n0, min(N, n0 + chunk)):              # ascending n from 0.0; the invisible items are SKIPPED
            k = see[n]
            g[k] = g[k] + (f[n][:, None] * f[n][None, :])[None]
            r[k] = r[k] + f[n][None, :, None] * tgt[n][k][:, None, :]
        G, R = G + g, R + r                                  # block order from 0.0
    return G, R, see.sum(axis=0).astype(np.int32)


def solve(G, R, cnt, lam):
    """-> (W [K,D,2], singular [K] bool): the Cholesky and the two substitutions in the header's order."""
    G, R = np.asarray(G, dtype=np.float64), np.asarray(R, dtype=np.float64)
    K, D, _ = G.shape
    A = G.copy()
    for a in range(D - 1):
        A[:, a, a] = A[:, a, a] + np.float64(lam)
    L = np.zeros((K, D, D))
    bad = np.asarray(cnt) <= 0
    with np.errstate(all="ignore"):
        for j in range(D):
            d = A[:, j, j].copy()
            for m in range(j):
                d = d - L[:, j, m] * L[:, j, m]
            bad = bad | ~((d > 0.0) & np.isfinite(d))
            l = np.sqrt(np.where(bad, 1.0, d))
            L[:, j, j] = l
            if j + 1 < D:
                v = A[:, j + 1:, j].copy()
                for m in range(j):
                    v = v - L[:, j + 1:, m] * L[:, j, m][:, None]
                L[:, j + 1:, j] = v / l[:, None]
        y = np.zeros((K, D, 2))
        for i in range(D):
            r = R[:, i, :].copy()
            for m in range(i):
                r = r - L[:, i, m][:, None] * y[:, m, :]
            y[:, i, :] = r / L[:, i, i][:, None]
        W = np.zeros((K, D, 2))
        for i in range(D - 1, -1, -1):
            r = y[:, i, :].copy()
            for m in range(D - 1, i, -1):
                r = r - L[:, m, i][:, None] * W[:, m, :]
            W[:, i, :] = r / L[:, i, i][:, None]
    W[bad] = 0.0
    return W, bad


def predict(feat, W, target=None, vis=None):
    """-> (pred [N,K,2], d2 [N,K] | None): sum over ascending a from 0.0; d2 = dx dx + dy dy where visible, -1 where not."""
    f = with_one(np.asarray(feat, dtype=np.float64))
    N, D = f.shape
    pred = np.zeros((N, W.shape[0], 2))
    for a in range(D):
        pred = pred + f[:, a][:, None, None] * W[None, :, a, :]
    if target is None:
        return pred, None
    see = np.asarray(vis) != 0
    d = pred - np.where(see[..., None], np.asarray(target, dtype=np.float64), 0.0)
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return pred, np.where(see, d2, -1.0)


def metrics(d2, pck):
    """The host arithmetic of LandmarkRegressor.evaluate, restated: error = sqrt(d2) / 2 over the entries with d2 >= 0."""
    see = d2 >= 0
    err = np.sqrt(np.where(see, d2, 0.0)) / 2.0
    n_vis = see.sum(axis=0)
    mean_k = np.array([err[see[:, k], k].mean() if n_vis[k] else np.nan for k in range(d2.shape[1])])
    out = {"n_visible": n_vis, "mean_error_k": mean_k,
           "mean_error": float(np.nanmean(mean_k)) if n_vis.any() else float("nan"),
           "mean_error_instances": float(err[see].mean()) if see.any() else float("nan")}
    for t in pck:
        out["pck@{:g}".format(t)] = np.array([float((err[see[:, k], k] <= t).mean()) if n_vis[k] else np.nan
                                              for k in range(d2.shape[1])])
    return out
