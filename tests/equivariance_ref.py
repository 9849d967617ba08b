"""Shared by test_host_equivariance.py and test_gpu_equivariance.py: the NumPy float64 restatement of ups_part_equivariance
(csrc/equivariance.hip; the definitions stand in include/upsparts_hip.h), of evalutil.equivariance_from_counts, the bilinear form of
ups_tps_warp at given pixel positions, the derived tolerance of `tv`, and the maps and grids the tests run on.  Nothing here imports the
package: the definitions are written out a second time, part by part in explicit loops."""
import math

import numpy as np


def inside_mask(grid, h, w):
    """grid [N,h,w,2] float32 (px, py) -> bool [N,h,w]: px, py finite and 0 <= px <= w - 1, 0 <= py <= h - 1."""
    g = np.asarray(grid).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(g).all(axis=-1) & (g[..., 0] >= 0) & (g[..., 0] <= w - 1) & (g[..., 1] >= 0) & (g[..., 1] <= h - 1)


def part_equivariance(soft_a, soft_b, pred_b, grid):
    """soft_a, soft_b [N,h,w,P] float32, pred_b [N,h,w] integers, grid [N,h,w,2] float32 ->
    (counts [N,P,P] int64, invalid, tv [N] float64, terms [N] = the sum of the per-pixel distances (they are >= 0: the scale of the
    tolerance), la [N,h,w] with -1 where nothing was counted).  float64, one rounding per operation, p ascending."""
    a, b = np.asarray(soft_a), np.asarray(soft_b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and np.asarray(grid).dtype == np.float32
    N, h, w, P = a.shape
    a, b = a.astype(np.float64), b.astype(np.float64)
    lb = np.asarray(pred_b).reshape(N, h, w).astype(np.int64)
    g = np.asarray(grid).reshape(N, h, w, 2).astype(np.float64)
    ins = inside_mask(grid, h, w)
    counts, tv, la_map = np.zeros((N, P, P), dtype=np.int64), np.zeros(N), np.full((N, h, w), -1, dtype=np.int64)
    invalid = 0
    for i in range(N):
        ys, xs = np.nonzero(ins[i])
        if len(ys) == 0:
            continue
        X, Y = g[i, ys, xs, 0], g[i, ys, xs, 1]
        x0f, y0f = np.floor(X), np.floor(Y)
        fx, fy = X - x0f, Y - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        gx, gy = 1.0 - fx, 1.0 - fy
        nan = np.zeros(len(ys), dtype=bool)
        best, la, acc = None, np.zeros(len(ys), dtype=np.int64), np.zeros(len(ys))
        with np.errstate(invalid="ignore"):
            for p in range(P):
                top = gx * a[i, y0, x0, p] + fx * a[i, y0, x1, p]
                bot = gx * a[i, y1, x0, p] + fx * a[i, y1, x1, p]
                v = gy * top + fy * bot
                bp = b[i, ys, xs, p]
                nan |= np.isnan(v) | np.isnan(bp)
                if p == 0:
                    best = v.copy()
                else:
                    more = v > best                      # strictly: the FIRST maximal part stays
                    la[more] = p
                    best[more] = v[more]
                acc = acc + np.abs(v - bp)
        t = 0.5 * acc
        l = lb[i, ys, xs]
        ok = ~nan & (l >= 0) & (l < P)
        invalid += int((~ok).sum())
        np.add.at(counts[i], (la[ok], l[ok]), 1)
        la_map[i, ys[ok], xs[ok]] = la[ok]
        tv[i] = math.fsum(t[ok].tolist())               # the correctly rounded sum: the restatement adds no order of its own
    return counts, invalid, tv, tv.copy(), la_map


def tv_atol(HW, terms):
    """The summation-order bound of tv: at most HW non-negative terms added in some order, each partial sum rounded once (relative
    2^-53, and no partial sum exceeds the whole) -> HW 2^-53 sum t per image."""
    return HW * 2.0 ** -53 * np.asarray(terms, dtype=np.float64)


def equivariance_from_counts(counts, tv, HW):
    counts = np.asarray(counts).astype(np.int64)
    n, P = counts.shape[0], counts.shape[1]
    total = int(counts.sum())
    if total == 0:
        raise ValueError("nothing counted")
    C = counts.sum(axis=0)
    iou, present = [], []
    for p in range(P):
        den = int(C[p, :].sum() + C[:, p].sum() - C[p, p])
        iou.append(C[p, p] / den if den > 0 else -1.0)
        if den > 0:
            present.append(C[p, p] / den)
    return {"valid": total / (n * HW), "agreement": sum(int(np.trace(c)) for c in counts) / total, "iou": [float(v) for v in iou],
            "miou": float(np.mean(present)), "tv": float(np.asarray(tv, dtype=np.float64).sum() / total)}


def bilinear_at(img, px, py):
    """The bilinear form of ups_tps_warp (oracle.tps.interpolate) at GIVEN pixel positions px, py [n,h,w], in float64: corner indices
    clamped to the image, weights from the clamped corners.  img [n,h,w,c] -> [n,h,w,c]."""
    img, px, py = np.asarray(img, dtype=np.float64), np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    n, h, w, c = img.shape
    x0, y0 = np.floor(px), np.floor(py)
    x0c, x1c = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    y0c, y1c = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    i = np.arange(n).reshape(n, 1, 1)
    at = lambda yy, xx: img[i, yy.astype(np.int64), xx.astype(np.int64)]
    wa, wb = ((x1c - px) * (y1c - py))[..., None], ((x1c - px) * (py - y0c))[..., None]
    wc, wd = ((px - x0c) * (y1c - py))[..., None], ((px - x0c) * (py - y0c))[..., None]
    return wa * at(y0c, x0c) + wb * at(y1c, x0c) + wc * at(y0c, x1c) + wd * at(y1c, x1c)


# ---------------------------------------------------------------------------------------------- maps
def softmax_maps(rng, N, h, w, P, sharp=3.0):
    """(soft [N,h,w,P] float32: a seeded soft-max rounded to float32, pred [N,h,w] int64: its first maximal part)."""
    z = rng.randn(N, h, w, P) * sharp
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    soft = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    return soft, np.argmax(soft, axis=-1).astype(np.int64)


def tie_maps(N, h, w, P):
    """One-hot maps built to tie under half-pixel shifts: pixel (y, x) of image i belongs to part (x + y + i) mod P, so a sample half
    way between two neighbours is (0.5, 0.5) on two parts and the first one must win."""
    i, y, x = np.meshgrid(np.arange(N), np.arange(h), np.arange(w), indexing="ij")
    pred = ((x + y + i) % P).astype(np.int64)
    return np.eye(P, dtype=np.float32)[pred], pred


def closed_form_case(shift):
    """The issue's closed-form case: h = 4, w = 6, P = 3; soft_a one-hot, part 0 on columns 0-2 and part 2 on columns 3-5; soft_b and
    pred_b the same map; px = x + shift, py = y."""
    h, w, P = 4, 6, 3
    pred = np.where(np.arange(w) < 3, 0, 2).astype(np.int64)[None, None, :].repeat(h, axis=1)
    soft = np.eye(P, dtype=np.float32)[pred]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    grid = np.stack([x + shift, y + 0.0], axis=-1).astype(np.float32)[None]
    return soft, soft.copy(), pred, grid


# ---------------------------------------------------------------------------------------------- grids (everything but "tps")
GRID_KINDS = ("integer", "half", "affine", "edges", "nonfinite")


def make_grid(kind, N, h, w):
    """grid [N,h,w,2] float32 of one kind.  Every kind has inside and outside pixels as soon as the map has more than one pixel."""
    i, y, x = (v.astype(np.float64) for v in np.meshgrid(np.arange(N), np.arange(h), np.arange(w), indexing="ij"))
    if kind == "integer":       # whole-pixel shifts that differ per image; px = w - 1 and py = h - 1 occur exactly (the x1 / y1 clamp, fx = 0)
        px, py = x + 1 + (i % 2), y - 1 + 2 * (i % 2)
    elif kind == "half":        # half a pixel along x on even images, along y on odd ones
        px, py = x + 0.5 * (1 - i % 2), y + 0.5 * (i % 2)
    elif kind == "affine":      # scale 1.25 about the centre plus shear: leaves all four borders
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        px = cx + 1.25 * (x - cx) + 0.3 * (y - cy) + 0.1 * i
        py = cy + 0.3 * (x - cx) + 1.25 * (y - cy) - 0.1 * i
    elif kind == "edges":       # 0, -0.0, size - 1 and their float32 neighbours on both sides, in every combination of px and py
        def ladder(size):
            top = np.float32(size - 1)
            return np.array([0.0, -0.0, np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(0), np.float32(1)), top,
                             np.nextafter(top, np.float32(np.inf)), np.nextafter(top, np.float32(-np.inf))], dtype=np.float32)
        lx, ly = ladder(w), ladder(h)
        k = (i * h * w + y * w + x).astype(np.int64)
        px, py = lx[k % 7], ly[(k // 7) % 7]
    elif kind == "nonfinite":   # the identity moved by a third of a pixel, with NaN, +inf and -inf planted in px or in py
        px, py = x + 1.0 / 3.0, y - 1.0 / 3.0
        k = (i * h * w + y * w + x).astype(np.int64)
        px = np.where(k % 11 == 3, np.nan, np.where(k % 11 == 7, np.inf, px))
        py = np.where(k % 13 == 5, -np.inf, np.where(k % 13 == 9, np.nan, py))
    else:
        raise ValueError(kind)
    return np.stack([px, py], axis=-1).astype(np.float32)
