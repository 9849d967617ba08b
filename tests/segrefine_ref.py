"""NumPy restatement of the edge-aware refinement of the segmentation export (csrc/segexport.hip: ups_segment_guide and
ups_segment_render_guided): joint bilateral upsampling of the S x S soft-max guided by the photograph.  The guide
is integer arithmetic; everything else is one IEEE float64 operation per step in the kernel's order (taps j outer, k inner, ascending;
a tap outside the map contributes nothing), so guides, labels, confidences, overlays and counts compare with ==.  Nothing here is
imported from the package: the range table is restated too."""
import numpy as np

from segexport_ref import source_coords, to_byte, table, soft_maps  # noqa: F401  (soft_maps: re-exported for the tests)

RANGE = 766           # L1 distances of two RGB byte triples: 0 .. 3 * 255
FLOOR = 2.0 ** -64    # of a range weight: every denominator stays positive


def tap_ranges(n, S):
    """Source index ranges [a, b) of the S taps of an axis of extent n: never empty, also when n < S."""
    t = np.arange(S, dtype=np.int64)
    a = (t * n) // S
    return a, np.maximum(a + 1, ((t + 1) * n) // S)


def guide(src, S):
    """src uint8 [h,w,3] -> uint8 [S,S,3]: the rounded integer box mean (2 sum + cnt) // (2 cnt) of the pixels each tap covers."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    ya, yb = tap_ranges(src.shape[0], S)
    xa, xb = tap_ranges(src.shape[1], S)
    # an inclusive prefix sum with a leading zero: sum over [a, b) = c[b] - c[a]
    c = np.zeros((src.shape[0] + 1, src.shape[1] + 1, 3), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(src.astype(np.int64), axis=0), axis=1)
    tot = c[yb][:, xb] - c[ya][:, xb] - c[yb][:, xa] + c[ya][:, xa]
    cnt = ((yb - ya)[:, None] * (xb - xa)[None, :])[..., None]
    return ((2 * tot + cnt) // (2 * cnt)).astype(np.uint8)


def range_table(sigma):
    """wr[d] = max(exp(-(d/3)^2 / (2 sigma^2)), 2^-64), d = 0 .. 765; sigma in uint8 levels of mean absolute channel difference."""
    sigma = float(sigma)
    d = np.arange(RANGE, dtype=np.float64) / 3.0
    return np.maximum(np.exp(-(d * d) / (2.0 * (sigma * sigma))), FLOOR)


def refine(soft, src, g, wr, R):
    """One image: soft [S,S,P] float32, src uint8 [h,w,3], g = guide(src, S), wr float64 [766], radius R ->
    (num [h,w,P], den [h,w]) float64, accumulated tap by tap in the kernel's order."""
    soft, src, g = np.asarray(soft), np.asarray(src), np.asarray(g)
    assert soft.dtype == np.float32 and src.dtype == np.uint8 and g.dtype == np.uint8 and 0 <= R <= 3
    S, P = soft.shape[0], soft.shape[2]
    h, w = src.shape[:2]
    a = soft.astype(np.float64)
    gi, si = g.astype(np.int64), src.astype(np.int64)
    y0, _, fy = source_coords(h, S)
    x0, _, fx = source_coords(w, S)
    rad = float(R + 1)
    num = np.zeros((h, w, P), np.float64)
    den = np.zeros((h, w), np.float64)
    for j in range(-R, R + 2):
        ty = y0 + j
        oky = (ty >= 0) & (ty <= S - 1)
        wy = 1.0 - np.abs(fy - float(j)) / rad
        tyc = np.clip(ty, 0, S - 1)
        for k in range(-R, R + 2):
            tx = x0 + k
            okx = (tx >= 0) & (tx <= S - 1)
            wx = 1.0 - np.abs(fx - float(k)) / rad
            txc = np.clip(tx, 0, S - 1)
            d1 = np.abs(si - gi[tyc][:, txc]).sum(axis=2)
            wt = (wy[:, None] * wx[None, :]) * wr[d1]
            ok = oky[:, None] & okx[None, :]
            den = np.where(ok, den + wt, den)
            num = np.where(ok[..., None], num + wt[..., None] * a[tyc][:, txc], num)
    return num, den


def render_guided(soft, src, wr, R, colors=None, alpha=0.5, g=None):
    """One image, as segexport_ref.render: {"labels", "confidence", "counts", "guide", "den", and with colors "overlay"}."""
    S, P = soft.shape[0], soft.shape[2]
    h, w = src.shape[:2]
    g = guide(src, S) if g is None else g
    num, den = refine(soft, src, g, wr, R)
    labels = np.argmax(num, axis=2)
    best = np.take_along_axis(num, labels[..., None], axis=2)[..., 0]
    out = {"labels": labels.astype(np.uint8), "confidence": to_byte((best / den) * 255.0), "guide": g, "den": den,
           "counts": np.bincount(labels.reshape(-1), minlength=P).astype(np.int64)}
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (P, 3)
        alpha = float(alpha)
        out["overlay"] = to_byte(alpha * colors[labels].astype(np.float64) + (1.0 - alpha) * src.astype(np.float64))
    return out


def render_packed_guided(soft, sizes, srcs, wr, R, colors=None, alpha=0.5, fill=0):
    """The packed planes of a whole launch, as segexport_ref.render_packed, and "guide" uint8 [n,S,S,3]."""
    tab, total = table(sizes)
    n, S, P = len(sizes), np.asarray(soft).shape[1], np.asarray(soft).shape[-1]
    out = {"labels": np.full(total, fill, np.uint8), "confidence": np.full(total, fill, np.uint8),
           "counts": np.zeros((n, P), np.int64), "guide": np.zeros((n, S, S, 3), np.uint8), "table": tab, "total": total}
    if colors is not None:
        out["overlay"] = np.full((total, 3), fill, np.uint8)
    for i, (h, w) in enumerate(sizes):
        r = render_guided(soft[i], srcs[i], wr, R, colors, alpha)
        o = int(tab[i, 0])
        out["labels"][o:o + h * w] = r["labels"].reshape(-1)
        out["confidence"][o:o + h * w] = r["confidence"].reshape(-1)
        out["counts"][i] = r["counts"]
        out["guide"][i] = r["guide"]
        if colors is not None:
            out["overlay"][o:o + h * w] = r["overlay"].reshape(-1, 3)
    return out
