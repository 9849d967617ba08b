"""NumPy float64 restatement of the segmentation export (csrc/segexport.hip, ups_segment_render): the
specification the kernel's bytes are compared with.  The definitions are this project's -- the reference only ever resizes the ground
truth down to the model's resolution -- and every operation below is one IEEE float64 operation in the order the kernel performs it
(no fused multiply-add, correctly rounded division), so labels, confidences, overlays and counts compare with ==."""
import numpy as np

CHUNK = 1024          # pixels per block of ups_segment_render (= ops.SEGMENT_CHUNK): only the table's fourth word depends on it
ALIGN = 16            # an image's pixel offset in the packed planes is a multiple of it


def source_coords(n_out, S):
    """Output indices 0 .. n_out-1 of an extent -> (i0, i1, f): the two taps in [0, S-1] and the weight of the second."""
    i = np.arange(n_out, dtype=np.int64)
    s = ((i + 0.5) * float(S)) / float(n_out) - 0.5
    s = np.clip(s, 0.0, float(S - 1))
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, S - 1), s - fl


def resample(soft, h, w):
    """soft [S,S,P] float32 -> v [h,w,P] float64: the bilinear values of every part at the output pixels."""
    soft = np.asarray(soft)
    assert soft.dtype == np.float32 and soft.ndim == 3 and soft.shape[0] == soft.shape[1]
    a = soft.astype(np.float64)
    S = a.shape[0]
    y0, y1, fy = source_coords(h, S)
    x0, x1, fx = source_coords(w, S)
    fx, fy = fx[None, :, None], fy[:, None, None]
    gx, gy = 1.0 - fx, 1.0 - fy
    top = gx * a[y0][:, x0] + fx * a[y0][:, x1]
    bot = gx * a[y1][:, x0] + fx * a[y1][:, x1]
    return gy * top + fy * bot


def to_byte(v):
    return np.clip(np.floor(v + 0.5), 0.0, 255.0).astype(np.uint8)


def render(soft, h, w, colors=None, src=None, alpha=0.5):
    """One image: {"labels" [h,w] uint8, "confidence" [h,w] uint8, "counts" [P] int64, and with colors "overlay" [h,w,3] uint8}.
    label = first part of maximal value (np.argmax: finite values); src uint8 [h,w,3] or None (the overlay is then the colour)."""
    v = resample(soft, h, w)
    P = v.shape[2]
    labels = np.argmax(v, axis=2)
    best = np.take_along_axis(v, labels[..., None], axis=2)[..., 0]
    out = {"labels": labels.astype(np.uint8), "confidence": to_byte(best * 255.0),
           "counts": np.bincount(labels.reshape(-1), minlength=P).astype(np.int64)}
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (P, 3)
        col = colors[labels]
        if src is None:
            out["overlay"] = col.copy()
        else:
            src = np.asarray(src)
            assert src.dtype == np.uint8 and src.shape == (h, w, 3)
            alpha = float(alpha)
            out["overlay"] = to_byte(alpha * col.astype(np.float64) + (1.0 - alpha) * src.astype(np.float64))
    return out


def table(sizes, chunk=CHUNK):
    """sizes [(h, w)] -> (int32 [n,4] rows (pixel_offset, h, w, first_block), total pixels of a packed plane): image i starts at the
    end of image i-1 rounded up to a multiple of 16; first_block is the prefix sum of ceil(h w / chunk)."""
    rows, off, blk = [], 0, 0
    for h, w in sizes:
        h, w = int(h), int(w)
        rows.append((off, h, w, blk))
        blk += -(-(h * w) // chunk)
        off = -(-(off + h * w) // ALIGN) * ALIGN
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), off


def render_packed(soft, sizes, colors=None, srcs=None, alpha=0.5, fill=0):
    """The packed planes of a whole launch: {"labels" [T], "confidence" [T], "overlay" [T,3], "counts" [n,P], "table", "total"}; the
    alignment gaps hold `fill`."""
    tab, total = table(sizes)
    n, P = len(sizes), np.asarray(soft).shape[-1]
    out = {"labels": np.full(total, fill, np.uint8), "confidence": np.full(total, fill, np.uint8),
           "counts": np.zeros((n, P), np.int64), "table": tab, "total": total}
    if colors is not None:
        out["overlay"] = np.full((total, 3), fill, np.uint8)
    for i, (h, w) in enumerate(sizes):
        r = render(soft[i], h, w, colors, None if srcs is None else srcs[i], alpha)
        o = int(tab[i, 0])
        out["labels"][o:o + h * w] = r["labels"].reshape(-1)
        out["confidence"][o:o + h * w] = r["confidence"].reshape(-1)
        out["counts"][i] = r["counts"]
        if colors is not None:
            out["overlay"][o:o + h * w] = r["overlay"].reshape(-1, 3)
    return out


def soft_maps(rng, n, S, P, kind="random"):
    """float32 [n,S,S,P] soft-max-like maps.  random: a soft-max of N(0, 2) logits computed in float32; onehot: exact 0 / 1 rows;
    ties: every value one of {0.25, 0.5} with the maximum shared by at least two parts wherever P >= 2 (sums are not 1: the kernel
    does not need them to be)."""
    if kind == "onehot":
        lab = rng.randint(0, P, size=(n, S, S))
        return np.eye(P, dtype=np.float32)[lab]
    if kind == "ties":
        m = np.where(rng.rand(n, S, S, P) < 0.5, np.float32(0.25), np.float32(0.5)).astype(np.float32)
        if P >= 2:
            k = rng.randint(0, P - 1, size=(n, S, S))
            np.put_along_axis(m, k[..., None], np.float32(0.5), axis=3)
            np.put_along_axis(m, (k + 1)[..., None], np.float32(0.5), axis=3)
        return m
    z = (rng.randn(n, S, S, P) * 2).astype(np.float32)
    e = np.exp(z - z.max(axis=3, keepdims=True)).astype(np.float32)
    return (e / e.sum(axis=3, keepdims=True, dtype=np.float32)).astype(np.float32)
