"""Shared by test_host_devaug.py and test_gpu_devaug.py:

  * the two pipelines' draw code as it stood before augment.py was split into draw and build halves (``appearance_ops_before`` /
    ``shape_ops_before``; the helpers the split did not touch are augment.py's);
  * a NumPy executor of the per-image records of data.fill_aug_plan (csrc/augment.hip's layout): appearance ops other than gray call
    the host functions of augment.py, gray, the three warps and the Gaussian field follow the kernels' float32 arithmetic;
  * the small PNG pair datasets (noise and 4 x 4-block images) and the comparison in uint8 levels.
"""
import numpy as np
from scipy import ndimage

F = np.float32


def _pkg():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import augment, data
    return augment, data


# ------------------------------------------------------------------------------------------------ the draw code before the split
def _draw_color_op_before(rng):
    A, _ = _pkg()
    k = rng.randint(3)
    if k == 0:
        a, b = 1.0 + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)
        return lambda im: np.clip(np.arange(256, dtype=np.float32) * a + b * 255.0, 0, 255).astype(np.uint8)[im]
    if k == 1:
        sh = [int(round(rng.uniform(-20, 20))) for _ in range(3)]
        return lambda im: A._rgb_shift(im, sh)
    dh, ds, dv = int(round(rng.uniform(-20, 20))), int(round(rng.uniform(-30, 30))), int(round(rng.uniform(-20, 20)))
    return lambda im: A._hue_sat_val(im, dh, ds, dv)


def appearance_ops_before(rng, p=0.9):
    A, _ = _pkg()
    ops = []
    if rng.rand() >= p:
        return ops
    if rng.rand() < 0.5:
        ops.append(A._median3 if rng.randint(2) == 0 else A._box3)
    for _ in range(3):
        if rng.rand() < 0.8:
            ops.append(_draw_color_op_before(rng))
    if rng.rand() < 0.1:
        ops.append(A._to_gray)
    if rng.rand() < 0.3:
        perm = rng.permutation(3)
        ops.append(lambda im: np.ascontiguousarray(im[..., perm]))
    return ops


def _shift_scale_rotate_before(rng, h, w):
    A, _ = _pkg()
    angle = np.deg2rad(rng.uniform(-25, 25))
    scale = 1.0 + rng.uniform(-0.25, 0.25)
    dx, dy = rng.uniform(-0.0625, 0.0625) * w, rng.uniform(-0.0625, 0.0625) * h
    cx, cy = w / 2.0, h / 2.0
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    fwd = np.array([[c, s, (1 - c) * cx - s * cy + dx], [-s, c, s * cx + (1 - c) * cy + dy], [0, 0, 1]], np.float64)
    inv = np.linalg.inv(fwd)[:2].astype(np.float32)
    ys, xs = A._affine_grid(h, w, inv)
    return lambda im: A._warp(im, ys, xs)


def _piecewise_affine_before(rng, h, w, rows=4, cols=4):
    A, _ = _pkg()
    scale = rng.uniform(0.03, 0.05)
    jy = rng.normal(0, scale, (rows, cols)).astype(np.float32) * h
    jx = rng.normal(0, scale, (rows, cols)).astype(np.float32) * w
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float32)
    cy, cx = gy * (rows - 1) / max(h - 1, 1), gx * (cols - 1) / max(w - 1, 1)
    dy = ndimage.map_coordinates(jy, [cy, cx], order=1, mode="nearest")
    dx = ndimage.map_coordinates(jx, [cy, cx], order=1, mode="nearest")
    ys, xs = gy + dy, gx + dx
    return lambda im: A._warp(im, ys, xs)


def _elastic_before(rng, h, w, alpha=1.0, sigma=50.0, alpha_affine=50.0):
    A, _ = _pkg()
    c = np.float32([w, h]) / 2.0
    sq = min(h, w) // 3
    p1 = np.float32([c + sq, [c[0] + sq, c[1] - sq], c - sq])
    p2 = p1 + rng.uniform(-alpha_affine, alpha_affine, p1.shape).astype(np.float32)
    a = np.concatenate([p1, np.ones((3, 1), np.float32)], 1)
    fwd = np.linalg.solve(a.astype(np.float64), p2.astype(np.float64)).T
    inv = np.linalg.inv(np.vstack([fwd, [0, 0, 1]]))[:2].astype(np.float32)
    ys, xs = A._affine_grid(h, w, inv)
    dx = ndimage.gaussian_filter(rng.rand(h, w).astype(np.float32) * 2 - 1, sigma) * alpha
    dy = ndimage.gaussian_filter(rng.rand(h, w).astype(np.float32) * 2 - 1, sigma) * alpha
    ys, xs = ys + dy, xs + dx
    return lambda im: A._warp(im, ys, xs)


def shape_ops_before(rng, h, w, p=0.9):
    ops = []
    if rng.rand() >= p:
        return ops
    if rng.rand() < 0.3:
        ops.append(lambda im: np.ascontiguousarray(im[:, ::-1]))
    if rng.rand() < 0.3:
        ops.append(_shift_scale_rotate_before(rng, h, w))
    if rng.rand() < 0.3:
        ops.append(_piecewise_affine_before(rng, h, w) if rng.randint(2) == 0 else _elastic_before(rng, h, w))
    return ops


# ------------------------------------------------------------------------------------------------ the executor of the records
def _tap(c, size):
    """Clamped bilinear footprint along one axis, float32: (i0, i1, f).  A NaN coordinate goes to 0."""
    hi = F(size - 1)
    cc = np.where(~(c >= 0), F(0), np.where(c > hi, hi, c)).astype(F)
    fl = np.floor(cc)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), cc - fl


def _lerp2(a00, a01, a10, a11, fx, fy):
    top = a00 + (a01 - a00) * fx
    bot = a10 + (a11 - a10) * fx
    return top + (bot - top) * fy


def warp32(img, ys, xs):
    """uint8 [S,S,3] resampled at float32 (ys, xs): clamp, floor, a + (b - a) * f along x then y, rint, clip."""
    S = img.shape[0]
    y0, y1, fy = _tap(ys.astype(F), S)
    x0, x1, fx = _tap(xs.astype(F), S)
    f = img.astype(F)
    out = _lerp2(f[y0, x0], f[y0, x1], f[y1, x0], f[y1, x1], fx[..., None], fy[..., None])
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _grid(S):
    yy, xx = np.mgrid[0:S, 0:S].astype(F)
    return yy, xx


def affine_coords(mat, S):
    yy, xx = _grid(S)
    m = mat.astype(F).reshape(2, 3)
    return (m[1, 0] * xx + m[1, 1] * yy) + m[1, 2], (m[0, 0] * xx + m[0, 1] * yy) + m[0, 2]


def grid_coords(jy, jx, S):
    yy, xx = _grid(S)
    den = F(max(S - 1, 1))
    cy, cx = (yy * F(3)) / den, (xx * F(3)) / den
    y0, y1, fy = _tap(cy, 4)
    x0, x1, fx = _tap(cx, 4)
    jy, jx = jy.astype(F).reshape(4, 4), jx.astype(F).reshape(4, 4)
    dy = _lerp2(jy[y0, x0], jy[y0, x1], jy[y1, x0], jy[y1, x1], fx, fy)
    dx = _lerp2(jx[y0, x0], jx[y0, x1], jx[y1, x0], jx[y1, x1], fx, fy)
    return yy + dy, xx + dx


def gauss_field(noise, weights):
    """noise float32 [..., S, S] -> the separable Gaussian of ups_augment_field: scipy `reflect` border repeated, axis -2 first, the
    accumulator starting at 0 and adding the taps in order, float32 throughout."""
    S = noise.shape[-1]
    radius = (len(weights) - 1) // 2
    pos = np.arange(S)
    out = noise.astype(F)
    for axis in (-2, -1):
        acc = np.zeros_like(out)
        for k, w in enumerate(weights.astype(F)):
            m = (pos + k - radius) % (2 * S)
            idx = np.where(m < S, m, 2 * S - 1 - m)
            acc = acc + w * np.take(out, idx, axis=axis)
        out = acc
    return out


def gray32(img):
    f = img.astype(F)
    g = np.rint((f[..., 0] * F(0.299) + f[..., 1] * F(0.587)) + f[..., 2] * F(0.114))
    return np.repeat(np.clip(g, 0, 255).astype(np.uint8)[..., None], 3, -1)


def record_valid(rec, n_images, n_fields):
    _, D = _pkg()
    ok = 0 <= rec[D.REC_SRC] < n_images and 0 <= rec[D.REC_FLIP] <= 3 and rec[D.REC_MID] in (0, 1) and 0 <= rec[D.REC_FILTER] <= 2
    ok = ok and all(0 <= rec[D.REC_COLOR + k] <= 3 and 0 <= rec[D.REC_PIDX + k] <= 2 for k in range(3))
    ok = ok and all(rec[w] in (0, 1) for w in (D.REC_GRAY, D.REC_PERM, D.REC_HFLIP, D.REC_AFFINE)) and 0 <= rec[D.REC_WARP] <= 2
    return bool(ok and (rec[D.REC_WARP] != 2 or 0 <= rec[D.REC_FIELD] < n_fields))


def execute_image(store, rec, fields):
    """One output image float32 [S,S,3] from its int32 record; fields float32 [n_fields,2,S,S] (dx, dy), already smoothed."""
    A, D = _pkg()
    S = store.shape[1]
    if not record_valid(rec, store.shape[0], len(fields)):
        return np.full((S, S, 3), np.nan, dtype=F)
    luts = D.aug_luts()
    f32 = rec.view(F)
    u = store[rec[D.REC_SRC]]
    if rec[D.REC_FLIP] & 1:
        u = u[:, ::-1]
    if rec[D.REC_FLIP] & 2:
        u = u[::-1]
    u = luts[0][u]
    if rec[D.REC_FILTER]:
        u = (A._median3 if rec[D.REC_FILTER] == 1 else A._box3)(u)
    for k in range(3):
        kind, par = rec[D.REC_COLOR + k], [int(v) for v in rec[D.REC_CPAR + 3 * k:D.REC_CPAR + 3 * k + 3]]
        if kind == 1:
            u = rec[D.REC_BC + 64 * k:D.REC_BC + 64 * (k + 1)].view(np.uint8)[u]
        elif kind == 2:
            u = A._rgb_shift(u, par)
        elif kind == 3:
            u = A._hue_sat_val(u, *par)
    if rec[D.REC_GRAY]:
        u = gray32(u)
    if rec[D.REC_PERM]:
        u = np.ascontiguousarray(u[..., rec[D.REC_PIDX:D.REC_PIDX + 3]])
    if rec[D.REC_MID]:
        u = luts[1][u]
    if rec[D.REC_HFLIP]:
        u = np.ascontiguousarray(u[:, ::-1])
    if rec[D.REC_AFFINE]:
        u = warp32(u, *affine_coords(f32[D.REC_AMAT:D.REC_AMAT + 6], S))
    if rec[D.REC_WARP] == 1:
        u = warp32(u, *grid_coords(f32[D.REC_JY:D.REC_JY + 16], f32[D.REC_JX:D.REC_JX + 16], S))
    elif rec[D.REC_WARP] == 2:
        ys, xs = affine_coords(f32[D.REC_EMAT:D.REC_EMAT + 6], S)
        fld = fields[rec[D.REC_FIELD]]
        u = warp32(u, ys + fld[1], xs + fld[0])
    return u.astype(F) * 2.0 / 255.0 - 1.0


def execute(store, recs, noise, n_fields):
    """recs int32 [R,B,REC_WORDS] (R = 3 or 2 roles), noise float32 [>= n_fields,2,S,S] (unsmoothed) -> {"view0", "view1"[,
    "view0_target"]} float32 [B,S,S,3]."""
    _, D = _pkg()
    S = store.shape[1]
    fields = gauss_field(noise[:n_fields], D.gauss_weights()) if n_fields else np.zeros((0, 2, S, S), F)
    keys = ("view0", "view1", "view0_target")[:recs.shape[0]]
    return {k: np.stack([execute_image(store, recs[r, b], fields) for b in range(recs.shape[1])]) for r, k in enumerate(keys)}


def record_kinds(rec):
    """The record kinds present in one image's record (names of augment.py's records)."""
    _, D = _pkg()
    kinds = set()
    if rec[D.REC_FILTER]:
        kinds.add({1: "median", 2: "box"}[int(rec[D.REC_FILTER])])
    for k in range(3):
        if rec[D.REC_COLOR + k]:
            kinds.add({1: "bc", 2: "rgb", 3: "hsv"}[int(rec[D.REC_COLOR + k])])
    for w, name in ((D.REC_GRAY, "gray"), (D.REC_PERM, "perm"), (D.REC_HFLIP, "hflip"), (D.REC_AFFINE, "affine")):
        if rec[w]:
            kinds.add(name)
    if rec[D.REC_WARP]:
        kinds.add({1: "grid", 2: "elastic"}[int(rec[D.REC_WARP])])
    return kinds


ALL_KINDS = {"median", "box", "bc", "rgb", "hsv", "gray", "perm", "hflip", "affine", "grid", "elastic"}
INEXACT_KINDS = {"gray", "affine", "grid", "elastic"}       # the records whose host form runs in double precision (BLAS dot, scipy)


def levels(x):
    """float views in [-1, 1] -> their uint8 levels (every value of either path is v * 2 / 255 - 1 for an integer v)."""
    return np.rint((np.asarray(x, dtype=np.float64) + 1.0) * 127.5).astype(np.int64)


# ------------------------------------------------------------------------------------------------ datasets
def write_aug_dataset(root, n, S, singles=False, seed=0):
    """n S x S PNGs under `root` -- even rows uniform noise, odd rows 4 x 4-pixel blocks of noise -- and the csv; 3 character ids (or,
    with `singles`, one per image).  Returns the dataset config: both augmentations on, the device route on, both plan flips on."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    rows = ["character_id,relative_file_path_"]
    for i in range(n):
        if i % 2 == 0:
            img = rng.randint(0, 256, (S, S, 3), dtype=np.uint8)
        else:
            q = -(-S // 4)
            img = np.kron(rng.randint(0, 256, (q, q, 3), dtype=np.uint8), np.ones((4, 4, 1), np.uint8))[:S, :S]
        Image.fromarray(img).save(str(root / "im{}.png".format(i)))
        rows.append("{},im{}.png".format(i if singles else i * 3 // n, i))
    (root / "train.csv").write_text("\n".join(rows) + "\n")
    return {"data_root": str(root), "data_csv": str(root / "train.csv"), "data_csv_has_header": True,
            "data_csv_columns": ["character_id", "relative_file_path_"], "spatial_size": S, "data_avoid_identity": not singles,
            "data_flip_h": True, "data_flip_v": True, "batch_size": 4, "data_augment_appearance": True, "data_augment_shape": True,
            "data_on_device": True, "data_augment_on_device": True}
