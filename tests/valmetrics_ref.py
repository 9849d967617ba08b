"""Shared by test_host_valmetrics.py and test_gpu_valmetrics.py: the NumPy float64 restatement of ups_image_metrics and ups_part_usage
(csrc/valmetrics.hip), of evalutil.reconstruction_from_sums / usage_from_counts, the derived tolerances, and a small csv dataset of PNG
views without label images.  Nothing here imports the package: the definitions are written out a second time."""
import numpy as np

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    """The 11 normalised float64 weights of the Gaussian window (sigma 1.5, Wang et al. 2004)."""
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    w = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def unit(v):
    """Source values in [-1, 1] -> float64 in [0, 1], clamped."""
    return np.clip((np.asarray(v).astype(np.float64) + 1.0) / 2.0, 0.0, 1.0)


def filter_valid(x, w):
    """x [..,H,W] float64 -> [..,H-10,W-10]: the separable window along W, then along H, valid region only."""
    H, W = x.shape[-2:]
    h = sum(w[k] * x[..., :, k:k + W - WIN + 1] for k in range(WIN))
    return sum(w[k] * h[..., k:k + H - WIN + 1, :] for k in range(WIN))


def ssim_map(x, y, w):
    """x, y [..,H,W] float64 in [0, 1] -> the SSIM map [..,H-10,W-10] (no unbiased correction)."""
    mx, my = filter_valid(x, w), filter_valid(y, w)
    vx = filter_valid(x * x, w) - mx * mx
    vy = filter_valid(y * y, w) - my * my
    cxy = filter_valid(x * y, w) - mx * my
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def image_metrics(a, b, w=None):
    """a, b [N,H,W,>=3] (float32 values; a bf16 operand is given as its float32 widening) -> float64 [N,3] = (sse, sae, ssim_sum)."""
    w = window() if w is None else np.asarray(w, dtype=np.float64)
    x = unit(np.asarray(a)[..., :3]).transpose(0, 3, 1, 2)
    y = unit(np.asarray(b)[..., :3]).transpose(0, 3, 1, 2)
    d = x - y
    return np.stack([(d * d).sum(axis=(1, 2, 3)), np.abs(d).sum(axis=(1, 2, 3)), ssim_map(x, y, w).sum(axis=(1, 2, 3))], axis=1)


def part_usage(soft, pred, P):
    """soft [N,HW,P] float32, pred [N,HW] integers -> (counts [N,P] int32, invalid, sharp float64 [N,2], terms [N,2]): sharp =
    (sum of max_p soft, sum of -sum_p s ln s with 0 ln 0 = 0) and terms = the sums of the absolute values of what was added (the scale
    of the tolerance)."""
    soft = np.asarray(soft)
    N = soft.shape[0]
    s = soft.reshape(N, -1, P).astype(np.float64)
    pred = np.asarray(pred).reshape(N, -1)
    counts, invalid = np.zeros((N, P), dtype=np.int32), 0
    for i in range(N):
        for v in pred[i].tolist():
            if 0 <= v < P:
                counts[i, v] += 1
            else:
                invalid += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(s > 0, -s * np.log(s), 0.0)
    mx = s.max(axis=2)
    sharp = np.stack([mx.sum(axis=1), e.sum(axis=(1, 2))], axis=1)
    terms = np.stack([np.abs(mx).sum(axis=1), np.abs(e).sum(axis=(1, 2))], axis=1)
    return counts, invalid, sharp, terms


def reconstruction_from_sums(rows, H, W):
    rows = np.asarray(rows, dtype=np.float64)
    mse, l1, ssim = [], [], []
    for sse, sae, ss in rows:
        mse.append(sse / (3 * H * W))
        l1.append(sae / (3 * H * W))
        ssim.append(ss / (3 * (H - 10) * (W - 10)))
    psnr = [10.0 * np.log10(1.0 / max(m, 1e-10)) for m in mse]
    return {"mse": float(np.mean(mse)), "l1": float(np.mean(l1)), "psnr": float(np.mean(psnr)), "ssim": float(np.mean(ssim))}


def usage_from_counts(counts, sharp, HW, min_area):
    counts, sharp = np.asarray(counts, dtype=np.int64), np.asarray(sharp, dtype=np.float64)
    n = counts.shape[0]
    area = [int(counts[:, p].sum()) / (n * HW) for p in range(counts.shape[1])]
    return {"part_area": area, "parts_active": sum(1 for a in area if a >= min_area),
            "confidence": float(sharp[:, 0].sum() / (n * HW)), "entropy": float(sharp[:, 1].sum() / (n * HW))}


# ---- tolerances (derived, not tuned)
def sum_rtol(n):
    """A float64 sum of n non-negative terms in another order: relative 2 n 2^-53 (each of the two orders is within n 2^-53)."""
    return 2.0 * n * 2.0 ** -53


SSIM_ATOL = 1e-10       # per image, on the mean: window sums round by a few 1e-15, divided by C2 = 9e-4 -> below 1e-11


def sharp_rtol(n):
    """ups_part_usage's sums of n terms, relative to the sum of |terms|: 2 n 2^-52 (reordering, and one rounding of ln per term)."""
    return 2.0 * n * 2.0 ** -52


# ---- inputs
def bf16_round(x):
    """float32 array -> the nearest bfloat16 values (ties to even), as float32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def image_pair(rng, N, H, W, lda=3, ldb=3):
    """Two image batches [N,H,W,ld] float32 in about [-1.3, 1.3] with values below -1, above 1 and exactly +-1 planted; b is a
    blurred-noise relative of a so that the SSIM is neither 0 nor 1.  Channels >= 3 hold large garbage that must not be read."""
    a = rng.uniform(-1.3, 1.3, (N, H, W, lda)).astype(np.float32)
    b = np.empty((N, H, W, ldb), dtype=np.float32)
    b[..., :3] = 0.7 * a[..., :3] + rng.uniform(-0.4, 0.4, (N, H, W, 3)).astype(np.float32)
    a[..., 3:] = 1.0e4
    b[..., 3:] = -1.0e4
    flat = a[..., :3].reshape(N, -1)
    k = flat.shape[1]
    planted = np.array([1.0, -1.0, 1.5, -1.5, 1.0, -1.0], dtype=np.float32)
    pos = rng.permutation(k)[:len(planted)]
    for i in range(N):
        av = a[i, ..., :3].reshape(-1)
        bv = b[i, ..., :3].reshape(-1)
        av[pos] = planted
        bv[pos[::-1]] = planted
        a[i, ..., :3] = av.reshape(H, W, 3)
        b[i, ..., :3] = bv.reshape(H, W, 3)
    return a, b


def soft_maps(rng, N, HW, P):
    """soft [N,HW,P] float32 rows that sum to about 1, with exact zeros and one-hot pixels; pred [N,HW] int64 with -1 and P planted
    (when HW allows: the first pixels keep their arg-max so that tiny cases stay meaningful)."""
    s = rng.gamma(0.5, 1.0, (N, HW, P)).astype(np.float64) + 1e-3
    s[rng.uniform(size=s.shape) < 0.2] = 0.0
    s[..., 0] += (s.sum(axis=2) == 0)
    s = (s / s.sum(axis=2, keepdims=True)).astype(np.float32)
    hot = rng.uniform(size=(N, HW)) < 0.25
    onehot = np.eye(P, dtype=np.float32)[rng.randint(0, P, (N, HW))]
    s[hot] = onehot[hot]
    pred = s.argmax(axis=2).astype(np.int64)
    if HW >= 4:
        pred[:, HW // 2] = -1
        pred[:, HW - 1] = P
    return s, pred


def write_view_dataset(root, n=5, S=16, seed=0, name="val", ids=None):
    """n PNG views under `root` with <name>.csv (header, no label column); ids: the character_id per row (default i // 2)."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    rows = ["character_id,relative_file_path_"]
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (S + 4, S + 2, 3), dtype=np.uint8)).save(str(root / "{}_im{}.png".format(name, i)))
        rows.append("{},{}_im{}.png".format(i // 2 if ids is None else ids[i], name, i))
    (root / (name + ".csv")).write_text("\n".join(rows) + "\n")
    return {"dataset": "eddata.stochastic_pair.StochasticPairs", "data_root": str(root), "data_csv": str(root / (name + ".csv")),
            "data_csv_has_header": True, "data_csv_columns": ["character_id", "relative_file_path_"], "data_avoid_identity": False}
