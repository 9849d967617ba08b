"""NumPy float64 restatement of the guarded optimizer step's kernels (csrc/stepguard.hip; the definitions: include/upsparts_hip.h,
"guarded optimizer step"), with equal bits: the per-chunk partial sums of squares and their fixed order, the non-finite count, the clip
scale, the record's transitions and the guarded state update's decision.  Imports neither torch nor the package."""
import numpy as np

CHUNK, SLOTS, ROWS, LANES = 8192, 1024, 8, 256       # ups_grad_guard_chunk(); slots of a chunk; elements per slot; the tree's width
RECORD_BYTES = 64


def tree256(f):
    """`for d = 128, 64, .., 1: f[i] += f[i + d] (i < d)` over the last axis (256 values) -> f[0]."""
    f = np.array(f, dtype=np.float64, copy=True)
    d = LANES // 2
    while d >= 1:
        f[..., :d] = f[..., :d] + f[..., d:2 * d]
        d //= 2
    return f[..., 0]


def chunk_partials(x):
    """One fp64 partial per chunk of CHUNK elements of the flat float32 array x.  Absent elements of the last chunk count as +0.0 (the
    kernel does not add them: x + 0.0 has x's bits, the sums start from +0.0 and squares are never -0.0)."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    nc = (x.size + CHUNK - 1) // CHUNK
    if nc == 0:
        return np.zeros(0, np.float64)
    pad = np.zeros(nc * CHUNK, np.float32)
    pad[:x.size] = x
    with np.errstate(all="ignore"):
        d = pad.astype(np.float64).reshape(nc, ROWS, SLOTS)
        sq = d * d                                   # exact: 24-bit significands
        s = np.zeros((nc, SLOTS), np.float64)
        for r in range(ROWS):                        # a slot takes its elements in ascending order
            s = s + sq[:, r]
        fold = (s[:, 0:256] + s[:, 256:512]) + (s[:, 512:768] + s[:, 768:1024])
        return tree256(fold)


def sum_partials(partials):
    """The finalize launch: t[i] = partial[i] + partial[i + 256] + ... from 0.0, then the tree."""
    p = np.asarray(partials, np.float64)
    rows = max(1, (p.size + LANES - 1) // LANES)
    pad = np.zeros(rows * LANES, np.float64)
    pad[:p.size] = p
    with np.errstate(all="ignore"):
        t = np.zeros(LANES, np.float64)
        for r in pad.reshape(rows, LANES):
            t = t + r
        return np.float64(tree256(t))


def sumsq(x):
    return sum_partials(chunk_partials(x))


def nonfinite_count(x):
    """Elements whose exponent bits are all ones: NaN, +inf, -inf (denormals and zeros are finite)."""
    bits = np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)
    return int(np.count_nonzero((bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)))


def clip_scale(norm, clip_norm):
    """float32(clip_norm / max(norm, clip_norm)) when clip_norm > 0 (tf.clip_by_global_norm), else 1; a NaN norm gives NaN."""
    if not clip_norm > 0:
        return np.float32(1.0)
    norm, clip_norm = np.float64(norm), np.float64(clip_norm)
    den = norm if (norm > clip_norm or norm != norm) else clip_norm
    with np.errstate(all="ignore"):
        return np.float32(clip_norm / den)


def new_record():
    return {"sumsq": np.float64(0), "norm": np.float64(0), "scale": np.float32(0), "skip": 0, "nonfinite": 0, "skipped": 0, "clipped": 0,
            "consecutive": 0}


def grad_guard(x, grad_scale, clip_norm, skip_nonfinite, rec=None):
    """ups_grad_guard on the record `rec` (a dict of ``new_record``; a new one when None) -> the updated record."""
    rec = dict(new_record() if rec is None else rec)
    with np.errstate(all="ignore"):
        ss = sumsq(x)
        norm = np.float64(np.sqrt(ss) * np.float64(grad_scale))
    nf = nonfinite_count(x)
    scale = clip_scale(norm, clip_norm)
    skip = int(bool(skip_nonfinite) and nf > 0)
    rec.update(sumsq=ss, norm=norm, scale=scale, skip=skip, nonfinite=nf)
    if skip:
        rec["skipped"] += 1
        rec["consecutive"] += 1
    else:
        rec["consecutive"] = 0
        if scale < 1:
            rec["clipped"] += 1
    return rec


def state_guard(stats, counters):
    """ups_state_update_guarded's decision: (keep the old state?, (total, consecutive) afterwards)."""
    bad = nonfinite_count(stats) > 0
    total, consecutive = counters
    return bad, ((total + 1, consecutive + 1) if bad else (total, 0))


def same_bits(a, b):
    """Equal bit patterns, or both NaN (a NaN's payload and sign are not part of the definitions)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype:
        return False
    if a != a and b != b:
        return True
    return a.tobytes() == b.tobytes()
