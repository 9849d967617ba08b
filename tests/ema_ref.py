"""NumPy restatement of the weight-EMA kernels (csrc/ema.hip; definitions in include/upsparts_hip.h): the decay in Python floats
(IEEE fp64, one rounding per operation), the element update in np.float32 operations (one rounding each, nothing fused).

NaN results: IEEE 754 leaves the sign and payload of a NaN that an operation produces or propagates to the implementation, and an x86
host and a gfx950 device choose differently (inf - inf is 0xffc00000 on the one, 0x7fc00000 on the other).  ``canon`` maps every NaN to
0x7fc00000; the kernel tests compare canon(device bits) with canon(restated bits), i.e. bit for bit wherever the value is not a NaN and
"a NaN" where it is.  Buffers that must be UNTOUCHED (a skipped shadow, both sides after two swaps) are compared without it."""
import numpy as np

QNAN = np.uint32(0x7fc00000)


def effective_decay(decay, warmup, n):
    """The decay of the update taken with `n` earlier updates behind it (TF's num_updates rule when `warmup`)."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + float(n)) / (10.0 + float(n)))
    return d


def one_minus_decay(decay, warmup, n):
    return np.float32(1.0 - effective_decay(decay, warmup, n))


def update(shadow, weights, decay, warmup, n, skip=False):
    """One ups_ema_update of one item -> (new shadow, new count).  skip: the key's guard record has its skip flag set."""
    shadow = np.asarray(shadow, dtype=np.float32)
    if skip:
        return shadow.copy(), int(n)
    w = np.asarray(weights, dtype=np.float32)
    omd = one_minus_decay(decay, warmup, n)
    with np.errstate(all="ignore"):
        t = (shadow - w).astype(np.float32)
        u = (t * omd).astype(np.float32)
        s = (shadow - u).astype(np.float32)
    return s, int(n) + 1


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def canon(x):
    """The uint32 bits of float32 `x` with every NaN mapped to the one quiet NaN 0x7fc00000."""
    x = np.asarray(x, dtype=np.float32)
    b = bits(x).copy()
    b[np.isnan(x)] = QNAN
    return b
