"""fp64 / integer restatements of the trainer-side kernels (parity_ledger.md, section 8): the Philox noise, Adam, the critic head,
the full-covariance latent and the thin-plate-spline warp -- csrc/latent_adam.hip, the head of csrc/critic.hip and
tps_warp_kernel of csrc/pointwise.hip.  Plain restatements of the operation, none of them written from the kernels' code paths;
tests/test_host_trainer_kernels.py holds each to an independent statement (Random123's known answers, oracle.np_ops, oracle.tps,
a finite difference) without a GPU, tests/test_gpu_trainer_kernels.py holds the kernels to them.

The cases of the TPS and critic-head tests are built here as well, so that the CPU test can assert what they rest on (masked
share, border coverage, logit span) on the very inputs the GPU test launches with."""
import math

import numpy as np
import torch

from oracle import ref_model as R
from oracle import tps as OT

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------- Philox4x32-10 (Salmon et al., SC 2011) + Box-Muller
def philox4x32_10(ctr4, key2):
    """Four 32-bit counter words (ints or equal-length integer arrays) and a two-word key -> the four output words (uint64 arrays
    holding 32-bit values; products of two 32-bit words fit uint64)."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & np.uint64(M32) for x in ctr4]
    k0, k1 = int(key2[0]) & M32, int(key2[1]) & M32
    m0, m1, lo, sh = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def randn_ref(n, seed, offset):
    """ups_randn's stream in fp64: group g = values [4g, 4g + 4); counter = (lo32, hi32, 0, 0) of offset + g (mod 2^64), key =
    (lo32, hi32) of seed; u = ((word >> 8) + 0.5) / 2^24; words (0, 1) and (2, 3) -> Box-Muller (r cos, r sin)."""
    groups = (n + 3) // 4
    ctr = [(int(offset) + g) & M64 for g in range(groups)]
    zero = np.zeros(groups, dtype=np.uint64)
    w = philox4x32_10((np.array([c & M32 for c in ctr], dtype=np.uint64), np.array([c >> 32 for c in ctr], dtype=np.uint64), zero, zero),
                      (int(seed) & M32, (int(seed) & M64) >> 32))
    u = [((x >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0 for x in w]
    z = np.empty((groups, 4), dtype=np.float64)
    for h in range(2):
        rad = np.sqrt(-2.0 * np.log(u[2 * h]))
        z[:, 2 * h] = rad * np.cos(2.0 * math.pi * u[2 * h + 1])
        z[:, 2 * h + 1] = rad * np.sin(2.0 * math.pi * u[2 * h + 1])
    return z.reshape(-1)[:n]


# ----------------------------------------------------------------------------- Adam (tf.train.AdamOptimizer after its lr_t)
def adam_ref(p, g, m, v, lr_t, b1, b2, eps, grad_scale=1.0):
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    g = g * grad_scale
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def lr_t_of(lr, b1, b2, t):
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


# ----------------------------------------------------------------------------- critic head
HEAD_WEIGHTINGS = ((1.0, 0.0), (0.0, 1.0), (0.7, -2.5))      # (d loss, d mean joint logit): those of test_gpu_kernels.test_critic_head
HEAD_JUNK = 3.0e4                                            # the padding channels K..ld: large, finite in bf16


class HeadRef(object):
    pass


def critic_head_ref(hp, ha, B, K):
    """hp, ha [2B, ld] (any float dtype: taken as the numbers they hold).  fp64 logits over channels [0, K), rows [0, B) joint and
    [B, 2B) marginal; loss = (mean softplus(-joint) + mean softplus(marg)) / 2, accuracy = (#joint > 0 + #marg < 0) / 2B (a zero
    logit is wrong on both sides), mim = mean joint.  grads(wl, wm) = d (wl loss + wm mim) / d (hp, ha) by autograd on the full
    [2B, ld] tensors: channels K..ld get exact zeros."""
    r = HeadRef()
    hpo = hp.detach().double().cpu().reshape(2 * B, -1).requires_grad_(True)
    hao = ha.detach().double().cpu().reshape(2 * B, -1).requires_grad_(True)
    logits = (hpo[:, :K] * hao[:, :K]).sum(dim=1)
    joint, marg = logits[:B], logits[B:]
    loss = 0.5 * ((-torch.nn.functional.logsigmoid(joint)).mean() + (-torch.nn.functional.logsigmoid(-marg)).mean())
    mim = joint.mean()
    r.logits, r.loss, r.mim = logits.detach(), float(loss.detach()), float(mim.detach())
    r.acc = float(((joint > 0).sum() + (marg < 0).sum()).double() / (2 * B))
    r.grads = lambda wl, wm: tuple(t.detach() for t in torch.autograd.grad(wl * loss + wm * mim, [hpo, hao], retain_graph=True))
    return r


def head_inputs(dtype, B, K, ld, seed, scale=0.2, zero_rows=()):
    """(hp, ha) [2B, ld] of `dtype` on the CPU: N(0, scale^2) in channels [0, K), HEAD_JUNK of alternating sign in [K, ld); rows
    `zero_rows` of hp are zero (logit exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        t = torch.empty(2 * B, ld)
        t[:, :K] = torch.randn(2 * B, K, generator=g) * scale            # (the same draw whatever ld)
        t[:, K:] = HEAD_JUNK * (1.0 - 2.0 * (torch.arange(ld - K) % 2).float())
        out.append(t)
    for r in zero_rows:
        out[0][r, :K] = 0.0
    return tuple(t.to(dtype) for t in out)


def device_view(t, dev, lead=0):
    """`t` on the device as a contiguous view that starts `lead` elements into a flat buffer (lead = 0: a plain copy).  lead = 4 in a
    2-byte type: 8 bytes off the allocation's 16-byte boundary."""
    if not lead:
        return t.to(dev)
    flat = torch.zeros(t.numel() + 2 * lead, dtype=t.dtype, device=dev)
    view = flat[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    return view


SATURATED = dict(dtype=torch.bfloat16, B=40, K=512, ld=512, seed=401, scale=2.1, zero_rows=(0, 7, 40, 79))


# ----------------------------------------------------------------------------- full-covariance latent
LEVELS = [1.0, 0.7, 0.4, 1.3, 0.0, 1.0, 0.55, 0.9, 1.0, 0.25, 2.0, 0.8]         # MAXS = 12 noise levels, not all 1, one 0


def latent_inputs(Z, B, S, seed):
    g = torch.Generator().manual_seed(seed)
    params = torch.randn(B, Z + Z * (Z + 1) // 2, generator=g) * 0.3
    return params, torch.randn(S, B, Z, generator=g), torch.randn(S, B, Z, generator=g)


def latent_ref(params, eps, levels, g_samples, w_kl):
    """R.FullLatent on fp64 copies: samples [S, B, Z], per-row KL [B, Z] (kl = rows.sum(1).mean(), N:1196-1208) and the gradient of
    sum(samples * g_samples) + w_kl * kl w.r.t. params."""
    S, B, Z = eps.shape
    po = params.detach().double().cpu().requires_grad_(True)
    d = R.FullLatent(po, Z)
    samples = torch.stack([d.sample(eps[s].double().cpu(), noise_level=levels[s]).reshape(B, Z) for s in range(S)])
    kl_rows = 0.5 * ((d.L ** 2).sum(dim=2) - 1.0 + d.mean ** 2 - 2.0 * d.log_diag)
    kl = kl_rows.sum(dim=1).mean()
    (gp,) = torch.autograd.grad((samples * g_samples.double().cpu()).sum() + w_kl * kl, [po])
    return samples.detach(), kl_rows.detach(), gp


# ----------------------------------------------------------------------------- thin-plate-spline warp
TPS_EDGE = 1.0e-3          # |px| or |px - (size - 1)| below this: the clamped-corner weights collapse there, fp32 and fp64 may floor apart
TPS_MASK_CAP = 0.02
TPS_SHAPES = [(2, 24, 40, 3, 9), (1, 40, 24, 1, 1), (2, 17, 19, 8, 32), (1, 1, 33, 3, 9), (1, 33, 1, 3, 9)]     # n, h, w, c, K
TPS_KINDS = ("affine", "spline")


def tps_warp_ref(img, T, coord):
    """img [n, h, w, c], T [n, 2, K + 3], coord [n, K, 2] -> (warped image, px, py) in fp64; px, py [n, h, w] are the source pixel
    coordinates (x_s + 1) * w / 2, (y_s + 1) * h / 2 the bilinear form of oracle.tps.interpolate floors and clamps."""
    img, T, coord = img.double().cpu(), T.double().cpu(), coord.double().cpu()
    n, h, w, c = img.shape
    x_s, y_s = OT.sample_positions(T, coord, h, w)
    return OT.interpolate(img, x_s, y_s), (x_s + 1.0) * w / 2.0, (y_s + 1.0) * h / 2.0


def tps_image(n, h, w, c):
    """Distinct content per image, row, column and channel (incommensurate frequencies; values in about [-2.5, 2.5])."""
    i = torch.arange(n, dtype=torch.float64).view(n, 1, 1, 1)
    y = torch.arange(h, dtype=torch.float64).view(1, h, 1, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, w, 1)
    k = torch.arange(c, dtype=torch.float64).view(1, 1, 1, c)
    return (torch.sin(0.37 * y + 0.9 * k + 1.3 * i) + torch.cos(0.23 * x - 0.5 * k) + 0.5 * torch.sin(0.11 * x * (k + 1.0) + 0.07 * y)).float()


def tps_control_points(n, K, g):
    """K jittered control points per image in about [-0.8, 0.8]^2: a ceil(sqrt(K))-wide lattice (distinct points: the TPS system is
    regular), each moved by up to a quarter of the spacing."""
    side = int(math.ceil(math.sqrt(K)))
    lat = torch.linspace(-0.6, 0.6, side) if side > 1 else torch.zeros(1)
    pts = torch.stack(torch.meshgrid(lat, lat, indexing="xy"), dim=-1).reshape(-1, 2)[:K]
    step = 1.2 / max(side - 1, 1)
    return pts.view(1, K, 2) + (torch.rand(n, K, 2, generator=g) - 0.5) * 0.5 * step


def tps_case(shape, kind):
    """(img, T, coord) in float32, as the kernel takes them.
    affine: zero spline weights; x_s = t + 1.3 x + 0.5 y, y_s = t + 0.5 x + 1.3 y with t = +0.4 for even images, -0.4 for odd ones:
            scale 1.3 and the shifts reach past all four borders on two images, the 0.5 cross terms make a single image (and a
            single row or column, where one of x, y is pinned to -1) do so on its own.
    spline: T from oracle.tps.solve_system on jittered control points and random target offsets (K = 1: see below)."""
    n, h, w, c, K = shape
    g = torch.Generator().manual_seed(1000 * TPS_SHAPES.index(shape) + 31)
    coord = tps_control_points(n, K, g).double()
    if kind == "affine":
        T = torch.zeros(n, 2, K + 3, dtype=torch.float64)
        T[:, 0, 0] = T[:, 1, 0] = 0.4 * (1.0 - 2.0 * (torch.arange(n) % 2).double())
        T[:, 0, 1], T[:, 0, 2] = 1.3, 0.5
        T[:, 1, 1], T[:, 1, 2] = 0.5, 1.3
    elif K >= 3:
        vector = (torch.rand(n, K, 2, generator=g).double() - 0.5) * 0.3
        T = OT.solve_system(coord, vector)
    else:                   # (fewer than three control points: the TPS system is singular; a near-identity map with random spline weights)
        T = (torch.rand(n, 2, K + 3, generator=g).double() - 0.5) * 0.2
        T[:, 0, 1] += 1.0
        T[:, 1, 2] += 1.0
    return tps_image(n, h, w, c), T.float(), coord.float()


def tps_edge_mask(px, py, h, w):
    """True where the comparison holds: away from the four lines on which the bilinear form is discontinuous."""
    near = lambda p, size: ((p.abs() < TPS_EDGE) | ((p - (size - 1)).abs() < TPS_EDGE))
    return ~(near(px, w) | near(py, h))


def tps_border_counts(px, py, h, w):
    """Output pixels whose source lies beyond the left, right, top, bottom border."""
    return {"left": int((px < 0).sum()), "right": int((px > w - 1).sum()), "top": int((py < 0).sum()), "bottom": int((py > h - 1).sum())}
