"""fp64 restatements of the NHWC streaming operations of csrc/pointwise.hip for the point-wise tests, written from each operation's
definition in plain torch (no project code; `bilinear_up2` is the oracle's), and the one bound the arithmetic kernels are held to.

Backward references are `torch.autograd` on the fp64 forward (`vjp`) wherever the operation is differentiable without a tie rule;
the two hand-written ones (`maxpool2_grad`, `l1_mean_grad`) are pinned against autograd by tests/test_host_pointwise.py.

    depth_to_space   y[b, 2i+di, 2j+dj, c] = x[b, i, j, (2 di + dj) C + c]       (tf.depth_to_space(x, 2), NHWC)
    nearest2x        y[b, 2i+di, 2j+dj, :] = x[b, i, j, :]
    crop             y[b, i, j, :] = x[b, oy + i, ox + j, :],  (oy, ox) = the corner clamped into [0, h - ho] x [0, w - wo]
    maxpool2         2x2 / stride 2; the gradient goes to the FIRST maximum of the window in (0,0), (0,1), (1,0), (1,1) order
    act_mean         mean over the pixels of act(x)
    l1_mean          mean over rows and the c logical channels of |act(a) - act(b)|; gradient with respect to b
    vgg_preprocess   [-1,1] RGB (first three of ldx channels) -> BGR * 127.5 + 127.5 - mean, five zero pad channels
    pad_convert      [rows, c] -> [rows, ld] with zeros in [c, ld)
"""
import torch

from oracle.ref_model import bilinear_up2  # noqa: F401  (re-exported: the bilinear reference IS the oracle's)

VGG_BGR_MEAN = (103.939, 116.779, 123.68)
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_ELU = 0, 1, 2, 3

# unit round-off and smallest normal of the stored types
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FLOOR = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}


def vjp(fn, x, g):
    """Vector-Jacobian product of the fp64 forward `fn` at x with the output gradient g (autograd)."""
    x = x.detach().double().requires_grad_(True)
    (gx,) = torch.autograd.grad([fn(x)], [x], grad_outputs=[g.double()])
    return gx


def act(x, kind, slope=0.2):
    if kind == ACT_LRELU:
        return torch.where(x > 0, x, slope * x)
    if kind == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if kind == ACT_ELU:
        return elu(x)
    return x


def dact(x, kind, slope=0.2):
    one = torch.ones_like(x)
    if kind == ACT_LRELU:
        return torch.where(x > 0, one, slope * one)
    if kind == ACT_RELU:
        return torch.where(x > 0, one, 0 * one)
    if kind == ACT_ELU:
        return elu_grad(x)
    return one


# ----------------------------------------------------------------------------- data movement
def depth_to_space(x, C):
    """[n, h, w, >= 4C] -> [n, 2h, 2w, C] (logical channels; the callers add the pad channels)."""
    n, h, w = x.shape[:3]
    t = x[..., :4 * C].reshape(n, h, w, 2, 2, C)               # [..., di, dj, c]
    return t.permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, C)


def space_to_depth(y, C):
    """The inverse: [n, 2h, 2w, >= C] -> [n, h, w, 4C]."""
    n, h2, w2 = y.shape[:3]
    t = y[..., :C].reshape(n, h2 // 2, 2, w2 // 2, 2, C)       # [b, i, di, j, dj, c]
    return t.permute(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * C)


def pad_channels(x, ld):
    """Zeros appended to the channel axis up to width ld."""
    if ld == x.shape[-1]:
        return x
    return torch.cat([x, x.new_zeros(x.shape[:-1] + (ld - x.shape[-1],))], dim=-1)


def nearest2x(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def sum_of_four(y):
    """The transpose of nearest2x: every input pixel collects its 2x2 block."""
    n, h2, w2, c = y.shape
    return y.reshape(n, h2 // 2, 2, w2 // 2, 2, c).sum(dim=(2, 4))


def clamp_corner(h, w, ho, wo, y0, x0):
    return min(max(int(y0), 0), h - ho), min(max(int(x0), 0), w - wo)


def crop(x, y0, x0, ho, wo):
    oy, ox = clamp_corner(x.shape[1], x.shape[2], ho, wo, y0, x0)
    return x[:, oy:oy + ho, ox:ox + wo, :]


def crop_inverse(g, h, w, y0, x0):
    """g placed at the (clamped) corner of an all-zero [n, h, w, c] tensor."""
    n, ho, wo, c = g.shape
    oy, ox = clamp_corner(h, w, ho, wo, y0, x0)
    out = g.new_zeros((n, h, w, c))
    out[:, oy:oy + ho, ox:ox + wo, :] = g
    return out


def pad_convert(x, ld):
    return pad_channels(x.reshape(-1, x.shape[-1]), ld)


# ----------------------------------------------------------------------------- 2x2 max pool with the stated tie rule
def _windows(x):
    """[n, h, w, c] -> [n, h/2, w/2, c, 4]: the window in (0,0), (0,1), (1,0), (1,1) order."""
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], dim=-1)


def maxpool2(x):
    return _windows(x).amax(dim=-1)


def maxpool2_grad(x, g):
    """g routed to the first maximum of every window in row-major window order; zero elsewhere (+0.0 == -0.0 compare equal)."""
    wv = _windows(x)
    hit = wv == wv.amax(dim=-1, keepdim=True)
    first = hit & (hit.long().cumsum(dim=-1) == 1)
    r = torch.where(first, g.unsqueeze(-1).expand(first.shape), torch.zeros((), dtype=g.dtype, device=g.device))      # (+0.0 elsewhere)
    out = torch.zeros(x.shape, dtype=g.dtype, device=g.device)
    out[:, 0::2, 0::2], out[:, 0::2, 1::2], out[:, 1::2, 0::2], out[:, 1::2, 1::2] = r.unbind(dim=-1)
    return out


def tied_windows(x):
    """Number of (window, channel) pairs whose maximum is attained more than once."""
    wv = _windows(x)
    return int(((wv == wv.amax(dim=-1, keepdim=True)).sum(dim=-1) > 1).sum())


# ----------------------------------------------------------------------------- arithmetic
def elu(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def elu_grad(x):
    return torch.where(x > 0, torch.ones_like(x), torch.exp(torch.clamp(x, max=0)))


def act_mean(x, kind, slope=0.2):
    return act(x, kind, slope).mean(dim=(1, 2), keepdim=True)


def l1_mean(a, b, c, kind):
    return (act(a[..., :c], kind) - act(b[..., :c], kind)).abs().mean()


def l1_mean_grad(a, b, c, kind, scale=1.0):
    """d (scale * l1_mean) / d b over the physical width of b: -scale / (rows c) sign(act(a) - act(b)) act'(b), zero in the pad."""
    rows = b.numel() // b.shape[-1]
    d = act(a[..., :c], kind) - act(b[..., :c], kind)
    return pad_channels(-scale / (rows * c) * torch.sign(d) * dact(b[..., :c], kind), b.shape[-1])


def vgg_preprocess(x):
    """[..., ldx >= 3] in [-1, 1], RGB -> [..., 8]: BGR * 255 scale minus the ImageNet mean, five zero channels."""
    mean = torch.tensor(VGG_BGR_MEAN, dtype=x.dtype, device=x.device)
    return pad_channels(torch.flip((x[..., :3] + 1.0) * 127.5, dims=[-1]) - mean, 8)


# ----------------------------------------------------------------------------- the bound of the arithmetic kernels
def rounds_once_excess(got, ref, S, out_dtype, k):
    """max over elements of |got - ref| / (2 u_out |ref| + k 2^-23 S + floor); <= 1 passes.  NaN anywhere in `got` gives inf."""
    got, ref, S = got.double(), ref.double(), (S.double() if torch.is_tensor(S) else torch.full_like(ref.double(), float(S)))
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    bound = 2.0 * U_OUT[out_dtype] * ref.abs() + k * 2.0 ** -23 * S.abs() + FLOOR[out_dtype]
    ratio = (got - ref).abs() / bound
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_rounds_once(got, ref, S, out_dtype, k, what=""):
    """An operation that rounds once into `out_dtype` after k fp32 operations on terms of size S:
        |got - ref| <= 2 u_out |ref| + k 2^-23 S + floor      for EVERY element.
    u_out: unit round-off of the stored type (the factor 2 covers the double rounding fp32 -> 16 bit); S: the reference operation
    applied to |inputs| (cancellation is judged on the size of the terms); floor: the smallest normal of the stored type."""
    x = rounds_once_excess(got, ref, S, out_dtype, k)
    assert x <= 1.0, "{}: |got - ref| exceeds 2 u |ref| + {} * 2^-23 S + floor by {:.3g}x ({})".format(what, k, x, out_dtype)
    return x
