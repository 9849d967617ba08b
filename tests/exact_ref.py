"""Exact (tolerance-free) reference of the convolution kernels on lattice inputs.  CPU only, no GPU import.

When every operand is a small integer (or a small dyadic number), every product and every partial sum of a convolution is
exactly representable in fp32 -- the MFMA accumulator's type -- so the result does not depend on the order of summation, on split-K
slabs, on FMA contraction or on the tile shape.  The only rounding left is the one RNE conversion to the stored type, which
`.to(torch.bfloat16 / float16 / float32)` reproduces bit for bit.  `headroom` is the condition of that argument: the largest
sum of |products| of a case, in units of the smallest LSB among them, must stay below 2**24.

Leaky ReLU runs at slope 0.25 here (`ops.ConvLayer(..., slope=0.25)`): act(x), act'(x) and the inverted residual r / slope are
then exact; the shipped 0.2 is not dyadic.  CoordConv cases use square maps of 9 / 17 / 33 / 65 pixels: the coordinates
i / (H - 1) * 2 - 1 are dyadic only when H - 1 is a power of two.

The fp8 paths have a lattice of their own at the end of this file (FP8_CASES): integers in [-7, 7] with a 7 wherever a scale is
derived from a maximum, so that every per-row weight scale and every delayed tensor scale is a power of two and every quantisation
lossless; `fp8_headroom` is the same condition stated in the quantised domain.
"""
import zlib

import torch

SLOPE = 0.25
LIMIT = 2 ** 24
TORCH_T = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# ---------------------------------------------------------------------------------------------------------------------------------
# lattice generators
def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7fffffff)


def ints(g, shape, amp, density=1.0):
    """Integers uniform in [-amp, amp] as float64; with density < 1 an entry is kept with that probability, else zero."""
    t = torch.randint(-amp, amp + 1, tuple(shape), generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density).double()
    return t


def activations(g, shape, amp=4):
    return ints(g, shape, amp)


def weights(g, shape, amp=1, density=1.0):
    return ints(g, shape, amp, density)


def biases(g, n, amp=3):
    return ints(g, (n,), amp)


def out_grads(g, shape, amp=4):
    return ints(g, shape, amp)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plain reference (float64: exact on these values)
def lrelu(x, slope=SLOPE):
    return torch.where(x > 0, x, x * slope)


def act_fn(x, act, slope=SLOPE):
    if act == "leaky_relu":
        return lrelu(x, slope)
    if act == "relu":
        # as a factor, the way the kernels apply it (max(x, 0 * x) on load, act'(x) * sum in the input gradient): a negative value
        # becomes -0, and so does the gradient behind it -- the sign of a zero is part of the bits compared
        return x * (x > 0).to(x.dtype)
    assert act is None
    return x


def act_inverse(a, slope=SLOPE):
    """The pre-activation value a stored leaky-ReLU tensor stands for."""
    return torch.where(a > 0, a, a / slope)


def same_pad(size, k, stride):
    out = -(-size // stride)
    pad = max((out - 1) * stride + k - size, 0)
    return out, pad // 2, pad - pad // 2


def conv_same(x, V, b, stride=1):
    """tf.nn.conv2d(x, V, [1, s, s, 1], 'SAME') + b, NHWC / HWIO, one matrix product per tap."""
    n, h, w, ci = x.shape
    kh, kw, civ, co = V.shape
    assert civ == ci
    ho, pt, pb = same_pad(h, kh, stride)
    wo, pl, pr = same_pad(w, kw, stride)
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    y = None
    for r in range(kh):
        for s in range(kw):
            tap = xp[:, r:r + (ho - 1) * stride + 1:stride, s:s + (wo - 1) * stride + 1:stride, :]
            t = tap.reshape(-1, ci) @ V[r, s]
            y = t if y is None else y + t
    y = y.view(n, ho, wo, co)
    return y if b is None else y + b


def add_coordinates(x):
    from oracle.ref_model import Scope
    return Scope.add_coordinates(x)


def staged(x_pre, act, coords, slope=SLOPE):
    """What meets the weights: act(x) with the two CoordConv channels appended."""
    xa = act_fn(x_pre, act, slope)
    return add_coordinates(xa) if coords else xa


def conv_block(x_stored, V, b, g=None, stride=1, coords=False, act=None, res_self=False, in_post=False, out_act=False,
               slope=SLOPE):
    """One ConvLayer as ops.conv runs it, in float64 with autograd.
    x_stored: the input tensor as stored (in_post: it holds act(x)); pre = conv(act(x) (+ coords), V) + b (+ x); the stored output is
    out_act(pre).  g: gradient w.r.t. `pre`; gradients are w.r.t. the pre-activation x, V (CoordConv rows included) and b.
    Returns a dict of float64 tensors: y, and with g also gx, gV, gb."""
    x_pre = act_inverse(x_stored, slope) if in_post else x_stored
    x_pre = x_pre.detach().clone().requires_grad_(g is not None)
    Vr = V.detach().clone().requires_grad_(g is not None)
    br = b.detach().clone().requires_grad_(g is not None)
    pre = conv_same(staged(x_pre, act, coords, slope), Vr, br, stride)
    if res_self:
        pre = pre + x_pre
    out = {"y": (lrelu(pre, slope) if out_act else pre).detach()}
    if g is not None:
        out["gx"], out["gV"], out["gb"] = torch.autograd.grad([pre], [x_pre, Vr, br], grad_outputs=[g])
    return out


def rounded(t, dtype):
    """The one rounding of the kernels: float64 (exact) -> the stored type, RNE."""
    return t.to(TORCH_T[dtype] if isinstance(dtype, str) else dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# headroom
def lsb(t, hi=0):
    """The largest power of two <= 2**hi that divides every entry of t."""
    t = t.detach().double()
    for e in range(-hi, 20):
        s = t * (2.0 ** e)
        if torch.equal(s, s.round()):
            return 2.0 ** -e
    raise ValueError("not a dyadic lattice")


def headroom(x_stored, V, b, g=None, stride=1, coords=False, act=None, res_self=False, in_post=False, out_act=False,
             slope=SLOPE):
    """The largest sum of |products| over all outputs of conv_block -- forward, and with g the input, weight and bias gradient
    sums -- in units of the smallest LSB among the products (the stored activation and act' each add the slope's bits).
    Below 2**24 every partial sum of every order of accumulation is exact in fp32."""
    x_pre = act_inverse(x_stored, slope) if in_post else x_stored
    xa = staged(x_pre, act, coords, slope)
    A = xa.abs().requires_grad_(g is not None)
    W = V.abs().clone().requires_grad_(g is not None)
    B = b.abs().clone().requires_grad_(g is not None)
    Y = conv_same(A, W, B, stride)
    top = Y.detach()
    if res_self:
        top = top + x_pre.abs()
    unit = min(lsb(xa) * lsb(V), lsb(b), lsb(x_pre) if res_self else 1.0) * (slope if out_act else 1.0)
    worst = float(top.max()) / unit
    if g is not None:
        gA, gW, gB = torch.autograd.grad([Y], [A, W, B], grad_outputs=[g.abs()])
        gA = gA[..., :x_pre.shape[-1]]
        if res_self:
            gA = gA + g.abs()
        worst = max(worst,
                    float(gA.max()) / (lsb(g) * lsb(V) * (slope if act == "leaky_relu" else 1.0)),
                    float(gW.max()) / (lsb(xa) * lsb(g)),
                    float(gB.max()) / lsb(g))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table: one case per kernel instance the dispatch can select, at the smallest shape that still selects it
class Case(object):
    def __init__(self, name, family, n, h, w, cin, cout, k=3, stride=1, coords=False, act=None, res_self=False, in_post=False,
                 out_act=False, dtypes=("bf16",), xamp=4, wamp=1, wdens=1.0, gamp=4, extra=None, instance=""):
        self.name, self.family = name, family
        self.n, self.h, self.w, self.cin, self.cout, self.k, self.stride = n, h, w, cin, cout, k, stride
        self.coords, self.act, self.res_self, self.in_post, self.out_act = coords, act, res_self, in_post, out_act
        self.dtypes, self.xamp, self.wamp, self.wdens, self.gamp = dtypes, xamp, wamp, wdens, gamp
        self.extra = extra or {}
        self.instance = instance

    def kw(self):
        return dict(stride=self.stride, coords=self.coords, act=self.act, res_self=self.res_self, in_post=self.in_post,
                    out_act=self.out_act)

    def __repr__(self):
        return self.name


LR = "leaky_relu"
ALL = ("bf16", "f16", "fp32")
CASES = [
    # ---- generic gather kernel (conv_igemm.hip) and the generic weight gradient (conv_wgrad.hip)
    Case("gen_s2_ragged", "conv", 2, 12, 20, 32, 40, stride=2, act=LR, dtypes=("bf16", "fp32"), wamp=2,
         instance="conv_igemm, 3x3 stride 2, ragged channels; conv_wgrad split-K"),
    Case("gen_odd", "conv", 2, 9, 7, 8, 8, stride=2, wamp=2, instance="conv_igemm, odd sizes: pad_before = 1"),
    Case("gen_odd_coords", "conv", 2, 9, 9, 8, 8, stride=2, coords=True, wamp=2,
         instance="conv_igemm, odd sizes with CoordConv (9 x 9: dyadic coordinates)"),
    Case("gen_1x1_map", "conv", 4, 1, 1, 16, 72, k=1, dtypes=ALL, wamp=2, instance="conv_igemm, 1x1 on 1x1 maps"),
    Case("gen_1x1_res", "conv", 5, 4, 4, 16, 16, k=1, act=LR, res_self=True, wamp=2, instance="conv_igemm, 1x1 residual block"),
    Case("dense_512", "conv", 128, 1, 1, 512, 512, k=1, act=LR, res_self=True, dtypes=("bf16", "fp32"),
         instance="conv_igemm split-K dense layer; conv_wgrad single split in place"),
    Case("dense_64", "conv", 128, 1, 1, 64, 512, k=1, instance="conv_igemm split-K dense layer, 64 inputs"),
    Case("dense_512_post", "conv", 128, 1, 1, 512, 512, k=1, act=LR, res_self=True, in_post=True, out_act=True,
         instance="conv_igemm split-K epilogue: inverted residual + stored activation"),
    # ---- patch kernel (conv3x3_patch.hip): every N-tile width; the wgrad3x3 tile pair is the one CONV_CASES names for the shape
    Case("patch_bn32", "conv", 2, 16, 16, 16, 16, act=LR, res_self=True, dtypes=ALL, wamp=2, instance="patch <32,1>"),
    Case("patch_bn64_w6464", "conv", 2, 48, 32, 72, 64, act="relu", instance="patch <64,1>; wgrad3x3 <64,64>"),
    Case("patch_bn128", "conv", 2, 32, 32, 32, 96, act=LR, dtypes=("bf16", "fp32"), instance="patch <128,1>; wgrad3x3 <32,128>"),
    Case("patch_bn128_ragged_w64128", "conv", 3, 32, 48, 64, 136, act=LR, dtypes=("bf16", "f16"),
         instance="patch <128,1>, ragged second N-tile; wgrad3x3 <64,128>"),
    Case("patch_res_post", "conv", 2, 32, 32, 128, 128, act=LR, res_self=True, in_post=True, out_act=True, dtypes=("bf16", "f16"),
         instance="patch, staged epilogue: inverted residual + stored activation"),
    Case("patch_sub8", "conv", 8, 8, 8, 72, 72, act=LR, res_self=True, instance="patch SUB=8: whole 8x8 images packed 4 to a tile"),
    Case("patch_sub4", "conv", 32, 4, 4, 136, 136, act=LR, res_self=True, instance="patch SUB=4: whole 4x4 images packed 16 to a tile"),
    Case("patch_ragged_coords33", "conv", 2, 33, 33, 64, 136, coords=True, act=LR, dtypes=("bf16", "f16"),
         instance="patch, ragged tiles (33 x 33) with CoordConv, ragged second N-tile"),
    Case("patch_coords17_res", "conv", 3, 17, 17, 32, 32, coords=True, act=LR, res_self=True, dtypes=("bf16", "fp32"),
         instance="patch, ragged tiles (17 x 17) with CoordConv + residual"),
    Case("patch_kchunks16", "conv", 2, 16, 16, 512, 512, act="relu", wdens=0.5, instance="patch, kchunks 16 (one block per CU, 3-stage ring)"),
    Case("patch_occ2_bn64", "conv", 32, 64, 64, 64, 64, act="relu", res_self=True, instance="patch <64,2>: 512 blocks"),
    Case("patch_occ2_bn128_thin", "conv", 16, 64, 64, 32, 136,
         instance="patch <128,2> through the single-chunk gate (ci <= 32, co_fill > 64, at least 512 blocks of 128 columns): 512 blocks, LDS-DMA patch"),
    Case("patch_occ2_bn128", "conv", 16, 64, 64, 40, 136, act=LR,
         instance="patch <128,2> through the ci > 32 gate: 512 blocks, two chunks, static-tap form, ragged second N-tile"),
    Case("patch_thin_1536", "conv", 24, 128, 128, 32, 32, act=LR, res_self=True,
         instance="patch <32,1>, single chunk, 1536 tiles through the XCD remap"),
    Case("w3_3264", "conv", 5, 16, 32, 24, 40, instance="patch <64,1>; wgrad3x3 <32,64>"),
    Case("w3_6432", "conv", 2, 32, 16, 80, 16, instance="patch <32,1>; wgrad3x3 <64,32>"),
    Case("w3_3232", "conv", 2, 64, 64, 8, 32, instance="first-layer form through ops.conv; wgrad3x3 <32,32>"),
    # ---- depth-to-space input gradient of a stride-2 layer
    Case("d2s", "conv", 2, 32, 32, 32, 64, stride=2, instance="d2s input gradient (patch kernel over the gradient lattice)"),
    Case("d2s_dact", "conv", 2, 32, 32, 32, 64, stride=2, act=LR, instance="d2s input gradient with act'"),
    # ---- row-stream kernels (conv3x3_rows.hip) under UPS_ROWS_KERNEL=force, and the patch kernel on the same inputs
    Case("rows_one_band", "rows", 5, 32, 128, 32, 32, act=LR, res_self=True, in_post=True, out_act=True, dtypes=("bf16", "f16"),
         instance="rows <32,7,8>: one band per image"),
    Case("rows_two_planes", "rows", 3, 64, 64, 64, 64, act=LR, res_self=True, in_post=True, out_act=True, dtypes=("bf16", "fp32"),
         instance="rows <64,6,10>: two planes"),
    Case("rows_two_tiles", "rows", 2, 32, 256, 32, 32, act=LR, res_self=True, in_post=True, out_act=True,
         instance="rows2 <32,8,8>: two column tiles per wave"),
    Case("rows_s2_32", "rows_s2", 2, 128, 128, 32, 64, stride=2, instance="rows_s2 <32,7,7>"),
    Case("rows_s2_64", "rows_s2", 3, 64, 64, 64, 128, stride=2, out_act=True, dtypes=("bf16", "fp32"), instance="rows_s2 <64,6,9>, stored activation"),
    Case("s2_odd", "s2", 2, 31, 63, 32, 64, stride=2, out_act=True, instance="conv3x3_s2 64-wide, odd input: pad_before = 1"),
    # ---- thin-out logit kernel
    Case("thinout_p3_f32", "thinout", 2, 32, 32, 256, 3, extra={"out_f32": True}, dtypes=("bf16", "fp32"), instance="thinout, P = 3, fp32 output"),
    Case("thinout_p16_bf16", "thinout", 2, 32, 64, 256, 16, extra={"out_f32": False}, dtypes=("bf16", "f16"), instance="thinout, P = 16 stored as bf16"),
    # ---- first-layer kernel at the shapes of test_first_layer_kernel (x holds 3 of 8 channels)
    Case("first_vgg", "first", 5, 32, 64, 3, 64, wamp=2, dtypes=("bf16", "fp32"), instance="first: 3 -> 64"),
    Case("first_ragged", "first", 3, 16, 16, 3, 24, wamp=2, instance="first: all-border tile, ragged channel tail"),
    Case("first_16rows", "first", 2, 128, 32, 3, 32, out_act=True, wamp=2, instance="first: 16 rows per wave, stored activation"),
    Case("first_16rows_64", "first", 2, 64, 48, 3, 64, wamp=2, instance="first: 16 rows per wave, 64 outputs"),
    Case("first_coord_table", "first", 3, 16, 16, 3, 24, coords=True, wamp=2, extra={"zero_coord_rows": True},
         instance="first: CoordConv table path with zero coordinate rows (the kernel takes 16-aligned maps only: no dyadic coordinates)"),
    # ---- part-masked input fused into the load, and its mask_grad reduction
    Case("mask_p3", "mask", 5, 16, 16, 3, 32, wamp=2, extra={"P": 3}, instance="part mask fused, P = 3"),
    Case("mask_p25", "mask", 2, 48, 48, 3, 32, wamp=2, extra={"P": 25}, instance="part mask fused, P = 25"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_inputs(case):
    """(x_stored, V, b, g) of a case, float64 lattice tensors.  first / mask cases: x has the 3 image channels only."""
    g = gen(case.name)
    cin_v = case.cin + (2 if case.coords else 0)
    x = activations(g, (case.n, case.h, case.w, case.cin), case.xamp)
    V = weights(g, (case.k, case.k, cin_v, case.cout), case.wamp, case.wdens)
    b = biases(g, case.cout)
    ho, wo = same_pad(case.h, case.k, case.stride)[0], same_pad(case.w, case.k, case.stride)[0]
    n_img = case.n * case.extra.get("P", 1)
    go = out_grads(g, (n_img, ho, wo, case.cout), case.gamp)
    return x, V, b, go


def part_bits(case):
    """Ownership words of a mask case: mostly one part per pixel, some pixels with two owners, some with none."""
    P = case.extra["P"]
    g = gen(case.name + "/bits")
    owner = torch.randint(0, P, (case.n, case.h, case.w), generator=g)
    bits = (torch.ones_like(owner) << owner).to(torch.int32)
    bits[0, :3, :3] = 0b101
    bits[0, 5, 5] = 0
    hard = ((bits.unsqueeze(-1) >> torch.arange(P)) & 1).double()
    return bits, hard


def part_images(x, hard):
    """[P * B, h, w, 3] part-major, as MaskPartsFn materialises them."""
    P = hard.shape[-1]
    n, h, w, c = x.shape
    return (x.unsqueeze(3) * hard.unsqueeze(-1)).permute(3, 0, 1, 2, 4).reshape(P * n, h, w, c)


_REF = {}
_REF_KEEP = 4 << 20         # input elements: the few larger cases (~0.5 GB of float64 each) are recomputed instead of kept


def case_reference(case):
    """(inputs, reference dict, headroom) of a case: computed once per process and shared (the large cases: once per call);
    callers must not modify it."""
    if case.name in _REF:
        return _REF[case.name]
    if True:
        x, V, b, go = case_inputs(case)
        kw = case.kw()
        if case.extra.get("zero_coord_rows"):
            V[:, :, case.cin:] = 0.0
        xin = part_images(x, part_bits(case)[1]) if case.family == "mask" else x
        fwd_only = case.family in ("first", "thinout", "rows_s2", "s2")
        ref = conv_block(xin, V, b, None if fwd_only else go, **kw)
        if case.family == "mask":
            # d loss / d hard[b, y, x, p] = sum_c gx[p * B + b, y, x, c] * view[b, y, x, c], gx rounded to bf16 as the tensor it replaces
            P = case.extra["P"]
            gxq = ref["gx"].to(torch.bfloat16).double().reshape(P, case.n, case.h, case.w, case.cin)
            ref["gh"] = (gxq * x.unsqueeze(0)).sum(-1).permute(1, 2, 3, 0).contiguous()
        if case.extra.get("zero_coord_rows"):       # coordinates that are not dyadic only ever meet zero weights
            hr = headroom(xin, V[:, :, :case.cin], b, None, **dict(kw, coords=False))
        else:
            hr = headroom(xin, V, b, None if fwd_only else go, **kw)
        out = ((x, V, b, go), ref, hr)
        if xin.numel() <= _REF_KEEP:
            _REF[case.name] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the grouped critic towers (ops.TowersFn): nin, (L - 2) x residual_block(k = 1), nin on [M, k] rows; every stored tensor bf16
class TowerCase(object):
    """T = 3 towers of six 1x1 layers, input widths as in test_critic_towers_grouped.  Weights are {-1, 0, 1} with `nnz` non-zero
    entries per output column, so that six layers of residual growth and of slope bits keep the headroom."""
    def __init__(self, name, M, widths=(256, 64, 256), D=512, Ln=6, nnz=2):
        self.name, self.M, self.widths, self.D, self.Ln, self.nnz = name, M, widths, D, Ln, nnz

    def __repr__(self):
        return self.name


TOWER_CASES = [TowerCase("towers_m6", 6), TowerCase("towers_m40", 40)]


def bf16_round(t):
    return t.to(torch.bfloat16).double()


def sparse_weights(g, k, n, nnz):
    W = torch.zeros(k, n, dtype=torch.float64)
    rows = torch.randint(0, k, (nnz, n), generator=g)
    sign = torch.randint(0, 2, (nnz, n), generator=g).double() * 2 - 1
    return W.scatter_(0, rows, sign)


def tower_inputs(case):
    """Per tower: (x0 [M, k], [W_l [k_l, D]], [b_l [D]], g_out [M, D]), float64 lattice tensors."""
    g = gen(case.name)
    out = []
    for c in case.widths:
        Ws = [sparse_weights(g, c if l == 0 else case.D, case.D, case.nnz) for l in range(case.Ln)]
        bs = [ints(g, (case.D,), 1) for _ in range(case.Ln)]
        out.append((ints(g, (case.M, c), 1), Ws, bs, ints(g, (case.M, case.D), 1)))
    return out


def _sum_lsbs(total_abs, unit):
    return float(total_abs.max()) / unit


def tower_reference(x0, Ws, bs, g_out, slope=SLOPE):
    """One tower as ups_towers_fwd / _bwd run it, layer by layer in float64 with the kernels' one bf16 rounding per stored tensor:
      a_0 = bf16(lrelu(x0 W_0 + b_0));  a_l = bf16(lrelu(a_{l-1} W_l + b_l + inv(a_{l-1})));  out = bf16(a_{L-2} W_{L-1} + b_{L-1})
      g_{L-1} = g_out;  g_{l-1} = bf16(act'(a_{l-1}) * (g_l W_l^T) (+ g_l for a residual layer));  gx0 = bf16(g_0 W_0^T)
      dW_l = X_l^T g_l (X_0 = x0, X_l = a_{l-1}),  db_l = sum_m g_l        (fp32, not rounded again)
    Returns (dict, headroom): headroom = the largest sum of |products| of any of these sums in units of its smallest LSB."""
    Ln = len(Ws)
    acts, worst = [], 0.0
    a = x0
    for l in range(Ln):
        res = act_inverse(a, slope) if 0 < l < Ln - 1 else None
        v = a @ Ws[l] + bs[l]
        tot = a.abs() @ Ws[l].abs() + bs[l].abs()
        unit = min(lsb(a) * lsb(Ws[l]), lsb(bs[l]))
        if res is not None:
            v, tot, unit = v + res, tot + res.abs(), min(unit, lsb(res))
        if l < Ln - 1:
            v, unit = lrelu(v, slope), unit * slope
        worst = max(worst, _sum_lsbs(tot, unit))
        a = bf16_round(v)
        acts.append(a)
    gs = [None] * Ln
    gs[Ln - 1] = g_out
    for l in range(Ln - 1, 0, -1):
        dact = torch.where(acts[l - 1] > 0, torch.ones_like(acts[l - 1]), torch.full_like(acts[l - 1], slope))
        s_ = gs[l] @ Ws[l].t()
        tot, unit = gs[l].abs() @ Ws[l].abs().t(), lsb(gs[l]) * lsb(Ws[l]) * slope
        v = dact * s_
        if l < Ln - 1:
            v, tot = v + gs[l], tot + gs[l].abs()
        worst = max(worst, _sum_lsbs(tot, unit))
        gs[l - 1] = bf16_round(v)
    gx0 = gs[0] @ Ws[0].t()
    worst = max(worst, _sum_lsbs(gs[0].abs() @ Ws[0].abs().t(), lsb(gs[0]) * lsb(Ws[0])))
    gW, gb = [], []
    for l in range(Ln):
        X = x0 if l == 0 else acts[l - 1]
        gW.append(X.t() @ gs[l])
        gb.append(gs[l].sum(0))
        worst = max(worst, _sum_lsbs(X.abs().t() @ gs[l].abs(), lsb(X) * lsb(gs[l])), _sum_lsbs(gs[l].abs().sum(0), lsb(gs[l])))
    return {"acts": acts, "out": acts[-1], "gx0": bf16_round(gx0), "gW": gW, "gb": gb}, worst


def tower_case_reference(case):
    """[(inputs, reference dict)] per tower and the case's headroom."""
    if case.name not in _REF:
        ins = tower_inputs(case)
        refs = [tower_reference(*t) for t in ins]
        _REF[case.name] = ([(t, r[0]) for t, r in zip(ins, refs)], max(r[1] for r in refs))
    return _REF[case.name]


AXES_NHWC = ("image", "y", "x", "channel")
AXES_HWIO = ("tap_y", "tap_x", "cin", "cout")


def first_diff(a, b, axes=None):
    """None when the two tensors hold the same bits, else a message: the number of differing elements, the first differing index
    decoded (for a 4-d tensor: image, y, x, channel) and the two values there."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    iv = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    ne = a.contiguous().view(iv) != b.contiguous().view(iv)
    if not bool(ne.any()):
        return None
    idx = tuple(int(i) for i in ne.nonzero()[0])
    names = axes if axes is not None else (AXES_NHWC if a.ndim == 4 else None)
    where = ", ".join("{}={}".format(k, v) for k, v in zip(names, idx)) if names else str(idx)
    return "{} of {} elements differ; first at ({}): got {!r} want {!r}".format(
        int(ne.sum()), ne.numel(), where, float(a[idx]), float(b[idx]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp8 lattice: data on which every scale the fp8 kernels derive is a power of two and every quantisation is lossless
#
# weight_prep_f8_kernel scales a row by 448 / m (m = the row's |max|) and dequantises by m / 448: with m = 7 these are 64 and 2**-6.
# The delayed scales are fmax * MARGIN / amax (MARGIN = 0.5; fmax = 448 for e4m3, 57344 for e5m2): with amax = 7 they are 32 and
# 4096.  Integers in [-7, 7] times 64 and leaky_relu(., 0.25) of them times 32 are e4m3 values, integers in [-7, 7] times 4096
# are e5m2 values.  So the accumulator sees integer multiples of one LSB, the dequantisation factors are exact, and the fp8
# kernels must give the bits of the plain integer convolution.
F8_AMP = 7
E4M3_MAX, E5M2_MAX, F8_MARGIN = 448.0, 57344.0, 0.5
F8_SW = E4M3_MAX / F8_AMP                       # 64: per-row weight scale
F8_SA = E4M3_MAX * F8_MARGIN / F8_AMP           # 32: delayed scale of an activation tensor
F8_SG = E5M2_MAX * F8_MARGIN / F8_AMP           # 4096: delayed scale of a gradient tensor
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


def f8_weights(g, k, cin, cout, density=1.0):
    """Integers in [-7, 7] [k, k, cin, cout]; every output-channel column over (taps, cin) and every input-channel row over
    (taps, cout) holds a +-7: the forward copy is scaled per column, the transposed copy of the input gradient per row."""
    V = ints(g, (k, k, cin, cout), F8_AMP, density)
    co, ci = torch.arange(cout), torch.arange(cin)
    t = co % (k * k)
    V[t // k, t % k, (3 * co + 1) % cin, co] = F8_AMP * (1.0 - 2.0 * (co % 2)).double()
    t = ci % (k * k)
    V[t // k, t % k, ci, (5 * ci + 3) % cout] = F8_AMP * (1.0 - 2.0 * (ci // 2 % 2)).double()
    assert bool((V.abs().amax(dim=(0, 1, 2)) == F8_AMP).all()) and bool((V.abs().amax(dim=(0, 1, 3)) == F8_AMP).all())
    return V


def f8_activations(g, shape, density=1.0):
    """Integers in [-7, 7] with a +7 (the recorded maximum is of act(x): behind a leaky ReLU a -7 counts 1.75) and a -7."""
    x = ints(g, shape, F8_AMP, density)
    x.view(-1)[0], x.view(-1)[-1] = F8_AMP, -F8_AMP
    return x


def f8_out_grads(g, shape, density=1.0):
    """Integers in [-7, 7] with both signs of 7."""
    return f8_activations(g, shape, density)


def is_pow2(t):
    """Every entry of a float32 tensor is a power of two (mantissa bits zero, finite, positive)."""
    t = t.float().contiguous().view(-1)
    bits = t.view(torch.int32)
    return bool(((bits & 0x007fffff) == 0).all() and (t > 0).all() and torch.isfinite(t).all())


def f8_quantise(t, scale, dtype):
    """(t * scale) as the fp8 type (saturating RNE, as v_cvt_pk_{fp8,bf8}_f32) and whether the round trip is lossless."""
    fmax = E4M3_MAX if dtype == E4M3 else E5M2_MAX
    s = t.double() * scale
    q = s.clamp(-fmax, fmax).float().to(dtype)
    return q, torch.equal(q.double(), s)


class Fp8Case(object):
    """One fp8 launch family member.  route: "convert" (the kernel quantises its 16-bit operand), "copy" (a pre-quantised
    copy is handed in: the grid-size gates of launch_t choose the instance) or "wgrad".  dirs: which launches the case drives.
    emit: which launches also write an fp8 copy of their output (the output's maximum is then arranged to be 7 * 2**k)."""
    k, stride, in_post, out_act = 3, 1, False, False

    def __init__(self, name, route, n, h, w, cin, cout, dirs=("fwd", "dgrad"), coords=False, act=None, res_self=False, emit=(),
                 f16=False, xdens=1.0, wdens=1.0, gdens=1.0, splitk=None, instance=""):
        self.name, self.route, self.n, self.h, self.w, self.cin, self.cout = name, route, n, h, w, cin, cout
        self.dirs, self.coords, self.act, self.res_self, self.emit, self.f16 = dirs, coords, act, res_self, emit, f16
        self.xdens, self.wdens, self.gdens, self.splitk, self.instance = xdens, wdens, gdens, splitk, instance
        assert not res_self or cin == cout

    def __repr__(self):
        return self.name


FP8_CASES = [
    # ---- in-kernel conversion (Fp8State(True, copy_only=False)): launch_bn<T, BN, 1, TS, 1 / 2>
    Fp8Case("f8_cvt_ragged_hw", "convert", 2, 16, 32, 64, 192, act=LR, emit=("fwd", "dgrad"),
            instance="fwd e4m3 <128,1> with a ragged second N-tile (192 = 128 + 64), h != w; dgrad e5m2 <64,1>, three chunks"),
    Fp8Case("f8_cvt_chunks4", "convert", 2, 16, 16, 256, 64, emit=("fwd", "dgrad"),
            instance="fwd e4m3 <64,1>, four channel chunks; dgrad e5m2 <128,1>, two N-tiles"),
    Fp8Case("f8_cvt_res_lrelu", "convert", 2, 32, 16, 128, 128, act=LR, res_self=True, emit=("fwd", "dgrad"),
            instance="fwd e4m3 <128,1>, leaky ReLU on load + residual; dgrad e5m2 <128,1> with act' and the residual gradient"),
    Fp8Case("f8_cvt_coords", "convert", 3, 16, 16, 64, 64, coords=True, act=LR, emit=("fwd", "dgrad"),
            instance="fwd e4m3 <64,1> with the CoordConv table (zero coordinate rows); dgrad e5m2 <64,1> (forward ci_log = 64)"),
    # ---- pre-quantised input, K = 32 MFMA, one block per CU (small grids)
    Fp8Case("f8_copy_occ1_64to128", "copy", 2, 32, 32, 64, 128, act=LR, emit=("fwd", "dgrad"),
            instance="fwd <128,1,PRE> e4m3; dgrad <64,1,PRE> e5m2 (8 tiles: below every 512-block gate)"),
    Fp8Case("f8_copy_occ1_128to64", "copy", 2, 32, 32, 128, 64, act=LR, emit=("fwd", "dgrad"),
            instance="fwd <64,1,PRE> e4m3 (ci % 128 == 0 but a small grid: K = 32); dgrad <128,1,PRE> e5m2"),
    # ---- pre-quantised input, K = 32 MFMA, two blocks per CU (>= 512 blocks, ci % 128 != 0)
    Fp8Case("f8_copy_occ2_192to136", "copy", 64, 32, 32, 192, 136, dirs=("fwd",), act=LR,
            instance="fwd <128,2,PRE> e4m3, K = 32: 256 tiles x 2 N-tiles (one ragged), three chunks"),
    Fp8Case("f8_copy_occ2_64to64", "copy", 128, 32, 32, 64, 64, emit=("fwd", "dgrad"),
            instance="fwd <64,2,PRE> e4m3 and dgrad <64,2,PRE> e5m2, K = 32: 512 tiles"),
    Fp8Case("f8_copy_occ2_dgrad_136", "copy", 64, 32, 32, 136, 192, dirs=("dgrad",), act=LR,
            instance="dgrad <128,2,PRE> e5m2, K = 32 (forward co = 192): 256 tiles x 2 N-tiles (one ragged)"),
    # ---- block-scaled K = 128 MFMA (ci % 128 == 0, >= 512 blocks): F8 = 3 (e4m3) / 4 (e5m2)
    Fp8Case("f8_scaled_128to136", "copy", 64, 32, 32, 128, 136, dirs=("fwd",), act=LR,
            instance="fwd <128,2,F8=3>: one double chunk, ragged second N-tile"),
    Fp8Case("f8_scaled_256to136", "copy", 64, 32, 32, 256, 136, dirs=("fwd",),
            instance="fwd <128,2,F8=3>: two double chunks, ragged second N-tile"),
    Fp8Case("f8_scaled_128to64", "copy", 128, 32, 32, 128, 64, act=LR, emit=("fwd",),
            instance="fwd <64,2,F8=3>: 512 tiles; dgrad <128,2,PRE> e5m2 on K = 32 (forward co = 64)"),
    Fp8Case("f8_scaled_dgrad_64", "copy", 128, 32, 32, 64, 128, act=LR, emit=("dgrad",),
            instance="dgrad <64,2,F8=4> (forward co = 128: one double chunk); fwd <128,2,PRE> e4m3 on K = 32"),
    Fp8Case("f8_scaled_dgrad_136", "copy", 64, 32, 32, 136, 256, dirs=("dgrad",), act=LR,
            instance="dgrad <128,2,F8=4>: two double chunks (forward co = 256), ragged second N-tile (forward ci = 136)"),
    # ---- conv_wgrad3x3_f8_kernel<fp16 input, activation on load>; splitk is what ups_conv_wgrad_plan gives
    Fp8Case("f8_wgrad_bf16_plain", "wgrad", 2, 16, 32, 64, 128, dirs=("wgrad",), splitk=2,
            instance="wgrad8 <false,false>: 8 units, split-K 2"),
    Fp8Case("f8_wgrad_bf16_lrelu_odd", "wgrad", 3, 16, 48, 128, 128, dirs=("wgrad",), act=LR, splitk=4,
            instance="wgrad8 <false,true>: odd n, w != h, 18 units over 4 splits (a short last split)"),
    Fp8Case("f8_wgrad_f16_plain_coords", "wgrad", 3, 32, 32, 64, 128, dirs=("wgrad",), coords=True, f16=True, splitk=6,
            instance="wgrad8 <true,false>: CoordConv rows beside it from the fp32 coordinate kernels"),
    Fp8Case("f8_wgrad_f16_lrelu_256", "wgrad", 5, 32, 32, 256, 256, dirs=("wgrad",), act=LR, f16=True, splitk=8,
            instance="wgrad8 <true,true>: 256 -> 256, 8 tile pairs, 40 units: split-K 10 & ~7 = 8"),
]
FP8_BY_NAME = {c.name: c for c in FP8_CASES}
assert len(FP8_BY_NAME) == len(FP8_CASES)


def fp8_case_inputs(case):
    """(x, V, b, g) float64 lattice tensors; CoordConv rows of V are zero (16-aligned maps: no dyadic coordinates)."""
    g = gen(case.name)
    x = f8_activations(g, (case.n, case.h, case.w, case.cin), case.xdens)
    V = torch.zeros(3, 3, case.cin + (2 if case.coords else 0), case.cout, dtype=torch.float64)
    V[:, :, :case.cin] = f8_weights(g, 3, case.cin, case.cout, case.wdens)
    b = biases(g, case.cout)
    go = f8_out_grads(g, (case.n, case.h, case.w, case.cout), case.gdens)
    return x, V, b, go


def _flipped(W):
    """The weights of the input gradient as a forward convolution of the output gradient (3x3, stride 1, 'SAME')."""
    return W.flip(0, 1).transpose(2, 3).contiguous()


def _tap_wgrad(x, g):
    """dV[r][s] = sum over pixels of x[pix + (r - 1, s - 1)]^T g[pix]."""
    n, h, w, ci = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    G = g.reshape(-1, g.shape[-1])
    return torch.stack([torch.stack([xp[:, r:r + h, s:s + w].reshape(-1, ci).t() @ G for s in range(3)]) for r in range(3)])


def _big(case):
    return case.n * case.h * case.w * max(case.cin, case.cout) > _REF_KEEP


def fp8_headroom(case, inputs=None):
    """{"fwd", "dgrad", "wgrad", "bgrad"} (the launches the case drives): the largest sum of |products| in units of the smallest LSB
    among them, IN THE QUANTISED DOMAIN the accumulator sees -- (act(x) * s_a)(w * 64), (g * s_g)(w * 64), (act(x) * s_x)(g * s_g),
    and g * s_g against the ones operand of the bias sum -- computed as convolutions of |x| with |w|; and of the epilogue's sums
    (dequantised accumulator + bias + residual, act' * accumulator + residual gradient) in units of their own LSB.
    Every entry must be below 2**24.  (In float32 for the large cases: a sum of non-negative integers that reaches 2**24 in exact
    arithmetic cannot round to less, so the comparison with LIMIT is still exact.)"""
    x, V, b, go = inputs if inputs is not None else fp8_case_inputs(case)
    T = torch.float32 if _big(case) else torch.float64
    W = (V[:, :, :case.cin] * F8_SW).abs().to(T)
    xa = act_fn(x, case.act)
    A, G = (xa * F8_SA).abs().to(T), (go * F8_SG).abs().to(T)
    uA, uW, uG = lsb(A, 20), lsb(W, 20), lsb(G, 20)
    out = {}
    if "fwd" in case.dirs:
        acc = conv_same(A, W, None)
        top = acc.double() / (F8_SA * F8_SW) + b.abs() + (x.abs() if case.res_self else 0.0)
        tmax = float(top.max()) + (2.0 * _arranged_top(top) if "fwd" in case.emit else 0.0)     # (the arranged bias: |b_c| <= 2 top)
        out["fwd"] = max(float(acc.max()) / (uA * uW), tmax / min(lsb(xa) * lsb(V), lsb(b)))
    if "dgrad" in case.dirs:
        acc = conv_same(G, _flipped(W), None)
        slope_bits = SLOPE if case.act == "leaky_relu" else 1.0
        top = acc.double() / (F8_SG * F8_SW) + (go.abs() if case.res_self else 0.0)
        tmax = _arranged_top(top) if "dgrad" in case.emit else float(top.max())                # (the arranged residual gradient)
        out["dgrad"] = max(float(acc.max()) / (uG * uW), tmax / (lsb(go) * lsb(V) * slope_bits))
    if "wgrad" in case.dirs:
        out["wgrad"] = float(_tap_wgrad(A, G).max()) / (uA * uG)
        out["bgrad"] = float(G.sum(dim=(0, 1, 2)).max()) / uG
    return out


def _arranged_top(t):
    """7 * 2**k >= max |t|: the maximum an emitting launch's output is arranged to have, so that ITS delayed scale is dyadic."""
    m, top = float(t.abs().max()), float(F8_AMP)
    while top < m:
        top *= 2.0
    return top


def fp8_reference(case, inputs, T=torch.float64):
    """The emulation the fp8 kernel tests state, on the lattice: quantise with .to(torch.float8_*), accumulate exactly, dequantise,
    bias / residual / act', round once to bf16 (weight and bias gradient stay fp32).  T = float32 is used for the large cases once
    fp8_headroom has shown every sum below 2**24 LSBs: float32 accumulation is then exact too, in any order.
    Returns a dict: y / gx / gV / gb (float64, unrounded), "lossless" (every quantisation round-trips), and for the emitting launches
    the arrangement that makes the OUTPUT's maximum 7 * 2**k: "b" (one seeded channel's bias moved so that the maximum of
    leaky_relu(y) is "y_top"), "res_g" (a residual-gradient tensor, zero but for one element where the sum is zero, which puts
    "gx_top" there; None if no element qualifies)."""
    x, V, b, go = inputs
    cin = case.cin
    xa = act_fn(x, case.act)
    xq, okx = f8_quantise(xa, F8_SA, E4M3)
    gq, okg = f8_quantise(go, F8_SG, E5M2)
    wq, okw = f8_quantise(V[:, :, :cin], F8_SW, E4M3)       # (m = 7 in every column AND every row: both copies are V * 64)
    out = {"lossless": okx and okg and okw, "b": b, "res_g": None}
    if "fwd" in case.dirs:
        pre0 = conv_same(xq.to(T), wq.to(T), None).double() * ((1.0 / F8_SW) * (1.0 / F8_SA))
        if case.res_self:
            pre0 = pre0 + x
        if "fwd" in case.emit:
            c = int(torch.randint(0, case.cout, (1,), generator=gen(case.name + "/emit")))
            top = _arranged_top(lrelu(pre0 + b))
            b = b.clone()
            b[c] = top - float(pre0[..., c].max())
            out["b"], out["y_top"], out["emit_channel"] = b, top, c
        out["y"] = pre0 + b
    if "dgrad" in case.dirs:
        s = conv_same(gq.to(T), _flipped(wq.to(T)), None).double() * ((1.0 / F8_SW) * (1.0 / F8_SG))
        if case.act == "leaky_relu":
            s = s * torch.where(x > 0, 1.0, SLOPE).double()
        if case.res_self:
            s = s + go
        if "dgrad" in case.emit:
            top = _arranged_top(s)
            zero = ((s == 0) & (go == 0) if case.res_self else (s == 0)).view(-1).nonzero()     # (its sum with go[e] stays a bf16 value)
            if zero.numel():
                r = torch.zeros_like(s)
                r.view(-1)[int(zero[0])] = top
                out["res_g"], out["gx_top"] = r, top
                s = s + r
        out["gx"] = s
    if "wgrad" in case.dirs:
        out["gV"] = _tap_wgrad(xq.to(T), gq.to(T)).double() * ((1.0 / F8_SA) * (1.0 / F8_SG))
        out["gb"] = gq.to(T).sum(dim=(0, 1, 2)).double() * (1.0 / F8_SG)
    return out


def plain_reference(case, inputs, ref, T=torch.float64):
    """The same launches as the plain integer convolution (no quantisation anywhere), with the arrangement `ref` made (bias,
    residual gradient), by the tap loop; tests/test_host_exact_fp8.py holds it to conv_block + autograd where the case is small."""
    x, V, b, go = inputs
    Vm = V[:, :, :case.cin]
    out = {}
    if "fwd" in case.dirs:
        out["y"] = conv_same(act_fn(x, case.act).to(T), Vm.to(T), None).double() + ref["b"] + (x if case.res_self else 0.0)
    if "dgrad" in case.dirs:
        s = conv_same(go.to(T), _flipped(Vm.to(T)), None).double()
        if case.act == "leaky_relu":
            s = s * torch.where(x > 0, 1.0, SLOPE).double()
        out["gx"] = s + (go if case.res_self else 0.0) + (ref["res_g"] if ref["res_g"] is not None else 0.0)
    if "wgrad" in case.dirs:
        out["gV"] = _tap_wgrad(act_fn(x, case.act).to(T), go.to(T)).double()
        out["gb"] = go.sum(dim=(0, 1, 2))
    return out


def fp8_case_reference(case):
    """(inputs, reference dict, headroom dict) of an fp8 case, cached like case_reference (the large cases: recomputed)."""
    if case.name in _REF:
        return _REF[case.name]
    inputs = fp8_case_inputs(case)
    hr = fp8_headroom(case, inputs)
    exact32 = _big(case) and max(hr.values()) < LIMIT
    out = (inputs, fp8_reference(case, inputs, torch.float32 if exact32 else torch.float64), hr)
    if not _big(case):
        _REF[case.name] = out
    return out
