"""Kernel-level parity of the NHWC streaming kernels of csrc/pointwise.hip (through the C ABI, `lib.call`, so that every output
buffer can be handed over pre-filled with 0xFF.. NaN patterns) against the fp64 restatements of tests/pointwise_ref.py.

* Pure data movement is bit-exact; pad channels and out-of-window elements are exactly zero.
* Arithmetic kernels meet `pointwise_ref.assert_rounds_once` element by element; k (the fp32 operations behind one output) is
  written beside each call with its count.
* Every case launches twice into fresh NaN-filled buffers and compares the two results bit for bit.
* The shapes past the grid cap (16 384 blocks x 256 threads: the grid-stride loop takes a second, partial pass) are too large for a
  CPU reference: there the SAME restatement is evaluated in fp64 on the device (torch's kernels, not the code under test), in batch
  slices so that no tensor reaches 1 GiB.
* `test_wrappers_*`: the `ops.*Fn` autograd wrappers reach the same kernels (bit-identical results).
"""
import numpy as np
import pytest
import torch

import pointwise_ref as P

pytestmark = pytest.mark.gpu

CAP = 16384 * 256                      # work items of one full grid (grid_for)
SLOPE = float(np.float32(0.2))         # the slope as the kernels receive it (a C float)
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ELEMS = {"fp32": 4, "bf16": 8, "f16": 8}       # elements of one 16-byte chunk


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _code(lib, dtype):
    return {"fp32": lib.F32, "bf16": lib.BF16, "f16": lib.F16}[dtype]


def _past_cap(per_image):
    """The batch that puts a launch of `per_image` work items per image at about 1.13 grids: a second, partial grid-stride pass."""
    n = CAP // per_image + 1 + CAP // per_image // 8
    assert CAP < n * per_image < 2 * CAP and (n * per_image) % CAP != 0
    return n


def _is_big(numel):
    return numel > (1 << 22)


def _randn(shape, dtype, dev, seed, scale=1.0):
    """N(0, scale) rounded to the stored type; large tensors are drawn on the device."""
    numel = int(np.prod(shape))
    if _is_big(numel):
        g = torch.Generator(device=dev).manual_seed(seed)
        return (torch.randn(shape, generator=g, device=dev) * scale).to(TDT[dtype])
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(TDT[dtype]).to(dev)


def _nan(shape, tdt, dev):
    """A buffer of all-ones bit patterns (a NaN in every float format of the ABI; 0xFF bytes)."""
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[torch.empty((), dtype=tdt).element_size()]
    return torch.full(shape, 255 if it == torch.uint8 else -1, dtype=it, device=dev).view(tdt)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a).cpu(), _bits(b).cpu())


def _twice(fn):
    """fn allocates NaN-filled outputs, launches and returns them: run it twice, the results must agree bit for bit."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(_bits(u), _bits(v)), "two launches on the same input differ"
    return a


def _slices(n, big):
    """Batch ranges over which a reference is evaluated: one for a small case, eight-odd for a past-the-cap one."""
    step = max(1, n // 8) if big else n
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def _hp(t, big):
    """The fp64 operand of a reference: on the CPU, or (past-the-cap shapes) on the device."""
    return t.double() if big else t.cpu().double()


def _to(t, ref):
    return t.to(ref.device)


# ----------------------------------------------------------------------------- case lists
# (n, h, w, c, why): the INPUT of the x2 up-sampling kernels (bilinear, nearest) and the OUTPUT of the 2x2 pool -- the extents their
# flat index is decoded over.  n = None: chosen per dtype by _past_cap (the chunk count depends on the element size).
# idx_decode belongs to the bilinear kernels alone (nearest, pool and crop decode with plain 64-bit % and /, which the same shapes
# exercise); of its three branches the two reachable below 2^31 chunks are run -- the 64-bit one would need ~32 GiB of bf16.
GRID_CASES = [
    (2, 4, 4, 256, "headline: decoder level 4 -> 8 at 256 channels (batch cut from 64)"),
    (2, 8, 8, 128, "headline: decoder level 8 -> 16 at 128 channels"),
    (2, 16, 16, 128, "headline: decoder level 16 -> 32 at 128 channels"),
    (2, 32, 32, 32, "headline: decoder level 32 -> 64 at 32 channels"),
    (2, 64, 64, 32, "headline: decoder level 64 -> 128 at 32 channels"),
    (1, 64, 64, 256, "headline: the widest launch of the step, 64 x 64 at 256 channels"),
    (3, 8, 16, 64, "idx_decode: chunk count, w and h all powers of two (shifts)"),
    (2, 8, 24, 64, "idx_decode: chunk count a power of two, w = 24 not (32-bit divisions)"),
    (2, 6, 16, 64, "idx_decode: w a power of two, h not"),
    (2, 6, 5, 24, "idx_decode: no extent a power of two"),
    (2, 1, 7, 8, "degenerate: h = 1 (every row is the clamped last row); c = 8: one bf16 chunk, two fp32"),
    (2, 7, 1, 8, "degenerate: w = 1"),
    (3, 1, 1, 8, "degenerate: 1 x 1 maps"),
    (1, 5, 6, 136, "n = 1, c = 136 (17 chunks)"),
    (None, 48, 40, 136, "past the cap: ~1.13 grids of chunks, no extent a power of two, partial second pass"),
]
# the pools of the perceptual trunk (OUTPUT extents; the input is twice as large): 128 / 64 / 32 / 16 inputs at the VGG widths
POOL_CASES = [
    (1, 64, 64, 64, "headline: pool 1, 128 -> 64 at 64 channels (batch cut from 64)"),
    (1, 32, 32, 128, "headline: pool 2, 64 -> 32 at 128 channels"),
    (1, 16, 16, 256, "headline: pool 3, 32 -> 16 at 256 channels"),
    (2, 8, 8, 512, "headline: pool 4, 16 -> 8 at 512 channels"),
    (1, 56, 56, 128, "resize256_crop224: pool 2 on a 112 x 112 map (not a power of two)"),
] + [c for c in GRID_CASES if c[1] <= 8 or c[0] is None]
# (n, h, w, C, extra, why): depth_to_space of [n, h, w, round8(4C) + extra] into [n, 2h, 2w, round8(C)]
D2S_CASES = [
    (2, 16, 16, 64, 0, "headline-like: subpixel up-sampling to 64 channels"),
    (2, 6, 5, 3, 0, "C = 3: 12 logical of 16 physical channels in, 3 of 8 out"),
    (2, 6, 5, 10, 0, "C = 10"),
    (2, 4, 8, 13, 8, "C = 13 (odd), ldx larger than round8(4C)"),
    (1, 8, 8, 16, 16, "C = 16, all powers of two, ldx larger than 4C"),
    (2, 1, 5, 10, 0, "degenerate: h = 1"),
    (2, 5, 1, 3, 8, "degenerate: w = 1"),
    (1, 1, 1, 13, 0, "degenerate: 1 x 1, n = 1"),
    (None, 24, 20, 10, 8, "past the cap in both directions (one thread per element)"),
]
# (n, h, w, c, ho, wo, why): crop windows
CROP_CASES = [
    (1, 256, 256, 8, 224, 224, "headline of resize256_crop224: 256 -> 224 at 8 channels (batch cut)"),
    (2, 12, 20, 24, 5, 7, "non-square map and window, c = 24"),
    (2, 6, 5, 8, 6, 5, "full-size window (ho = h, wo = w): every corner clamps to (0, 0)"),
    (3, 7, 9, 136, 1, 1, "1 x 1 window, c = 136"),
    (1, 1, 9, 8, 1, 4, "degenerate: h = 1, n = 1"),
    (None, 60, 52, 136, 48, 40, "past the cap (forward: chunks of the window; backward: of the map)"),
]
# (rows, c, why): flat kernels (ELU on rows * c elements; copy / add of c channels between row widths lds, ldd)
FLAT_CASES = [
    (2 * 16 * 16, 64, "headline-like: a 16 x 16 x 64 map, batch 2"),
    (75, 24, "non-power-of-two row count, c = 24"),
    (1, 8, "degenerate: one chunk (two in fp32)"),
    (3, 136, "c = 136"),
    (None, 136, "past the cap"),
]
# (n, h, w, c, why): activate + global mean (no grid-stride loop: one thread per (image, channel) / per element)
MEAN_CASES = [
    (4, 4, 4, 256, "headline: the encoder's 4 x 4 x 256 map (batch cut)"),
    (2, 6, 5, 24, "non-power-of-two"),
    (3, 1, 1, 8, "degenerate: one pixel"),
    (1, 7, 1, 10, "n = 1, c = 10 (element-wise kernel: c need not be a multiple of 8)"),
    (2, 16, 16, 136, "256 pixels, c = 136"),
]
# (rows, c, ld, why): L1 feature distance over c logical of ld physical channels
L1_CASES = [
    (2 * 32 * 32, 64, 64, "headline-like: a 32 x 32 x 64 feature map, batch 2"),
    (75, 6, 8, "ragged: 6 of 8 channels"),
    (75, 13, 16, "ragged: 13 of 16"),
    (1, 8, 8, "degenerate: one row"),
    (7, 20, 24, "c = 20 of 24"),
    (None, 20, 24, "past the cap (backward) / many passes of the 1 024-block forward"),
]
# (pixels, ldx, why): VGG pre-processing of [pixels, ldx] images into [pixels, 8]
VGG_CASES = [
    (2 * 128 * 128, 8, "headline: 128 x 128 images in an 8-channel container (batch cut)"),
    (224 * 224, 3, "224 x 224, bare RGB"),
    (75, 5, "non-power-of-two, ldx = 5"),
    (1, 3, "degenerate: one pixel"),
    (300, 4, "ldx = 4, a partial last block"),
]
# (rows, c, ld, why): pad_convert of fp32 [rows, c] into [rows, ld]
PAD_CASES = [
    (2 * 128 * 128, 3, 8, "headline: RGB images into the 8-channel container (batch cut)"),
    (75, 10, 16, "c = 10 of 16"), (75, 8, 8, "no pad"), (5, 13, 24, "c = 13 of 24"), (1, 3, 8, "degenerate: one row"),
    (None, 13, 24, "past the cap (one thread per element of the result)"),
]


def _ids(cases):
    return ["{}:{}".format(i, c[-1].split(":")[0].replace(" ", "_")) for i, c in enumerate(cases)]


def _grid_n(case, dtype):
    n, h, w, c = case[:4]
    return n if n is not None else _past_cap(h * w * (c // ELEMS[dtype]))


# ----------------------------------------------------------------------------- bilinear x2
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", GRID_CASES, ids=_ids(GRID_CASES))
def test_bilinear(case, dtype, dev):
    """k: forward 4, plain and stored post-activation (three additions and the slope product; the halvings are exact);
    backward 9 (nine weighted terms, weights exact).  No f16 backward instance: gradients of fp16 tensors are bf16."""
    lib, _ = _mods()
    n, (h, w, c), code, tdt = _grid_n(case, dtype), case[1:4], _code(lib, dtype), TDT[dtype]
    big = case[0] is None
    x = _randn((n, h, w, c), dtype, dev, 1)

    def fwd():
        y = _nan((n, 2 * h, 2 * w, c), tdt, dev)
        lib.call("ups_bilinear2x_fwd", lib.ptr(x), lib.ptr(y), code, n, h, w, c, lib.stream())
        return y
    y = _twice(fwd)
    for lo, hi in _slices(n, big):
        xr = _hp(x[lo:hi], big)
        P.assert_rounds_once(_to(y[lo:hi], xr), P.bilinear_up2(xr), P.bilinear_up2(xr.abs()), tdt, 4, "bilinear fwd")
    for act, slope in ((lib.ACT_LRELU, SLOPE), (lib.ACT_RELU, 0.0)) if not big else ((lib.ACT_LRELU, SLOPE),):
        def fwd_act():
            ya = _nan((n, 2 * h, 2 * w, c), tdt, dev)
            lib.call("ups_bilinear2x_fwd_act", lib.ptr(x), lib.ptr(ya), code, n, h, w, c, act, SLOPE, lib.stream())
            return ya
        ya = _twice(fwd_act)
        for lo, hi in _slices(n, big):
            xr = _hp(x[lo:hi], big)
            P.assert_rounds_once(_to(ya[lo:hi], xr), P.act(P.bilinear_up2(xr), act, slope), P.bilinear_up2(xr.abs()), tdt, 4, "bilinear fwd_act")
    del y
    if dtype == "f16":
        return
    g = _randn((n, 2 * h, 2 * w, c), dtype, dev, 2)

    def bwd():
        gx = _nan((n, h, w, c), tdt, dev)
        lib.call("ups_bilinear2x_bwd", lib.ptr(g), lib.ptr(gx), code, n, h, w, c, lib.stream())
        return gx
    gx = _twice(bwd)
    for lo, hi in _slices(n, big):
        xr, gr = _hp(x[lo:hi], big), _hp(g[lo:hi], big)
        P.assert_rounds_once(_to(gx[lo:hi], xr), P.vjp(P.bilinear_up2, xr, gr), P.vjp(P.bilinear_up2, xr, gr.abs()), tdt, 9, "bilinear bwd")


# ----------------------------------------------------------------------------- nearest-neighbour x2
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", GRID_CASES, ids=_ids(GRID_CASES))
def test_nearest2x(case, dtype, dev):
    """Forward: a copy, bit-exact.  Backward (fp32, bf16: the launcher has no f16 instance): the sum of four, k = 4."""
    lib, _ = _mods()
    n, (h, w, c), code, tdt = _grid_n(case, dtype), case[1:4], _code(lib, dtype), TDT[dtype]
    big = case[0] is None
    x = _randn((n, h, w, c), dtype, dev, 3)

    def fwd():
        y = _nan((n, 2 * h, 2 * w, c), tdt, dev)
        lib.call("ups_nearest2x", lib.ptr(x), lib.ptr(y), code, n, h, w, c, 0, lib.stream())
        return y
    y = _twice(fwd)
    assert _same_bits(y, P.nearest2x(x if big else x.cpu()))
    del y
    if dtype == "f16":
        return
    g = _randn((n, 2 * h, 2 * w, c), dtype, dev, 4)

    def bwd():
        gx = _nan((n, h, w, c), tdt, dev)
        lib.call("ups_nearest2x", lib.ptr(g), lib.ptr(gx), code, n, h, w, c, 1, lib.stream())
        return gx
    gx = _twice(bwd)
    for lo, hi in _slices(n, big):
        xr, gr = _hp(x[lo:hi], big), _hp(g[lo:hi], big)
        P.assert_rounds_once(_to(gx[lo:hi], xr), P.vjp(P.nearest2x, xr, gr), P.sum_of_four(gr.abs()), tdt, 4, "nearest bwd")


# ----------------------------------------------------------------------------- depth to space
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", D2S_CASES, ids=_ids(D2S_CASES))
def test_depth_to_space(case, dtype, dev):
    """Both directions are copies: bit-exact, with exact zeros in the pad channels [C, ldy) forward and [4C, ldx) backward.  The pad
    channels of the INPUT hold random values: they must not reach the result."""
    lib, _ = _mods()
    n, h, w, C, extra = case[:5]
    ldx, ldy, code, tdt = (4 * C + 7) // 8 * 8 + extra, (C + 7) // 8 * 8, _code(lib, dtype), TDT[dtype]
    big = n is None
    if big:
        n = _past_cap(h * w * ldx)
        assert CAP < n * 4 * h * w * ldy < 2 * CAP        # (forward items; the backward's are checked by _past_cap)
    x = _randn((n, h, w, ldx), dtype, dev, 5)
    g = _randn((n, 2 * h, 2 * w, ldy), dtype, dev, 6)

    def fwd():
        y = _nan((n, 2 * h, 2 * w, ldy), tdt, dev)
        lib.call("ups_depth_to_space", lib.ptr(x), lib.ptr(y), code, n, h, w, C, ldx, ldy, 0, lib.stream())
        return y

    def bwd():
        gx = _nan((n, h, w, ldx), tdt, dev)
        lib.call("ups_depth_to_space", lib.ptr(g), lib.ptr(gx), code, n, h, w, C, ldx, ldy, 1, lib.stream())
        return gx
    y, gx = _twice(fwd), _twice(bwd)
    xs, gs = (x, g) if big else (x.cpu(), g.cpu())
    assert _same_bits(y, P.pad_channels(P.depth_to_space(xs, C), ldy)), "depth_to_space fwd"
    assert _same_bits(gx, P.pad_channels(P.space_to_depth(gs, C), ldx)), "depth_to_space bwd"
    if not big:         # the backward reference as autograd has it (values; the bits are held above)
        want = P.vjp(lambda t: P.pad_channels(P.depth_to_space(t, C), ldy), xs, gs)
        assert torch.equal(gx.cpu().double(), want)


# ----------------------------------------------------------------------------- crop
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", CROP_CASES, ids=_ids(CROP_CASES))
def test_crop(case, dtype, dev):
    """Copies: bit-exact, exact zeros outside the window backward.  The corner is a device tensor that is overwritten (device to
    device, same stream) between launches with no host synchronisation in between; out-of-range corners act as the clamped one.
    f16 moves through the bf16 instance (a copy of 16-bit words)."""
    lib, _ = _mods()
    n, h, w, c, ho, wo = case[:6]
    code, tdt = _code(lib, dtype), TDT[dtype]
    big = n is None
    if big:
        n = _past_cap(ho * wo * (c // ELEMS[dtype]))
        assert n * h * w * (c // ELEMS[dtype]) > CAP
    corners = [(0, 0), (h - ho, w - wo), ((h - ho) // 2, (w - wo + 1) // 2), (-3, 1), (1, -2), (h, w), (h - ho + 1, 0), (-(2 ** 31), 2 ** 31 - 1)]
    if big:
        corners = [((h - ho) // 2, (w - wo + 1) // 2), (h, -1)]
    corners_dev = torch.tensor(corners, dtype=torch.int32, device=dev)
    x = _randn((n, h, w, c), dtype, dev, 7)
    g = _randn((n, ho, wo, c), dtype, dev, 8)
    yx = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def run():
        outs = []
        for i in range(len(corners)):                   # no host sync inside this loop
            yx.copy_(corners_dev[i])
            y, gx = _nan((n, ho, wo, c), tdt, dev), _nan((n, h, w, c), tdt, dev)
            lib.call("ups_crop_fwd", lib.ptr(x), lib.ptr(y), code, n, h, w, c, ho, wo, lib.ptr(yx), lib.stream())
            lib.call("ups_crop_bwd", lib.ptr(g), lib.ptr(gx), code, n, h, w, c, ho, wo, lib.ptr(yx), lib.stream())
            outs += [y, gx]
        return tuple(outs)
    outs = _twice(run)
    xs, gs = (x, g) if big else (x.cpu(), g.cpu())
    for i, (y0, x0) in enumerate(corners):
        assert _same_bits(outs[2 * i], P.crop(xs, y0, x0, ho, wo).contiguous()), ("crop fwd", (y0, x0))
        assert _same_bits(outs[2 * i + 1], P.crop_inverse(gs, h, w, y0, x0)), ("crop bwd", (y0, x0))
    if not big:
        y0, x0 = corners[2]
        assert torch.equal(outs[5].cpu().double(), P.vjp(lambda t: P.crop(t, y0, x0, ho, wo), xs, gs))


# ----------------------------------------------------------------------------- 2x2 max pool
def _pool_launch(lib, x, g, code, dev):
    n, h, w, c = x.shape

    def run():
        y, gx = _nan((n, h // 2, w // 2, c), x.dtype, dev), _nan((n, h, w, c), x.dtype, dev)
        lib.call("ups_maxpool2_fwd", lib.ptr(x), lib.ptr(y), code, n, h, w, c, lib.stream())
        lib.call("ups_maxpool2_bwd", lib.ptr(x), lib.ptr(g), lib.ptr(gx), code, n, h, w, c, lib.stream())
        return y, gx
    return _twice(run)


def _pool_check(x, g, y, gx, big, bits=True):
    """Forward and routed gradient equal to the reference (bit for bit unless the windows mix +0.0 and -0.0, where either zero is a
    maximum); at most one non-zero per window; the window sums reproduce g bit for bit."""
    n = x.shape[0]
    for lo, hi in _slices(n, big):
        xs, gs = (x[lo:hi], g[lo:hi]) if big else (x[lo:hi].cpu(), g[lo:hi].cpu())
        yr = P.maxpool2(xs.float()).to(x.dtype)                     # (a maximum is one of its operands: no rounding)
        gr = P.maxpool2_grad(xs.double(), gs.double()).to(x.dtype)  # (a routed copy: no rounding)
        yg, gg = _to(y[lo:hi], xs), _to(gx[lo:hi], xs)
        if bits:
            assert _same_bits(yg, yr), "maxpool fwd"
        else:
            assert torch.equal(yg.double(), yr.double()), "maxpool fwd"
        assert _same_bits(gg, gr), "maxpool bwd"
        wg = P._windows(gg.float())
        assert int((wg != 0).sum(dim=-1).max()) <= 1, "more than one non-zero per window"
        assert _same_bits(wg.sum(dim=-1).to(x.dtype), gs), "window sums do not reproduce g"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_maxpool2(case, dtype, dev):
    lib, _ = _mods()
    n, (ho, wo, c) = _grid_n(case, dtype), case[1:4]
    big = case[0] is None
    x = _randn((n, 2 * ho, 2 * wo, c), dtype, dev, 9)
    g = _randn((n, ho, wo, c), dtype, dev, 10)
    y, gx = _pool_launch(lib, x, g, _code(lib, dtype), dev)
    _pool_check(x, g, y, gx, big)


def _tie_maps(kind, dtype):
    gen = torch.Generator().manual_seed(11)
    shape = (2, 12, 10, 24)
    if kind == "relu":                  # a sparse post-ReLU feature map: most windows are all zero
        x = torch.relu(torch.randn(shape, generator=gen) - 1.5)
    elif kind == "quantised":           # three values
        x = torch.randint(-1, 2, shape, generator=gen).float() * 0.25
    elif kind == "all_equal":
        x = torch.full(shape, 1.5)
    elif kind == "small":               # values a fraction of one bf16 step apart
        x = (torch.randn(shape, generator=gen) * 0.004 + 1.0).to(torch.bfloat16).float()
    elif kind == "signed_zeros":        # +0.0 and -0.0 (equal as numbers) next to negative values
        x = torch.where(torch.rand(shape, generator=gen) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        x = torch.where(torch.rand(shape, generator=gen) < 0.3, -torch.rand(shape, generator=gen), x)
    else:                               # all-negative windows, quantised so that they tie
        x = -(torch.randint(1, 4, shape, generator=gen).float() * 0.5)
    return x.to(TDT[dtype])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["relu", "quantised", "all_equal", "small", "signed_zeros", "negative"])
def test_maxpool2_ties(kind, dtype, dev):
    """Inputs built to tie: the gradient goes to the FIRST maximum in (0,0), (0,1), (1,0), (1,1) order."""
    lib, _ = _mods()
    x = _tie_maps(kind, dtype)
    tied, windows = P.tied_windows(x.double()), x.numel() // 4
    assert tied > windows // 2 if kind in ("relu", "all_equal", "signed_zeros") else tied > windows // 4, (kind, tied, windows)
    g = _randn((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3]), dtype, dev, 12)
    xd = x.to(dev)
    y, gx = _pool_launch(lib, xd, g, _code(lib, dtype), dev)
    _pool_check(xd, g, y, gx, False, bits=kind != "signed_zeros")


@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_maxpool2_fwd_f8(case, act, dev):
    """The pool as an fp8 producer (as test_bilinear_fp8_copies; bf16 only), an instance of its own with its own store path: at every
    pool shape -- the trunk's, 1 x 1 outputs, n = 1, past the cap (second-pass byte offsets, 16 384 blocks on 64 maximum slots) -- the
    bf16 result is that of ups_maxpool2_fwd, the bytes are e4m3(act(y) * scale), the recorded maximum is max |act(y)|, and the
    maxima-only call (y_f8 = NULL) leaves the same y.  The byte and maximum references are torch's, on the device."""
    lib, _ = _mods()
    n, h, w, c = _grid_n(case, "bf16"), 2 * case[1], 2 * case[2], case[3]
    code = {"none": lib.ACT_NONE, "relu": lib.ACT_RELU, "lrelu": lib.ACT_LRELU}[act]
    x = _randn((n, h, w, c), "bf16", dev, 13, scale=2.0)
    scale = torch.tensor([37.5], dtype=torch.float32, device=dev)
    y_ref = _nan((n, h // 2, w // 2, c), torch.bfloat16, dev)
    lib.call("ups_maxpool2_fwd", lib.ptr(x), lib.ptr(y_ref), lib.BF16, n, h, w, c, lib.stream())

    def run(with_bytes):
        def fn():
            y, y8 = _nan(y_ref.shape, torch.bfloat16, dev), _nan(y_ref.shape, torch.uint8, dev)
            amax = torch.zeros(64, dtype=torch.float32, device=dev)
            lib.call("ups_maxpool2_fwd_f8", lib.ptr(x), lib.ptr(y), n, h, w, c, lib.ptr(y8) if with_bytes else None, lib.ptr(scale),
                     lib.ptr(amax), code, SLOPE, lib.stream())
            return y, y8, amax.max().reshape(1)
        return fn
    y, y8, amax = _twice(run(True))
    y0, y80, amax0 = _twice(run(False))
    assert _same_bits(y, y_ref) and _same_bits(y0, y_ref)
    yf = y_ref.float()
    ya = yf if act == "none" else torch.maximum(yf, (SLOPE if act == "lrelu" else 0.0) * yf)      # the kernel's max(v, slope_eff * v)
    assert float(amax) == float(ya.abs().max()) and float(amax0) == float(amax)
    assert torch.equal(y8, (ya * scale).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    assert int(y80.min()) == 255, "the maxima-only call wrote fp8 bytes"


# ----------------------------------------------------------------------------- activate + global mean
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("act", ["none", "lrelu", "relu"])
@pytest.mark.parametrize("case", MEAN_CASES, ids=_ids(MEAN_CASES))
def test_act_mean(case, act, dtype, dev):
    """k: forward hw (hw additions from 0.f, the first one exact: that leaves room for the slope product and the division); backward 2
    (g / hw, times act')."""
    lib, _ = _mods()
    n, h, w, c = case[:4]
    code, tdt = _code(lib, dtype), TDT[dtype]
    kind = {"none": P.ACT_NONE, "lrelu": P.ACT_LRELU, "relu": P.ACT_RELU}[act]
    x = _randn((n, h, w, c), dtype, dev, 14)
    g = _randn((n, 1, 1, c), dtype, dev, 15)

    def run():
        y, gx = _nan((n, 1, 1, c), tdt, dev), _nan((n, h, w, c), tdt, dev)
        lib.call("ups_act_mean_fwd", lib.ptr(x), lib.ptr(y), code, n, h * w, c, kind, SLOPE, lib.stream())
        lib.call("ups_act_mean_bwd", lib.ptr(x), lib.ptr(g), lib.ptr(gx), code, n, h * w, c, kind, SLOPE, lib.stream())
        return y, gx
    y, gx = _twice(run)
    xr, gr = x.cpu().double(), g.cpu().double()
    P.assert_rounds_once(y.cpu(), P.act_mean(xr, kind, SLOPE), P.act_mean(xr.abs(), P.ACT_NONE), tdt, h * w, "act_mean fwd")
    ref = P.vjp(lambda t: P.act_mean(t, kind, SLOPE), xr, gr)
    P.assert_rounds_once(gx.cpu(), ref, ref.abs(), tdt, 2, "act_mean bwd")


# ----------------------------------------------------------------------------- ELU
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", FLAT_CASES, ids=_ids(FLAT_CASES))
def test_elu(case, dtype, dev):
    """k = 4 for expm1f / expf (and the product with g backward)."""
    lib, _ = _mods()
    rows, c = case[:2]
    big = rows is None
    if big:
        rows = _past_cap(c // ELEMS[dtype])
    code, tdt, cnt = _code(lib, dtype), TDT[dtype], rows * c
    x = _randn((rows, c), dtype, dev, 16, scale=2.0)
    g = _randn((rows, c), dtype, dev, 17)

    def run():
        y, gx = _nan((rows, c), tdt, dev), _nan((rows, c), tdt, dev)
        lib.call("ups_elu_fwd", lib.ptr(x), lib.ptr(y), code, cnt, lib.stream())
        lib.call("ups_elu_bwd", lib.ptr(x), lib.ptr(g), lib.ptr(gx), code, cnt, lib.stream())
        return y, gx
    y, gx = _twice(run)
    for lo, hi in _slices(rows, big):
        xr, gr = _hp(x[lo:hi], big), _hp(g[lo:hi], big)
        ref = P.elu(xr)
        P.assert_rounds_once(_to(y[lo:hi], xr), ref, ref.abs(), tdt, 4, "elu fwd")
        ref = P.vjp(P.elu, xr, gr)
        P.assert_rounds_once(_to(gx[lo:hi], xr), ref, ref.abs(), tdt, 4, "elu bwd")


# ----------------------------------------------------------------------------- channel copy / add (ABI surface: no Python caller)
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", FLAT_CASES, ids=_ids(FLAT_CASES))
def test_copy_and_add_channels(case, dtype, dev):
    """c channels of rows of width lds into rows of width ldd.  copy: bit-exact (f16: through the bf16 instance, a copy of 16-bit
    words); add (fp32, bf16): k = 1.  The columns [c, ldd) of the destination keep the bits they had."""
    lib, _ = _mods()
    rows, c = case[:2]
    big = rows is None
    if big:
        rows = _past_cap(c // ELEMS[dtype])
    lds, ldd, code, tdt = c + 8, c + 16, _code(lib, dtype), TDT[dtype]
    src = _randn((rows, lds), dtype, dev, 18)
    dst0 = _randn((rows, ldd), dtype, dev, 19)

    def copy():
        d = _nan((rows, ldd), tdt, dev)
        lib.call("ups_copy_channels", lib.ptr(src), lds, lib.ptr(d), ldd, code, rows, c, lib.stream())
        return d
    d = _twice(copy)
    assert _same_bits(d[:, :c], src[:, :c]) and int(_bits(d[:, c:]).max()) == -1 and int(_bits(d[:, c:]).min()) == -1
    if dtype == "f16":
        return

    def add():
        d = dst0.clone()
        lib.call("ups_add_channels", lib.ptr(src), lds, lib.ptr(d), ldd, code, rows, c, lib.stream())
        return d
    d = _twice(add)
    assert _same_bits(d[:, c:], dst0[:, c:])
    for lo, hi in _slices(rows, big):
        a, b = _hp(src[lo:hi, :c], big), _hp(dst0[lo:hi, :c], big)
        P.assert_rounds_once(_to(d[lo:hi, :c], a), a + b, a.abs() + b.abs(), tdt, 1, "add_channels")


# ----------------------------------------------------------------------------- dtype conversion
CONVERT_PAIRS = [("fp32", "bf16"), ("bf16", "fp32"), ("fp32", "fp32"), ("fp32", "f16"), ("f16", "fp32"), ("bf16", "bf16"), ("f16", "bf16")]
CONVERT_COUNTS = [(2 * 128 * 128 * 8, "headline-like: an image batch in the 8-channel container"), (1000, "not a power of two"),
                  (1, "degenerate: one element"), (7, "odd count"), (CAP + 1234567, "past the cap (one thread per element)")]


@pytest.mark.parametrize("pair", CONVERT_PAIRS, ids=["{}_to_{}".format(*p) for p in CONVERT_PAIRS])
@pytest.mark.parametrize("case", CONVERT_COUNTS, ids=_ids(CONVERT_COUNTS))
def test_convert(case, pair, dev):
    """Equal types and widening conversions are bit-exact; narrowing ones round once (k = 0)."""
    lib, _ = _mods()
    cnt, (sd, dd) = case[0], pair
    big = _is_big(cnt)
    x = _randn((cnt,), sd, dev, 20)

    def run():
        y = _nan((cnt,), TDT[dd], dev)
        lib.call("ups_convert", lib.ptr(x), _code(lib, sd), lib.ptr(y), _code(lib, dd), cnt, lib.stream())
        return y
    y = _twice(run)
    if sd == dd or dd == "fp32":
        assert _same_bits(y, x.to(TDT[dd]))                     # (16 -> 32 bit is exact in any implementation)
    else:
        xr = _hp(x, big)
        P.assert_rounds_once(_to(y, xr), xr, xr.abs(), TDT[dd], 0, "convert {} -> {}".format(sd, dd))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("case", PAD_CASES, ids=_ids(PAD_CASES))
def test_pad_convert(case, dtype, dev):
    """fp32 [rows, c] into [rows, ld]: to fp32 bit-exact, to 16 bit rounded once (k = 0); the pad channels exactly zero."""
    lib, _ = _mods()
    rows, c, ld = case[:3]
    big = rows is None
    if big:
        rows = _past_cap(ld)
    tdt = TDT[dtype]
    x = _randn((rows, c), "fp32", dev, 21)

    def run():
        y = _nan((rows, ld), tdt, dev)
        lib.call("ups_pad_convert", lib.ptr(x), c, lib.ptr(y), _code(lib, dtype), ld, rows, lib.stream())
        return y
    y = _twice(run)
    assert int((_bits(y[:, c:]) != 0).sum()) == 0, "pad channels are not +0.0"
    if dtype == "fp32":
        assert _same_bits(y[:, :c], x)
    else:
        xr = _hp(x, big)
        P.assert_rounds_once(_to(y[:, :c], xr), xr, xr.abs(), tdt, 0, "pad_convert")
    if not big:
        assert torch.equal(y.cpu().double(), P.pad_convert(y[:, :c].cpu().double(), ld))


# ----------------------------------------------------------------------------- VGG pre-processing
@pytest.mark.parametrize("form", ["fp32", "bf16", "fp32_to_bf16"])
@pytest.mark.parametrize("case", VGG_CASES, ids=_ids(VGG_CASES))
def test_vgg_preprocess(case, form, dev):
    """k: forward 4 (add, multiply, subtract, and the mean as a C float); backward 1.  Pad channels exactly zero: [3, 8) forward,
    [3, ldx) backward.  Input pad channels hold random values."""
    lib, _ = _mods()
    pixels, ldx = case[:2]
    xdt, ydt = ("fp32" if form != "bf16" else "bf16"), ("fp32" if form == "fp32" else "bf16")
    gen = torch.Generator().manual_seed(22)
    x = (torch.rand((pixels, ldx), generator=gen) * 2 - 1).to(TDT[xdt]).to(dev)

    def fwd():
        y = _nan((pixels, 8), TDT[ydt], dev)
        lib.call("ups_vgg_preprocess_fwd", lib.ptr(x), int(xdt == "fp32"), ldx, lib.ptr(y), _code(lib, ydt), pixels, lib.stream())
        return y
    y = _twice(fwd)
    xr = x.cpu().double()
    S = P.pad_channels(torch.flip((xr[..., :3].abs() + 1.0) * 127.5, dims=[-1]) + torch.tensor(P.VGG_BGR_MEAN, dtype=torch.float64), 8)
    P.assert_rounds_once(y.cpu(), P.vgg_preprocess(xr), S, TDT[ydt], 4, "vgg fwd")
    assert int((_bits(y[:, 3:]) != 0).sum()) == 0
    if form == "fp32_to_bf16":
        return                  # (the gradient flows back to an activation-dtype image: VggPreFn asserts it)
    g = _randn((pixels, 8), ydt, dev, 23)

    def bwd():
        gx = _nan((pixels, ldx), TDT[ydt], dev)
        lib.call("ups_vgg_preprocess_bwd", lib.ptr(g), lib.ptr(gx), _code(lib, ydt), ldx, pixels, lib.stream())
        return gx
    gx = _twice(bwd)
    ref = P.vjp(P.vgg_preprocess, xr, g.cpu().double())
    P.assert_rounds_once(gx.cpu(), ref, ref.abs(), TDT[ydt], 1, "vgg bwd")
    assert int((_bits(gx[:, 3:]) != 0).sum()) == 0


# ----------------------------------------------------------------------------- L1 feature distance
L1_BLOCKS = 1024


def _l1_sum_k(chunks, E, blocks):
    """fp32 operations on the longest path to the L1 sum (see test_l1)."""
    return E * -(-chunks // (blocks * 256)) + 1 + 8 + -(-blocks // 256) + 8 + 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_l1_forward_every_block_loops(dtype, dev):
    """The grid-stride loop of l1_fwd_kernel with a bound that would notice a dropped or misplaced pass: 2^22 logical terms (c = 20
    of ld = 24) on 8 blocks, so that every thread makes ~100 passes; k = _l1_sum_k, about 1e-4 of S in bf16.  The partial sums of
    the blocks are held to the same bound one by one (block b owns the chunks b * 256 + t + 2048 j)."""
    lib, _ = _mods()
    E, blocks, c, ld = ELEMS[dtype], 8, 20, 24
    rows = (1 << 22) // c + 3
    a, b = _randn((rows, ld), dtype, dev, 34), _randn((rows, ld), dtype, dev, 35)

    def run():
        partial, out = _nan((blocks,), torch.float32, dev), _nan((1,), torch.float32, dev)
        lib.call("ups_l1_fwd", lib.ptr(a), lib.ptr(b), _code(lib, dtype), rows, c, ld, P.ACT_RELU, lib.ptr(partial), blocks, lib.stream())
        lib.call("ups_sum_scale", lib.ptr(partial), blocks, 1.0 / (rows * c), lib.ptr(out), 0, lib.stream())
        return partial, out
    partial, out = _twice(run)
    ar, br = a.double(), b.double()                  # (2^22 terms: the fp64 restatement runs on the device)
    k = _l1_sum_k(rows * (ld // E), E, blocks)
    assert k * 2.0 ** -23 < 1e-3
    ref = P.l1_mean(ar, br, c, P.ACT_RELU).reshape(1)
    S = (ar[..., :c].abs() + br[..., :c].abs()).mean().reshape(1)
    P.assert_rounds_once(out, ref, S, torch.float32, k, "l1 fwd on 8 blocks")
    mask = (torch.arange(ld, device=dev) < c).double()
    terms = ((torch.relu(ar) - torch.relu(br)).abs() * mask).reshape(-1, E).sum(dim=1)           # one value per chunk
    sizes = ((ar.abs() + br.abs()) * mask).reshape(-1, E).sum(dim=1)
    owner = (torch.arange(terms.numel(), device=dev) // 256) % blocks
    zero = torch.zeros(blocks, dtype=torch.float64, device=dev)
    P.assert_rounds_once(partial, zero.index_add(0, owner, terms), zero.index_add(0, owner, sizes), torch.float32, k, "l1 partial sums")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("case", L1_CASES, ids=_ids(L1_CASES))
def test_l1(case, act, dtype, dev):
    """k: the sum rows * c; the gradient 2 (1 / (rows c) as a C float, times the device scalar).  rows * c bounds a serial sum and says
    nothing once rows * c 2^-23 passes 1 (the past-the-cap case), so the sum is also held to the bound of the order it is actually
    taken in: every thread adds its own terms serially (ceil(chunks / threads) chunks of E terms, each term one subtraction), then
    a tree over the 256 threads of a block (8 levels), ups_sum_scale's serial pass over the partials per thread and its tree (8), the
    scale: k = E * ceil(chunks / (blocks * 256)) + 1 + 8 + ceil(blocks / 256) + 8 + 1 (_l1_sum_k), in units of 2^-23 = 2 u.
    The pad channels [c, ld) hold random values in both operands: they must not reach the sum, and their gradient is exactly zero."""
    lib, _ = _mods()
    rows, c, ld = case[:3]
    big = rows is None
    if big:
        rows = _past_cap(ld // ELEMS[dtype])
    code, tdt = _code(lib, dtype), TDT[dtype]
    kind = {"none": P.ACT_NONE, "relu": P.ACT_RELU}[act]
    a, b = _randn((rows, ld), dtype, dev, 24), _randn((rows, ld), dtype, dev, 25)
    gscale = torch.tensor([3.0], dtype=torch.float32, device=dev)

    def run():
        partial, out, gb = _nan((L1_BLOCKS,), torch.float32, dev), _nan((1,), torch.float32, dev), _nan((rows, ld), tdt, dev)
        lib.call("ups_l1_fwd", lib.ptr(a), lib.ptr(b), code, rows, c, ld, kind, lib.ptr(partial), L1_BLOCKS, lib.stream())
        lib.call("ups_sum_scale", lib.ptr(partial), L1_BLOCKS, 1.0 / (rows * c), lib.ptr(out), 0, lib.stream())
        lib.call("ups_l1_bwd", lib.ptr(a), lib.ptr(b), lib.ptr(gb), code, rows, c, ld, kind, lib.ptr(gscale), 1.0 / (rows * c), lib.stream())
        return out, gb
    out, gb = _twice(run)
    ar, br = _hp(a, big), _hp(b, big)
    ref = P.l1_mean(ar, br, c, kind).reshape(1)
    S = (ar[..., :c].abs() + br[..., :c].abs()).mean().reshape(1)
    P.assert_rounds_once(_to(out, ref), ref, S, torch.float32, rows * c, "l1 fwd")
    P.assert_rounds_once(_to(out, ref), ref, S, torch.float32, _l1_sum_k(rows * (ld // ELEMS[dtype]), ELEMS[dtype], L1_BLOCKS), "l1 fwd, summation order")
    for lo, hi in _slices(rows, big):
        ref = P.l1_mean_grad(ar[lo:hi], br[lo:hi], c, kind, scale=3.0) * ((hi - lo) / rows)         # (the slice's rows -> all rows)
        P.assert_rounds_once(_to(gb[lo:hi], ref), ref, ref.abs(), tdt, 2, "l1 bwd")
    assert int((_bits(gb[:, c:]) != 0).sum()) == 0, "pad channels of the gradient are not +0.0"
    if not big:
        want = P.vjp(lambda t: 3.0 * P.l1_mean(ar, t, c, kind), br, torch.tensor(1.0, dtype=torch.float64))
        assert torch.allclose(P.l1_mean_grad(ar, br, c, kind, scale=3.0), want, rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------- the ops.*Fn wrappers reach the same kernels
def test_wrappers_give_the_kernels_results(dev):
    lib, ops = _mods()
    x = _randn((2, 6, 8, 24), "bf16", dev, 26)
    n, h, w, c = x.shape

    def grad(y, xr, seed):
        g = _randn(tuple(y.shape), "bf16", dev, seed)
        return g, torch.autograd.grad([y], [xr], grad_outputs=[g])[0]

    def raw(name, shape, *args):
        out = _nan(shape, torch.bfloat16, dev)
        lib.call(name, *[lib.ptr(out) if a is Ellipsis else a for a in args], lib.stream())
        return out
    xr = x.clone().requires_grad_(True)
    y = ops.BilinearFn.apply(xr)
    assert _same_bits(y.detach(), raw("ups_bilinear2x_fwd", (n, 2 * h, 2 * w, c), lib.ptr(x), ..., lib.BF16, n, h, w, c))
    g, gx = grad(y, xr, 27)
    assert _same_bits(gx, raw("ups_bilinear2x_bwd", (n, h, w, c), lib.ptr(g), ..., lib.BF16, n, h, w, c))
    y = ops.Nearest2xFn.apply(xr)
    assert _same_bits(y.detach(), P.nearest2x(x))
    g, gx = grad(y, xr, 28)
    assert _same_bits(gx, raw("ups_nearest2x", (n, h, w, c), lib.ptr(g), ..., lib.BF16, n, h, w, c, 1))
    y = ops.DepthToSpaceFn.apply(xr, 5)                         # 20 of 24 channels -> 5 of 8
    assert _same_bits(y.detach(), P.pad_channels(P.depth_to_space(x, 5), 8))
    g, gx = grad(y, xr, 29)
    assert _same_bits(gx, P.pad_channels(P.space_to_depth(g, 5), 24))
    yx = torch.tensor([2, 10], dtype=torch.int32, device=dev)  # (the column is out of range: clamps to 8 - 3)
    y = ops.CropFn.apply(xr, yx, 3, 3)
    assert _same_bits(y.detach(), P.crop(x, 2, 10, 3, 3).contiguous())
    g, gx = grad(y, xr, 30)
    assert _same_bits(gx, P.crop_inverse(g, h, w, 2, 10))
    y = ops.MaxPoolFn.apply(xr)
    assert _same_bits(y.detach(), P.maxpool2(x.float()).to(torch.bfloat16))
    g, gx = grad(y, xr, 31)
    assert _same_bits(gx, P.maxpool2_grad(x.double(), g.double()).to(torch.bfloat16))
    y = ops.EluFn.apply(xr)
    assert _same_bits(y.detach(), raw("ups_elu_fwd", x.shape, lib.ptr(x), ..., lib.BF16, x.numel()))
    g, gx = grad(y, xr, 32)
    assert _same_bits(gx, raw("ups_elu_bwd", x.shape, lib.ptr(x), lib.ptr(g), ..., lib.BF16, x.numel()))
    y = ops.ActMeanFn.apply(xr, lib.ACT_LRELU, 0.2)
    assert _same_bits(y.detach(), raw("ups_act_mean_fwd", (n, 1, 1, c), lib.ptr(x), ..., lib.BF16, n, h * w, c, lib.ACT_LRELU, 0.2))
    g, gx = grad(y, xr, 33)
    assert _same_bits(gx, raw("ups_act_mean_bwd", x.shape, lib.ptr(x), lib.ptr(g), ..., lib.BF16, n, h * w, c, lib.ACT_LRELU, 0.2))


# ----------------------------------------------------------------------------- dtype codes
def _dtype_entries(lib, dev):
    """name -> (launch(code) returning the output viewed as fp16, fp64 reference on the fp16 data, S, k).  Every buffer is an fp16
    tensor of TWICE the element count the call names, fully allocated: a launcher that wrongly accepts a code runs in bounds whatever
    element size it assumes."""
    n, h, w, c = 2, 4, 4, 8
    f16 = torch.float16

    def buf(shape, seed=None):
        numel = int(np.prod(shape))
        t = _nan((2 * numel,), f16, dev)
        if seed is not None:
            t[:numel] = _randn((numel,), "f16", dev, seed)
        return t

    def view(t, shape):
        return t[:int(np.prod(shape))].reshape(shape)
    X, G2, G1 = buf((n, h, w, c), 40), buf((n, 2 * h, 2 * w, c), 41), buf((n, 1, 1, c), 42)
    x, g2, g1 = view(X, (n, h, w, c)).cpu().double(), view(G2, (n, 2 * h, 2 * w, c)).cpu().double(), view(G1, (n, 1, 1, c)).cpu().double()
    B = buf((n, h, w, c), 43)
    b = view(B, (n, h, w, c)).cpu().double()
    yx = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    XF = torch.zeros(2 * n * h * w * c, dtype=torch.float32, device=dev)
    XF[:n * h * w * c] = view(X, (n * h * w * c,)).float()
    one = torch.ones(1, dtype=torch.float32, device=dev)
    up, same, half, pix = (n, 2 * h, 2 * w, c), (n, h, w, c), (n, h // 2, w // 2, c), n * h * w
    E = {}

    def entry(name, shape, args, ref, S=None, k=0):
        def launch(code):
            out = buf(shape)
            lib.call(name.split("@")[0], *[lib.ptr(out) if a is Ellipsis else (code if a == "dtype" else a) for a in args], lib.stream())
            torch.cuda.synchronize()
            return view(out, shape).cpu()
        E[name] = (launch, ref, ref.abs() if S is None else S, k)
    P_ = lib.ptr
    entry("ups_bilinear2x_fwd", up, [P_(X), ..., "dtype", n, h, w, c], P.bilinear_up2(x), P.bilinear_up2(x.abs()), 4)
    entry("ups_bilinear2x_fwd_act", up, [P_(X), ..., "dtype", n, h, w, c, lib.ACT_RELU, 0.0], P.act(P.bilinear_up2(x), P.ACT_RELU), P.bilinear_up2(x.abs()), 4)
    entry("ups_bilinear2x_bwd", same, [P_(G2), ..., "dtype", n, h, w, c], P.vjp(P.bilinear_up2, x, g2), P.vjp(P.bilinear_up2, x, g2.abs()), 9)
    sign = buf((n, 2 * h, 2 * w, c // 8))
    entry("ups_bilinear2x_fwd_bits", up, [P_(X), ..., "dtype", n, h, w, c, lib.ACT_NONE, 0.0, P_(sign)], P.bilinear_up2(x), P.bilinear_up2(x.abs()), 4)
    entry("ups_depth_to_space@fwd", (n, 2 * h, 2 * w, 8), [P_(X), ..., "dtype", n, h, w, 2, c, 8, 0], P.pad_channels(P.depth_to_space(x, 2), 8))
    entry("ups_depth_to_space@bwd", same, [P_(G2), ..., "dtype", n, h, w, 2, c, 8, 1], P.space_to_depth(g2, 2))
    entry("ups_nearest2x@fwd", up, [P_(X), ..., "dtype", n, h, w, c, 0], P.nearest2x(x))
    entry("ups_nearest2x@bwd", same, [P_(G2), ..., "dtype", n, h, w, c, 1], P.sum_of_four(g2), P.sum_of_four(g2.abs()), 4)
    entry("ups_crop_fwd", (n, 2, 2, c), [P_(X), ..., "dtype", n, h, w, c, 2, 2, P_(yx)], P.crop(x, 1, 1, 2, 2))
    entry("ups_crop_bwd", up, [P_(X), ..., "dtype", n, 2 * h, 2 * w, c, h, w, P_(yx)], P.crop_inverse(x, 2 * h, 2 * w, 1, 1))
    entry("ups_act_mean_fwd", (n, 1, 1, c), [P_(X), ..., "dtype", n, h * w, c, lib.ACT_RELU, 0.0], P.act_mean(x, P.ACT_RELU), P.act_mean(x.abs(), P.ACT_NONE), h * w)
    entry("ups_act_mean_bwd", same, [P_(X), P_(G1), ..., "dtype", n, h * w, c, lib.ACT_RELU, 0.0], P.vjp(lambda t: P.act_mean(t, P.ACT_RELU), x, g1), None, 2)
    entry("ups_elu_fwd", same, [P_(X), ..., "dtype", n * h * w * c], P.elu(x), None, 4)
    entry("ups_elu_bwd", same, [P_(X), P_(B), ..., "dtype", n * h * w * c], P.vjp(P.elu, x, b), None, 4)
    entry("ups_maxpool2_fwd", half, [P_(X), ..., "dtype", n, h, w, c], P.maxpool2(x))
    entry("ups_maxpool2_bwd", same, [P_(X), P_(G2), ..., "dtype", n, h, w, c], P.maxpool2_grad(x, view(G2, half).cpu().double()))
    entry("ups_copy_channels", same, [P_(X), c, ..., c, "dtype", pix, c], x)
    entry("ups_vgg_preprocess_fwd", same, [P_(X), 0, c, ..., "dtype", pix], P.vgg_preprocess(x.clamp(-1, 1)))
    entry("ups_vgg_preprocess_bwd", same, [P_(X), ..., "dtype", c, pix], P.vjp(P.vgg_preprocess, x, x), None, 1)
    entry("ups_l1_bwd", same, [P_(X), P_(B), ..., "dtype", pix, c, c, lib.ACT_NONE, P_(one), 1.0], P.l1_mean_grad(x, b, c, P.ACT_NONE, scale=float(pix * c)), None, 2)
    entry("ups_pad_convert", same, [P_(XF), c, ..., "dtype", c, pix], x)

    # launchers whose result is not one tensor of the dtype: their own launch / reference pairs
    def add_channels(code):
        out = buf(same)
        out[:x.numel()] = view(B, (x.numel(),))
        lib.call("ups_add_channels", P_(X), c, P_(out), c, code, pix, c, lib.stream())
        torch.cuda.synchronize()
        return view(out, same).cpu()
    E["ups_add_channels"] = (add_channels, x + b, x.abs() + b.abs(), 1)

    def l1_fwd(code):
        partial = _nan((2 * L1_BLOCKS,), torch.float32, dev)
        lib.call("ups_l1_fwd", P_(X), P_(B), code, pix, c, c, lib.ACT_NONE, P_(partial), L1_BLOCKS, lib.stream())
        torch.cuda.synchronize()
        return partial[:L1_BLOCKS].cpu().double().sum().reshape(1).to(torch.float32)
    E["ups_l1_fwd"] = (l1_fwd, (x - b).abs().sum().reshape(1), (x.abs() + b.abs()).sum().reshape(1), pix * c)

    def sign_pack(code):
        out = _nan((2 * pix,), torch.uint8, dev)
        lib.call("ups_sign_pack", P_(X), code, pix, P_(out), lib.stream())
        torch.cuda.synchronize()
        return out[:pix].cpu().double()
    signs = ((x > 0).reshape(pix, 8).double() * (2.0 ** torch.arange(8, dtype=torch.float64))).sum(dim=1)        # bit e = element e > 0
    E["ups_sign_pack"] = (sign_pack, signs, signs, 0)
    return E, [X, G2, G1, B, yx, XF, one, sign]          # (the launch lists hold raw pointers: the caller keeps the tensors alive)


DTYPE_LAUNCHERS = ["ups_bilinear2x_fwd", "ups_bilinear2x_fwd_act", "ups_bilinear2x_bwd", "ups_bilinear2x_fwd_bits", "ups_depth_to_space@fwd",
                   "ups_depth_to_space@bwd", "ups_nearest2x@fwd", "ups_nearest2x@bwd", "ups_crop_fwd", "ups_crop_bwd", "ups_act_mean_fwd",
                   "ups_act_mean_bwd", "ups_elu_fwd", "ups_elu_bwd", "ups_maxpool2_fwd", "ups_maxpool2_bwd", "ups_copy_channels",
                   "ups_add_channels", "ups_vgg_preprocess_fwd", "ups_vgg_preprocess_bwd", "ups_l1_fwd", "ups_l1_bwd", "ups_pad_convert",
                   "ups_sign_pack"]


# what each launcher does with UPS_F16 (docs/design/kernels.md, "The dtype contract of the streaming launchers")
F16_COMPUTES = {"ups_bilinear2x_fwd", "ups_bilinear2x_fwd_act", "ups_bilinear2x_fwd_bits", "ups_depth_to_space@fwd", "ups_depth_to_space@bwd",
                "ups_nearest2x@fwd", "ups_crop_fwd", "ups_crop_bwd", "ups_elu_fwd", "ups_elu_bwd", "ups_copy_channels", "ups_pad_convert",
                "ups_sign_pack"}


@pytest.fixture(scope="module")
def dtype_entries(dev):
    """The launch table and the tensors its raw pointers point into, built once and kept alive for the module."""
    lib, _ = _mods()
    return _dtype_entries(lib, dev)


@pytest.mark.parametrize("name", DTYPE_LAUNCHERS)
def test_dtype_codes(name, dev, dtype_entries):
    """Every launcher of pointwise.hip that takes a dtype code: with UPS_F16 on fp16 data it either computes the operation (the fp64
    reference on that data, at the operation's own bound) or refuses; an undefined code (7) is refused.  It never runs another type's
    arithmetic on the bits and reports success."""
    lib, _ = _mods()
    entries, _alive = dtype_entries
    assert sorted(entries) == sorted(DTYPE_LAUNCHERS)
    launch, ref, S, k = entries[name]
    try:
        got = launch(lib.F16)
    except lib.UpsError:
        got = None
    assert (got is not None) == (name in F16_COMPUTES), "the launcher's answer to UPS_F16 is not the documented one"
    if got is not None:
        assert got.shape == ref.shape, (got.shape, ref.shape)
        P.assert_rounds_once(got, ref, S, torch.float16, k, name + " with UPS_F16")
    with pytest.raises(lib.UpsError):
        launch(7)


def test_convert_refuses_undefined_codes(dev):
    lib, _ = _mods()
    x, y = torch.zeros(64, dtype=torch.float32, device=dev), torch.zeros(64, dtype=torch.float32, device=dev)
    for sd, dd in [(7, lib.F32), (lib.F32, 7), (lib.BF16, lib.F16), (lib.F16, lib.F16)]:      # (the last two: no instance)
        with pytest.raises(lib.UpsError):
            lib.call("ups_convert", lib.ptr(x), sd, lib.ptr(y), dd, 16, lib.stream())
