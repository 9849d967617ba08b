"""Bit-exact parity of the 16-bit and fp32 convolution kernels on lattice inputs (tests/exact_ref.py).

All operands are small integers (leaky ReLU at slope 0.25, CoordConv on maps of 2^k + 1 pixels), so every product and every partial
sum is exact in the fp32 accumulator whatever the order, the split or the tile: each kernel family must produce the bits of the
integer reference rounded once to the stored type, and all families the same bits as each other.  There is no tolerance anywhere
in this file: one dropped or duplicated product, one wrong lane, tap, chunk or halo pixel changes an integer.  The headroom
condition (sum of |products| < 2^24 LSBs) is asserted before anything is launched.  docs/design/parity_ledger.md has the table of
kernel instance -> case."""
import pytest
import torch

import exact_ref as E

pytestmark = pytest.mark.gpu


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _ff(shape, dtype, dev):
    """A caller buffer pre-filled with 0xFF bytes (NaN in every float type): an element the kernel does not write shows."""
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _layer(case, V, b, dev, f16=False):
    lib, ops = _mods()
    lay = ops.ConvLayer("exact/conv2d_0", V.float().to(dev).requires_grad_(True), b.float().to(dev).requires_grad_(True), case.k,
                        case.stride, case.coords, case.act, slope=E.SLOPE)
    lay.in_post = case.in_post
    lay.out_act = lib.ACT_LRELU if case.out_act else lib.ACT_NONE
    lay.f16 = f16
    lay.grad_V, lay.grad_b = _ff(lay.V.shape, torch.float32, dev), _ff(lay.b.shape, torch.float32, dev)
    return lay


def _to_dev(t, dtype, dev):
    """A lattice tensor in the storage the kernels read: fp16 lives in bf16 containers."""
    if dtype == "f16":
        return t.to(torch.float16).to(dev).view(torch.bfloat16)
    return t.to(E.TORCH_T[dtype]).to(dev)


def _host(t, dtype):
    t = t.detach().cpu()
    return t.view(torch.float16) if (dtype == "f16" and t.dtype == torch.bfloat16) else t


def _same(got, want, what, axes=None):
    msg = E.first_diff(got, want, axes)
    assert msg is None, "{}: {}".format(what, msg)


def _check_out(y, ref_y, dtype, cout, what):
    """Channels [0, cout) hold the reference's bits; the padding channels [cout, round8(cout)) are exactly zero."""
    y = _host(y, dtype)
    _same(y[..., :cout].contiguous(), E.rounded(ref_y, y.dtype), what)
    if y.shape[-1] > cout:
        pad = y[..., cout:].contiguous()
        _same(pad, torch.zeros_like(pad), what + " (padding channels)")


def _start(case):
    inputs, ref, hr = E.case_reference(case)
    assert hr < E.LIMIT, "{}: headroom {:.0f} >= 2**24".format(case, hr)
    return inputs, ref


def _params(family):
    return [pytest.param(c, d, id="{}-{}".format(c.name, d)) for c in E.CASES if c.family == family for d in c.dtypes]


@pytest.mark.parametrize("case,dtype", _params("conv"))
def test_conv_exact(case, dtype, dev):
    """ops.conv + torch.autograd.grad: forward, input gradient, weight gradient (CoordConv rows included) and bias gradient.
    fp16 is a forward format (the gradients of such a layer are bf16 and run the bf16 kernels checked here): forward only."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    f16 = dtype == "f16"
    lay = _layer(case, V, b, dev, f16)
    xd = _to_dev(x, dtype, dev).requires_grad_(True)
    y = ops.conv(xd, lay, res_self=case.res_self, fmt=lib.F16 if f16 else None)
    assert y.shape[-1] == ops.round8(case.cout)
    _check_out(y, ref["y"], dtype, case.cout, "{} forward".format(case))
    if f16:
        return
    T = E.TORCH_T[dtype]
    gd = torch.zeros(y.shape, dtype=T, device=dev)
    gd[..., :case.cout] = go.to(T).to(dev)
    gx, gV, gb = torch.autograd.grad([y], [xd, lay.V, lay.b], grad_outputs=[gd])
    ops.Streams.join(dev)
    torch.cuda.synchronize()
    _same(_host(gx, dtype), E.rounded(ref["gx"], T), "{} input gradient".format(case))
    _same(gV.cpu(), ref["gV"].float(), "{} weight gradient".format(case), E.AXES_HWIO)
    _same(gb.cpu(), ref["gb"].float(), "{} bias gradient".format(case))


@pytest.mark.parametrize("case,dtype", _params("rows"))
def test_rows_exact(case, dtype, dev, monkeypatch):
    """conv3x3_rows.hip under UPS_ROWS_KERNEL=force and the patch kernel (switch at 0) on the same stored tensors: forward with the
    inverted residual and the stored activation, input gradient with act' and the residual gradient; both against the reference
    and against each other."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    f16 = dtype == "f16"
    lay = _layer(case, V, b, dev, f16)
    TG = "fp32" if dtype == "fp32" else "bf16"          # (the gradients of an fp16 layer are bf16)
    xd, gd = _to_dev(x, dtype, dev), _to_dev(go, TG, dev)
    out = {}
    for mode in ("force", "0"):
        monkeypatch.setenv("UPS_ROWS_KERNEL", mode)
        y = ops.conv_forward(xd, lay, res=xd, fmt=lib.F16 if f16 else None, res_post=True)
        gx = None if f16 else ops.conv_dgrad(gd, xd, lay, res=gd)
        torch.cuda.synchronize()
        out[mode] = (_host(y, dtype), None if gx is None else gx.cpu())
        _check_out(y, ref["y"], dtype, case.cout, "{} forward, UPS_ROWS_KERNEL={}".format(case, mode))
        if gx is not None:
            _same(out[mode][1], E.rounded(ref["gx"], TG), "{} input gradient, UPS_ROWS_KERNEL={}".format(case, mode))
    _same(out["force"][0], out["0"][0], "{} forward, rows vs patch kernel".format(case))
    if not f16:
        _same(out["force"][1], out["0"][1], "{} input gradient, rows vs patch kernel".format(case))


S2_MODES = {"rows_s2": (("rows_s2", "force", "0"), ("s2", "0", "force"), ("generic", "0", "0")),
            "s2": (("s2", "0", "force"), ("generic", "0", "0"))}


@pytest.mark.parametrize("case,dtype", _params("rows_s2") + _params("s2"))
def test_stride2_forward_exact(case, dtype, dev, monkeypatch):
    """The stride-2 forwards: the row-stream form, the 64-wide kernel of conv3x3_s2.hip and the generic gather kernel on one input."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    lay = _layer(case, V, b, dev)
    xd = _to_dev(x, dtype, dev)
    out = {}
    for name, rows, s2 in S2_MODES[case.family]:
        monkeypatch.setenv("UPS_ROWS_KERNEL", rows)
        monkeypatch.setenv("UPS_S2_KERNEL", s2)
        y = ops.conv_forward(xd, lay)
        torch.cuda.synchronize()
        out[name] = _host(y, dtype)
        _check_out(y, ref["y"], dtype, case.cout, "{} forward on the {} kernel".format(case, name))
    for name in out:
        _same(out[name], out["generic"], "{}: {} vs generic kernel".format(case, name))


@pytest.mark.parametrize("case,dtype", _params("thinout"))
def test_thinout_exact(case, dtype, dev, monkeypatch):
    """The K-deep logit convolution (256 -> P <= 16): thin-out kernel (force) and patch kernel (0)."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    f16 = dtype == "f16"
    lay = _layer(case, V, b, dev, f16)
    xd = _to_dev(x, dtype, dev)
    out_f32 = case.extra["out_f32"]
    out = {}
    for mode in ("force", "0"):
        monkeypatch.setenv("UPS_ROWS_KERNEL", mode)
        y = ops.conv_forward(xd, lay, out_f32=out_f32, fmt=lib.F16 if f16 else None)
        torch.cuda.synchronize()
        assert y.dtype == (torch.float32 if (out_f32 or dtype == "fp32") else torch.bfloat16)
        out[mode] = _host(y, dtype)
        _check_out(y, ref["y"], "fp32" if out_f32 else dtype, case.cout, "{} forward, UPS_ROWS_KERNEL={}".format(case, mode))
    _same(out["force"], out["0"], "{}: thin-out vs patch kernel".format(case))


def _image8(x, dev, dtype="bf16"):
    x8 = torch.zeros(x.shape[:-1] + (8,), dtype=E.TORCH_T[dtype])
    x8[..., :3] = x.to(E.TORCH_T[dtype])
    return x8.to(dev)


@pytest.mark.parametrize("case,dtype", _params("first"))
def test_first_layer_exact(case, dtype, dev, monkeypatch):
    """conv3x3_first.hip (UPS_FIRST_LAYER=1) and the patch kernel (0) on an image tensor of 3 + 5 zero channels."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    xd = _image8(x, dev, dtype)
    out = {}
    for first in ("1", "0"):
        monkeypatch.setenv("UPS_FIRST_LAYER", first)
        lay = _layer(case, V, b, dev)
        y = ops.conv_forward(xd, lay)
        torch.cuda.synchronize()
        out[first] = y.cpu()
        _check_out(y, ref["y"], dtype, case.cout, "{} forward, UPS_FIRST_LAYER={}".format(case, first))
    _same(out["1"], out["0"], "{}: first-layer vs patch kernel".format(case))


@pytest.mark.parametrize("case,dtype", _params("mask"))
def test_part_masked_exact(case, dtype, dev, monkeypatch):
    """The part mask fused into the load and its mask_grad reduction, and the path that materialises the P * B part images, each on
    the first-layer kernel and on the patch kernel: forward, d loss / d hard, weight and bias gradient.  Bits everywhere but for
    d hard of the materialised path, whose pointwise kernel may write -0 where the fused epilogue writes +0: exact values there."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    P = case.extra["P"]
    bits, hard = E.part_bits(case)
    bits_d, view = bits.to(dev), x.float().to(dev)
    view_act = _image8(x, dev)
    gd = go.to(torch.bfloat16).to(dev)
    out = {}
    for first in ("1", "0"):
        monkeypatch.setenv("UPS_FIRST_LAYER", first)
        for mode in ("fused", "materialised"):
            lay = _layer(case, V, b, dev)
            h = hard.float().to(dev).requires_grad_(True)
            if mode == "fused":
                y = ops.conv(view_act, lay, mask=(h, bits_d, view))
            else:
                y = ops.conv(ops.MaskPartsFn.apply(view, h, torch.bfloat16), lay)
            gh, gV, gb = torch.autograd.grad([y], [h, lay.V, lay.b], grad_outputs=[gd])
            ops.Streams.join(dev)
            torch.cuda.synchronize()
            what = "{} {}, UPS_FIRST_LAYER={}".format(case, mode, first)
            _check_out(y, ref["y"], dtype, case.cout, what + " forward")
            if mode == "fused":
                _same(gh.cpu(), ref["gh"].float(), what + " d hard", ("image", "y", "x", "part"))
            else:       # ups_mask_parts_bwd (part path, out of scope here) sums its three products without a +0 start: where all three
                        # are -0 it writes -0.  Exact values, sign of a zero not compared (parity_ledger.md)
                assert torch.equal(gh.cpu(), ref["gh"].float()), what + " d hard: " + str(E.first_diff(gh.cpu(), ref["gh"].float()))
            _same(gV.cpu(), ref["gV"].float(), what + " weight gradient", E.AXES_HWIO)
            _same(gb.cpu(), ref["gb"].float(), what + " bias gradient")
            out[(first, mode)] = (y.cpu(), gh.cpu())
    base = out[("1", "fused")]
    for key, val in out.items():
        _same(val[0], base[0], "{}: forward {} vs fused first-layer".format(case, key))
        if key[1] == "fused":
            _same(val[1], base[1], "{}: d hard {} vs fused first-layer".format(case, key), ("image", "y", "x", "part"))
        else:
            assert torch.equal(val[1], base[1]), "{}: d hard {} vs fused first-layer".format(case, key)


@pytest.mark.parametrize("case", E.TOWER_CASES, ids=repr)
def test_towers_exact(case, dev):
    """ops.TowersFn (ups_towers_fwd / _bwd: one launch per layer index for all towers, one for every weight and bias gradient) and
    the generic convolution path on the SAME layer objects, against the layer-by-layer reference that rounds every stored tensor
    to bf16 as the kernels do: the towers' outputs, the input gradients of the 256-wide towers, every grad_V and grad_b."""
    lib, ops = _mods()
    ref, hr = E.tower_case_reference(case)
    assert hr < E.LIMIT, "{}: headroom {:.0f} >= 2**24".format(case, hr)
    M, Ln = case.M, case.Ln
    towers = []
    for t, ((x0, Ws, bs, g), _) in enumerate(ref):
        tw = []
        for l in range(Ln):
            lay = ops.ConvLayer("t{}/conv2d_{}".format(t, l), Ws[l].float().view(1, 1, *Ws[l].shape).to(dev).requires_grad_(True),
                                bs[l].float().to(dev).requires_grad_(True), 1, 1, False, None if l == 0 else "leaky_relu", slope=E.SLOPE)
            lay.in_post = l > 0
            lay.out_act = lib.ACT_LRELU if l < Ln - 1 else lib.ACT_NONE
            lay.grad_V, lay.grad_b = _ff(lay.V.shape, torch.float32, dev), _ff(lay.b.shape, torch.float32, dev)
            tw.append(lay)
        towers.append(tw)
    params = [p for tw in towers for lay in tw for p in (lay.V, lay.b)]
    gos = [g.to(torch.bfloat16).view(M, 1, 1, -1).to(dev) for (_, _, _, g), _ in ref]
    wide = [t for t, c in enumerate(case.widths) if c % 128 == 0]        # (the towers whose input gradient the grouped launch gives)

    def inputs():
        return [x0.to(torch.bfloat16).view(M, 1, 1, -1).to(dev).requires_grad_(c % 128 == 0) for ((x0, _, _, _), _), c in zip(ref, case.widths)]

    def check(outs, grads, what):
        for t, (_, r) in enumerate(ref):
            _same(outs[t].detach().cpu().view(M, -1), E.rounded(r["out"], "bf16"), "{} {}: tower {} output".format(case, what, t),
                  ("row", "channel"))
        for i, t in enumerate(wide):
            _same(grads[len(params) + i].cpu().view(M, -1), E.rounded(ref[t][1]["gx0"], "bf16"),
                  "{} {}: tower {} input gradient".format(case, what, t), ("row", "channel"))
        for t, (_, r) in enumerate(ref):
            for l in range(Ln):
                _same(grads[2 * (t * Ln + l)].cpu().view(r["gW"][l].shape), r["gW"][l].float(),
                      "{} {}: tower {} layer {} grad_V".format(case, what, t, l), ("cin", "cout"))
                _same(grads[2 * (t * Ln + l) + 1].cpu(), r["gb"][l].float(), "{} {}: tower {} layer {} grad_b".format(case, what, t, l))

    xd = inputs()
    assert ops.towers_eligible(towers, xd)
    hs = ops.TowersFn.apply(towers, *(xd + params))
    gr = torch.autograd.grad(list(hs), params + [xd[t] for t in wide], grad_outputs=gos)
    torch.cuda.synchronize()
    gr = [g_.clone() for g_ in gr]
    check(hs, gr, "grouped launches")
    # the generic path on the same layers, into the same (re-poisoned) gradient buffers
    for tw in towers:
        for lay in tw:
            lay.grad_V.view(torch.uint8).fill_(0xFF)
            lay.grad_b.view(torch.uint8).fill_(0xFF)
    xg = inputs()
    outs_g = []
    for t, tw in enumerate(towers):
        h = ops.conv(xg[t], tw[0])
        for l in range(1, Ln - 1):
            h = ops.conv(h, tw[l], res_self=True)
        outs_g.append(ops.conv(h, tw[Ln - 1]))
    gg = torch.autograd.grad(outs_g, params + [xg[t] for t in wide], grad_outputs=gos)
    ops.Streams.join(dev)
    torch.cuda.synchronize()
    check(outs_g, gg, "generic path")
    for t in range(len(towers)):
        _same(hs[t].detach().cpu(), outs_g[t].detach().cpu(), "{}: tower {} output, grouped vs generic".format(case, t))
    for i, (a, b_) in enumerate(zip(gr, gg)):
        _same(a.cpu(), b_.cpu().view(a.shape), "{}: gradient {}, grouped vs generic".format(case, i))
