"""Bit-exact parity of the fp8 convolution paths on the fp8 lattice of tests/exact_ref.py.

Weights are integers in [-7, 7] with a +-7 in every output-channel column and every input-channel row, activations and output
gradients integers in [-7, 7] holding a 7, leaky ReLU runs at slope 0.25: the per-row weight scales are 64 / 2**-6, the delayed
scales 32 (e4m3) and 4096 (e5m2), every quantisation is lossless, every product and partial sum an integer number of LSBs below
2**24, every dequantisation factor a power of two.  So the fp8 kernels must give the bits of the integer reference rounded once
to bf16 (weight and bias gradients: fp32), the same bits as the bf16 kernels on the same layer, and their fp8 copies and recorded
maxima must be those of the stored tensor.  There is no tolerance in this file.  Before anything is compared the scales and
dequantisation factors are read back and held to the expected powers of two by their bits (a failure there is a failure of the
test's premise, and says so), and the Fp8State counters must show that the fp8 route was taken.
docs/design/parity_ledger.md section 6 has the table of instance -> case and the gates that route them."""
import pytest
import torch

import exact_ref as E
from test_gpu_exact import _check_out, _ff, _layer, _mods, _same, _to_dev

pytestmark = pytest.mark.gpu


def _bits_are(t, value, what):
    """Premise: every entry of the float32 device tensor t has exactly the bits of `value`."""
    t = t.detach().float().cpu().reshape(-1)
    msg = E.first_diff(t, torch.full_like(t, value))
    assert msg is None, "premise of the test, not the kernel's result: {} is not {!r} bit for bit: {}".format(what, value, msg)


def _amax(F, slot):
    return F.amax[slot].max().reshape(1)


def _start(case):
    inputs, ref, hr = E.fp8_case_reference(case)
    for name, v in hr.items():
        assert v < E.LIMIT, "{} {}: headroom {:.0f} >= 2**24".format(case, name, v)
    assert ref["lossless"], "premise of the test: a quantisation of {} does not round-trip".format(case)
    return inputs, ref


def _bytes(t, scale, dtype, dev=None):
    q = E.f8_quantise(t, scale, dtype)[0].view(torch.uint8)
    return q if dev is None else q.to(dev)


@pytest.mark.parametrize("case", [c for c in E.FP8_CASES if c.route != "wgrad"], ids=repr)
def test_conv_fp8_exact(case, dev):
    """ops.conv_forward / ops.conv_dgrad under a fresh Fp8State: in-kernel conversion (route "convert") or pre-quantised copies
    handed in (route "copy": Handoff(f8_in=...), register_grad_copy), output and input gradient against the reference and against
    the bf16 kernels; where the launch emits a copy (second call, after F.update()): its bytes against the quantisation of the
    stored bf16 tensor, its scale against 2**k, the recorded maxima against the tensor's -- all by bits."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    lay = _layer(case, V, ref["b"], dev)
    xd, gd = _to_dev(x, "bf16", dev), _to_dev(go, "bf16", dev)
    fwd, dgrad, convert = "fwd" in case.dirs, "dgrad" in case.dirs, case.route == "convert"
    act_code = lay.act_in
    res_g = None
    if dgrad and (case.res_self or ref["res_g"] is not None):
        res_g = _to_dev((go if case.res_self else 0.0) + (ref["res_g"] if ref["res_g"] is not None else 0.0), "bf16", dev)
    if "dgrad" in case.emit and ref["res_g"] is None:
        print("{}: no element of the input gradient has a zero sum to carry 7 * 2**k: e5m2 copy check skipped".format(case))
    emit_f, emit_g = "fwd" in case.emit, "dgrad" in case.emit and ref["res_g"] is not None
    y = gx = None
    with ops.fp8_scope(True, copy_only=False if convert else None) as F:
        F.PRODUCER = True
        if not convert:         # the producer's side of the hand-off, restated: the copies and the slots that hold their scales
            sa, sg = F.slot(dev), F.slot(dev)
            F.fmax[sg] = F.E5M2_MAX
            F.scale[sa], F.scale[sg] = E.F8_SA, E.F8_SG
            x8 = _bytes(E.act_fn(x, case.act), E.F8_SA, E.E4M3, dev)
            g8 = _bytes(go, E.F8_SG, E.E5M2, dev)
        for call in range(2 if (emit_f or emit_g) else 1):
            what = "{} call {}".format(case, call)
            if fwd:
                side = ops.Handoff(f8_in=None if convert else {"t": x8, "slot": sa, "act": act_code, "site": None},
                                   f8_out_act=lib.ACT_LRELU if emit_f else None)
                assert F.eligible(lay, xd)
                y = ops.conv_forward(xd, lay, res=xd if case.res_self else None, side=side)
            if dgrad:
                assert F.eligible_grad(lay, gd, xd)
                if not convert:
                    F.register_grad_copy(gd, {"t": g8, "slot": sg, "site": None})
                gx = ops.conv_dgrad(gd, xd, lay, res=res_g)
            torch.cuda.synchronize()
            # ---- the route taken, then the premise: scales and dequantisation factors by bits
            if fwd:
                assert F.stats["fwd_f8"] == call + 1 and F.stats["fwd_copy_in"] == (0 if convert else call + 1), (what, F.stats)
                f8 = lay.copies["f8"].bufs
                _bits_are(f8["deq"], 1.0 / E.F8_SW, what + ": forward dequantisation factors")
                _bits_are(F.scale[f8["slot"] if convert else sa].reshape(1), E.F8_SA, what + ": e4m3 activation scale")
                if convert:
                    _same(_amax(F, f8["slot"]).cpu(), torch.tensor([float(E.F8_AMP)]), what + ": recorded max |act(x)|")
            if dgrad:
                assert F.stats["dgrad_f8"] == call + 1 and F.stats["dgrad_copy_in"] == (0 if convert else call + 1), (what, F.stats)
                f8g = lay.copies["f8g"].bufs
                _bits_are(f8g["deq"], 1.0 / E.F8_SW, what + ": input-gradient dequantisation factors")
                _bits_are(F.scale[f8g["slot"] if convert else sg].reshape(1), E.F8_SG, what + ": e5m2 gradient scale")
                if convert:
                    _same(_amax(F, f8g["slot"]).cpu(), torch.tensor([float(E.F8_AMP)]), what + ": recorded max |g|")
            # ---- the results
            if fwd:
                _check_out(y, ref["y"], "bf16", case.cout, what + " forward")
            if dgrad:
                _same(gx.cpu(), E.rounded(ref["gx"], "bf16"), what + " input gradient")
            # ---- the producer copies: recorded maximum in the first call, copy with the delayed scale in the second
            if emit_f:
                ya = E.lrelu(y.cpu().double())
                slot = lay.f8["f8o"]["slot"]
                _same(_amax(F, slot).cpu(), ya.abs().max().float().reshape(1), what + ": recorded max |act(y)|")
                assert float(ya.abs().max()) == ref["y_top"], (what, float(ya.abs().max()), ref["y_top"])
                if call == 0:
                    assert side.f8_out is None
                else:
                    copy = side.f8_out
                    assert copy is not None and copy["act"] == lib.ACT_LRELU and copy["slot"] == slot and F.stats["fwd_copy_out"] == 1
                    s = E.E4M3_MAX * E.F8_MARGIN / ref["y_top"]
                    _bits_are(F.scale[slot].reshape(1), s, what + ": delayed e4m3 scale of the output")
                    _same(copy["t"].cpu(), _bytes(ya, s, E.E4M3), what + ": e4m3 copy of the output vs the quantised bf16 tensor")
            if emit_g:
                ga = gx.cpu().double()
                slot = lay.f8["f8go"]["slot"]
                _same(_amax(F, slot).cpu(), ga.abs().max().float().reshape(1), what + ": recorded max |gx|")
                assert float(ga.abs().max()) == ref["gx_top"], (what, float(ga.abs().max()), ref["gx_top"])
                ent = F.grad_side.get(gx.data_ptr())
                if call == 0:
                    assert ent is None
                else:
                    assert ent is not None and F.stats["dgrad_copy_out"] == 1, "no e5m2 copy registered for the returned gradient"
                    s = E.E5M2_MAX * E.F8_MARGIN / ref["gx_top"]
                    _bits_are(F.scale[slot].reshape(1), s, what + ": delayed e5m2 scale of the input gradient")
                    _same(ent[2]["t"].cpu(), _bytes(ga, s, E.E5M2), what + ": e5m2 copy of the input gradient vs the quantised bf16 tensor")
            F.update()
        F.grad_side.clear()
    # ---- the bf16 kernels on the same layer: the same bits on this lattice
    with ops.fp8_scope(False):
        if fwd:
            y16 = ops.conv_forward(xd, lay, res=xd if case.res_self else None)
            _same(y.cpu(), y16.cpu(), "{} forward, fp8 vs bf16 kernels".format(case))
        if dgrad:
            gx16 = ops.conv_dgrad(gd, xd, lay, res=res_g)
            _same(gx.cpu(), gx16.cpu(), "{} input gradient, fp8 vs bf16 kernels".format(case))


@pytest.mark.parametrize("case", [c for c in E.FP8_CASES if c.route == "wgrad"], ids=repr)
def test_wgrad_fp8_exact(case, dev):
    """conv_wgrad3x3_f8_kernel through ops.conv_wgrad(f8_src=...): the e5m2 copy of the gradient handed in, the forward input (bf16,
    or fp16 in a bf16 container; with or without the activation on load) quantised while it is staged.  grad_V (main rows) and
    grad_b -- the column sums through the ones operand -- against the reference, in buffers pre-filled with 0xFF; the whole
    grad_V, CoordConv rows (fp32 coordinate kernels, non-zero gradients) included, and grad_b against the bf16 route's bits."""
    lib, ops = _mods()
    (x, V, b, go), ref = _start(case)
    lay = _layer(case, V, b, dev)
    fmt = lib.F16 if case.f16 else None
    xd, gd = _to_dev(x, "f16" if case.f16 else "bf16", dev), _to_dev(go, "bf16", dev)
    cin = case.cin
    with ops.fp8_scope(True) as F:
        sg = F.slot(dev)
        F.fmax[sg] = F.E5M2_MAX
        F.scale[sg] = E.F8_SG
        copy = {"t": _bytes(go, E.F8_SG, E.E5M2, dev), "slot": sg}
        assert F.eligible_wgrad(lay, gd, xd, None)
        gV, gb = ops.conv_wgrad(gd, xd, lay, fmt=fmt, f8_src=copy)
        torch.cuda.synchronize()
        assert F.stats["wgrad_f8"] == 1, F.stats
        ew = lay.f8["f8w"]
        _bits_are(F.scale[ew["slot"]].reshape(1), E.F8_SA, "{}: e4m3 scale of the forward input".format(case))
        _bits_are(F.scale[sg].reshape(1), E.F8_SG, "{}: e5m2 scale of the gradient copy".format(case))
        _same(_amax(F, ew["slot"]).cpu(), torch.tensor([float(E.F8_AMP)]), "{}: recorded max |act(x)|".format(case))
        gV, gb = gV.cpu(), gb.cpu()
    _same(gV[:, :, :cin].contiguous(), ref["gV"].float(), "{} weight gradient".format(case), E.AXES_HWIO)
    _same(gb, ref["gb"].float(), "{} bias gradient (ones-operand column sums)".format(case))
    lay.grad_V, lay.grad_b = _ff(lay.V.shape, torch.float32, dev), _ff(lay.b.shape, torch.float32, dev)
    with ops.fp8_scope(False):
        gV16, gb16 = ops.conv_wgrad(gd, xd, lay, fmt=fmt)
        torch.cuda.synchronize()
    if case.coords:     # rows of the fp32 coordinate kernels: not exact on 16-aligned maps, but the same launches in both routes
        rows = gV[:, :, cin:]
        assert bool(torch.isfinite(rows).all()) and float(rows.abs().max()) > 0, "{}: CoordConv rows of the weight gradient".format(case)
    _same(gV, gV16.cpu(), "{} weight gradient, fp8 vs bf16 route".format(case), E.AXES_HWIO)
    _same(gb, gb16.cpu(), "{} bias gradient, fp8 vs bf16 route".format(case))
