"""Bit-exact parity of the weight-normalised deconvolution (csrc/deconv3x3_s2.hip) on lattice inputs (tests/deconv_exact_ref.py).

V holds 4**k entries of +-1 per filter, g is 0.5 / 1 / 2, x, dy and b are small integers and the coordinates dyadic: the
normalisation, every product, every partial sum, the CoordConv table and the whole backward through the normalisation are exact in
fp32, so ups_deconv_prep, ups_deconv3x3_s2_fwd, the class launches, the stride-2 input gradient, the swapped weight gradient,
ups_deconv_bias_coord_grad and ups_deconv_wn_bwd must give the bits of the float64 reference rounded once to the stored type.
The premise -- rsqrtf(4**k) = 2**-k on the device -- is read back first and named as such when it fails.  The only tolerances in
this file are the three docs/design/parity_ledger.md section 12 names: the row-coordinate column of dc_coords_x (2/15 is not
dyadic) and the two clamped-filter cases at the end.  The headroom condition is asserted before anything is launched."""
import pytest
import torch

import deconv_exact_ref as X
import deconv_ref as D
import exact_ref as E
from util import rel_err

pytestmark = pytest.mark.gpu


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _ff(t):
    """0xFF in every byte (NaN in every float type): an element the kernels do not write shows."""
    t.view(torch.uint8).fill_(0xFF)
    return t


def _to_dev(t, dtype, dev, ld):
    """A lattice tensor [.., c] in the storage the kernels read, channels padded with zeros to ld; fp16 lives in bf16 containers."""
    t = torch.nn.functional.pad(t, (0, ld - t.shape[-1]))
    if dtype == "f16":
        return t.to(torch.float16).to(dev).view(torch.bfloat16)
    return t.to(E.TORCH_T[dtype]).to(dev)


def _host(t, dtype):
    t = t.detach().cpu()
    return t.view(torch.float16) if (dtype == "f16" and t.dtype == torch.bfloat16) else t


def _cmp(errs, got, want, what, axes=None):
    msg = E.first_diff(got.contiguous(), want.contiguous(), axes)
    if msg is not None:
        errs.append("{}: {}".format(what, msg))


def _cmp_padded(errs, t, ref, T, c, what):
    """Channels [0, c) hold the reference's bits, the pad channels [c, ld) zero bits."""
    _cmp(errs, t[..., :c], E.rounded(ref, T), what)
    if t.shape[-1] > c:
        _cmp(errs, t[..., c:], torch.zeros_like(t[..., c:]), what + " (pad channels)")


class _Layer(object):
    """ops.DeconvLayer on the device with 0xFF-filled gradient buffers, its prepared operands, and one run per route."""
    def __init__(self, dev, dtype, inputs, coords):
        lib, ops = _mods()
        self.lib, self.ops, self.dev, self.dtype = lib, ops, dev, dtype
        x, V, g, b, dy = inputs
        self.n, self.h, self.w, self.cin = x.shape
        self.nf = V.shape[2]
        self.TG = "fp32" if dtype == "fp32" else "bf16"                  # (the gradients of an fp16 layer are bf16)
        self.fmt = lib.F16 if dtype == "f16" else None
        self.fcode = {"bf16": lib.BF16, "f16": lib.F16, "fp32": lib.F32}[dtype]
        self.dcode = lib.F32 if dtype == "fp32" else lib.BF16
        Vt, gt, bt = (t.float().to(dev).requires_grad_(True) for t in (V, g, b))
        self.lay = ops.DeconvLayer("exact/deconv2d_0", Vt, gt, bt, coords)
        self.lay.f16 = dtype == "f16"
        self.lay.grad_V, self.lay.grad_g, self.lay.grad_b = (torch.empty_like(t) for t in (Vt, gt, bt))
        self.x = _to_dev(x, dtype, dev, ops.round8(self.cin))
        self.dy = _to_dev(dy, self.TG, dev, ops.round8(self.nf))

    def prepared(self):
        ent = self.lay.prepared(self.fcode, self.dcode, self.h, self.w)
        torch.cuda.synchronize()
        return ent

    def run(self, one_launch, monkeypatch):
        """(y, dx, dV, dg, db) on the host and the number of ups_conv_igemm calls the forward made (0: the one-launch kernel)."""
        lib, ops, lay = self.lib, self.ops, self.lay
        for t in (lay.grad_V, lay.grad_g, lay.grad_b):
            _ff(t)
        names = []
        orig = lib.call

        def spy(name, *args):
            names.append(name)
            return orig(name, *args)
        xt = self.x.clone().requires_grad_(True)
        prev = ops.DECONV_ONE_LAUNCH
        ops.DECONV_ONE_LAUNCH = one_launch
        try:
            with monkeypatch.context() as m:
                m.setattr(lib, "call", spy)
                y = ops.DeconvFn.apply(xt, lay.V, lay.g, lay.b, lay, self.fmt)
            dx, dV, dg, db = torch.autograd.grad([y], [xt, lay.V, lay.g, lay.b], grad_outputs=[self.dy])
        finally:
            ops.DECONV_ONE_LAUNCH = prev
        ops.Streams.join(self.dev)
        torch.cuda.synchronize()
        out = {"y": _host(y, self.dtype), "dx": dx.cpu(), "dV": dV.cpu(), "dg": dg.cpu(), "db": db.cpu()}
        return out, names.count("ups_conv_igemm")


def _premise(errs, case, ent, ref, inputs):
    """inv = 2**-k and w32 = W by their bits.  Where the device's rsqrtf is not that, the failure is named as the premise's and the
    comparisons that follow take the reference's inv from the device (exact only if that value is still a power of two)."""
    x, V, g, b, dy = inputs
    inv = ent["inv"].cpu()
    msg = E.first_diff(inv, ref["inv"].float())
    if msg is not None:
        errs.append("premise of {}: rsqrtf(4^k): {} (read back {!r}, power of two: {})".format(
            case, msg, sorted(set(inv.tolist())), E.is_pow2(inv)))
        ref = X.reference(x, V, g, b, dy, case.coords, inv=inv.double())
    msg = E.first_diff(ent["w32"].cpu(), ref["W"].float(), X.AXES_V)
    if msg is not None:
        errs.append("premise of {}: rsqrtf(4^k): w32: {}".format(case, msg))
    return ref


def _layouts(errs, case, dtype, ent, ref):
    bkf, bkd = (16 if dtype == "fp32" else 32), (16 if dtype == "fp32" else 32)
    axes_f, axes_d = ("tap", "k_chunk", "filter", "k"), ("tap", "k_chunk", "cin", "k")
    wf = ent["w_fwd"].cpu()
    _cmp(errs, wf, E.rounded(X.layout_w_fwd(ref["W"], case.cin, bkf), dtype), "{} w_fwd".format(case), axes_f)
    wd = ent["w_dx"].cpu()
    _cmp(errs, wd, E.rounded(X.layout_w_dx(ref["W"], case.cin, bkd), "fp32" if dtype == "fp32" else "bf16"), "{} w_dx".format(case), axes_d)
    if case.coords:
        _cmp(errs, ent["ctab"].cpu(), X.layout_ctab(ref["W"], case.cin, case.h, case.w).float(), "{} ctab".format(case),
             ("class", "mask", "term", "filter"))
    else:
        assert ent["ctab"] is None


def _outputs(errs, case, L, out, ref, what):
    _cmp_padded(errs, out["y"], ref["y"], L.dtype, case.nf, "{} {} y".format(case, what))
    _cmp_padded(errs, out["dx"], ref["dx"], L.TG, case.cin, "{} {} dx".format(case, what))
    _cmp(errs, out["db"], ref["db"].float(), "{} {} db".format(case, what))
    _cmp(errs, out["dg"], ref["dg"].float(), "{} {} dg".format(case, what))
    exact = X.exact_mask_dV(case)
    if bool(exact.all()):
        _cmp(errs, out["dV"], ref["dV"].float(), "{} {} dV".format(case, what), X.AXES_V)
    else:
        # dc_coords_x: the row-coordinate column's dW entries are sums of dy * (-1 + i * 2/15) -- not dyadic.  Those entries alone are
        # held to the fp64 reference at the 1e-3 tests/test_gpu_deconv.py uses for fp32; every other entry by bits.
        got, want = out["dV"].clone(), ref["dV"].float()
        col_g, col_w = got[..., case.cin + 1].double(), ref["dV"][..., case.cin + 1]
        e = rel_err(col_g, col_w)
        print("{} {} dV row-coordinate column: rel err {:.3e}".format(case, what, e))
        if not e <= 1e-3:
            errs.append("{} {} dV row-coordinate column: rel err {}".format(case, what, e))
        got[..., case.cin + 1] = want[..., case.cin + 1]
        _cmp(errs, got, want, "{} {} dV (all but the row-coordinate column)".format(case, what), X.AXES_V)


def _params():
    return [pytest.param(c, d, id="{}-{}".format(c.name, d)) for c in X.CASES for d in c.dtypes]


@pytest.mark.parametrize("case,dtype", _params())
def test_deconv_exact(case, dtype, dev, monkeypatch):
    """ups_deconv_prep's operands, then ops.DeconvFn + torch.autograd.grad through the class launches and -- where the one-launch
    kernel takes the shape -- through it as well: y, dx, db, dV, dg against the reference and the two routes against each other."""
    inputs, ref, hr = X.case_reference(case)
    for name, v in hr.items():
        assert v < X.LIMIT, "{} {}: headroom {:.0f} >= 2**24".format(case, name, v)
    errs = []
    L = _Layer(dev, dtype, inputs, case.coords)
    ent = L.prepared()
    ref = _premise(errs, case, ent, ref, inputs)
    _layouts(errs, case, dtype, ent, ref)
    outs = {}
    for one_launch in ((False, True) if X.takes_one_launch(case, dtype) else (False,)):
        what = "one launch" if one_launch else "class launches"
        out, igemm_fwd = L.run(one_launch, monkeypatch)
        assert igemm_fwd == (0 if one_launch else 4), "{} {}: the forward made {} ups_conv_igemm calls".format(case, what, igemm_fwd)
        _outputs(errs, case, L, out, ref, what)
        outs[what] = out
    if len(outs) == 2:
        for k in ("y", "dx", "dV", "dg", "db"):
            _cmp(errs, outs["one launch"][k], outs["class launches"][k], "{} {}: one launch vs class launches".format(case, k))
    # the input gradient once more on the stride-2 kernels the case is there for (the runs above took the generic kernel)
    for name, rows, s2 in case.dx_force:
        monkeypatch.setenv("UPS_ROWS_KERNEL", rows)
        monkeypatch.setenv("UPS_S2_KERNEL", s2)
        dx = L.ops.deconv_dgrad(L.dy, L.x, L.lay, fmt=L.fmt)
        torch.cuda.synchronize()
        _cmp_padded(errs, dx.cpu(), ref["dx"], L.TG, case.cin, "{} dx on {}".format(case, name))
        _cmp(errs, dx.cpu(), outs["class launches"]["dx"], "{} dx: {} vs generic kernel".format(case, name))
    assert not errs, "\n".join(errs)


# ------------------------------------------------------------------------------------------------------------- clamped filters
# dV[:, :, 0, :] of the all-zero filter is fl(fl(g_0 * rsqrtf(1e-12f)) * dW), dW an exact integer.  The issue allowed 1e-5 relative for
# the fp32 evaluation of rsqrtf and the products, to be fixed at 4x the error measured against the fp64 value g_0 * 1e6 * dW if that
# is smaller.  Measured on the MI355X, bf16 and fp32: 0 -- 1e-12f is 9.99999996e-13, its reciprocal square root 1000000.02 rounds
# to the float 1e6 (spacing 0.0625 there), and 1e6 = 2**6 * 15625, so g_0 * 1e6 * dW is a float32 while 15625 |dW| < 2**24.  Four times
# nothing is nothing: the comparison is by value with no tolerance (section 12 of the ledger).
ZERO_FILTER_TOL = 0.0


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_all_zero_filter(dtype, dev, monkeypatch):
    """Filter 0 all zero (the existing test only asserts finiteness): its output channel is b[0] by bits, dg[0] is exactly 0, and dV of
    that filter is g[0] * rsqrt(1e-12) * dW with no projection term.  Every other filter stays on the lattice: bits."""
    case, inputs = X.clamped_inputs("zero")
    x, V, g, b, dy = inputs
    ref = X.reference(x, V, g, b, dy, False)
    L = _Layer(dev, dtype, inputs, False)
    L.prepared()
    out, _ = L.run(True, monkeypatch)
    errs = []
    T = E.TORCH_T[dtype]
    _cmp(errs, out["y"][..., 0], b[0].to(T).expand_as(out["y"][..., 0]), "all-zero filter: output channel 0 is not b[0]")
    _cmp_padded(errs, out["y"], ref["y"], dtype, case.nf, "all-zero filter y")
    _cmp_padded(errs, out["dx"], ref["dx"], L.TG, case.cin, "all-zero filter dx")
    _cmp(errs, out["db"], ref["db"].float(), "all-zero filter db")
    assert float(out["dg"][0]) == 0.0, "all-zero filter: dg[0] = {!r}".format(float(out["dg"][0]))
    _cmp(errs, out["dg"][1:], ref["dg"].float()[1:], "all-zero filter dg[1:]")
    _cmp(errs, out["dV"][:, :, 1:], ref["dV"].float()[:, :, 1:], "all-zero filter dV of the other filters", X.AXES_V)
    want = float(g[0]) * 1e6 * ref["dW"][:, :, 0]                  # (float64: rsqrt(1e-12) = 1e6)
    got = out["dV"][:, :, 0].double()
    assert 0 < float(want.abs().max()) and 15625 * float(ref["dW"][:, :, 0].abs().max()) < 2 ** 24
    nz = want != 0
    assert bool((got[~nz] == 0).all()), "all-zero filter: dV is not zero where dW is"
    e = float(((got - want).abs()[nz] / want.abs()[nz]).max())
    print("all-zero filter {}: max relative error of dV[:, :, 0, :] against g rsqrt(1e-12) dW: {:.3e}".format(dtype, e))
    assert e <= ZERO_FILTER_TOL, "all-zero filter dV[:, :, 0, :]: relative error {}".format(e)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_below_clamp_filter(dtype, dev, monkeypatch):
    """Filter 1 scaled to |V| = 1e-7, below the clamp: W, y, dV and dg against fp64 autograd of tests/deconv_ref.py, whose clamp
    has zero gradient there (no projection term), at the 1e-3 of tests/test_gpu_deconv.py; in fp32 the clamped channel also on its
    own norm.  The other filters stay on the lattice and are held by bits."""
    from oracle import ref_model as R
    case, inputs = X.clamped_inputs("below")
    x, V, g, b, dy = inputs
    xr, Vr, gr, br = (t.clone().requires_grad_(True) for t in inputs[:4])
    yr = D.layer(xr, Vr, gr, br, False, R.Scope.add_coordinates)
    _, gV, gg, _ = torch.autograd.grad([yr], [xr, Vr, gr, br], grad_outputs=[dy])
    ref = X.reference(x, V, g, b, dy, False)
    L = _Layer(dev, dtype, inputs, False)
    ent = L.prepared()
    out, _ = L.run(True, monkeypatch)
    errs = []
    others = [o for o in range(case.nf) if o != 1]
    _cmp(errs, out["y"][..., others], E.rounded(ref["y"][..., others], dtype), "below-clamp filter: y of the other filters")
    _cmp(errs, out["dV"][:, :, others], ref["dV"].float()[:, :, others], "below-clamp filter: dV of the other filters", X.AXES_V)
    _cmp(errs, out["dg"][others], ref["dg"].float()[others], "below-clamp filter: dg of the other filters")
    _cmp(errs, out["db"], ref["db"].float(), "below-clamp filter db")
    got = {"W": ent["w32"].cpu(), "y": out["y"][..., :case.nf], "dV": out["dV"], "dg": out["dg"]}
    want = {"W": D.weight(V, g), "y": yr.detach(), "dV": gV, "dg": gg}
    for k in ("W", "y", "dV", "dg"):
        e = rel_err(got[k].double(), want[k])
        print("below-clamp filter {} {}: rel err {:.3e}".format(dtype, k, e))
        if not e <= 1e-3:
            errs.append("below-clamp filter {}: rel err {}".format(k, e))
    sel = {"W": lambda t: t[:, :, 1], "dV": lambda t: t[:, :, 1], "dg": lambda t: t[1:2]}
    if dtype == "fp32":
        sel["y"] = lambda t: t[..., 1]
    for k, f in sel.items():
        e = rel_err(f(got[k]).double(), f(want[k]))
        print("below-clamp filter {} {} of filter 1 alone: rel err {:.3e}".format(dtype, k, e))
        if not e <= 1e-3:
            errs.append("below-clamp filter {} of filter 1 alone: rel err {}".format(k, e))
    # no projection term: dV_1 = g_1 rsqrt(1e-12) dW_1, far from what the unclamped formula would subtract
    plain = float(g[1]) * 1e6 * ref["dW"][:, :, 1]
    if not rel_err(out["dV"][:, :, 1].double(), plain) <= 1e-3:
        errs.append("below-clamp filter: dV carries a projection term: rel err {}".format(rel_err(out["dV"][:, :, 1].double(), plain)))
    assert not errs, "\n".join(errs)
