"""CPU checks of tests/deconv_exact_ref.py: on every case the premises of exactness hold (ss = 4**k, W representable in every stored
type, dyadic coordinates where claimed, headroom below 2**24), every rounded reference is representable, the tap-loop reference
equals tests/deconv_ref.py + autograd by value, the one-launch kernel's `sub` and the swapped weight gradient's split-K are what
the case table says (the plan is host code), and the clamped-filter restatement has the gradient autograd gives."""
import ctypes as C

import pytest
import torch

import deconv_exact_ref as X
import deconv_ref as D
import exact_ref as E
from oracle import ref_model as R


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_case_premises(case):
    (x, V, g, b, dy), ref, hr = X.case_reference(case)
    nnz = 4 ** case.k
    assert nnz <= 9 * case.cin_v < 4 * nnz
    assert bool(((V != 0).sum(dim=(0, 1, 3)) == nnz).all()) and float(V.abs().max()) == 1.0
    assert bool((ref["ss"] == nnz).all())
    # the fmaf sum of deconv_norm_kernel in float32, in any order, is that integer; 2**-k is a float32
    assert float((V.float() * V.float()).sum(dim=(0, 1, 3)).max()) == nnz and nnz < 2 ** 24
    assert bool((ref["inv"] == 2.0 ** -case.k).all()) and E.is_pow2(ref["inv"])
    assert set(g.tolist()) <= set(X.G_VALUES)
    for T in ("bf16", "f16", "fp32"):
        assert torch.equal(E.rounded(ref["W"], T).double(), ref["W"]), "{}: W is not exact in {}".format(case, T)
        for t in (x, dy, b):
            assert torch.equal(E.rounded(t, T).double(), t)
    if case.coords:
        ax, ay = X.coord_scales(case.h, case.w)
        assert E.is_pow2(torch.tensor([ax]))
        assert E.is_pow2(torch.tensor([ay])) != case.zero_row
        col, row = V[..., case.cin], V[..., case.cin + 1]
        assert bool(((col != 0).sum(dim=(0, 1)) >= 1).all()), "a filter without a column-coordinate weight"
        if case.zero_row:
            assert float(row.abs().sum()) == 0.0 and case.w % 16 == 0
        else:
            assert bool(((row != 0).sum(dim=(0, 1)) >= 1).all()), "a filter without a row-coordinate weight"
            assert E.lsb(X.add_coordinates(x)) == min(ax, ay, 1.0)
    for name, v in hr.items():
        assert v < X.LIMIT, "{} {}: {:.0f} LSBs (2**{:.2f}) >= 2**24".format(case, name, v, torch.log2(torch.tensor(v)).item())
    assert set(hr) == {"fwd", "dx", "dW", "db", "dot", "dV"}


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_reference_equals_deconv_ref_and_autograd(case):
    """The tap loop and the closed-form gradients against F.conv_transpose2d + autograd through the normalisation (by value: the
    autograd chain divides by the norm where the closed form multiplies by 2**-k), and every rounded reference is representable:
    rounding it to the stored type and back changes nothing the GPU comparison could then blame on the kernel."""
    (x, V, g, b, dy), ref, _ = X.case_reference(case)
    xr, Vr, gr, br = (t.clone().requires_grad_(True) for t in (x, V, g, b))
    yr = D.layer(xr, Vr, gr, br, case.coords, R.Scope.add_coordinates)
    gx, gV, gg, gb = torch.autograd.grad([yr], [xr, Vr, gr, br], grad_outputs=[dy])
    if case.coords and not case.zero_row:           # the convention: the column coordinate steps by 2 / (hi - 1), the row by 2 / (wi - 1)
        ax, ay = X.coord_scales(case.h, case.w)
        xa = X.add_coordinates(x)
        assert float(xa[0, 0, 1, case.cin] - xa[0, 0, 0, case.cin]) == ax and float(xa[0, 1, 0, case.cin + 1] - xa[0, 0, 0, case.cin + 1]) == ay
    exact = X.exact_mask_dV(case)
    for name, a, want in (("y", ref["y"], yr.detach()), ("dx", ref["dx"], gx), ("db", ref["db"], gb), ("dg", ref["dg"], gg),
                          ("dV", ref["dV"], gV), ("W", ref["W"], D.weight(V, g))):
        scale = max(1.0, float(want.abs().max()))
        assert float((a - want).abs().max()) <= 1e-12 * scale, "{} {}: {}".format(case, name, float((a - want).abs().max()))
    assert torch.equal(ref["y"], yr.detach()) and torch.equal(ref["dx"], gx) and torch.equal(ref["db"], gb)
    # representable: y and dx in each stored type of the case within one rounding (checked as idempotence), fp32 gradients exactly
    for T in case.dtypes:
        for k in ("y", "dx"):
            r = E.rounded(ref[k], T)
            assert torch.equal(E.rounded(r.double(), T), r)
    for k in ("db", "dg", "dot"):
        assert torch.equal(ref[k].float().double(), ref[k]), "{} {} is not a float32".format(case, k)
    for k in ("dW", "dV"):
        assert torch.equal(ref[k].float().double()[exact], ref[k][exact]), "{} {} is not a float32".format(case, k)
    if case.zero_row:
        assert not torch.equal(ref["dV"].float().double(), ref["dV"])           # (the 2/15 column really is inexact)


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_one_launch_gate_and_split_k_are_the_tables(case):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    assert X.one_launch_sub(case) == case.sub, (case, X.one_launch_sub(case))
    assert all(X.takes_one_launch(case, d) == (case.sub is not None and d != "fp32") for d in case.dtypes)
    for T, want in case.splitk.items():
        d = lib.WgradDesc()
        d.dtype = lib.F32 if T == "fp32" else lib.BF16
        d.n, d.hi, d.wi, d.ci, d.ldi = case.n, 2 * case.h, 2 * case.w, X.round8(case.nf), X.round8(case.nf)
        d.ci_log, d.cin_v = case.nf, case.nf
        d.ho, d.wo, d.co, d.ldo = case.h, case.w, case.cin, X.round8(case.cin)
        d.in_sy = d.in_sx = 2
        for t in range(9):
            d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = t // 3, t % 3, t
        d.ntaps = 9
        sk, wsb = C.c_int32(0), C.c_size_t(0)
        assert lib.load().ups_conv_wgrad_plan(C.byref(d), C.byref(sk), C.byref(wsb)) == 0
        assert sk.value == want, (case, T, sk.value)
        assert wsb.value == sk.value * (9 * d.cin_v * d.co + d.co) * 4
    assert set(case.splitk) == {"fp32" if d == "fp32" else "bf16" for d in case.dtypes}


def test_case_table_reaches_what_it_says():
    subs = [c.sub for c in X.CASES]
    assert {1, 2, 4, None} <= set(subs)
    fb = X.BY_NAME["dc_lds_fallback"]
    assert fb.w % 64 == 0 and fb.sub == 1                                    # (its width would allow sub = 4: LDS decides)
    assert X.BY_NAME["dc_sub2_h1"].h == 1 and X.BY_NAME["dc_sub4_two_blocks"].w // (16 * 4) == 2
    assert any(c.coords and c.sub is not None for c in X.CASES) and any(c.coords and c.sub is None for c in X.CASES)
    # the stride-2 row stream's and conv3x3_s2's shape gates on the input gradient of dc_dx_s2 (ci = round8(nf), wi = 2 w, co = cin)
    c = X.BY_NAME["dc_dx_s2"]
    assert (X.round8(c.nf), 2 * c.w, c.cin) == (64, 64, 128) and c.h == c.w and c.h % 8 == 0 and c.w % 16 == 0
    for o in X.CASES:
        if o is not c:
            assert not (X.round8(o.nf) in (32, 64) and o.h % 8 == 0 and o.w % 16 == 0), o


def test_layouts_restate_the_comments():
    W = torch.arange(9 * 3 * 5, dtype=torch.float64).view(3, 3, 3, 5) + 1
    wf = X.layout_w_fwd(W, 3, 32)
    assert wf.shape == (9, 1, 3, 32) and float(wf[4, 0, 2, 1]) == float(W[1, 1, 2, 1]) and float(wf[..., 3:].abs().sum()) == 0
    wd = X.layout_w_dx(W, 3, 16)
    assert wd.shape == (9, 1, 3, 16) and float(wd[5, 0, 1, 2]) == float(W[1, 2, 2, 1]) and float(wd[..., 3:].abs().sum()) == 0
    # the table of the full mask is the coordinate part of the forward at an interior pixel: y = k0 + j kj + i ki
    case = X.BY_NAME["dc_coords17"]
    (x, V, g, b, dy), ref, _ = X.case_reference(case)
    tab = X.layout_ctab(ref["W"], case.cin, case.h, case.w)
    y = X.deconv_taps(X.add_coordinates(torch.zeros_like(x)), ref["W"], torch.zeros_like(b))
    for i, j in ((0, 0), (3, 5), (16, 16), (0, 7), (9, 0)):
        for cls in range(4):
            py, px = cls >> 1, cls & 1
            ym = 1 if py else (1 | ((i > 0) << 1))
            xm = 1 if px else (1 | ((j > 0) << 1))
            t = tab[cls, ym * 8 + xm]
            assert torch.equal(t[0] + j * t[1] + i * t[2], y[0, 2 * i + py, 2 * j + px]), (i, j, cls)
    assert torch.equal(tab.float().double(), tab)


@pytest.mark.parametrize("kind", ["zero", "below"])
def test_clamped_restatement_has_autograds_gradient(kind):
    """Below the clamp deconv_ref.weight's `clamp` has zero gradient: dV = g rsqrt(1e-12) dW with no projection term, which is
    what the closed form states (and the kernel comment promises)."""
    case, (x, V, g, b, dy) = X.clamped_inputs(kind)
    o = 0 if kind == "zero" else 1
    ref = X.reference(x, V, g, b, dy, False)
    assert float(ref["ss"][o]) < X.WN_EPS and bool((ref["ss"][[i for i in range(case.nf) if i != o]] == 4 ** case.k).all())
    xr, Vr, gr, br = (t.clone().requires_grad_(True) for t in (x, V, g, b))
    yr = D.layer(xr, Vr, gr, br, False, R.Scope.add_coordinates)
    gx, gV, gg, gb = torch.autograd.grad([yr], [xr, Vr, gr, br], grad_outputs=[dy])
    for name, a, want in (("y", ref["y"], yr.detach()), ("dx", ref["dx"], gx), ("dg", ref["dg"], gg), ("dV", ref["dV"], gV)):
        assert float((a - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), (kind, name)
    plain = float(g[o]) * 1e6 * ref["dW"][:, :, o]
    assert float((gV[:, :, o] - plain).abs().max()) <= 1e-9 * float(plain.abs().max())
    assert float(plain.abs().max()) > 0
    if kind == "zero":
        assert float(ref["dg"][0]) == 0.0 and torch.equal(ref["y"][..., 0], b[0].expand_as(ref["y"][..., 0]))
    else:
        assert float(ref["y"][..., 1].abs().max()) <= 0.6 and float(ref["dg"][1].abs()) > 0
