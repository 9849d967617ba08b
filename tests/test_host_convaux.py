"""CPU side of the conv_aux.hip edge tests: every restatement of convaux_ref.py against the oracle (conv2d_same, add_coordinates and
their fp64 autograd), and every premise the GPU cases of test_gpu_convaux.py rest on -- the chunk positions of the batched list
(from ups_prep_item_blocks and the kernel's own two constants), the sizes that reach a second grid-stride trip, the exactness
headroom of the integer cases, dyadic ax / ay, the planted rows of the fp8 weights.  No GPU: only host entry points are called."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import convaux_ref as A
from oracle import ref_model as R

F32, BF16, F16 = A.F32, A.BF16, A.F16
DTYPES = [BF16, F16, F32]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    return lib


def _ids(c):
    return c[0] if isinstance(c[0], str) else "x".join(map(str, c))


# ----------------------------------------------------------------------------- blocked-K
@pytest.mark.parametrize("dtype", DTYPES, ids=A.DT_NAME.get)
@pytest.mark.parametrize("case", A.PREP_CASES, ids=_ids)
def test_blocked_k_unblocks_to_the_rounded_weights(case, dtype):
    """Un-blocking w_fwd gives V[:, :ci_log, :] rounded once, un-blocking w_dgrad its transpose, and every other bit is zero."""
    name, k, ci_log, coords, co = case
    ntaps, cin_v = k * k, ci_log + (2 if coords else 0)
    V = A.edge_weights((ntaps, cin_v, co), 11, dtype)
    wf, wd = A.blocked_k(V, ntaps, ci_log, co, A.round8(ci_log), ci_log, A.round8(co), dtype)
    bk = A.bk_of(dtype)
    assert wf.shape == (ntaps, A.cdiv(A.round8(ci_log), bk), co, bk) and wd.shape == (ntaps, A.cdiv(A.round8(co), bk), ci_log, bk)
    want = A.rounded(V[:, :ci_log, :], dtype)
    uf, ud = A.unblock(wf), A.unblock(wd)
    assert torch.equal(A.bits(uf[:, :ci_log]), A.bits(want))
    assert torch.equal(A.bits(ud[:, :co]), A.bits(want.transpose(1, 2)))
    assert int(A.bits(uf[:, ci_log:]).abs().max() if uf.shape[1] > ci_log else 0) == 0
    assert int(A.bits(ud[:, co:]).abs().max() if ud.shape[1] > co else 0) == 0
    if dtype == F16:                      # saturation, not inf
        assert float(want.float().abs().max()) == 65504.0 and bool(torch.isfinite(want.float()).all())
    flat = A.bits(want).view(-1)
    assert int(flat[0]) == 0 and int(flat[1]) != 0 and float(want.reshape(-1)[1]) == 0.0          # +0 and -0 stay apart
    if dtype != F16:
        assert float(want.reshape(-1)[2]) != 0.0                                                  # a denormal survives bf16 / fp32


def test_blocked_images_are_the_convolution_and_its_input_gradient():
    """A 3x3 convolution evaluated by index from w_fwd equals oracle.ref_model.conv2d_same, and from w_dgrad its autograd input
    gradient, on a lattice (integers: every product and sum is exact in fp64); the activations' and the gradient's padding channels
    hold junk that only zero weights keep out."""
    k, ci_log, co, h, w = 3, 20, 10, 6, 7
    ntaps, bk = 9, 32
    V = A.int_weights((ntaps, ci_log, co), 3)
    wf, wd = A.blocked_k(V, ntaps, ci_log, co, A.round8(ci_log), ci_log, A.round8(co), BF16)
    g0 = A.gen(4)
    x = torch.randint(-4, 5, (1, h, w, ci_log), generator=g0).double().requires_grad_(True)
    gy = torch.randint(-4, 5, (1, h, w, co), generator=g0).double()
    y = R.conv2d_same(x, V.double().view(3, 3, ci_log, co), torch.zeros(co, dtype=torch.float64), 1)
    (gx,) = torch.autograd.grad((y * gy).sum(), x)
    dy, dx = A.taps(h, 3, 1), A.taps(w, 3, 1)

    def shifted(t, oy, ox):               # t[i + oy][j + ox], zero outside
        out = torch.zeros_like(t)
        ys, xs = slice(max(0, -oy), min(h, h - oy)), slice(max(0, -ox), min(w, w - ox))
        yd, xd = slice(max(0, oy), min(h, h + oy)), slice(max(0, ox), min(w, w + ox))
        out[ys, xs] = t[yd, xd]
        return out
    xp = torch.full((h, w, wf.shape[1] * bk), 7.0, dtype=torch.float64)
    xp[..., :ci_log] = x.detach()[0]
    gp = torch.full((h, w, wd.shape[1] * bk), -5.0, dtype=torch.float64)
    gp[..., :co] = gy[0]
    yb = torch.zeros(h, w, co, dtype=torch.float64)
    gb = torch.zeros(h, w, ci_log, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            t = r * 3 + s
            xs = shifted(xp, dy[r], dx[s]).view(h, w, -1, bk)
            yb += torch.einsum("hwqk,qck->hwc", xs, wf[t].double())
            gs = shifted(gp, -dy[r], -dx[s]).view(h, w, -1, bk)
            gb += torch.einsum("hwqk,qrk->hwr", gs, wd[t].double())
    assert torch.equal(yb, y.detach()[0]) and float(y.detach().abs().max()) > 0
    assert torch.equal(gb, gx[0]) and float(gx.abs().max()) > 0


# ----------------------------------------------------------------------------- d2s
@pytest.mark.parametrize("hi,wi", [(8, 6), (7, 6), (8, 5), (7, 5)])
@pytest.mark.parametrize("case", A.D2S_CASES, ids=_ids)
def test_d2s_image_is_the_stride2_input_gradient(case, hi, wi):
    """Even and odd heights and widths give the four (pad_y, pad_x) pairs; integers, so fp64 is exact and the comparison is equality."""
    ci_log, Cc, co = case
    V = A.int_weights((9, ci_log + 2, co), 5 + co)
    pad_y, pad_x = A.same_pad(hi, 3, 2)[1], A.same_pad(wi, 3, 2)[1]
    assert (pad_y, pad_x) == (hi % 2, wi % 2)
    w = A.d2s_image(V, ci_log, co, pad_y, pad_x, Cc)
    assert w.shape == (9, A.cdiv(co, 32), 4 * Cc, 32)
    x = torch.zeros(1, hi, wi, ci_log, dtype=torch.float64, requires_grad=True)
    Vm = V[:, :ci_log, :].double().view(3, 3, ci_log, co)
    y = R.conv2d_same(x, Vm, torch.zeros(co, dtype=torch.float64), 2)
    g = torch.randint(-4, 5, tuple(y.shape), generator=A.gen(6)).double()
    (gx,) = torch.autograd.grad((y * g).sum(), x)
    got = A.d2s_input_gradient(w, g[0], Cc, hi, wi)
    assert torch.equal(got[..., :ci_log], gx[0]) and float(gx.abs().max()) > 0
    assert float(got[..., ci_log:].abs().max() if Cc > ci_log else 0.0) == 0.0


# ----------------------------------------------------------------------------- fp8 rows
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("case", A.F8_CASES, ids=_ids)
def test_f8_rows_premises(case, transpose):
    """Row 0 is all zero (sc = deq = 1, zero bytes), row 1 has the maximum 2^-100, row 2 holds +-max (bytes 0x7e and 0xfe); the
    coordinate rows of a CoordConv V, 100 times larger, are not in any maximum; deq * 448 gives the row maximum back to an ulp."""
    name, k, ci_log, coords, co = case
    V = A.f8_weights(case, 21)
    by, deq = A.f8_rows(V, k * k, ci_log, co, transpose)
    rows, kdim = (ci_log, co) if transpose else (co, ci_log)
    assert by.shape == (k * k, A.cdiv(kdim, 64), rows, 64) and deq.shape == (rows,)
    E = V[:, :ci_log, :] if transpose else V[:, :ci_log, :].transpose(1, 2)
    m = E.abs().amax(dim=(0, 2))
    assert float(m[0]) == 0.0 and float(deq[0]) == 1.0 and int(by[:, :, 0].max()) == 0
    assert float(m[1]) == 2.0 ** -100 and float(deq[1]) == float(np.float32(2.0 ** -100) / np.float32(448.0))
    assert 0x7e in by[:, :, 1].flatten().tolist()
    r2 = by[:, :, 2].flatten().tolist()
    assert 0x7e in r2 and 0xfe in r2
    assert bool((m[2:] > 1e-3).all()) and float(m.max()) < 1.0
    if coords:
        assert float(V[:, ci_log:].abs().max()) > 3.0 * float(m.max())
    if kdim % 64:
        assert int(by[:, -1, :, kdim % 64:].max()) == 0
    back = torch.where(m > 0, deq * 448.0, torch.zeros_like(m))
    assert bool(((back - m).abs() <= m * 2.0 ** -22).all())
    # the quantised values, dequantised, are the weights to e4m3's 2^-4 relative step (or its 2^-9 denormal step at scale)
    q = by.permute(0, 2, 1, 3).reshape(k * k, rows, -1)[:, :, :kdim].contiguous().view(torch.float8_e4m3fn).float()
    err = (q * deq.view(1, rows, 1) - E).abs()
    assert bool((err <= E.abs() * 2.0 ** -4 + (deq * 2.0 ** -10).view(1, rows, 1)).all())


# ----------------------------------------------------------------------------- CoordConv table
def _coord_V(k, ci_log, co, seed, integer):
    V = A.int_weights((k * k, ci_log + 2, co), seed) if integer else torch.randn(k * k, ci_log + 2, co, generator=A.gen(seed))
    return V


@pytest.mark.parametrize("k,stride", A.TABLE_KS)
@pytest.mark.parametrize("hi,wi", A.TABLE_DYADIC + A.TABLE_GAUSS + [(8, 9), (1, 5)], ids=lambda v: str(v))
def test_coord_table_is_the_convolution_of_the_coordinate_planes(hi, wi, k, stride):
    """k0 + kj j + ki i, with each pixel's own class, equals the fp64 conv2d_same of add_coordinates(zeros)'s two planes with V's
    coordinate rows -- at h != w, so the oracle's pairing (column / (H - 1), row / (W - 1)) is what is pinned."""
    ci_log, co = 4, 5
    V = _coord_V(k, ci_log, co, 31 + hi + wi, integer=False)
    dy, dx = A.taps(hi, k, stride), A.taps(wi, k, stride)
    ax, ay = 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)                 # fp64 here: the comparison is with the fp64 oracle
    tab = torch.zeros(64, 3, co, dtype=torch.float64)
    Vd = V.double()
    for cls in range(64):                                               # (A.coord_table with unrounded ax, ay)
        for r in range(k):
            for s in range(k):
                if (cls >> 3 >> r) & 1 and (cls & 7) >> s & 1:
                    vx, vy = Vd[r * k + s, ci_log], Vd[r * k + s, ci_log + 1]
                    tab[cls, 0] += (ax * dx[s] - 1.0) * vx + (ay * dy[r] - 1.0) * vy
                    tab[cls, 1] += ax * stride * vx
                    tab[cls, 2] += ay * stride * vy
    got = A.table_map(tab, hi, wi, k, stride, dy, dx)
    x = R.Scope.add_coordinates(torch.zeros(1, hi, wi, ci_log, dtype=torch.float64))
    want = R.conv2d_same(x, Vd.view(k, k, ci_log + 2, co), torch.zeros(co, dtype=torch.float64), stride)[0]
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    assert err <= 1e-12 * max(1.0, float(want.abs().max())), err
    # the restatement proper differs from this one only by ax, ay rounded to fp32
    ax32, ay32 = A.axy(hi, wi)
    ref = A.coord_table(V, k, ci_log, co, dy, dx, stride, ax32, ay32)
    absr = A.coord_table(V, k, ci_log, co, dy, dx, stride, ax32, ay32, absolute=True)
    assert bool(((ref - tab).abs() <= 2.0 ** -23 * absr + 1e-300).all())
    if float(np.float32(ax)) == ax and float(np.float32(ay)) == ay:
        assert torch.equal(ref, tab)


@pytest.mark.parametrize("hi,wi", A.TABLE_DYADIC)
def test_dyadic_maps_have_exact_steps(hi, wi):
    """hi - 1 and wi - 1 are powers of two: ax, ay and every table entry of integer coordinate rows are exact in fp32."""
    ax, ay = A.axy(hi, wi)
    for v in (ax, ay):
        assert float(np.float32(v)) == v and np.log2(v) == int(np.log2(v))
    for k, stride in A.TABLE_KS:
        V = _coord_V(k, 8, 16, 41, integer=True)
        dy, dx = A.taps(hi, k, stride), A.taps(wi, k, stride)
        tab = A.coord_table(V, k, 8, 16, dy, dx, stride, ax, ay)
        absr = A.coord_table(V, k, 8, 16, dy, dx, stride, ax, ay, absolute=True)
        assert torch.equal(tab.float().double(), tab) and float(absr.max()) / min(ax, ay, 1.0) < 2 ** 24


# ----------------------------------------------------------------------------- CoordConv weight gradient
@pytest.mark.parametrize("case", A.WGRAD_DYADIC + A.WGRAD_GAUSS, ids=_ids)
def test_coord_wgrad_is_the_autograd_gradient(case):
    hi, wi, k, stride, co = case
    ci_log = 3
    ho, wo = A.same_pad(hi, k, stride)[0], A.same_pad(wi, k, stride)[0]
    dy, dx = A.taps(hi, k, stride), A.taps(wi, k, stride)
    V = torch.randn(k, k, ci_log + 2, co, generator=A.gen(51), dtype=torch.float64).requires_grad_(True)
    b = torch.zeros(co, dtype=torch.float64, requires_grad=True)
    x = R.Scope.add_coordinates(torch.randn(1, hi, wi, ci_log, generator=A.gen(52), dtype=torch.float64))
    y = R.conv2d_same(x, V, b, stride)
    assert tuple(y.shape) == (1, ho, wo, co)
    g = torch.randn(ho, wo, co, generator=A.gen(53), dtype=torch.float64)
    gV, gb = torch.autograd.grad((y[0] * g).sum(), [V, b])
    ax, ay = 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)
    exact = float(np.float32(ax)) == ax and float(np.float32(ay)) == ay
    ref = A.coord_wgrad(g, hi, wi, k, stride, dy, dx, ax, ay)
    gV = gV.view(k * k, ci_log + 2, co)
    for name, want in (("vx", gV[:, ci_log]), ("vy", gV[:, ci_log + 1]), ("b", gb)):
        bound = (1e-12 if exact else 2.0 ** -23) * ref["abs_" + name] + 1e-300
        assert bool(((ref[name] - want).abs() <= bound).all()), name


@pytest.mark.parametrize("case", A.WGRAD_DYADIC, ids=_ids)
def test_integer_wgrad_cases_are_exact_in_fp32(case):
    """Integer gsum in [-4, 4] on a dyadic map: every term is a multiple of min(ax, ay, 1) and the sum of magnitudes stays below
    2^24 of that unit, so every partial sum of the kernel, in any order, is exact."""
    hi, wi, k, stride, co = case
    ax, ay = A.axy(hi, wi)
    for v in (ax, ay):
        assert float(np.float32(v)) == v and np.log2(v) == int(np.log2(v))
    ho, wo = A.same_pad(hi, k, stride)[0], A.same_pad(wi, k, stride)[0]
    worst = torch.full((ho, wo, co), 4.0)
    ref = A.coord_wgrad(worst, hi, wi, k, stride, A.taps(hi, k, stride), A.taps(wi, k, stride), ax, ay)
    unit = min(ax, ay, 1.0)
    assert max(float(ref[n].max()) for n in ("abs_vx", "abs_vy", "abs_b")) / unit < 2 ** 24


def test_integer_sum_cases_are_exact_in_fp32():
    for n, pix, co, ldo in A.BATCH_SUM_CASES + [A.BATCH_SUM_BIG]:
        assert 4 * n < 2 ** 24 and ldo % 8 == 0 and ldo >= co
    for rows, co, ldo in A.COL_SUM_CASES:
        assert 4 * rows < 2 ** 24 and ldo >= co
    n, pix, co, ldo = A.BATCH_SUM_BIG
    assert 2 * 16384 * 256 > pix * A.cdiv(co, 8) > 16384 * 256            # past the grid cap: a second trip for the first threads
    assert [A.col_sum_blocks(r, c) for r, c, _ in A.COL_SUM_CASES] == [(32, 1), (256, 3), (32, 157)]


# ----------------------------------------------------------------------------- the batched list
def _prep_item(lib, it, dtype):
    ntaps, cin_v, ci_pad, drows, dk = A.item_geometry(it, dtype)[:5]
    p = lib.PrepItem()
    p.src, p.w_fwd, p.w_dgrad, p.ctab = 16, (16 if it.fwd else None), (16 if it.dgrad else None), (16 if it.tab else None)
    p.ntaps, p.cin_v, p.ci_log, p.co, p.ci_pad, p.dgrad_rows, p.dgrad_k = ntaps, cin_v, it.ci_log, it.co, ci_pad, drows, dk
    return p


@pytest.mark.parametrize("dtype", DTYPES, ids=A.DT_NAME.get)
def test_batched_list_sits_where_the_cases_say(dtype):
    """The prefix, from ups_prep_item_blocks as ops.PrepRegistry builds it, and the path of every chunk, from the kernel's own two
    constants: in the 16-bit lists item co64_coord starts at chunk 14 of a block -- two chunks fall back at j = 14, 15, two more at
    j = 0, 1 of the next block (c0i = 2, 3), the 4-chunk unit starts at c0i = 4 --, its aligned twin takes the unit from c0i = 0,
    the view at element 1 never does, and the launch holds every path; fp32 items take the scalar path and the table alone."""
    lib = _lib()
    h = lib.load()
    cpb, lds_items = h.ups_prep_chunks_per_block(), h.ups_prep_lds_items()
    assert (cpb, lds_items) == (16, 1024)
    prefix = [0]
    for it in A.BATCH_ITEMS:
        n = h.ups_prep_item_blocks(C.byref(_prep_item(lib, it, dtype)), dtype)
        assert n == A.item_chunks(it, dtype), it.name
        prefix.append(prefix[-1] + n)
    routes = A.batch_routes(A.BATCH_ITEMS, prefix, dtype, cpb)
    kinds = set(r[3] for r in routes)
    names = [it.name for it in A.BATCH_ITEMS]
    if dtype == F32:
        assert kinds == {"scalar", "table"}
        return
    assert prefix == A.BATCH_PREFIX_16BIT
    assert kinds == {"unit4", "turn8", "scalar", "table"}
    i = names.index("co64_coord")
    assert prefix[i] % cpb == 14 and A.BATCH_ITEMS[i].co % 32 == 0
    mine = [(c0i, j, route) for n, c0i, j, route in routes if n == i]
    assert mine[:6] == [(0, 14, "turn8"), (1, 15, "turn8"), (2, 0, "turn8"), (3, 1, "turn8"), (4, 2, "unit4"), (8, 6, "scalar")]
    assert [r for r in mine if r[2] == "table"][0][0] == 16 and mine[-1][0] == 31
    twin = [(c0i, j, route) for n, c0i, j, route in routes if n == names.index("co64_aligned")]
    assert twin[:2] == [(0, 0, "unit4"), (4, 4, "unit4")]
    view = [route for n, c0i, j, route in routes if n == names.index("co64_view")]
    assert "unit4" not in view and view.count("turn8") == 8
    # an item boundary inside a block, and a block that ends the launch short
    assert any(prefix[n] % cpb for n in range(1, len(prefix) - 1)) and prefix[-1] % cpb
    assert set(r[3] for r in routes if r[0] == names.index("co10")) == {"scalar"}
    assert set(r[3] for r in routes if r[0] == names.index("co24")) == {"turn8", "scalar"}
    assert 1030 > lds_items


def test_per_layer_big_case_reaches_a_third_trip():
    name, k, ci_log, coords, co = A.PREP_BIG
    ntaps, cin_v, ci_pad, drows, dk, nf, nd, nc = A.item_geometry(A.item(name, k, ci_log, coords, co), BF16)
    assert nf + nd > 2 * 8192 * 256 and nf + nd < 2 ** 31


def test_header_declares_the_new_entry_points():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    for name in ("ups_prep_chunks_per_block", "ups_prep_lds_items"):
        assert name in lib.EXPORTS and re.search(r"\b{}\s*\(".format(name), hdr) and hasattr(lib.load(), name), name


def test_sum_entry_points_refuse_fp16_on_the_host():
    """The dtype check stands in front of every launch and of the pointer's use: non-NULL, aligned, never dereferenced."""
    lib = _lib()
    p = C.c_void_p(4096)
    for args in (("ups_batch_sum", p, F16, 1, 1, 8, 8, p, None), ("ups_col_sum", p, F16, 1, 8, 8, p, p, None),
                 ("ups_batch_sum", p, 3, 1, 1, 8, 8, p, None), ("ups_col_sum", p, -1, 1, 8, 8, p, p, None)):
        with pytest.raises(lib.UpsError, match="argument check failed: dtype == UPS_F32"):
            lib.call(*args)
