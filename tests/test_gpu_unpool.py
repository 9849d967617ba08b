"""ups_unpool_bwd at its edges, through the C ABI, against the fp64 restatement of unpool_ref.py: the three-slot ring of the
matrix-core form at 1, 2, 3, 5, 7 and 17 tiles per block, and every route of the generic form -- ragged slabs, several tiles per slab,
the direct-copy loop, tpx = 32, P = 1 and 64, unaligned hard / g_hard (parity_ledger.md, section 10, has the branch -> case table;
test_host_unpool.py holds each case to the route ups_unpool_bwd_plan gives it).  Every launch writes into NaN-filled results with
64 sentinel floats behind them and is made twice: the two results have the same bits.  The lattice regimes are compared with
torch.equal, the Gaussian regime at the bars of test_gpu_kernels.py; the figures are printed before they are asserted."""
import ctypes as C

import pytest
import torch

import unpool_ref as U
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu

SENT = -777.0           # sentinel of the guard bands: not a value these kernels write
GUARD = 64


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _setenv(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("UPS_UNPOOL_MFMA", raising=False)
    else:
        monkeypatch.setenv("UPS_UNPOOL_MFMA", env)


def _planned_form(lib, case, aligned16):
    out = (C.c_int64 * 6)()
    lib.call("ups_unpool_bwd_plan", lib.BF16 if case.dtype == "bf16" else lib.F32, case.B, U.hw_of(case), case.P, case.F, case.ldo,
             int(aligned16), out)
    return int(out[0])


def _lead_view(t, lead, dev):
    """t on the device as a view `lead` elements into a larger 16-byte-aligned buffer."""
    buf = torch.empty(lead + t.numel(), dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[lead:] = t.reshape(-1).to(dev)
    return buf[lead:]


def _launch(lib, case, hd, fd, gd, dev):
    """One ups_unpool_bwd into NaN-filled g_hard and g_feat (scratch included), SENT before and behind them.
    -> g_hard [B, hw, P], g_feat [B, P, F] on the host."""
    B, hw, P, F = case.B, U.hw_of(case), case.P, case.F
    lead, n_h = case.ghard_lead, B * hw * P
    nfl = lib.load().ups_unpool_bwd_floats(B, P, F)
    gh = torch.full((lead + n_h + GUARD,), float("nan"), device=dev)
    gf = torch.full((nfl + GUARD,), float("nan"), device=dev)
    gh[:lead] = SENT
    gh[lead + n_h:] = SENT
    gf[nfl:] = SENT
    assert gh.data_ptr() % 16 == 0 and gf.data_ptr() % 16 == 0
    lib.call("ups_unpool_bwd", lib.ptr(hd), lib.ptr(fd), lib.ptr(gd), lib.ptr(gh[lead:lead + n_h]), lib.ptr(gf), lib.dt(gd), B, hw, P, F,
             case.ldo, lib.stream())
    torch.cuda.synchronize()
    gh, gf = gh.cpu(), gf.cpu()
    assert bool((gh[:lead] == SENT).all()) and bool((gh[lead + n_h:] == SENT).all()), "g_hard: a guard band was written"
    assert bool((gf[nfl:] == SENT).all()), "g_feat: the guard band behind the scratch was written"
    return gh[lead:lead + n_h].view(B, hw, P), gf[:B * P * F].view(B, P, F)


def _run(lib, case, regime, env, dev, monkeypatch, data):
    """The case under UPS_UNPOOL_MFMA=env (None: unset), twice; -> (g_hard, g_feat) after the checks every case gets."""
    hard, feat, g = data
    _setenv(monkeypatch, env)
    hd = _lead_view(hard, case.hard_lead, dev)
    fd, gd = feat.to(dev), g.to(dev)
    aligned = all(t.data_ptr() % 16 == 0 for t in (hd, gd)) and case.ghard_lead == 0
    assert aligned == (case.hard_lead == 0 and case.ghard_lead == 0)
    want_form = case.form if env == case.env else 0
    assert _planned_form(lib, case, aligned) == want_form, "the case is not on the route it names"
    gh, gf = _launch(lib, case, hd, fd, gd, dev)
    gh2, gf2 = _launch(lib, case, hd, fd, gd, dev)
    assert not bool(torch.isnan(gh).any()), "g_hard: " + U.first_difference(gh, gh)
    assert not bool(torch.isnan(gf).any()), "g_feat: " + U.first_difference(gf, gf, "part")
    assert torch.equal(gh.view(torch.int32), gh2.view(torch.int32)) and torch.equal(gf.view(torch.int32), gf2.view(torch.int32)), \
        "two launches differ: g_hard {}, g_feat {}".format(U.first_difference(gh, gh2), U.first_difference(gf, gf2, "part"))
    return gh, gf


def _hold(case, regime, got, want, what):
    """One form's results against the fp64 reference: by value in the lattice regimes, at the existing bars in the Gaussian one."""
    (gh, gf), (want_h, want_f) = got, want
    if regime in U.LATTICE:
        dh, df = U.first_difference(gh, want_h.float()), U.first_difference(gf, want_f.float(), "part")
        assert dh is None and df is None, "{} {} {}: g_hard {}; g_feat {}".format(case.name, regime, what, dh, df)
        return
    print("{} {} {}: d hard max-rel {:.3e} (bar 1e-5), d feat max-rel {:.3e} (bar {})".format(
        case.name, regime, what, rel_err(gh, want_h), rel_err(gf, want_f), "2e-5" if case.dtype == "bf16" else "1e-5"))
    assert_close(gh, want_h.float(), 1e-5, "{} unpool d hard ({})".format(case.name, what))
    if case.dtype == "bf16":         # test_unpool_backward_on_the_matrix_cores
        assert_close(gf, want_f.float(), 2e-5, "{} unpool d feat ({})".format(case.name, what), elementwise=False)
    else:                            # test_mask_parts_unpool
        assert_close(gf, want_f.float(), 1e-5, "{} unpool d feat ({})".format(case.name, what))


def _data_and_reference(case, regime):
    if regime in U.LATTICE:
        bound_h, bound_f = U.headroom(case, regime)
        assert max(bound_h, bound_f) < 2 ** 24
    data = U.inputs(case, regime)
    return data, U.reference_of(case, regime, *data)


def _case_regimes(cases):
    return [pytest.param(c, r, id="{}-{}".format(c.name, r)) for c in cases for r in c.regimes]


@pytest.mark.parametrize("case,regime", _case_regimes(U.MFMA_CASES + U.MFMA_BIG + [U.F32FEAT_CASE]))
def test_matrix_core_form_over_the_ring(case, regime, dev, monkeypatch):
    """unpool_bwd_mfma_kernel at 1 to 17 tiles per block, one and several blocks per image and images per batch, and the generic form
    on the same inputs (UPS_UNPOOL_MFMA=0): each against fp64, and d hard of the two forms against each other."""
    lib, ops = _mods()
    data, want = _data_and_reference(case, regime)
    mf = _run(lib, case, regime, None, dev, monkeypatch, data)
    _hold(case, regime, mf, want, "matrix cores")
    va = _run(lib, case, regime, "0", dev, monkeypatch, data)
    _hold(case, regime, va, want, "UPS_UNPOOL_MFMA=0")
    if regime not in U.LATTICE:
        print("{} {}: d hard, matrix cores vs generic form {:.3e} (bar 1e-5)".format(case.name, regime, rel_err(mf[0], va[0])))
        assert_close(mf[0], va[0], 1e-5, "MFMA vs VALU form, d hard")


@pytest.mark.parametrize("case,regime", _case_regimes(U.FALL_CASES + U.GENERIC_CASES))
def test_generic_form_routes(case, regime, dev, monkeypatch):
    """unpool_bwd_kernel where it takes another path (the case's `reaches`), and every single reason that sends a matrix-core shape
    to it."""
    lib, ops = _mods()
    data, want = _data_and_reference(case, regime)
    _hold(case, regime, _run(lib, case, regime, case.env, dev, monkeypatch, data), want, "generic form")


@pytest.mark.parametrize("regime", U.REGIMES)
def test_unpool_fn_with_a_strided_incoming_gradient(regime, dev, monkeypatch):
    """ops.UnpoolFn.backward makes its incoming gradient contiguous: every other channel of a tensor twice as wide.  (The results are
    allocated by the function itself here: no NaN fill, no guard bands.)"""
    lib, ops = _mods()
    case = U.FN_CASE
    _setenv(monkeypatch, None)
    (hard, feat, g), want = _data_and_reference(case, regime)
    B, H, W, P, F, ld = case.B, case.H, case.W, case.P, case.F, case.ldo
    hd = hard.view(B, H, W, P).to(dev).requires_grad_(True)
    fd = feat.to(dev).requires_grad_(True)
    out = ops.UnpoolFn.apply(hd, fd, U.torch_dtype(case))
    assert out.shape == (B, H, W, ld)
    wide = torch.zeros(B, H, W, 2 * ld, dtype=g.dtype, device=dev)
    wide[..., ::2] = g.view(B, H, W, ld).to(dev)
    gd = wide[..., ::2]
    assert not gd.is_contiguous()
    res = [torch.autograd.grad([out], [hd, fd], grad_outputs=[gd], retain_graph=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    _hold(case, regime, (res[0][0].cpu().view(B, H * W, P), res[0][1].cpu()), want, "UnpoolFn")


def test_unpool_bwd_refusals(dev, monkeypatch):
    """Sizes of zero, F = 0 (the kernel divides by P and walks F in groups of 8), a gradient that is not 16-byte aligned, and the
    existing refusals (F = 72, P = 65, ldo < F + P): each on the message of its argument check, which is before any launch -- the
    NaN-filled results stay as they are."""
    lib, ops = _mods()
    _setenv(monkeypatch, None)
    B, hw, P, F, ld = 1, 128, 10, 64, 80
    hd = torch.zeros(2 * hw * 80, device=dev)
    fd = torch.zeros(80 * 80, device=dev)
    gd = torch.zeros(2 * hw * 160 + 8, dtype=torch.bfloat16, device=dev)
    gh = torch.full((2 * hw * 80,), float("nan"), device=dev)
    gf = torch.full((lib.load().ups_unpool_bwd_floats(2, 80, 80),), float("nan"), device=dev)
    assert gd.data_ptr() % 16 == 0

    def refused(fragment, g=gd, B=B, hw=hw, P=P, F=F, ld=ld):
        with pytest.raises(lib.UpsError) as e:
            lib.call("ups_unpool_bwd", lib.ptr(hd), lib.ptr(fd), lib.ptr(g), lib.ptr(gh), lib.ptr(gf), lib.BF16, B, hw, P, F, ld, lib.stream())
        assert "argument check failed" in str(e.value) and fragment in str(e.value), str(e.value)

    refused("B >= 1", B=0)
    refused("hw >= 1", hw=0)
    refused("P >= 1", P=0)
    refused("F >= 8", F=0)
    refused("F >= 8", F=-8)
    refused("& 15", g=gd[1:])                   # 2 bytes off
    refused("& 15", g=gd[4:])                   # 8 bytes off
    refused("F <= 64", F=72, ld=88)
    refused("P <= 64", P=65, ld=136)
    refused("ldo >= F + P", ld=72)
    refused("ldo % 8 == 0", ld=84)
    refused("F % 8 == 0", F=60)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gh).all()) and bool(torch.isnan(gf).all())
    lib.call("ups_unpool_bwd", lib.ptr(hd), lib.ptr(fd), lib.ptr(gd), lib.ptr(gh), lib.ptr(gf), lib.BF16, B, hw, P, F, ld, lib.stream())
    torch.cuda.synchronize()
    assert float(gh[:hw * P].abs().max()) == 0.0 and float(gf[:P * F].abs().max()) == 0.0      # ... and the same buffers are accepted


# ----------------------------------------------------------------------------- mask_parts backward over tiles
@pytest.mark.parametrize("B,S,P", U.MASK_PARTS_SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lattice", [False, True], ids=["gauss", "lattice"])
def test_mask_parts_backward_over_tiles(B, S, P, dtype, lattice, dev):
    """mask_parts_bwd_kernel over whole, partial and unaligned 256-pixel tiles that span image borders (the shapes and the bars of
    test_mask_parts_forward_over_tiles), through ops.MaskPartsFn against fp64; integers by value."""
    lib, ops = _mods()
    view, hard, g = U.mask_parts_inputs(B, S, P, dtype, lattice)
    want = U.mask_parts_bwd_reference(view, g, B, P)
    hd = hard.to(dev).requires_grad_(True)
    out = ops.MaskPartsFn.apply(view.to(dev), hd, dtype)
    gd = g.to(dev)
    res = [torch.autograd.grad([out], [hd], grad_outputs=[gd], retain_graph=True)[0] for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))
    gh = res[0].cpu()
    assert gh.shape == (B, S, S, P) and not bool(torch.isnan(gh).any())
    if lattice:
        diff = U.first_difference(gh.view(B, S * S, P), want.float().view(B, S * S, P))
        assert diff is None, diff
    else:
        tol = 1e-6 if dtype == torch.float32 else 1e-2
        print("mask_parts bwd B {} S {} P {} {}: max-rel {:.3e} (bar {:.0e})".format(B, S, P, dtype, rel_err(gh, want), tol))
        assert_close(gh, want.float(), tol, "mask_parts bwd")
