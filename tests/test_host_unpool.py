"""CPU side of the un-pool backward edge tests: every case of unpool_ref.py takes the route its name claims, by
ups_unpool_bwd_plan -- the function ups_unpool_bwd itself launches from --, its inputs hold what the case rests on (planted rows,
integer headroom below 2^24, padding channels), and the fp64 restatement agrees with torch.autograd over the einsum statement of
test_gpu_kernels.py::test_mask_parts_unpool.  No GPU: the plan is host code."""
import ctypes as C

import pytest
import torch

import unpool_ref as U

F32, BF16 = 0, 1


def _lib():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    return lib


def plan(case, monkeypatch, env=None, aligned16=None):
    """{form, bpi, tpb, tpx, slab_px, lds} of ups_unpool_bwd_plan for the case, under the case's UPS_UNPOOL_MFMA (or `env`)."""
    lib = _lib()
    env = case.env if env is None else env
    if env is None:
        monkeypatch.delenv("UPS_UNPOOL_MFMA", raising=False)
    else:
        monkeypatch.setenv("UPS_UNPOOL_MFMA", env)
    if aligned16 is None:
        aligned16 = int(case.hard_lead == 0 and case.ghard_lead == 0)
    out = (C.c_int64 * 6)()
    lib.call("ups_unpool_bwd_plan", BF16 if case.dtype == "bf16" else F32, case.B, U.hw_of(case), case.P, case.F, case.ldo, aligned16, out)
    return dict(zip(("form", "bpi", "tpb", "tpx", "slab_px", "lds"), [int(v) for v in out]))


@pytest.mark.parametrize("case", U.ALL_CASES, ids=lambda c: c.name)
def test_case_takes_the_route_it_names(case, monkeypatch):
    got = plan(case, monkeypatch)
    direct = got["form"] == 0 and U.direct_copy_reached(case, got["tpx"])
    print("{:32s} {} B {} hw {} P {} F {} ldo {}: form {} bpi {} tiles/block {} tpx {} slab_px {} lds {} direct-copy {}".format(
        case.name, case.dtype, case.B, U.hw_of(case), case.P, case.F, case.ldo, got["form"], got["bpi"], got["tpb"], got["tpx"],
        got["slab_px"], got["lds"], int(direct)))
    assert (got["form"], got["bpi"], got["tpb"], got["tpx"], direct) == (case.form, case.bpi, case.tpb, case.tpx, case.direct), got
    assert got["slab_px"] == got["tpb"] * got["tpx"]
    if case.form == 1:
        assert U.hw_of(case) == got["bpi"] * got["tpb"] * 128 and got["lds"] == 3 * 128 * (2 * case.ldo + 4 * case.P) + 512 * case.P
        # ... and the same arguments with the switch off, or without the alignment, take the generic form
        assert plan(case, monkeypatch, env="0")["form"] == 0
        assert plan(case, monkeypatch, aligned16=0)["form"] == 0
    else:
        assert got["bpi"] == 32 and got["lds"] <= 160 * 1024


def test_routes_the_case_names_promise(monkeypatch):
    """What single cases are there for, beyond the table entry: ring positions, the cap, the LDS size, the ragged tiles."""
    by = U.BY_NAME
    tpbs = {c.tpb for c in U.MFMA_CASES + U.MFMA_BIG}
    assert tpbs == {1, 2, 3, 5, 7, 17}                          # 1: no ring; 2, 3: no slot reuse; 5, 7, 17: reuse, one to five wraps
    for P in U.MFMA_P:
        assert {c.tpb for c in U.MFMA_CASES if c.P == P} == {1, 3, 5, 7, 17}
    big = by["mfma_256x16x32_P25"]
    assert big.B * big.bpi == 512 and U.hw_of(big) // 128 % (2 * big.bpi) == 0     # only the B bpi < 512 term stops the doubling
    assert big.B * U.hw_of(big) * big.ldo * 2 > 21e6
    assert plan(by["gen_1x12x20_P64_bf16"], monkeypatch)["lds"] > 64 * 1024
    assert 256 // 25 == 10 and 256 - 10 * 25 == 6 and 256 // 64 == 4
    c = by["gen_1x75x75_P10_bf16"]
    hw, slab = U.hw_of(c), plan(c, monkeypatch)["slab_px"]
    assert slab == 256 and hw - (hw - 1) // slab * slab == 128 + 121
    c = by["gen_2x17x19_P10_bf16"]
    assert U.hw_of(c) == 128 + 128 + 67
    for name in ("gen_3x7x7_P3_F8_bf16", "gen_3x7x7_P3_F8_f32"):
        c = by[name]
        assert [b * U.hw_of(c) * c.P * 4 % 16 for b in range(3)] == [0, 12, 8]     # hard / g_hard base of images 1, 2: 4-byte aligned
        assert U.hw_of(c) * c.ldo * U.esz(c) % 16 == 0                             # ... while the gradient rows stay 16-byte aligned
    assert by["gen_2x16x24_P3_f32"].ldo == 72 and 128 * 72 * 4 // 16 == 2304
    assert by["gen_2x16x24_P5_ldo96_bf16"].F + by["gen_2x16x24_P5_ldo96_bf16"].P == 69
    for c in U.FALL_CASES:                                       # one change each against the matrix-core case of the same shape
        base = by["mfma_1x16x40_P10"]
        diff = [f for f in ("dtype", "P", "F", "ldo", "env", "hard_lead", "ghard_lead") if getattr(c, f) != getattr(base, f)]
        assert len(diff) == 1 and (c.B, c.H, c.W) == (base.B, base.H, base.W), (c.name, diff)


@pytest.mark.parametrize("case", U.ALL_CASES, ids=lambda c: c.name)
def test_inputs_hold_the_premises_and_the_reference_is_autograd(case):
    B, hw, P, F, ld = case.B, U.hw_of(case), case.P, case.F, case.ldo
    for regime in case.regimes:
        hard, feat, g = U.inputs(case, regime)
        h2, f2, g2 = U.inputs(case, regime)
        assert torch.equal(hard, h2) and torch.equal(feat, f2) and torch.equal(g, g2)          # a pure function of the case
        assert hard.shape == (B, hw, P) and feat.shape == (B, P, F) and g.shape == (B, hw, ld) and g.dtype == U.torch_dtype(case)
        gf = g.float()
        if ld > F + P:
            assert bool((gf[..., F + P:].abs() == 3).all())
        if regime in U.LATTICE:
            lo, hi = (0, 1) if regime == "lattice01" else (-2, 2)
            assert bool(((hard == hard.round()) & (hard >= lo) & (hard <= hi)).all())
            assert torch.equal(hard.bfloat16().float(), hard)
            for t in (feat, gf[..., :F + P]):
                assert bool(((t == t.round()) & (t.abs() <= 4)).all())
            rows = U.planted(case)
            assert {k for _, k in rows} == {"tie", "all", "zero"} and len({px for px, _ in rows}) == len(rows)
            for tile in (0, (hw - 1) // 128):                    # all three kinds in the first and in the last 128-pixel tile
                assert {k for px, k in rows if px // 128 == tile} == {"tie", "all", "zero"}
            for px, kind in rows:
                assert bool((hard[:, px] == U.planted_row(kind, P)).all())
            assert bool((hard[:, 0] != 0).any(dim=1).all()) and bool((hard[:, hw - 1] != 0).any(dim=1).all())
            for kind, n in (("tie", min(2, P)), ("all", P), ("zero", 0)):
                assert float(U.planted_row(kind, P).sum()) == n
            bound_h, bound_f = U.headroom(case, regime)
            assert bound_h == 16 * F + 4 and bound_f <= 8 * hw and max(bound_h, bound_f) < 2 ** 24
        else:
            assert bool((hard[0, 0] == U.planted_row("tie", P)).all())
            assert not bool((hard[0, case.W:case.W + 8] == hard[0, case.W:case.W + 8].round()).all())
            if case.dtype == "bf16":
                assert torch.equal(feat.bfloat16().float(), feat) == (regime == "gauss")
        want_h, want_f = U.reference_of(case, regime, hard, feat, g)
        assert want_h.dtype == torch.float64 and want_h.shape == (B, hw, P) and want_f.shape == (B, P, F)
        if regime in U.LATTICE:
            assert float(want_h.abs().max()) <= bound_h and float(want_f.abs().max()) <= bound_f
            assert torch.equal(want_h, want_h.round()) and torch.equal(want_f, want_f.round())
        # torch.autograd over the statement of test_mask_parts_unpool (the first and last two images of a large batch)
        for sl in ([slice(0, B)] if B <= 4 else [slice(0, 2), slice(B - 2, B)]):
            ho = hard[sl].double().requires_grad_(True)
            fo = (feat.bfloat16().float() if regime == "gauss_f32feat" else feat)[sl].double().requires_grad_(True)
            inj = torch.cat([torch.einsum("bxp,bpf->bxf", ho, fo), ho], dim=2)
            inj.backward(g[sl, :, :F + P].double())
            # d hard of the statement carries the mask's own channel too: g[F + p], the term the kernel adds from the same row
            assert torch.allclose(ho.grad, want_h[sl], rtol=1e-12, atol=1e-12)
            assert torch.allclose(fo.grad, want_f[sl], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,S,P", U.MASK_PARTS_SHAPES)
def test_mask_parts_backward_reference_is_autograd(B, S, P):
    for dtype in (torch.float32, torch.bfloat16):
        for lattice in (False, True):
            view, hard, g = U.mask_parts_inputs(B, S, P, dtype, lattice)
            assert bool((g[..., 3:].float().abs() == 3).all())
            ho = hard.double().requires_grad_(True)
            parts = (view.double().unsqueeze(3) * ho.unsqueeze(4)).permute(3, 0, 1, 2, 4).reshape(P * B, S, S, 3)
            parts.backward(g[..., :3].double())
            want = U.mask_parts_bwd_reference(view, g, B, P)
            assert torch.allclose(ho.grad, want, rtol=1e-12, atol=1e-12)
            if lattice:
                assert torch.equal(want, want.round()) and float(want.abs().max()) <= 48


@pytest.mark.parametrize("fragment,args", [
    ("B >= 1", dict(B=0)), ("hw >= 1", dict(hw=0)), ("P >= 1", dict(P=0)), ("F >= 8", dict(F=0)), ("F >= 8", dict(F=-8)),
    ("F <= 64", dict(F=72, ldo=88)), ("F % 8 == 0", dict(F=60)), ("P <= 64", dict(P=65, ldo=136)), ("ldo >= F + P", dict(ldo=72)),
    ("ldo % 8 == 0", dict(ldo=84))])
def test_plan_refuses_what_the_launch_refuses(fragment, args):
    """ups_unpool_bwd takes its shape checks from the plan: sizes of zero (the kernel divides by P), F outside 8 ... 64 in steps of
    8, P above 64, a row pitch below F + P or not a multiple of 8 -- each on the message of its own argument check."""
    lib = _lib()
    a = dict(B=1, hw=128, P=10, F=64, ldo=80)
    a.update(args)
    out = (C.c_int64 * 6)()
    with pytest.raises(lib.UpsError) as e:
        lib.call("ups_unpool_bwd_plan", BF16, a["B"], a["hw"], a["P"], a["F"], a["ldo"], 1, out)
    assert "argument check failed" in str(e.value) and fragment in str(e.value), str(e.value)
