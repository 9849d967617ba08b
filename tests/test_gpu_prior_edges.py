"""Mask priors and the part path on trained-regime masks (prior_edge_ref.py; parity_ledger.md, section 7): saturated soft-max,
tied pixels (multi-hot `hard`), parts centred on the image border with clipped rectangles, parts absent from an image, and
rectangle centres planted in the four corners -- every form of priors.hip against torch-fp64 autograd over the oracle's building
blocks, on the float32 inputs the kernels see and with the kernels' own rectangle centres handed to the reference.  The bars are
those of test_part_path and test_mask_priors_forward_and_backward."""
import types

import numpy as np
import pytest
import torch

import prior_edge_ref as E
from util import assert_close, elem_excess, rel_err, rms_rel

pytestmark = pytest.mark.gpu


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _finite(what, t):
    assert bool(torch.isfinite(t).all()), "{}: {} non-finite value(s)".format(what, int((~torch.isfinite(t)).sum()))


def _part_path(ops, i, inp, dev):
    """l, m, hard, argmax, bits, closed-form hard-mask moments (or None), the centres px [2 B, P, 2] (row, column) on the device."""
    l, m, hard, am, bits, hstats = ops.part_softmax(inp["lm"].to(dev), inp["eps"].to(dev), want_argmax=True, want_bits=True,
                                                    moments_gamma=E.GAMMA)
    closed = hstats
    if hstats is None:
        hstats = ops.spatial_moments(hard, E.GAMMA)
    return l, m, hard, am, bits, closed, ops.moments_to_px(hstats, i.S, "xy")


@pytest.mark.parametrize("i", E.INPUTS, ids=E.inputs_id)
def test_part_path_on_edge_masks(i, dev):
    """ups_part_softmax(_moments)_fwd -> ups_moments_to_px -> ups_draw_rect -> masked ups_spatial_moments on the same inputs the
    prior kernels get, as test_part_path has it: l bit-equal to the float32 sum, m to 2e-6, `hard` equal to the reference's
    multi-hot map, bit sets and first-maximum arg-max, closed-form moments against the summation kernel, centres against
    R.patch_mask where stable (exactly S / 2 for a part that owns nothing), rectangles bit-equal to np_ops.draw_rect -- clipped and
    corner boxes included -- and the masked variance per part."""
    lib, ops = _mods()
    from oracle import np_ops, ref_model as R
    inp = E.build(i)
    p = E.premises(i, inp, cheap=True)
    E.check_premises(i, p)
    S, P, n = i.S, i.P, 2 * i.B
    l, m, hard, am, bits, closed, px = _part_path(ops, i, inp, dev)
    for what, t in (("l", l), ("m", m), ("hard", hard)):
        _finite(what, t)
    assert torch.equal(l.cpu(), inp["l"]), "l is not the float32 sum"
    mo = torch.softmax(inp["l"].double(), -1)
    assert_close(m, mo.float(), 2e-6, "softmax")
    ho = R.hard_max(mo)
    nd = int((hard.cpu().double() != ho).sum())
    assert nd == 0, "hard differs from the reference's multi-hot map in {} element(s) ({:.1%} of the pixels are tied)".format(nd, p["tied"])
    idx = torch.arange(P).expand(ho.shape)
    assert torch.equal(((bits.cpu().unsqueeze(-1) >> idx) & 1).double(), ho), "bit sets disagree with hard"
    first = torch.where(ho > 0, idx, torch.full_like(idx, P)).min(dim=-1).values
    assert torch.equal(am.cpu(), first), "arg-max is not the first maximum"
    if i.regime == "lattice_ties_noeps":       # eps = None is the same launch without the sum
        l2, m2, hard2, _ = ops.part_softmax(inp["lm"].to(dev), None)
        assert torch.equal(l2, l) and torch.equal(m2, m) and torch.equal(hard2, hard)
    direct = ops.spatial_moments(hard, E.GAMMA)
    _finite("moments of hard", direct)
    if closed is not None:
        _finite("closed-form moments", closed)
        for k in (1, 2, 3, 4, 5, 6):
            assert_close(closed[..., k], direct[..., k], 1e-3, "hard-mask moment {} (closed form vs summation)".format(k), elementwise=False)
    # centres
    rect_o, rc_o, stable = E.oracle_centres(ho, S)
    owned = p["owned"]
    pxc = px.cpu().long()
    assert torch.equal(pxc[stable & owned], rc_o[stable & owned]), "centres differ from R.patch_mask's on stable centres"
    if bool((~owned).any()) and closed is not None:
        assert bool((pxc[~owned] == S // 2).all()), "a part that owns no pixel has its centre at S / 2 exactly: {}".format(pxc[~owned].tolist())
    assert torch.equal(ops.moments_to_px(closed if closed is not None else direct, S, "yx").flip(-1), px)
    sets = [("natural", px)]
    if i.regime == "border_absent":
        sets.append(("planted", torch.cat([E.plant(px[:i.B], S), E.plant(px[i.B:], S)]).contiguous()))
    for name, pxs in sets:
        rect = ops.draw_rect(pxs, S, S, E.HALF)
        rect_np = np_ops.draw_rect(pxs.cpu().numpy().reshape(-1, 2), E.PATCH, E.PATCH, S, S, order="yx").reshape(n, P, S, S).transpose(0, 2, 3, 1)
        assert np.array_equal(rect.cpu().numpy(), rect_np), "draw_rect ({} centres)".format(name)
        assert torch.equal(E.rects(pxs.cpu(), S).float(), torch.from_numpy(rect_np)), "R.draw_rect vs np_ops.draw_rect"
        if name == "natural":
            sel = stable & owned
            assert np.array_equal(rect_np.transpose(0, 3, 1, 2)[sel.numpy()], rect_o.permute(0, 3, 1, 2)[sel].numpy()), "rectangles vs R.patch_mask"
        st2 = ops.spatial_moments(m, E.GAMMA, rect_px=pxs, half=E.HALF)
        _finite("masked moments", st2)
        v_o = E.variance_per_part(mo, E.rects(pxs.cpu(), S), E.GAMMA)
        Z = st2[..., 1]
        v = st2[..., 5] / Z - (st2[..., 3] / Z) ** 2 - (st2[..., 4] / Z) ** 2
        assert_close(v, v_o.float(), 1e-4, "variance per part ({} centres)".format(name))


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_mask_priors_on_edge_masks(case, dev, monkeypatch):
    """ups_prior_fwd / ups_prior_bwd through Trainer._prior: every logged sum (as Trainer.build_logs derives it) within
    2e-4 * max(|ref|, 1e-6), `dl` and `dl_rec` of both views and the total-only `dl` (the staged backward at every shape) within
    1e-3 on all three bars of assert_close, every output finite (the maps are handed in filled with NaN)."""
    lib, ops = _mods()
    from upsparts_amd.model import Trainer
    i = case.inputs
    inp = E.build(i)
    E.check_premises(i, E.premises(i, inp, cheap=True))
    if case.px_bpi:
        monkeypatch.setenv("UPS_PRIOR_PX_BPI", str(case.px_bpi))
    variant, P, S, B = i.variant, i.P, i.S, i.B
    w = dict(E.WEIGHTS)
    if variant == 1:
        w.update({"ms": 0.0, "area": 0.0, "patch": 0.0})
    ms_alpha, ms_lambda = E.MS[variant]
    stair = lambda v: {"var_type": "staircase", "options": {"start": 0, "start_value": v, "step_size": 1, "stair_factor": 1.0, "clip_min": v, "clip_max": v}}
    cfg = {"entropy_func": i.entropy_func, "gamma": E.GAMMA, "mumford_sha_alpha": stair(ms_alpha), "mumford_sha_lambda": stair(ms_lambda)}
    fake = types.SimpleNamespace(model=types.SimpleNamespace(patch_size=E.PATCH, df=variant == 1), config=cfg, global_step=0)

    # ---- HIP: the part path, then the product's own descriptor filling (Trainer._prior) on a stand-in trainer
    lmd = inp["lm"].to(dev)
    l, m, hard, _, _, _, px = _part_path(ops, i, inp, dev)
    px0, px1 = px[:B].contiguous(), px[B:].contiguous()
    if case.planted:
        px0, px1 = E.plant(px0, S).contiguous(), E.plant(px1, S).contiguous()
    pxa, pxb = (px0, px1) if variant == 0 else (None, None)          # SB_model48c draws no rectangles
    nfl = lib.load().ups_prior_sums_floats(B, P)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    sums0, sums1, sums1b = nan(nfl), nan(nfl), nan(nfl)
    per_np0 = nan(B, P, 8)
    l0, l1, m0, m1 = l[:B].contiguous(), l[B:].contiguous(), m[:B].contiguous(), m[B:].contiguous()
    h0, lm0d = hard[:B].contiguous(), lmd[:B].contiguous()
    Trainer._prior(fake, 0, B, S, P, l0, lm0d, m0, h0, pxa, per_np0, sums0, w)
    Trainer._prior(fake, 1, B, S, P, l1, None, m1, None, pxb, None, sums1, w)
    g1 = 1.0 if variant == 1 else E.GAMMA
    stats_v = ops.spatial_moments(m1, g1, rect_px=pxb, half=E.HALF)
    stats_vb = ops.spatial_moments(m1, g1, rect_px=pxb, half=E.HALF, kl_sums=sums1b)      # the product path: view 1's KL from this pass
    assert torch.equal(stats_vb, stats_v)
    assert abs(float(sums1b[0]) - float(sums1[0])) <= 1e-5 * abs(float(sums1[0])) and float(sums1b[1:16].abs().max()) == 0.0
    gh = inp["g_hard"].to(dev)
    dl_tot, dl_rec, dl_st = nan(*lmd.shape), nan(*lmd.shape), nan(*lmd.shape)
    Trainer._prior(fake, 0, B, S, P, l0, lm0d, m0, h0, pxa, per_np0, sums0, w, gh[:B].contiguous(), dl_tot[:B], bwd=True, dl_rec=dl_rec[:B])
    Trainer._prior(fake, 1, B, S, P, l1, None, m1, None, pxb, stats_v, sums1, w, gh[B:].contiguous(), dl_tot[B:], bwd=True, dl_rec=dl_rec[B:])
    # a caller that asks for the total alone gets the staged kernel at every shape
    Trainer._prior(fake, 0, B, S, P, l0, lm0d, m0, h0, pxa, per_np0, sums0, w, gh[:B].contiguous(), dl_st[:B], bwd=True)
    Trainer._prior(fake, 1, B, S, P, l1, None, m1, None, pxb, stats_v, sums1, w, gh[B:].contiguous(), dl_st[B:], bwd=True)

    # ---- finiteness: the saturated regime's own assertion (NaN compares false with every bar, but say it by name)
    for what, t in (("dl", dl_tot), ("dl_rec", dl_rec), ("dl alone", dl_st), ("sums view 0", sums0[:16]), ("sums view 1", sums1[:16]),
                    ("per-part records", per_np0[..., :4]), ("moments view 1", stats_v)):
        _finite(what, t)

    # ---- the reference, on the centres the kernels were given
    q, d = E.reference(i, inp, px0.cpu().long(), px1.cpu().long())
    npx = float(B * S * S)
    s0, s1, sv = sums0.double().cpu(), sums1.double().cpu(), stats_v.double().cpu()
    got = {"mask0_kl": (s0[0] + s1[0]) / npx, "weakly": s0[1] / npx, "gmrf": s0[3] / B}
    Zs = sv[..., 1]
    if variant == 0:
        got.update({"patch": s0[2] / B, "ms": s0[4] / B, "area": s0[5] / B, "smooth": s0[6] / B, "contour": s0[7] / B,
                    "var": (sv[..., 5] / Zs - (sv[..., 3] / Zs) ** 2 - (sv[..., 4] / Zs) ** 2).sum(dim=1).mean()})
    else:
        s00 = sv[..., 6] / Zs - (sv[..., 3] / Zs) ** 2
        s11 = (sv[..., 5] - sv[..., 6]) / Zs - (sv[..., 4] / Zs) ** 2
        got.update({"msl": s0[2] / B, "var": (s00 ** 2 + s11 ** 2).sum(dim=1).mean()})
    assert set(got) == set(q)
    bad = []
    for k, v in got.items():
        ref = float(q[k])
        err = abs(float(v) - ref) / max(abs(ref), 1e-6)
        print("prior {:9s} oracle {: .9e} hip {: .9e} rel {:.2e}".format(k, ref, float(v), err))
        if not err <= 2e-4:
            bad.append("prior {} ({}): oracle {} hip {}".format(k, case.id, ref, float(v)))
    assert not bad, "; ".join(bad)
    maps = [("view 0 dl", dl_tot[:B], d["d_tot0"]), ("view 1 dl", dl_tot[B:], d["d_tot1"]), ("view 0 dl_rec", dl_rec[:B], d["d_rec0"]),
            ("view 1 dl_rec", dl_rec[B:], d["d_rec1"]), ("view 0 dl alone", dl_st[:B], d["d_tot0"]), ("view 1 dl alone", dl_st[B:], d["d_tot1"])]
    for what, a, b in maps:
        print("prior_bwd {:15s} max-rel {:.2e} rms-rel {:.2e} element bound used {:.3f}".format(
            what, rel_err(a, b.float()), rms_rel(a, b.float()), elem_excess(a, b.float(), 1e-3)))
    for what, a, b in maps:
        assert_close(a, b.float(), 1e-3, "prior_bwd {} ({})".format(what, case.id))
