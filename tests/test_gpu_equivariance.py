"""GPU tests of the part-equivariance metric: ups_part_equivariance and ups_tps_grid (csrc/equivariance.hip, through the C ABI) against
the NumPy float64 restatement of equivariance_ref.py and the fp64 TPS of oracle/tps.py, the evaluator, `val_metrics: [equivariance]`
in the trainer and `eval_metrics` in `-e`.  Integers compare with ==; tv within the summation-order bound HW 2^-53 sum t per image.
Every output and scratch buffer sits between guard bands (test_gpu_valmetrics._Guarded)."""
import copy
import ctypes as C
import logging

import numpy as np
import pytest
import torch

import equivariance_ref as Q
import trainer_kernels_ref as T
from oracle import tps as OT
from parteval_ref import write_label_dataset
from test_gpu_valmetrics import E_ARG, E_UNSUPPORTED, FSENT, VGG_W, _Guarded, _train, _val_blocks
from util import assert_close

pytestmark = pytest.mark.gpu

SHIPPED = {"scal": 0.8, "tps_scal": 0.15, "rot_scal": 0.2, "off_scal": 0.2, "scal_var": 0.1, "augm_scal": 1.0}


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil, lib, ops
    return lib, ops, evalutil


def _launch(L, dev, soft_a, soft_b, pred_b, grid, prefill=None, P=None):
    """ups_part_equivariance on NumPy operands -> (rc, counts, invalid, tv, scratch) as _Guarded buffers.  P: the P handed to the entry
    (default: the maps')."""
    N, h, w, Pm = soft_a.shape
    P = Pm if P is None else P
    lib = L.load()
    ta, tb = torch.from_numpy(soft_a).to(dev), torch.from_numpy(soft_b).to(dev)
    tp, tg = torch.from_numpy(pred_b.astype(np.int64)).to(dev), torch.from_numpy(grid).to(dev)
    nbytes = lib.ups_part_equivariance_scratch_bytes(N, h * w)
    assert nbytes % 8 == 0
    counts, invalid = _Guarded(dev, N * max(P, 1) ** 2), _Guarded(dev, 1)
    if prefill is not None:
        counts.view.copy_(torch.from_numpy(prefill.reshape(-1)).to(dev))
    tv = _Guarded(dev, N, torch.float64, float("nan"))
    scratch = _Guarded(dev, max(1, nbytes // 8), torch.float64, FSENT)
    rc = lib.ups_part_equivariance(L.ptr(ta), L.ptr(tb), L.ptr(tp), L.ptr(tg), N, h, w, P, counts.ptr(), invalid.ptr(), tv.ptr(),
                                   scratch.ptr(), L.stream())
    torch.cuda.synchronize(dev)
    return rc, counts, invalid, tv, scratch


def _tps_grid_of_uniforms(dev, N, h, w, seed):
    """The output of ups_tps_grid for seeded uniforms and the shipped parameters, as NumPy."""
    _, ops, E = _mods()
    from upsparts_amd import tps
    u = E.equivariance_uniforms(N, seed).to(dev)
    coord, _, Tm = tps.tps_system(u, SHIPPED)
    return ops.tps_grid(Tm, coord, h, w).cpu().numpy()


CH = 1024       # = ops.PART_EQUIVARIANCE_CHUNK (asserted below): maps of CH - 1, CH and CH + 1 pixels with N = 5
CASES = [  # (N, h, w), P, kind of grid
    ((2, 5, 7), 2, "integer"), ((2, 5, 7), 10, "half"), ((2, 5, 7), 1, "affine"), ((2, 5, 7), 25, "edges"), ((2, 5, 7), 32, "nonfinite"),
    ((2, 5, 7), 10, "tps"),
    ((3, 17, 19), 10, "integer"), ((3, 17, 19), 25, "half"), ((3, 17, 19), 32, "affine"), ((3, 17, 19), 1, "edges"),
    ((3, 17, 19), 2, "nonfinite"), ((3, 17, 19), 32, "tps"),
    ((1, 33, 8), 32, "integer"), ((1, 33, 8), 10, "affine"), ((1, 33, 8), 25, "tps"), ((1, 33, 8), 2, "half"),
    ((5, 33, 31), 10, "affine"), ((5, 33, 31), 32, "nonfinite"), ((5, 33, 31), 25, "integer"),
    ((5, 32, 32), 10, "tps"), ((5, 32, 32), 25, "half"), ((5, 32, 32), 1, "edges"),
    ((5, 25, 41), 2, "integer"), ((5, 25, 41), 32, "edges"), ((5, 25, 41), 10, "tps"),
]
assert {c[1] for c in CASES} == {1, 2, 10, 25, 32} and {c[2] for c in CASES} == set(Q.GRID_KINDS) | {"tps"}
assert {c[0][1] * c[0][2] for c in CASES} >= {CH - 1, CH, CH + 1}


def _case_inputs(dev, shape, P, kind):
    N, h, w = shape
    rng = np.random.RandomState(1000 * P + sum(shape))
    soft_a = Q.tie_maps(N, h, w, P)[0] if kind == "half" else Q.softmax_maps(rng, N, h, w, P)[0]
    soft_b, pred_b = Q.softmax_maps(rng, N, h, w, P)
    grid = _tps_grid_of_uniforms(dev, N, h, w, 7 + h) if kind == "tps" else Q.make_grid(kind, N, h, w)
    return soft_a, soft_b, pred_b, grid


def _check(L, dev, soft_a, soft_b, pred_b, grid, what):
    """One comparison with the restatement: counts added to a pre-filled pattern, invalid, tv, guard bands, and the same bits from a
    second launch.  Returns the restatement's (counts, invalid)."""
    N, h, w, P = soft_a.shape
    want_c, want_bad, want_tv, terms, _ = Q.part_equivariance(soft_a, soft_b, pred_b, grid)
    pattern = (np.arange(N * P * P, dtype=np.int32) % 7 - 2).reshape(N, P, P)
    rc, counts, invalid, tv, scratch = _launch(L, dev, soft_a, soft_b, pred_b, grid, prefill=pattern)
    assert rc == 0, L.load().ups_last_error().decode()
    got_c, got_tv = counts.view.cpu().numpy().reshape(N, P, P), tv.view.cpu().numpy()
    print("equivariance", what, "inside", int(Q.inside_mask(grid, h, w).sum()), "of", N * h * w, "counted", int(want_c.sum()), "invalid",
          want_bad, "max |tv - ref| / bound", float((np.abs(got_tv - want_tv) / np.maximum(Q.tv_atol(h * w, terms), 1e-300)).max()))
    assert np.array_equal(got_c - pattern, want_c), "counts"
    assert int(invalid.view.cpu()) == want_bad
    assert np.isfinite(got_tv).all(), "tv was not written completely"
    assert (np.abs(got_tv - want_tv) <= Q.tv_atol(h * w, terms)).all()
    for g in (counts, invalid, tv, scratch):
        assert g.intact(), "wrote outside an output or the scratch"
    rc, again_c, _, again_tv, _ = _launch(L, dev, soft_a, soft_b, pred_b, grid, prefill=pattern)
    assert rc == 0 and torch.equal(again_tv.view, tv.view) and torch.equal(again_c.view, counts.view)
    return want_c, want_bad


@pytest.mark.parametrize("shape,P,kind", CASES, ids=["{}-P{}-{}".format("x".join(map(str, s)), p, k) for s, p, k in CASES])
def test_part_equivariance_equals_the_restatement(shape, P, kind, dev):
    L, ops, _ = _mods()
    assert ops.PART_EQUIVARIANCE_CHUNK == CH == L.load().ups_part_equivariance_chunk()
    soft_a, soft_b, pred_b, grid = _case_inputs(dev, shape, P, kind)
    ins = Q.inside_mask(grid, shape[1], shape[2])
    assert ins.any() and not ins.all(), "the case must have inside and outside pixels"     # (from the grid alone)
    want_c, want_bad = _check(L, dev, soft_a, soft_b, pred_b, grid, (shape, P, kind))
    assert want_bad == 0 and int(want_c.sum()) == int(ins.sum())


@pytest.mark.parametrize("P", [1, 10])
def test_part_equivariance_on_a_single_pixel(P, dev):
    """(N, h, w) = (1, 1, 1): the one pixel is inside at (0, 0) and (-0.0, 0) and outside anywhere else."""
    L, _, _ = _mods()
    rng = np.random.RandomState(P)
    soft_a, _ = Q.softmax_maps(rng, 1, 1, 1, P)
    soft_b, pred_b = Q.softmax_maps(rng, 1, 1, 1, P)
    seen = []
    for pos in ((0.0, 0.0), (-0.0, 0.0), (0.5, 0.0), (0.0, np.nextafter(np.float32(0), np.float32(1))), (np.nan, 0.0), (0.0, -np.inf)):
        grid = np.array(pos, dtype=np.float32).reshape(1, 1, 1, 2)
        want_c, want_bad = _check(L, dev, soft_a, soft_b, pred_b, grid, ("1x1x1", P, pos))
        assert want_bad == 0
        seen.append(int(want_c.sum()))
    assert seen == [1, 1, 0, 0, 0, 0]


def test_part_equivariance_counts_a_nan_or_a_foreign_label_as_invalid(dev):
    """Each plant moves exactly one pixel from `counts` to `invalid`.  Image 0 of the integer grid samples (y - 1, x + 1): original
    pixel (0, 1) is a tap of output pixel (1, 0) alone (as its (y0, x0) corner), so a NaN there spoils that one pixel."""
    L, _, _ = _mods()
    N, h, w, P = 3, 17, 19, 10
    soft_a, soft_b, pred_b, grid = _case_inputs(dev, (N, h, w), P, "integer")
    assert tuple(grid[0, 1, 0]) == (1.0, 0.0)
    base_c, base_bad = _check(L, dev, soft_a, soft_b, pred_b, grid, "plants: none")
    assert base_bad == 0
    plants = [("soft_a", lambda: soft_a.__setitem__((0, 0, 1, 3), np.nan)), ("soft_b", lambda: soft_b.__setitem__((1, 5, 6, 0), np.nan)),
              ("pred_b = -1", lambda: pred_b.__setitem__((2, 8, 9), -1)), ("pred_b = P", lambda: pred_b.__setitem__((0, 9, 2), P))]
    ins = Q.inside_mask(grid, h, w)
    assert ins[0, 1, 0] and ins[1, 5, 6] and ins[2, 8, 9] and ins[0, 9, 2]
    for k, (name, plant) in enumerate(plants):
        plant()
        c, bad = _check(L, dev, soft_a, soft_b, pred_b, grid, "plants: + " + name)
        assert bad == k + 1 and int(c.sum()) == int(base_c.sum()) - (k + 1), name


@pytest.mark.parametrize("shift", [2.0, 0.5])
def test_closed_forms_on_the_device(shift, dev):
    L, ops, E = _mods()
    soft_a, soft_b, pred_b, grid = Q.closed_form_case(shift)
    _check(L, dev, soft_a, soft_b, pred_b, grid, ("closed form", shift))
    t = lambda a: torch.from_numpy(a).to(dev)
    counts, invalid, tv = ops.part_equivariance(t(soft_a), t(soft_b), t(pred_b), t(grid))
    assert int(invalid) == 0
    c = counts.cpu().numpy()[0]
    res = E.equivariance_from_counts(counts.cpu().numpy(), tv.cpu().numpy(), 24)
    if shift == 2.0:
        assert (c[0, 0], c[2, 0], c[2, 2]) == (4, 8, 4) and int(c.sum()) == 16
        assert res == {"valid": 16 / 24, "agreement": 0.5, "iou": [1 / 3, -1.0, 1 / 3], "miou": 1 / 3, "tv": 0.5}
    else:
        assert (c[0, 0], c[2, 2]) == (12, 8) and int(c.sum()) == 20             # column 2 ties (0.5, 0, 0.5): part 0; column 5 is outside
        assert res["valid"] == 20 / 24 and res["agreement"] == 1.0 and res["tv"] == 2.0 / 20


def test_part_equivariance_refusals_leave_every_output_untouched(dev):
    L, ops, _ = _mods()
    lib = L.load()
    N, h, w = 2, 5, 7
    rng = np.random.RandomState(33)
    soft_a, _ = Q.softmax_maps(rng, N, h, w, 33)
    soft_b, pred_b = Q.softmax_maps(rng, N, h, w, 33)
    grid = Q.make_grid("integer", N, h, w)

    def untouched(counts, invalid, tv, scratch):
        return (int(counts.view.abs().sum()) == 0 and int(invalid.view.cpu()) == 0 and bool(torch.isnan(tv.view).all())
                and bool((scratch.view == FSENT).all()) and all(g.intact() for g in (counts, invalid, tv, scratch)))
    rc, *bufs = _launch(L, dev, soft_a, soft_b, pred_b, grid)                   # P = 33: the host route's business
    assert rc == E_UNSUPPORTED and untouched(*bufs)
    t = lambda a: torch.from_numpy(a).to(dev)
    with pytest.raises(L.UpsError):
        ops.part_equivariance(t(soft_a), t(soft_b), t(pred_b), t(grid))
    rc, *bufs = _launch(L, dev, soft_a, soft_b, pred_b, grid, P=0)
    assert rc == E_ARG and untouched(*bufs)
    ta, tb, tp, tg = t(soft_a[..., :10].copy()), t(soft_b[..., :10].copy()), t(pred_b), t(grid)
    counts, invalid = _Guarded(dev, N * 100), _Guarded(dev, 1)
    tv, scratch = _Guarded(dev, N, torch.float64, float("nan")), _Guarded(dev, 8, torch.float64, FSENT)
    good = [L.ptr(ta), L.ptr(tb), L.ptr(tp), L.ptr(tg), N, h, w, 10, counts.ptr(), invalid.ptr(), tv.ptr(), scratch.ptr(), L.stream()]
    for k in (0, 1, 2, 3, 8, 9, 10, 11):                                        # a NULL pointer
        bad = list(good)
        bad[k] = None
        assert lib.ups_part_equivariance(*bad) == E_ARG, k
    for k, v in ((4, 0), (5, 0), (6, 0), (4, -1), (5, 65536), (7, -3)):         # a size < 1; h * w = 65536 * 7 fits, see below
        bad = list(good)
        bad[k] = v
        if (k, v) == (5, 65536):
            bad[6] = 32768                                                      # h * w = 2^31 > 2^31 - 1
        assert lib.ups_part_equivariance(*bad) == E_ARG, (k, v)
    torch.cuda.synchronize(dev)
    assert untouched(counts, invalid, tv, scratch)
    assert lib.ups_part_equivariance_scratch_bytes(N, 2 ** 31) == 0 and lib.ups_part_equivariance_scratch_bytes(0, 35) == 0
    assert lib.ups_part_equivariance_scratch_bytes(N, CH + 1) == N * 2 * 8


# ---------------------------------------------------------------------------------------------- ups_tps_grid
GRID_SHAPES = [(2, 24, 40, 9), (1, 40, 24, 3), (2, 17, 19, 32), (1, 1, 33, 9)]       # n, h, w, K


def _grid_case(shape, kind):
    """(T, coord) in float32.  affine: zero spline weights, scale 1.3 with 0.5 cross terms and a shift of +-0.4 (the positions leave
    the image across all four borders); spline: oracle.tps.solve_system on jittered control points and random target offsets."""
    n, h, w, K = shape
    g = torch.Generator().manual_seed(77 * GRID_SHAPES.index(shape) + 8)        # (no fp64 position of the one-row case within the edge mask)
    coord = T.tps_control_points(n, K, g).double()
    if kind == "affine":
        Tm = torch.zeros(n, 2, K + 3, dtype=torch.float64)
        Tm[:, 0, 0] = Tm[:, 1, 0] = 0.4 * (1.0 - 2.0 * (torch.arange(n) % 2).double())
        Tm[:, 0, 1], Tm[:, 0, 2] = 1.3, 0.5
        Tm[:, 1, 1], Tm[:, 1, 2] = 0.5, 1.3
    else:
        Tm = OT.solve_system(coord, (torch.rand(n, K, 2, generator=g).double() - 0.5) * 0.3)
    return Tm.float(), coord.float()


class _GuardedF32(object):
    """float32 sibling of _Guarded (whose float sentinel does not fit float32): NaN inside, -3e38 in the bands."""
    SENT = -3.0e38

    def __init__(self, dev, n):
        self.buf = torch.full((64 + n + 64,), self.SENT, dtype=torch.float32, device=dev)
        self.view = self.buf[64:64 + n]
        self.view.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[:64] == self.SENT).all()) and bool((self.buf[-64:] == self.SENT).all())

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())


def _device_grid(L, dev, Tm, coord, n, h, w, K):
    out = _GuardedF32(dev, n * h * w * 2)
    Td, cd = Tm.to(dev), coord.to(dev)
    rc = L.load().ups_tps_grid(L.ptr(Td), L.ptr(cd), out.ptr(), n, h, w, K, L.stream())
    torch.cuda.synchronize(dev)
    return rc, out


@pytest.mark.parametrize("kind", ["affine", "spline"])
@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tps_grid_against_fp64_and_against_the_warp(shape, kind, dev):
    """The grid against oracle.tps.sample_positions in fp64: 2e-5 max(h, w) pixels (three times what an fp32 NumPy restatement of the
    arithmetic differs by; the device's logf is not NumPy's).  And the grid IS the warp's: ups_tps_warp of an image against the fp64
    bilinear form evaluated AT THE DEVICE GRID, with the edge mask, its 2 % cap and the 2e-4 bar of test_tps_warp_against_fp64."""
    L, ops, _ = _mods()
    n, h, w, K = shape
    Tm, coord = _grid_case(shape, kind)
    rc, out = _device_grid(L, dev, Tm, coord, n, h, w, K)
    assert rc == 0, L.load().ups_last_error().decode()
    got = out.view.cpu().view(n, h, w, 2)
    assert bool(torch.isfinite(got).all()) and out.intact()
    x_s, y_s = OT.sample_positions(Tm.double(), coord.double(), h, w)
    px, py = (x_s + 1.0) * w / 2.0, (y_s + 1.0) * h / 2.0
    err = max(float((got[..., 0].double() - px).abs().max()), float((got[..., 1].double() - py).abs().max()))
    if kind == "affine":
        assert all(v > 0 for v in T.tps_border_counts(got[..., 0], got[..., 1], h, w).values())
    # the same through the wrapper
    assert torch.equal(ops.tps_grid(Tm.to(dev), coord.to(dev), h, w).cpu(), got)
    img = T.tps_image(n, h, w, 3)
    warped = torch.full((img.numel() + 8,), -3.0e38, dtype=torch.float32, device=dev)
    imgd, Td, cd = img.to(dev), Tm.to(dev), coord.to(dev)
    L.call("ups_tps_warp", L.ptr(imgd), L.ptr(Td), L.ptr(cd), L.ptr(warped), n, h, w, 3, K, L.stream())
    warped = warped.cpu()[:img.numel()].view(n, h, w, 3)
    gx, gy = got[..., 0].double(), got[..., 1].double()
    want = torch.from_numpy(Q.bilinear_at(img.numpy(), gx.numpy(), gy.numpy()))
    keep = T.tps_edge_mask(gx, gy, h, w)
    masked = 1.0 - float(keep.double().mean())
    werr = float((warped.double() - want)[keep].abs().max())
    print("tps_grid {} {}: max |grid - fp64| {:.3e} px (bar {:.3e}); warp at the device grid: masked {:.4f}, max |got - ref| {:.3e}".format(
        shape, kind, err, 2e-5 * max(h, w), masked, werr))
    assert err <= 2e-5 * max(h, w)
    assert masked <= T.TPS_MASK_CAP
    if h == 1 or w == 1:
        assert werr <= 2e-4 * float(img.abs().max())
    else:
        assert_close(warped[keep], want[keep].float(), 2e-4, "warp at the device grid {} {}".format(shape, kind))


def test_tps_grid_refusals(dev):
    L, _, _ = _mods()
    lib = L.load()
    out = _GuardedF32(dev, 4 * 4 * 2)
    Tm, coord = torch.zeros(1, 2, 36, device=dev), torch.zeros(1, 33, 2, device=dev)
    s = L.stream()
    for K in (33, 0, -1):
        assert lib.ups_tps_grid(L.ptr(Tm), L.ptr(coord), out.ptr(), 1, 4, 4, K, s) == E_ARG
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 32768)):
        assert lib.ups_tps_grid(L.ptr(Tm), L.ptr(coord), out.ptr(), n, h, w, 9, s) == E_ARG
    assert lib.ups_tps_grid(None, L.ptr(coord), out.ptr(), 1, 4, 4, 9, s) == E_ARG
    assert lib.ups_tps_grid(L.ptr(Tm), None, out.ptr(), 1, 4, 4, 9, s) == E_ARG
    assert lib.ups_tps_grid(L.ptr(Tm), L.ptr(coord), None, 1, 4, 4, 9, s) == E_ARG
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out.view).all()) and out.intact()


# ---------------------------------------------------------------------------------------------- evaluator
def _tiny(dev, **over):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"precision": "bf16", "vgg_widths": VGG_W, "ckpt_freq": 0, "log_freq": 250})
    cfg.update(over)
    return cfg


def _expected(E, ev, model, views, uniforms, valid=None):
    """The restatement on what the evaluator hands to the kernel: the segment_soft maps and the device grid, copied to the host."""
    soft_a, soft_b, pred_b, grid = (t[:valid].cpu().numpy() for t in ev.maps(model, views, uniforms))
    c, bad, tv, terms, _ = Q.part_equivariance(soft_a, soft_b, pred_b, grid)
    assert bad == 0
    return c, tv, terms


def test_evaluator_equals_the_restatement_on_the_model_s_maps(dev):
    """Five views at batch_size 2 in updates of 3 and 2: originals and warped copies go through segment_soft together (passes of four
    images, the last one padded)."""
    L, ops, E = _mods()
    from upsparts_amd.model import TrainModel
    from oracle import ref_model as R
    cfg = _tiny(dev)
    S, P = cfg["spatial_size"], cfg["n_parts"]
    model = TrainModel(cfg, device=dev, seed=0)
    v = R.synthetic_views(cfg)
    views = torch.cat([torch.as_tensor(v["view0"]), torch.as_tensor(v["view1"]), torch.as_tensor(v["view0"]).flip(1)[:1]], 0).float().to(dev)
    assert tuple(views.shape) == (5, S, S, 3)
    u = E.equivariance_uniforms(5, 11)
    singular = torch.zeros(1, dtype=torch.int32, device=dev)
    ev = E.EquivarianceEvaluator(dev, P, SHIPPED, n_singular=singular)
    c0, tv0, t0 = _expected(E, ev, model, views[:3], u[:3])
    padded, padded_u = torch.cat([views[3:], views[:1]]), torch.cat([u[3:], u[:1]])
    c1, tv1, t1 = _expected(E, ev, model, padded, padded_u, valid=2)
    ev.update(model, views[:3], u[:3])
    ev.update(model, padded, padded_u, valid=2)
    assert ev.n == 5 and ev.HW == S * S
    counts, tv, bad = ev.sums()
    want_c, want_tv, terms = np.concatenate([c0, c1]), np.concatenate([tv0, tv1]), np.concatenate([t0, t1])
    assert bad == 0 and counts.dtype == np.int32 and np.array_equal(counts, want_c)
    assert 0 < int(counts.sum()) < 5 * S * S                                    # some sources are outside, not all
    assert (np.abs(tv - want_tv) <= Q.tv_atol(S * S, terms)).all()
    got, want = ev.result(), Q.equivariance_from_counts(want_c, want_tv, S * S)
    print("evaluator", got)
    assert sorted(got) == sorted(want)
    for k in ("valid", "agreement", "iou", "miou"):
        assert got[k] == want[k], k
    assert abs(got["tv"] - want["tv"]) <= Q.tv_atol(S * S, terms).sum() / counts.sum()
    assert int(singular) == 0
    with pytest.raises(ValueError):
        ev.update(model, views[:2], u[:3])                                      # one row of uniforms per view
    ev.reset()
    assert ev.n == 0
    with pytest.raises(ValueError):
        ev.result()


class _StubModel(object):
    """segment_soft alone: a seeded soft-max of a fixed random projection of the image, P parts (no network takes 40 parts here)."""

    def __init__(self, dev, P):
        g = torch.Generator().manual_seed(40)
        self.proj = (torch.randn(3, P, generator=g) * 4.0).to(dev)
        self.calls = 0

    def segment_soft(self, views):
        self.calls += 1
        soft = torch.softmax(views.float() @ self.proj, dim=-1).contiguous()
        return soft.argmax(dim=-1), soft


def test_more_than_32_parts_take_the_host_route(dev, caplog):
    L, ops, E = _mods()
    P, S = 40, 16
    with caplog.at_level(logging.INFO, logger="upsparts"):
        ev = E.EquivarianceEvaluator(dev, P, SHIPPED)
    assert not ev.on_device and sum("on the host" in r.getMessage() for r in caplog.records) == 1
    model = _StubModel(dev, P)
    views = T.tps_image(3, S, S, 3).to(dev) * 0.4
    u = E.equivariance_uniforms(3, 2)
    want_c, want_tv, terms = _expected(E, ev, model, views, u)
    calls = model.calls
    ev.update(model, views, u)
    assert model.calls == calls + 1                                             # ONE segment_soft per update
    counts, tv, bad = ev.sums()
    assert bad == 0 and np.array_equal(counts, want_c) and 0 < int(counts.sum()) < 3 * S * S
    assert (np.abs(tv - want_tv) <= Q.tv_atol(S * S, terms)).all()
    got, want = ev.result(), Q.equivariance_from_counts(want_c, want_tv, S * S)
    assert got["iou"] == want["iou"] and got["agreement"] == want["agreement"] and got["valid"] == want["valid"]


# ---------------------------------------------------------------------------------------------- trainer: `val_metrics`
def test_val_metrics_equivariance_reports_and_leaves_the_trajectory_alone(dev, tmp_path):
    _, _, E = _mods()
    base = _tiny(dev)
    B, S, P = base["batch_size"], base["spatial_size"], base["n_parts"]
    ds = write_label_dataset(tmp_path, n=5, S=S, seed=4, name="val")
    ds.pop("data_gt_segmentation_column")                                       # no label column in the config
    cfg = dict(base, **ds)
    cfg.update({"val_freq": 2, "val_csv": cfg.pop("data_csv"), "val_metrics": ["equivariance"], "val_seed": 3})
    assert not cfg.get("use_tps")                                               # the metric works without the augmentation
    _, plain_losses, plain_sample, plain_lines, _ = _train(copy.deepcopy(base), dev, 2)
    assert not any("val/" in ln for ln in plain_lines)
    trainer, losses, sample, lines, _ = _train(copy.deepcopy(cfg), dev, 2)
    assert len(losses) == len(plain_losses) == 2
    for s in range(2):
        assert losses[s] == plain_losses[s], s
    for name in plain_sample:
        assert torch.equal(sample[name], plain_sample[name]), name
    logged = _val_blocks(lines)
    assert sorted(logged) == [2]
    got, order = logged[2]
    names = sorted(["val/equiv_agreement", "val/equiv_miou", "val/equiv_tv", "val/equiv_valid"] + ["val/equiv_iou_{}".format(p) for p in range(P)])
    assert order == names + ["val/steps_done"], order
    # the weights are those of step 2: the restatement on the same views and rows of uniforms
    val = trainer._val
    pairs, ev = val["pairs"], val["equiv"]
    assert len(pairs) == 4 and ev.n == 4 and "evaluator" not in val and "rec" not in val and "usage" not in val
    assert torch.equal(val["equiv_uniforms"].cpu(), E.equivariance_uniforms(4, 3))
    cs, tvs, ts = [], [], []
    for ci in range(pairs.chunks()):
        c, tv, terms = _expected(E, ev, trainer.model, pairs.chunk_views(ci, dev)["view0"], val["equiv_uniforms"][ci * B:(ci + 1) * B])
        cs.append(c), tvs.append(tv), ts.append(terms)
    want = Q.equivariance_from_counts(np.concatenate(cs), np.concatenate(tvs), S * S)
    print("val/equiv", got, want)
    assert got["val/equiv_valid"] == want["valid"] and got["val/equiv_agreement"] == want["agreement"] and got["val/equiv_miou"] == want["miou"]
    for p in range(P):
        assert got["val/equiv_iou_{}".format(p)] == want["iou"][p]
    assert abs(got["val/equiv_tv"] - want["tv"]) <= Q.tv_atol(S * S, np.concatenate(ts)).sum() / np.concatenate(cs).sum()
    assert trainer.tps_singular_count() == 0
    assert trainer.fetch_logs()["val/equiv_valid"] == want["valid"]


# ---------------------------------------------------------------------------------------------- runner: `eval_metrics`
def test_runner_eval_metrics_equivariance_writes_metrics_yml(dev, tmp_path):
    """`-e` over five images at batch 2 (a ragged last batch): metrics.yml holds what the evaluator gives on the pickled view0 images
    with the rows of uniforms of the running image index."""
    import pickle
    import yaml
    _, _, E = _mods()
    from upsparts_amd import runner
    from upsparts_amd.model import TrainModel
    cfg = _tiny(dev)
    cfg.pop("ckpt_freq"), cfg.pop("log_freq")
    cfg.update(write_label_dataset(tmp_path, n=5, S=cfg["spatial_size"]))
    cfg.update({"vgg_widths": list(VGG_W), "val_seed": 9})
    S, P, B = cfg["spatial_size"], cfg["n_parts"], cfg["batch_size"]
    ypath = tmp_path / "eval.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    runner.main(["-e", str(ypath), "-p", str(tmp_path / "m"), "--strict-dataset", "--set", "eval_metrics=[equivariance]"])
    mdir = tmp_path / "m" / "eval" / "0"
    got = yaml.safe_load((mdir / "metrics.yml").read_text())
    assert sorted(got) == sorted(["equiv_agreement", "equiv_miou", "equiv_tv", "equiv_valid"] + ["equiv_iou_{}".format(p) for p in range(P)])
    v0 = torch.from_numpy(pickle.loads((mdir / "model_outputs.p").read_bytes())["inputs"]["view0"])
    assert tuple(v0.shape) == (5, S, S, 3)
    model = TrainModel(dict(cfg, test_mode=True), device=dev)
    ev = E.EquivarianceEvaluator(dev, P, SHIPPED)
    u = E.equivariance_uniforms(5, 9)
    for c0 in range(0, 5, B):
        k = min(B, 5 - c0)
        pad = lambda t: torch.cat([t[c0:c0 + k], t[c0 + k - 1:c0 + k].expand(B - k, *t.shape[1:])], 0)
        ev.update(model, pad(v0), pad(u), valid=k)
    want = ev.result()
    print("metrics.yml", got, want)
    assert 0 < got["equiv_valid"] < 1
    for k in ("agreement", "miou", "tv", "valid"):
        assert got["equiv_" + k] == want[k], k
    for p in range(P):
        assert got["equiv_iou_{}".format(p)] == want["iou"][p]
