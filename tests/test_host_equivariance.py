"""Host tests of the part-equivariance metric: the NumPy restatement (equivariance_ref.py) on two closed-form cases, the pure function
from counts to scores (evalutil.equivariance_from_counts), the host route (evalutil.equivariance_host) against the restatement, and the
`val_metrics` / `val_equivariance_tps` surface."""
import copy

import numpy as np
import pytest

import equivariance_ref as Q


def _E():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil
    return evalutil


def _M():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import model
    return model


# ---------------------------------------------------------------------------------------------- `val_metrics`
def test_validation_metrics_accept_equivariance_in_canonical_order():
    M = _M()
    assert M.VAL_METRICS == ("iou", "reconstruction", "parts", "equivariance")
    assert M.validation_metrics({"val_metrics": ["equivariance"]}) == ["equivariance"]
    assert M.validation_metrics({"val_metrics": ["equivariance", "parts", "iou"]}) == ["iou", "parts", "equivariance"]
    assert M.validation_metrics({}) == ["iou"]                                   # the default stays
    assert M.validation_metrics({"eval_metrics": ["equivariance"]}, "eval_metrics", ()) == ["equivariance"]
    with pytest.raises(ValueError, match="unknown metric"):
        M.validation_metrics({"val_metrics": ["equivariant"]})


def test_equivariance_needs_val_csv_and_no_label_column():
    M = _M()
    cfg = {"val_freq": 2, "val_metrics": ["equivariance"], "precision": "bf16"}
    with pytest.raises(ValueError, match="val_csv"):
        M.check_validation_config(cfg)
    M.check_validation_config(dict(cfg, val_csv="val.csv"))                      # no data_gt_segmentation_column
    with pytest.raises(ValueError, match="fp8"):                                 # the refusals of val_freq stay
        M.check_validation_config(dict(cfg, val_csv="val.csv", precision="fp8"))
    with pytest.raises(ValueError, match="hip_graph"):
        M.check_validation_config(dict(cfg, val_csv="val.csv", hip_graph=True))
    with pytest.raises(ValueError, match="missing"):
        M.check_validation_config(dict(cfg, val_csv="val.csv", val_equivariance_tps={"scal": 0.8}))


def test_warp_block_defaults():
    M = _M()
    from upsparts_amd import configs
    shipped = configs.cub_config()["tps_parameters"]
    assert shipped == configs.TPS_PARAMETERS == {"scal": 0.8, "tps_scal": 0.15, "rot_scal": 0.2, "off_scal": 0.2, "scal_var": 0.1,
                                                 "augm_scal": 1.0}
    assert M.equivariance_tps_parameters({}) == shipped
    mine = dict(shipped, scal=0.9)
    assert M.equivariance_tps_parameters({"tps_parameters": mine, "use_tps": False}) == mine
    other = dict(shipped, rot_scal=0.0)
    assert M.equivariance_tps_parameters({"tps_parameters": mine, "val_equivariance_tps": other}) == other


def test_uniforms_are_a_function_of_the_seed_and_the_row():
    E = _E()
    import torch
    from upsparts_amd import tps
    u = E.equivariance_uniforms(7, 3)
    assert tuple(u.shape) == (7, tps.N_UNIFORMS) and u.dtype == torch.float32 and float(u.min()) >= 0 and float(u.max()) < 1
    assert torch.equal(u, E.equivariance_uniforms(7, 3)) and not torch.equal(u, E.equivariance_uniforms(7, 4))
    assert torch.equal(E.equivariance_uniforms(40, 3)[:7], u)                    # row i belongs to image i, whatever the set's size
    g = torch.Generator(device="cpu")
    g.manual_seed(3)                                                             # ... and however the rows are drawn (the runner: per batch)
    parts = [torch.rand(k, tps.N_UNIFORMS, generator=g, dtype=torch.float32) for k in (2, 2, 3)]
    assert torch.equal(torch.cat(parts), u)


# ---------------------------------------------------------------------------------------------- counts -> scores
def test_from_counts_refusals():
    E = _E()
    c = np.zeros((2, 3, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="no pixel"):
        E.equivariance_from_counts(c, np.zeros(2), 24)
    c[0, 1, 1] = 5
    with pytest.raises(ValueError):
        E.equivariance_from_counts(c, np.zeros(3), 24)                          # tv of another length
    with pytest.raises(ValueError):
        E.equivariance_from_counts(c[:, :, :2], np.zeros(2), 24)                # not square
    with pytest.raises(ValueError):
        E.equivariance_from_counts(c[:0], np.zeros(0), 24)                      # no image
    with pytest.raises(ValueError):
        E.equivariance_from_counts(c, np.zeros(2), 0)
    got = E.equivariance_from_counts(c, np.array([1.0, 0.0]), 24)
    assert got == {"valid": 5 / 48, "agreement": 1.0, "iou": [-1.0, 1.0, -1.0], "miou": 1.0, "tv": 0.2}


def test_from_counts_equals_the_restatement():
    E = _E()
    rng = np.random.RandomState(5)
    counts = rng.randint(0, 50, (4, 6, 6)).astype(np.int32)
    counts[:, 2, :] = 0
    counts[:, :, 2] = 0                                                          # part 2 is absent on both sides
    tv = rng.uniform(0, 30, 4)
    got, want = E.equivariance_from_counts(counts, tv, 400), Q.equivariance_from_counts(counts, tv, 400)
    assert got["iou"][2] == -1.0 and sorted(got) == sorted(want)
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-15, atol=0), k


# ---------------------------------------------------------------------------------------------- closed forms
def test_closed_form_shift_by_two():
    E = _E()
    for fn in (lambda *a: Q.part_equivariance(*a)[:3], E.equivariance_host):
        counts, invalid, tv = fn(*Q.closed_form_case(2.0))
        want = np.zeros((3, 3), dtype=np.int64)
        want[0, 0], want[2, 0], want[2, 2] = 4, 8, 4
        assert np.array_equal(counts[0], want) and invalid == 0 and tv[0] == 8.0
        for res in (E.equivariance_from_counts(counts, tv, 24), Q.equivariance_from_counts(counts, tv, 24)):
            assert res["valid"] == 16 / 24 and res["agreement"] == 0.5 and res["iou"] == [1 / 3, -1.0, 1 / 3]
            assert res["miou"] == 1 / 3 and res["tv"] == 0.5


def test_closed_form_half_pixel_tie():
    soft_a, soft_b, pred_b, grid = Q.closed_form_case(0.5)
    counts, invalid, tv, _, la = Q.part_equivariance(soft_a, soft_b, pred_b, grid)
    assert invalid == 0
    assert np.array_equal(Q.inside_mask(grid, 4, 6)[0], np.arange(6)[None, :].repeat(4, axis=0) <= 4)      # column 5 is outside
    for y in range(4):
        assert la[0, y].tolist() == [0, 0, 0, 2, 2, -1]                         # column 2 samples (0.5, 0, 0.5): the tie goes to part 0
    want = np.zeros((3, 3), dtype=np.int64)
    want[0, 0], want[2, 2] = 12, 8
    assert np.array_equal(counts[0], want)
    assert tv[0] == 4 * 0.5                                                     # column 2: 0.5 (|0.5 - 1| + |0.5 - 0|) per row
    c2, bad2, tv2 = _E().equivariance_host(soft_a, soft_b, pred_b, grid)
    assert np.array_equal(c2, counts) and bad2 == 0 and np.array_equal(tv2, tv)


# ---------------------------------------------------------------------------------------------- the host route
@pytest.mark.parametrize("kind", Q.GRID_KINDS)
@pytest.mark.parametrize("P", [1, 3, 40])
def test_host_route_equals_the_restatement(kind, P):
    E = _E()
    N, h, w = 3, 9, 11
    rng = np.random.RandomState(100 + P)
    if kind == "half":
        soft_a, _ = Q.tie_maps(N, h, w, P)
    else:
        soft_a, _ = Q.softmax_maps(rng, N, h, w, P)
    soft_b, pred_b = Q.softmax_maps(rng, N, h, w, P)
    grid = Q.make_grid(kind, N, h, w)
    ins = Q.inside_mask(grid, h, w)
    assert ins.any() and not ins.all()
    ys, xs = np.nonzero(ins[0])
    soft_b = soft_b.copy()
    pred_b = pred_b.copy()
    soft_b[0, ys[0], xs[0], P - 1] = np.nan                                     # three inside pixels that must be counted as invalid
    pred_b[0, ys[1], xs[1]] = -1
    pred_b[0, ys[2], xs[2]] = P
    want_c, want_bad, want_tv, terms, _ = Q.part_equivariance(soft_a, soft_b, pred_b, grid)
    counts, bad, tv = E.equivariance_host(soft_a, soft_b, pred_b, grid)
    assert counts.dtype == np.int32 and np.array_equal(counts, want_c)
    assert bad == want_bad == 3 and int(counts.sum()) + bad == int(ins.sum())
    assert (np.abs(tv - want_tv) <= Q.tv_atol(h * w, terms)).all()


def test_validation_logs_name_the_five_key_families():
    E = _E()
    res = {"valid": 0.9, "agreement": 0.8, "iou": [0.5, -1.0], "miou": 0.5, "tv": 0.1}
    logs = E.validation_logs(equiv=res)
    assert logs == {"val/equiv_valid": 0.9, "val/equiv_agreement": 0.8, "val/equiv_iou_0": 0.5, "val/equiv_iou_1": -1.0,
                    "val/equiv_miou": 0.5, "val/equiv_tv": 0.1}
    assert all(k < "val/steps_done" for k in logs)
    assert E.validation_logs() == {}
