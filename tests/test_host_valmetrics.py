"""Host tests of the label-free validation metrics: the NumPy restatement (valmetrics_ref.py) against scipy, the two pure functions
from sums to metrics (evalutil.reconstruction_from_sums / usage_from_counts), the `val_metrics` refusals and the validation pair set."""
import copy

import numpy as np
import pytest

import valmetrics_ref as V


def _E():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil
    return evalutil


# ---------------------------------------------------------------------------------------------- the restatement
def test_filtered_maps_equal_scipy_correlate1d():
    from scipy import ndimage
    rng = np.random.RandomState(0)
    w = V.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    for H, W in ((11, 11), (12, 27), (40, 33)):
        x = rng.uniform(0, 1, (2, 3, H, W))
        want = ndimage.correlate1d(ndimage.correlate1d(x, w, axis=-1, mode="constant"), w, axis=-2, mode="constant")[..., 5:H - 5, 5:W - 5]
        got = V.filter_valid(x, w)
        assert got.shape == (2, 3, H - 10, W - 10)
        assert np.abs(got - want).max() <= 1e-12


def test_window_is_the_binding_s_window():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import ops
    assert np.array_equal(ops.ssim_weights(), V.window()) and ops.ssim_weights().dtype == np.float64


def test_identical_images():
    rng = np.random.RandomState(1)
    a, _ = V.image_pair(rng, 2, 13, 17)
    rows = V.image_metrics(a, a.copy())
    assert (rows[:, 0] == 0).all() and (rows[:, 1] == 0).all()
    assert np.abs(rows[:, 2] / (3 * 3 * 7) - 1.0).max() <= 1e-10
    for fill in (-1.0, 1.0, 0.25):          # flat images: zero variance, the constants alone
        f = np.full((1, 11, 11, 3), fill, dtype=np.float32)
        assert abs(V.image_metrics(f, f)[0, 2] / 3 - 1.0) <= 1e-10


def test_restatement_clamps_and_counts_every_value():
    a = np.full((1, 11, 11, 3), 3.0, dtype=np.float32)       # clamps to 1
    b = np.full((1, 11, 11, 3), -3.0, dtype=np.float32)      # clamps to 0
    rows = V.image_metrics(a, b)
    assert rows[0, 0] == 363.0 and rows[0, 1] == 363.0
    # mu_x = 1, mu_y = 0, no variance: (C1)(C2) / ((1 + C1)(C2)) per channel
    assert abs(rows[0, 2] / 3 - V.C1 / (1.0 + V.C1)) <= 1e-12


def test_part_usage_restatement_by_hand():
    soft = np.array([[[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.25, 0.25, 0.5]]], dtype=np.float32)
    pred = np.array([[0, -1, 3]])
    counts, invalid, sharp, terms = V.part_usage(soft, pred, 3)
    assert counts.tolist() == [[1, 0, 0]] and invalid == 2
    assert sharp[0, 0] == 2.0 and abs(sharp[0, 1] - (np.log(2.0) + 1.5 * np.log(2.0))) <= 1e-15
    assert np.array_equal(terms, sharp)
    E = _E()
    c2, i2, s2 = E.part_usage_host(soft, pred, 3)
    assert np.array_equal(c2, counts) and i2 == invalid and np.abs(s2 - sharp).max() <= 1e-15


# ---------------------------------------------------------------------------------------------- sums -> metrics
def test_reconstruction_from_sums():
    E = _E()
    H, W = 12, 21
    n = 3 * H * W
    rows = np.array([[0.0, 0.0, 3.0 * 2 * 11], [n * 0.01, n * 0.1, 0.5 * 3 * 2 * 11], [n * 1e-12, n * 1e-6, 0.0]])
    got = E.reconstruction_from_sums(rows, H, W)
    # image 0: perfect -> the floor: 100 dB; image 1: mse 0.01 -> 20 dB; image 2: mse 1e-12 < 1e-10 -> the floor as well
    assert abs(got["psnr"] - (100.0 + 20.0 + 100.0) / 3) <= 1e-9
    assert abs(got["mse"] - (0.01 + 1e-12) / 3) <= 1e-15
    assert abs(got["l1"] - (0.1 + 1e-6) / 3) <= 1e-15
    assert abs(got["ssim"] - 0.5) <= 1e-15
    want = V.reconstruction_from_sums(rows, H, W)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-13 * max(1.0, abs(want[k])), k
    with pytest.raises(ValueError):
        E.reconstruction_from_sums(np.zeros((0, 3)), H, W)
    with pytest.raises(ValueError, match="11"):
        E.reconstruction_from_sums(rows, 10, W)


def test_usage_from_counts():
    E = _E()
    HW = 100
    # two images, four parts: areas 0.795, 0.2, 0.005 (exactly min_area) and 0
    counts = np.array([[80, 20, 0, 0], [79, 20, 1, 0]], dtype=np.int32)
    sharp = np.array([[90.0, 10.0], [70.0, 30.0]])
    got = E.usage_from_counts(counts, sharp, HW, 0.005)
    assert got["part_area"] == [159 / 200, 40 / 200, 1 / 200, 0.0]
    assert 1 / 200 == 0.005 and got["parts_active"] == 3          # a part exactly at min_area counts as active
    assert E.usage_from_counts(counts, sharp, HW, 0.0050001)["parts_active"] == 2
    assert E.usage_from_counts(counts, sharp, HW, 0.0)["parts_active"] == 4
    assert got["confidence"] == 160.0 / 200 and got["entropy"] == 40.0 / 200
    assert got == V.usage_from_counts(counts, sharp, HW, 0.005)
    with pytest.raises(ValueError):
        E.usage_from_counts(np.zeros((0, 4), np.int32), np.zeros((0, 2)), HW, 0.005)
    logs = E.validation_logs(E.reconstruction_from_sums(np.ones((1, 3)), 11, 11), got, 1.25)
    assert sorted(logs) == ["val/confidence", "val/entropy", "val/l1", "val/mse", "val/part_area_0", "val/part_area_1", "val/part_area_2",
                            "val/part_area_3", "val/parts_active", "val/psnr", "val/rec", "val/ssim"]
    assert all(k < "val/steps_done" for k in logs)


# ---------------------------------------------------------------------------------------------- config refusals
def _val_cfg(**kw):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"precision": "bf16", "val_freq": 2, "val_csv": "val.csv", "val_metrics": ["reconstruction", "parts"]})
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("kw,word", [({"val_metrics": ["reconstruction", "sharpness"]}, "sharpness"),
                                     ({"val_metrics": []}, "empty"),
                                     ({"val_metrics": "parts"}, "list"),
                                     ({"val_metrics": ["iou", "parts"]}, "data_gt_segmentation_column"),
                                     ({"val_csv": None}, "val_csv"),
                                     ({"precision": "fp8"}, "fp8"),
                                     ({"hip_graph": True}, "hip_graph"),
                                     ({"val_metrics": ["parts"], "precision": "fp8"}, "fp8"),
                                     ({"val_metrics": ["parts"], "hip_graph": True}, "hip_graph"),
                                     ({"spatial_size": 8}, "SSIM window")])
def test_val_metrics_refusals(kw, word):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import Trainer, check_validation_config
    cfg = _val_cfg(**kw)
    with pytest.raises(ValueError, match=word):
        check_validation_config(cfg)
    with pytest.raises(ValueError, match=word):
        Trainer(cfg, None, object())
    check_validation_config(dict(cfg, val_freq=0))


def test_val_metrics_accepts_what_needs_no_labels():
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import check_validation_config, validation_metrics
    check_validation_config(_val_cfg())
    check_validation_config(_val_cfg(val_metrics=["parts"], spatial_size=8))        # the window only matters to reconstruction
    check_validation_config(_val_cfg(val_metrics=["iou", "parts"], data_gt_segmentation_column="seg"))
    assert validation_metrics({}) == ["iou"]
    assert validation_metrics({"val_metrics": ["parts", "reconstruction"]}) == ["reconstruction", "parts"]
    assert validation_metrics({}, "eval_metrics", ()) == []


@pytest.mark.parametrize("kw,word", [({"precision": "fp8"}, "fp8"), ({"hip_graph": True}, "hip_graph"), ({"val_csv": None}, "val_csv"),
                                     ({"data_gt_segmentation_column": None}, "data_gt_segmentation_column")])
def test_key_unset_raises_where_it_raised_before(kw, word):
    """Without `val_metrics` the metric is the part IoU and the label column stays required: the four refusals and their texts."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import check_validation_config
    cfg = _val_cfg(**dict({"data_gt_segmentation_column": "seg"}, **kw))
    del cfg["val_metrics"]
    with pytest.raises(ValueError, match=word):
        check_validation_config(cfg)
    ok = _val_cfg(data_gt_segmentation_column="seg")
    del ok["val_metrics"]
    check_validation_config(ok)
    for text_of in ({"val_csv": None}, {"data_gt_segmentation_column": None}):
        with pytest.raises(ValueError) as e:
            check_validation_config(dict(ok, **text_of))
        assert str(e.value) == "val_freq needs `val_csv` and `data_gt_segmentation_column` (the csv column with the label images)"


# ---------------------------------------------------------------------------------------------- the pair set
def _pairs_cfg(tmp_path, n, **kw):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(V.write_view_dataset(tmp_path, n=n, S=cfg["spatial_size"], ids=[0] * n))
    cfg.update({"val_csv": cfg.pop("data_csv"), "data_avoid_identity": True})
    cfg.update(kw)
    return cfg


def test_validation_pairs_plan(tmp_path):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import data
    cfg = _pairs_cfg(tmp_path, 9)
    B, S = cfg["batch_size"], cfg["spatial_size"]
    assert B == 2
    a, b = data.ValidationPairs(cfg), data.ValidationPairs(dict(cfg, val_seed=1))
    assert len(a) == 8 and a.chunks() == 4                          # nine rows at batch 2: the ninth is left out
    assert np.array_equal(a.rows, b.rows) and a.rows.dtype == np.int32
    assert a.rows[:, 0].tolist() == list(range(8))                  # pose images: the first rows, in csv order
    assert (a.rows[:, 1] != a.rows[:, 0]).all() and a.rows[:, 1].min() >= 0 and a.rows[:, 1].max() < 9      # avoid_identity, one id
    c = data.ValidationPairs(dict(cfg, val_seed=2))
    assert np.array_equal(c.rows[:, 0], a.rows[:, 0]) and not np.array_equal(c.rows[:, 1], a.rows[:, 1])
    # neither the training seed nor the flip keys reach the plan
    d = data.ValidationPairs(dict(cfg, data_seed=77, data_flip_h=True, data_flip_v=True))
    assert np.array_equal(d.rows, a.rows)
    # the store holds every named image once, decoded as the training path decodes it
    ds = data.StochasticPairs(dict(cfg, data_csv=cfg["val_csv"]))
    assert tuple(a.store.shape[1:]) == (S, S, 3) and a.store.shape[0] == len(np.unique(a.rows))
    used = np.unique(a.rows)
    for k in range(len(a)):
        for side in (0, 1):
            assert used[a.pairs[k, side]] == a.rows[k, side]
    k = 3
    assert np.array_equal(a.store[a.pairs[k, 1]].numpy(), ds.preprocess_u8(ds.labels["file_path_"][int(a.rows[k, 1])]))
    # val_max_images caps the rows before the truncation to whole chunks
    assert len(data.ValidationPairs(dict(cfg, val_max_images=5))) == 4
    assert len(data.ValidationPairs(dict(cfg, batch_size=4))) == 8
    assert len(data.ValidationPairs(dict(cfg, batch_size=5))) == 5


def test_validation_pairs_refusals(tmp_path):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import data
    cfg = _pairs_cfg(tmp_path, 3)
    with pytest.raises(ValueError, match="batch_size"):
        data.ValidationPairs(dict(cfg, batch_size=4))
    with pytest.raises(ValueError, match="batch_size"):
        data.ValidationPairs(dict(cfg, val_max_images=1))
    with pytest.raises(ValueError, match="val_csv"):
        data.ValidationPairs(dict(cfg, val_csv=None))
    assert len(data.ValidationPairs(cfg)) == 2


def test_library_exports_the_metric_entries():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    for name in ("ups_image_metrics", "ups_image_metrics_scratch_bytes", "ups_image_metrics_tile", "ups_part_usage",
                 "ups_part_usage_scratch_bytes", "ups_part_usage_chunk"):
        assert name in lib.EXPORTS
    h = lib.load()
    assert h.ups_image_metrics_tile() == ops.IMAGE_METRICS_TILE and h.ups_part_usage_chunk() == ops.PART_USAGE_CHUNK
    T = ops.IMAGE_METRICS_TILE
    assert h.ups_image_metrics_scratch_bytes(2, 10 + T, 10 + T + 1) == 2 * 2 * 3 * 8
    assert h.ups_image_metrics_scratch_bytes(2, 10, 64) == 0
    assert h.ups_part_usage_scratch_bytes(3, ops.PART_USAGE_CHUNK + 1) == 3 * 2 * 2 * 8
