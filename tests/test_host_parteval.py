"""Host tests of the counts route of the part-IoU protocol: evaluate_from_counts(confusion_counts(..)) against evaluate_parts
(exact: every quantity is an integer or a float64 quotient of the same integers), the written tables byte for byte, and the
refusals of `val_freq` / `eval_on_device` / PartEvaluator that are decided before the device is touched."""
import numpy as np
import pytest

from parteval_ref import StubModel, all_cases, crafted_cases, iou_case, random_case, sizes


def _E():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil
    return evalutil


def _same(a, b):
    """== on keys, ints and floats (a NaN `overall` -- no label but the background -- equals a NaN)."""
    assert set(a) == set(b) == {"mapping", "iou", "per_image", "overall", "pooled"}
    for k in ("mapping", "iou", "per_image", "pooled"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["overall"] == b["overall"] or (np.isnan(a["overall"]) and np.isnan(b["overall"]))
    for m in (a, b):
        assert all(type(k) is int and type(v) is int for k, v in m["mapping"].items())
        assert all(type(k) is int and type(v) is float for k, v in m["iou"].items())


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_counts_route_equals_evaluate_parts(name):
    E = _E()
    pred, gt = all_cases()[name]
    P, G = sizes(pred, gt)
    got = E.evaluate_from_counts(E.confusion_counts(pred, gt, P, G))
    _same(got, E.evaluate_parts(pred, gt))
    # a table larger than needed (the runner's default G = 32) adds empty rows and columns: nothing changes
    _same(E.evaluate_from_counts(E.confusion_counts(pred, gt, P + 3, 32)), got)


def test_tie_rules_hold_what_they_say():
    """The crafted cases do exercise their rule (otherwise the equality above would be vacuous)."""
    E = _E()
    c = crafted_cases()
    for name in ("equal_quotients_lower_label_wins", "equal_quotients_other_integers"):
        pred, gt = c[name]
        counts = E.confusion_counts(pred, gt, *sizes(pred, gt))[0]
        ious = [counts[0, g] / (counts[0].sum() + counts[:, g].sum() - counts[0, g]) for g in (0, 1)]
        assert ious[0] == ious[1] > 0 and E.evaluate_from_counts(counts[None])["mapping"][0] == 0, name
    r = E.evaluate_from_counts(E.confusion_counts(*c["part_ids_that_never_occur"], 8, 3))
    assert sorted(r["mapping"]) == [3, 5, 7]
    r = E.evaluate_from_counts(E.confusion_counts(*c["label_missing_from_one_image"], 8, 3))
    assert 2 in r["per_image"][0] and 2 not in r["per_image"][1]
    r = E.evaluate_from_counts(E.confusion_counts(*c["label_missing_from_the_set"], 8, 4))
    assert sorted(r["iou"]) == [0, 2, 3] and 1 not in r["pooled"]
    r = E.evaluate_from_counts(E.confusion_counts(*c["pred_equals_gt"], 3, 3))
    assert r["overall"] == 1.0 and r["mapping"] == {0: 0, 1: 1, 2: 2}


def test_confusion_counts_is_the_joint_histogram():
    E = _E()
    pred, gt = random_case(4)
    P, G = sizes(pred, gt)
    c = E.confusion_counts(pred, gt, P, G)
    assert c.dtype == np.int32 and c.shape == (len(pred), P, G)
    for i in range(len(pred)):
        for p in range(P):
            for g in range(G):
                assert c[i, p, g] == np.sum((pred[i] == p) & (gt[i] == g))
    # out-of-range keys are counted nowhere, and reported
    bad = pred.copy()
    bad[0, 0, 0], bad[0, 0, 1] = P, -1
    c2, n = E.confusion_counts(bad, gt, P, G, return_invalid=True)
    assert n == 2 and c2.sum() == c.sum() - 2


@pytest.mark.parametrize("name", ["test_part_iou_evaluation", "label_missing_from_one_image", "random03", "random07"])
def test_tables_are_byte_identical(name, tmp_path):
    E = _E()
    pred, gt = all_cases()[name]
    a = E.evaluate_parts(pred, gt)
    b = E.evaluate_from_counts(E.confusion_counts(pred, gt, *sizes(pred, gt)))
    names = {0: "background", 1: "head", 2: "tail"}
    E.write_eval_tables(a, str(tmp_path / "a"), 71000, names)
    E.write_eval_tables(b, str(tmp_path / "b"), 71000, names)
    for f in ("part_ious.csv", "mean_part_ios.csv", "best_remapping.yml"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    from upsparts_amd import runner
    runner.write_iou_files(a, str(tmp_path / "a"), {}, 1)
    runner.write_iou_files(b, str(tmp_path / "b"), {}, 1)
    assert (tmp_path / "a" / "iou.yml").read_bytes() == (tmp_path / "b" / "iou.yml").read_bytes()


def test_lut_round_trip():
    E = _E()
    rng = np.random.RandomState(3)
    pred = rng.randint(0, 5, (3, 8, 8))
    raw = rng.randint(0, 256, (3, 8, 8))
    lut = rng.randint(0, 4, 256).astype(np.uint8)
    assert np.array_equal(E.confusion_counts(pred, raw, 5, 4, lut), E.confusion_counts(pred, lut[raw], 5, 4))
    # the yaml form {raw: new}: unlisted labels keep their value
    d = {7: 1, 200: 2}
    t = E.lut_array(d)
    assert t.dtype == np.uint8 and t[7] == 1 and t[200] == 2 and t[3] == 3 and t[255] == 255
    assert np.array_equal(E.confusion_counts(pred, raw, 5, 4, d), E.confusion_counts(pred, t[raw], 5, 4))
    with pytest.raises(ValueError):
        E.lut_array({256: 1})
    with pytest.raises(ValueError):
        E.lut_array({1: 256})


def _val_cfg(**kw):
    import copy
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"precision": "bf16", "val_freq": 2, "val_csv": "val.csv", "data_gt_segmentation_column": "seg"})
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("key,value,word", [("precision", "fp8", "fp8"), ("hip_graph", True, "hip_graph"), ("val_csv", None, "val_csv"),
                                            ("data_gt_segmentation_column", None, "data_gt_segmentation_column")])
def test_val_freq_refusals(key, value, word):
    """ValueError at construction with the reason in the text -- before the trainer touches its model or the device."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import Trainer, check_validation_config
    cfg = _val_cfg(**{key: value})
    with pytest.raises(ValueError, match=word):
        Trainer(cfg, None, object())
    check_validation_config(dict(cfg, val_freq=0))              # without the key nothing is refused
    with pytest.raises(ValueError, match=word):
        check_validation_config(cfg)


def test_eval_on_device_without_ground_truth():
    import torch
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    batch = {"view0": torch.zeros(2, 8, 8, 3), "view1": torch.zeros(2, 8, 8, 3)}
    with pytest.raises(ValueError, match="gt_segmentation"):
        runner.evaluate_on_device(StubModel(), iter([batch]), {"batch_size": 2})


@pytest.mark.parametrize("bad", [256, -1])
def test_label_outside_a_byte_raises_before_any_launch(bad):
    E = _E()
    ev = E.PartEvaluator(StubModel(), 3)
    gt = np.zeros((2, 8, 8), dtype=np.int64)
    gt[1, 3, 3] = bad
    with pytest.raises(ValueError, match="0..255"):
        ev.update(np.zeros((2, 8, 8, 3), np.float32), gt)        # (StubModel.segment raises AssertionError if reached)


def test_library_exports_the_new_symbol():
    """(The header / library / binding comparison itself is test_host.py's ABI test.)"""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    assert "ups_part_confusion" in lib.EXPORTS and lib.ABI_VERSION == 6
    assert iou_case()[0].shape == (2, 8, 8)
