"""GPU tests of the part-IoU evaluation on the device: ups_part_confusion (csrc/evalparts.hip, through the C ABI) against
evalutil.confusion_counts, TrainModel.segment against forward, PartEvaluator / `-e` with eval_on_device / `val_freq` against
evaluate_parts.  Every comparison is exact: integers, or float64 quotients of the same integers."""
import copy
import ctypes as C
import re

import numpy as np
import pytest
import torch

from parteval_ref import block_labels, write_label_dataset

pytestmark = pytest.mark.gpu

GUARD = 64                  # int32 words in front of and behind `counts` and `invalid` that must keep the sentinel
SENTINEL = -0x5A5A5A5B
PER_LANE, CHUNK = 8, 2048   # csrc/evalparts.hip: a lane owns 8 consecutive pixels, a 256-thread block one chunk of 2048 pixels
VGG_W = (8, 8, 16, 16, 16)


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil, lib
    return lib, evalutil


class _Guarded(object):
    """`n` int32 words (zero, or `init`) inside a sentinel-filled buffer with GUARD words on each side."""

    def __init__(self, dev, n, init=None):
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.view = self.buf[GUARD:GUARD + n]
        self.view.copy_(torch.zeros(n, dtype=torch.int32) if init is None else torch.as_tensor(init, dtype=torch.int32).reshape(-1))

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


def _launch(L, dev, pred, gt, P, G, lut=None, gt_shift=0, pred_shift=0, counts=None, invalid=None, row0=0):
    """ups_part_confusion on NumPy maps [N,..]; gt_shift bytes / pred_shift int64 elements move the inputs off their alignment.
    counts / invalid: _Guarded buffers to add into (rows [row0, row0 + N) of counts).  Returns (counts, invalid) _Guarded."""
    N = pred.shape[0]
    HW = pred.size // N
    pbuf = torch.zeros(N * HW + 2, dtype=torch.int64, device=dev)
    pbuf[pred_shift:pred_shift + N * HW] = torch.from_numpy(pred.reshape(-1).astype(np.int64)).to(dev)
    gbuf = torch.zeros(N * HW + 8, dtype=torch.uint8, device=dev)
    gbuf[gt_shift:gt_shift + N * HW] = torch.from_numpy(gt.reshape(-1).astype(np.uint8)).to(dev)
    assert pbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 4 == 0
    lut_d = None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.uint8)).to(dev)
    counts = counts if counts is not None else _Guarded(dev, N * P * G)
    invalid = invalid if invalid is not None else _Guarded(dev, 1)
    rc = L.load().ups_part_confusion(C.c_void_p(pbuf.data_ptr() + 8 * pred_shift), C.c_void_p(gbuf.data_ptr() + gt_shift),
                                     L.ptr(lut_d), N, HW, P, G, C.c_void_p(counts.view.data_ptr() + 4 * row0 * P * G),
                                     L.ptr(invalid.view), L.stream())
    assert rc == 0, L.load().ups_last_error().decode()
    torch.cuda.synchronize(dev)
    return counts, invalid


def _check(L, E, dev, pred, gt, P, G, lut=None, **kw):
    want, bad = E.confusion_counts(pred, gt, P, G, lut, return_invalid=True)
    counts, invalid = _launch(L, dev, pred, gt, P, G, lut, **kw)
    got = counts.view.cpu().numpy().reshape(want.shape)
    assert np.array_equal(got, want), "counts differ at {}".format(np.argwhere(got != want)[:5].tolist())
    assert int(invalid.view.cpu()) == bad
    assert counts.intact() and invalid.intact(), "wrote outside counts / invalid"
    return want, bad


# (75, 83): 6 225 pixels = three whole chunks of 2 048 and a fourth of 81 pixels (ten whole lanes and one of a single pixel); HW is
# odd, so image 1 starts 8 bytes off the 16-byte alignment of `pred` and one byte off the dword alignment of `gt`
SHAPES = [(1, 1, 1, 1, 1), (3, 5, 7, 3, 2), (2, 16, 16, 10, 5), (2, 32, 32, 32, 32), (1, 64, 64, 25, 4), (2, 75, 83, 7, 3)]


@pytest.mark.parametrize("with_lut", [False, True], ids=["identity", "lut"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_confusion_equals_numpy(shape, with_lut, dev):
    L, E = _mods()
    N, H, W, P, G = shape
    rng = np.random.RandomState(sum(shape))
    pred = rng.randint(0, P, (N, H, W))
    lut = rng.randint(0, G, 256).astype(np.uint8) if with_lut else None
    gt = rng.randint(0, 256 if with_lut else G, (N, H, W))
    if shape == (2, 32, 32, 32, 32) and not with_lut:       # 2 048 pixels, 1 024 bins: a shuffled enumeration hits each one twice
        key = rng.permutation(N * H * W) % (P * G)
        pred, gt = (key // G).reshape(N, H, W), (key % G).reshape(N, H, W)
    want, bad = _check(L, E, dev, pred, gt, P, G, lut)
    assert bad == 0 and want.sum() == N * H * W
    if shape == (2, 32, 32, 32, 32) and not with_lut:
        assert (want.sum(axis=0) > 0).all()         # every bin of the largest table is hit


@pytest.mark.parametrize("gt_shift,pred_shift", [(1, 0), (3, 0), (0, 1), (1, 1)], ids=["gt+1", "gt+3", "pred+8B", "both"])
def test_unaligned_inputs(gt_shift, pred_shift, dev):
    """gt one and three bytes off a dword, pred at an 8-byte but not 16-byte aligned address: the element path, same integers."""
    L, E = _mods()
    rng = np.random.RandomState(7)
    _check(L, E, dev, rng.randint(0, 10, (2, 16, 16)), rng.randint(0, 5, (2, 16, 16)), 10, 5, gt_shift=gt_shift, pred_shift=pred_shift)


def _piecewise(kind):
    HW = 2 * CHUNK + 24
    k = np.arange(HW)
    if kind == "one_bin":
        return np.full(HW, 2), np.full(HW, 1)
    if kind == "half_planes":
        return (k >= HW // 2).astype(np.int64), (k >= HW // 2).astype(np.int64) * 2
    if kind == "checkerboard":              # a key change at every pixel
        return k % 2, (k + 1) % 2
    if kind == "runs_end_at_lane_boundaries":
        return (k // PER_LANE) % 3, (k // (2 * PER_LANE)) % 3
    if kind == "runs_end_at_block_boundaries":
        return (k // CHUNK) % 3, (k // CHUNK + 1) % 3
    if kind == "runs_straddle_boundaries":   # runs of 11: they end inside lanes, across lanes and across blocks
        return (k // 11) % 3, (k // 29) % 3
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["one_bin", "half_planes", "checkerboard", "runs_end_at_lane_boundaries",
                                  "runs_end_at_block_boundaries", "runs_straddle_boundaries"])
def test_piecewise_constant_keys(kind, dev):
    """The inputs the run-length path exists for; one image of two whole chunks and 24 pixels."""
    L, E = _mods()
    pred, gt = _piecewise(kind)
    want, _ = _check(L, E, dev, pred[None], gt[None], 3, 3)
    if kind == "one_bin":
        assert want[0, 2, 1] == pred.size and want.sum() == pred.size


def test_accumulation(dev):
    L, E = _mods()
    rng = np.random.RandomState(11)
    P, G = 6, 4
    pred, gt = rng.randint(0, P, (4, 20, 23)), rng.randint(0, G, (4, 20, 23))
    pred2, gt2 = rng.randint(0, P, (4, 20, 23)), rng.randint(0, G, (4, 20, 23))
    want = E.confusion_counts(pred, gt, P, G)
    # two launches on the same counts give the sum
    counts, invalid = _launch(L, dev, pred, gt, P, G)
    _launch(L, dev, pred2, gt2, P, G, counts=counts, invalid=invalid)
    assert np.array_equal(counts.view.cpu().numpy().reshape(want.shape), want + E.confusion_counts(pred2, gt2, P, G))
    assert counts.intact() and invalid.intact() and int(invalid.view.cpu()) == 0
    # the two halves of a batch into row-offset views of one buffer give the whole
    halves = _Guarded(dev, 4 * P * G)
    inv = _Guarded(dev, 1)
    _launch(L, dev, pred[:2], gt[:2], P, G, counts=halves, invalid=inv, row0=0)
    _launch(L, dev, pred[2:], gt[2:], P, G, counts=halves, invalid=inv, row0=2)
    assert np.array_equal(halves.view.cpu().numpy().reshape(want.shape), want) and halves.intact()
    # the same launch repeated gives the same integers
    again, _ = _launch(L, dev, pred, gt, P, G)
    assert np.array_equal(again.view.cpu().numpy().reshape(want.shape), want)


def test_out_of_range_keys_are_ignored_and_counted(dev):
    """pred = P, -1, 2**40 and lut values >= G at known pixels of ordinary in-bounds buffers: `invalid` is their number, `counts`
    the reference without those pixels, the guards intact."""
    L, E = _mods()
    rng = np.random.RandomState(5)
    P, G = 5, 3
    pred = rng.randint(0, P, (2, 48, 50)).astype(np.int64)
    gt = rng.randint(0, 200, (2, 48, 50))
    lut = rng.randint(0, G, 256).astype(np.uint8)
    lut[200], lut[201] = G, 255
    clean = E.confusion_counts(pred, gt, P, G, lut)
    flat_p, flat_g = pred.reshape(2, -1), gt.reshape(2, -1)
    planted = {(0, 0): ("p", P), (0, 7): ("p", -1), (0, 8): ("p", 2 ** 40), (0, 2047): ("p", 31), (1, 2048): ("p", -2 ** 63),
               (1, 2399): ("g", 200), (1, 9): ("g", 201), (0, 1000): ("p", 2 ** 32), (1, 1001): ("p", 2 ** 32 + 1)}
    removed = np.zeros_like(clean)
    for (i, k), (what, v) in planted.items():
        removed[i, flat_p[i, k], lut[flat_g[i, k]]] += 1
        if what == "p":
            flat_p[i, k] = v
        else:
            flat_g[i, k] = v
    want, bad = _check(L, E, dev, pred, gt, P, G, lut)
    assert bad == len(planted) and np.array_equal(want, clean - removed)


def test_unsupported_table_sizes(dev):
    L, _ = _mods()
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    g = torch.zeros(64, dtype=torch.uint8, device=dev)
    counts, invalid = _Guarded(dev, 33 * 33), _Guarded(dev, 1)
    fn = L.load().ups_part_confusion
    for P, G in ((33, 2), (2, 33), (0, 2), (2, 0)):
        assert fn(L.ptr(z), L.ptr(g), None, 1, 64, P, G, L.ptr(counts.view), L.ptr(invalid.view), L.stream()) == -2     # UPS_E_UNSUPPORTED
    assert fn(None, L.ptr(g), None, 1, 64, 2, 2, L.ptr(counts.view), L.ptr(invalid.view), L.stream()) == -1             # UPS_E_ARG
    torch.cuda.synchronize(dev)
    assert int(counts.view.abs().sum()) == 0 and counts.intact()


# ---------------------------------------------------------------------------------------------- segment / PartEvaluator
def _model(precision, dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel
    from oracle import configs, ref_model as R
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(precision=precision, vgg_widths=VGG_W)
    return cfg, TrainModel(cfg, device=dev, seed=0), R


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_segment_and_part_evaluator(precision, dev):
    L, E = _mods()
    cfg, model, R = _model(precision, dev)
    B, S = cfg["batch_size"], cfg["spatial_size"]
    views = R.synthetic_views(cfg)
    a, b = views["view0"], views["view1"]
    hard = model.forward({"view0": a, "view1": b})["out_parts_hard"].clone()
    seg = model.segment(torch.cat([a, b], 0))
    assert seg.dtype == torch.int64 and tuple(seg.shape) == (2 * B, S, S) and seg.device.type == "cuda"
    assert torch.equal(seg[:B], hard)
    # N = 2B + 1: a whole pass and a ragged one (one image, padded with copies of itself)
    gen = torch.Generator().manual_seed(3)
    more = torch.cat([a, b, torch.rand(1, S, S, 3, generator=gen) * 2 - 1], 0)
    gt = block_labels(np.random.RandomState(2), 2 * B + 1, S)
    ev = E.PartEvaluator(model, 3)
    ev.update(more, gt)
    got = ev.result()
    host = model.segment(more).cpu().numpy()
    assert np.array_equal(host[:2 * B], seg.cpu().numpy())
    want = E.evaluate_parts(host, gt.astype(np.int64))
    assert got == want
    # a table wider than the labels, and a second update after a reset, change nothing
    ev32 = E.PartEvaluator(model, 32)
    ev32.update(more[:3], gt[:3])
    ev32.update(more[3:], gt[3:], valid=2 * B + 1 - 3)
    counts, invalid = ev32.counts()
    assert invalid == 0 and counts.shape == (2 * B + 1, cfg["n_parts"], 32)
    # too few labels for the maps: the pixels are counted as invalid and result() says how many
    ev2 = E.PartEvaluator(model, 2)
    ev2.update(more, gt)
    with pytest.raises(L.UpsError, match=str(int((gt >= 2).sum()))):
        ev2.result()


class _SegmentStub(object):
    """What PartEvaluator needs of a model: `segment` hands out prepared int64 maps on the device, one tensor per call."""
    n_parts = 3

    def __init__(self, dev, maps):
        self.device, self.maps = dev, [torch.from_numpy(m).to(dev) for m in maps]

    def segment(self, views):
        return self.maps.pop(0)[:len(views)]


def test_part_evaluator_grows_past_its_first_rows(dev):
    """33 images, then 36 of 37: 69 rows cross the 64-row buffer while the kernel adds into row-offset views of it."""
    _, E = _mods()
    rng = np.random.RandomState(13)
    P, G = 3, 4
    pred = [rng.randint(0, P, (n, 4, 4)).astype(np.int64) for n in (33, 37)]
    gt = [rng.randint(0, G, (n, 4, 4)).astype(np.uint8) for n in (33, 37)]
    ev = E.PartEvaluator(_SegmentStub(dev, pred), G)
    assert ev.on_device
    ev.update(torch.zeros((33, 4, 4, 3)), gt[0])
    ev.update(torch.zeros((37, 4, 4, 3)), gt[1], valid=36)
    counts, invalid = ev.counts()
    want = E.confusion_counts(np.concatenate([pred[0], pred[1][:36]]), np.concatenate([gt[0], gt[1][:36]]), P, G)
    assert ev.n == 69 and invalid == 0 and counts.dtype == np.int32 and np.array_equal(counts, want)


def test_runner_eval_on_device_writes_the_same_tables(dev, tmp_path):
    """`-e` over a csv dataset with label images, five images at batch 2 (a ragged last batch), with and without eval_on_device:
    iou.yml, part_ious.csv, mean_part_ios.csv and best_remapping.yml byte for byte; no model_outputs.p from the device route."""
    import yaml
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(write_label_dataset(tmp_path, n=5, S=cfg["spatial_size"]))
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "part_names": {0: "background", 1: "head", 2: "tail"}})
    ypath = tmp_path / "eval.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    runner.main(["-e", str(ypath), "-p", str(tmp_path / "host"), "--strict-dataset"])
    res = runner.main(["-e", str(ypath), "-p", str(tmp_path / "device"), "--strict-dataset", "--set", "eval_on_device=true"])
    hdir, ddir = tmp_path / "host" / "eval" / "0", tmp_path / "device" / "eval" / "0"
    for f in ("iou.yml", "part_ious.csv", "mean_part_ios.csv", "best_remapping.yml"):
        assert (hdir / f).read_bytes() == (ddir / f).read_bytes(), f
    assert (hdir / "model_outputs.p").exists() and not (ddir / "model_outputs.p").exists()
    assert len(res["per_image"]) == 5 and sorted(res["iou"]) == [0, 1, 2]


def _train(cfg, dev, steps, val_views=None, val_labels=None):
    """`steps` steps of Trainer.iterate on one fixed batch with the trainer's seeded noise.  Returns (trainer, losses of every step,
    a seeded sample of the master weights, log lines, evaluate_parts of segment outputs after steps 2 and 4 when val_views is given)."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil as E
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as R
    model = TrainModel(cfg, device=dev, seed=0)
    trainer = Trainer(cfg, None, model)
    views = R.synthetic_views(cfg)
    losses, expected, lines = [], {}, []

    def feed():
        for s in range(steps + 1):
            yield views
            losses.append({k: float(v) for k, v in trainer.losses.items()})
            if val_views is not None and trainer.global_step in (2, 4):
                expected[trainer.global_step] = E.evaluate_parts(model.segment(val_views).cpu().numpy(), val_labels)
    trainer.iterate(feed(), num_steps=steps, log_fn=lines.append)
    rng = np.random.RandomState(0)
    sample = {}
    for name in sorted(model.variables):
        flat = model.variables[name].detach().reshape(-1)
        idx = torch.from_numpy(rng.randint(0, flat.numel(), min(16, flat.numel()))).to(flat.device)
        sample[name] = flat[idx].cpu()
    return trainer, losses[:steps], sample, lines, expected


def test_val_freq_reports_the_metric_and_leaves_the_trajectory_alone(dev, tmp_path):
    from oracle import configs
    base = copy.deepcopy(configs.tiny_config())
    base.update({"precision": "bf16", "vgg_widths": VGG_W, "ckpt_freq": 0, "log_freq": 250})
    ds = write_label_dataset(tmp_path, n=5, S=base["spatial_size"], seed=4, name="val")
    cfg = dict(base, **ds)
    cfg.update({"val_freq": 2, "val_csv": cfg.pop("data_csv")})
    _, plain_losses, plain_sample, plain_lines, _ = _train(copy.deepcopy(base), dev, 4)
    assert not any("val/" in ln for ln in plain_lines)
    from upsparts_amd import data
    vs = data.ValidationSet(cfg)
    val_views = torch.from_numpy(vs.views.numpy().astype(np.float32) / 127.5 - 1.0)
    val_labels = vs.labels.numpy().astype(np.int64)
    assert len(vs) == 5 and sorted(np.unique(val_labels)) == [0, 1, 2]
    trainer, losses, sample, lines, expected = _train(copy.deepcopy(cfg), dev, 4, val_views, val_labels)
    # the trajectory: the four steps' losses and a seeded sample of every master weight, bit for bit
    assert len(losses) == len(plain_losses) == 4
    for s in range(4):
        assert losses[s] == plain_losses[s], s
    for name in plain_sample:
        assert torch.equal(sample[name], plain_sample[name]), name
    # the metric: logged after steps 2 and 4, equal to evaluate_parts on segment outputs from the same weights
    # (the val/ keys are logged in alphabetical order, val/steps_done last: one block per report)
    logged, block = {}, {}
    for ln in lines:
        m = re.match(r"\[INFO\] \[LoggingHook\]: (val/\S+): (\S+)", ln)
        if m:
            block[m.group(1)] = float(m.group(2))
            if m.group(1) == "val/steps_done":
                logged.setdefault(int(block["val/steps_done"]), block)
                block = {}
    assert sorted(expected) == [2, 4] and sorted(logged) == [2, 4]
    for step in (2, 4):
        assert logged[step]["val/overall"] == expected[step]["overall"], step
        assert sorted(k for k in logged[step] if k.startswith("val/iou_")) == ["val/iou_{}".format(g) for g in sorted(expected[step]["iou"])]
        for g, v in expected[step]["iou"].items():
            assert logged[step]["val/iou_{}".format(g)] == v, (step, g)
    assert trainer.fetch_logs()["val/overall"] == expected[4]["overall"]
