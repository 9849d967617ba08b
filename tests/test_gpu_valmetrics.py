"""GPU tests of the label-free validation metrics: ups_image_metrics and ups_part_usage (csrc/valmetrics.hip, through the C ABI)
against the NumPy float64 restatement of valmetrics_ref.py, the two evaluators, `val_metrics` in the trainer and `eval_metrics` in
`-e`.  Integers compare with ==; float64 sums within the derived bounds of valmetrics_ref (reordered sums; SSIM 1e-10 per image)."""
import copy
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import valmetrics_ref as V
from parteval_ref import write_label_dataset

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements in front of and behind every output and scratch buffer that must keep the sentinel
ISENT = -0x5A5A5A5B
FSENT = -7.0e77
VGG_W = (8, 8, 16, 16, 16)
E_ARG, E_UNSUPPORTED = -1, -2


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil, lib, ops
    return lib, ops, evalutil


class _Guarded(object):
    """`n` elements inside a sentinel-filled buffer with GUARD elements on each side.  float64: the inside starts as NaN (an output
    must be written completely) or as the sentinel (scratch: nothing may be read before it is written); int32: zero."""

    def __init__(self, dev, n, dtype=torch.int32, inside=0):
        self.sent = ISENT if dtype == torch.int32 else FSENT
        self.buf = torch.full((GUARD + n + GUARD,), self.sent, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n]
        self.view.fill_(inside)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())


def _wptr(w):
    return w.ctypes.data_as(C.POINTER(C.c_double))


def _image_metrics(L, dev, ta, tb):
    """ups_image_metrics on device tensors [N,H,W,ld] -> (rc, out _Guarded [N*3], scratch _Guarded)."""
    N, H, W = ta.shape[:3]
    lib = L.load()
    nbytes = lib.ups_image_metrics_scratch_bytes(N, H, W)
    assert nbytes % 8 == 0
    out = _Guarded(dev, N * 3, torch.float64, float("nan"))
    scratch = _Guarded(dev, max(1, nbytes // 8), torch.float64, FSENT)
    w = V.window()
    rc = lib.ups_image_metrics(L.ptr(ta), L.dt(ta), ta.shape[3], L.ptr(tb), L.dt(tb), tb.shape[3], N, H, W, _wptr(w), out.ptr(),
                               scratch.ptr(), L.stream())
    torch.cuda.synchronize(dev)
    return rc, out, scratch


def _operands(dev, a, b, pair):
    """NumPy float32 operands -> (device a, device b, the values the device sees as float32 NumPy)."""
    if pair == "bf16x8_f32x3":
        a = V.bf16_round(a)
        return torch.from_numpy(a).to(dev).to(torch.bfloat16), torch.from_numpy(b).to(dev), a, b
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), a, b


T = 32          # = ops.IMAGE_METRICS_TILE (asserted below): valid extents T-1, T, T+1 and 2T+1 occur in each dimension, non-square
IMAGE_SHAPES = [(1, 11, 11), (2, 12, 27), (2, 10 + T - 1, 10 + T), (1, 10 + T, 10 + 2 * T + 1), (5, 10 + T + 1, 10 + T - 1),
                (1, 10 + 2 * T + 1, 10 + T + 1)]


@pytest.mark.parametrize("pair", ["f32x3_f32x3", "bf16x8_f32x3"])
@pytest.mark.parametrize("shape", IMAGE_SHAPES, ids=["x".join(map(str, s)) for s in IMAGE_SHAPES])
def test_image_metrics_equal_the_restatement(shape, pair, dev):
    L, ops, _ = _mods()
    assert ops.IMAGE_METRICS_TILE == T == L.load().ups_image_metrics_tile()
    N, H, W = shape
    rng = np.random.RandomState(sum(shape))
    a, b = V.image_pair(rng, N, H, W, 8 if pair == "bf16x8_f32x3" else 3, 3)
    ta, tb, a, b = _operands(dev, a, b, pair)
    assert a[..., :3].min() < -1 and a[..., :3].max() > 1 and (a[..., :3] == 1).any() and (a[..., :3] == -1).any()
    want = V.image_metrics(a, b)
    rc, out, scratch = _image_metrics(L, dev, ta, tb)
    assert rc == 0, L.load().ups_last_error().decode()
    got = out.view.cpu().numpy().reshape(N, 3)
    print("image_metrics", shape, pair, "rel sse", np.abs(got[:, 0] / want[:, 0] - 1).max(), "rel sae", np.abs(got[:, 1] / want[:, 1] - 1).max(),
          "abs ssim", np.abs(got[:, 2] - want[:, 2]).max() / (3 * (H - 10) * (W - 10)))
    assert np.isfinite(got).all(), "an output was not written"
    assert out.intact() and scratch.intact(), "wrote outside out / scratch"
    n = 3 * H * W
    assert (np.abs(got[:, 0] - want[:, 0]) <= V.sum_rtol(n) * want[:, 0]).all()
    assert (np.abs(got[:, 1] - want[:, 1]) <= V.sum_rtol(n) * want[:, 1]).all()
    assert (np.abs(got[:, 2] - want[:, 2]) / (3 * (H - 10) * (W - 10)) <= V.SSIM_ATOL).all()
    # a second launch on the same inputs: the same bits
    rc, again, _ = _image_metrics(L, dev, ta, tb)
    assert rc == 0 and torch.equal(again.view, out.view)


def test_image_metrics_identical_operands(dev):
    L, _, _ = _mods()
    N, H, W = 2, 10 + T - 1, 10 + T
    a, _ = V.image_pair(np.random.RandomState(9), N, H, W)
    ta = torch.from_numpy(a).to(dev)
    rc, out, scratch = _image_metrics(L, dev, ta, ta.clone())
    assert rc == 0
    got = out.view.cpu().numpy().reshape(N, 3)
    assert (got[:, 0] == 0).all() and (got[:, 1] == 0).all()
    assert np.abs(got[:, 2] / (3 * (H - 10) * (W - 10)) - 1.0).max() <= 1e-10
    assert out.intact() and scratch.intact()


def test_image_metrics_refusals(dev):
    L, _, _ = _mods()
    lib = L.load()
    w = V.window()
    out = _Guarded(dev, 6, torch.float64, float("nan"))
    scratch = _Guarded(dev, 64, torch.float64, FSENT)
    x3 = torch.zeros((2, 16, 16, 3), device=dev)
    x2 = torch.zeros((2, 16, 16, 2), device=dev)
    s = L.stream()

    def call(a, dta, lda, b, dtb, ldb, H, W, wp=_wptr(w), o=out.ptr(), sc=scratch.ptr()):
        return lib.ups_image_metrics(a, dta, lda, b, dtb, ldb, 2, H, W, wp, o, sc, s)
    assert call(L.ptr(x3), L.F32, 3, L.ptr(x3), L.F32, 3, 10, 16) == E_ARG          # H = 10
    assert call(L.ptr(x3), L.F32, 3, L.ptr(x3), L.F32, 3, 16, 10) == E_ARG
    assert call(L.ptr(x2), L.F32, 2, L.ptr(x3), L.F32, 3, 16, 16) == E_ARG          # ld = 2
    assert call(L.ptr(x3), L.F32, 3, L.ptr(x2), L.F32, 2, 16, 16) == E_ARG
    assert call(None, L.F32, 3, L.ptr(x3), L.F32, 3, 16, 16) == E_ARG               # a null operand
    assert call(L.ptr(x3), L.F32, 3, None, L.F32, 3, 16, 16) == E_ARG
    assert call(L.ptr(x3), L.F16, 3, L.ptr(x3), L.F32, 3, 16, 16) == E_ARG          # another dtype
    assert call(L.ptr(x3), L.F32, 3, L.ptr(x3), L.F32, 3, 16, 16, o=None) == E_ARG
    assert call(L.ptr(x3), L.F32, 3, L.ptr(x3), L.F32, 3, 16, 16, sc=None) == E_ARG
    assert call(L.ptr(x3), L.F32, 3, L.ptr(x3), L.F32, 3, 16, 16, wp=None) == E_ARG
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out.view).all()) and bool((scratch.view == FSENT).all()) and out.intact() and scratch.intact()


# ---------------------------------------------------------------------------------------------- ups_part_usage
def _part_usage(L, dev, soft, pred, P):
    N = soft.shape[0]
    HW = pred.size // N
    lib = L.load()
    ts, tp = torch.from_numpy(soft).to(dev), torch.from_numpy(pred.astype(np.int64)).to(dev)
    nbytes = lib.ups_part_usage_scratch_bytes(N, HW)
    counts, invalid = _Guarded(dev, N * P), _Guarded(dev, 1)
    sharp = _Guarded(dev, N * 2, torch.float64, float("nan"))
    scratch = _Guarded(dev, max(1, nbytes // 8), torch.float64, FSENT)
    rc = lib.ups_part_usage(L.ptr(ts), L.ptr(tp), N, HW, P, counts.ptr(), invalid.ptr(), sharp.ptr(), scratch.ptr(), L.stream())
    torch.cuda.synchronize(dev)
    return rc, counts, invalid, sharp, scratch


CH = 1024       # = ops.PART_USAGE_CHUNK (asserted below)
USAGE_SHAPES = [(1, 1, 1), (2, 7, 3), (3, CH - 1, 10), (3, CH, 10), (3, CH + 1, 10), (3, 2 * CH + 5, 10), (2, 256, 25), (1, 4096, 32)]


@pytest.mark.parametrize("shape", USAGE_SHAPES, ids=["x".join(map(str, s)) for s in USAGE_SHAPES])
def test_part_usage_equals_the_restatement(shape, dev):
    L, ops, _ = _mods()
    assert ops.PART_USAGE_CHUNK == CH == L.load().ups_part_usage_chunk()
    N, HW, P = shape
    soft, pred = V.soft_maps(np.random.RandomState(sum(shape)), N, HW, P)
    if HW >= 4:
        assert (soft == 0).any() and (soft == 1).any() and (pred == -1).any() and (pred == P).any()
    want_c, want_bad, want_s, terms = V.part_usage(soft, pred, P)
    rc, counts, invalid, sharp, scratch = _part_usage(L, dev, soft, pred, P)
    assert rc == 0, L.load().ups_last_error().decode()
    assert np.array_equal(counts.view.cpu().numpy().reshape(N, P), want_c)
    assert int(invalid.view.cpu()) == want_bad == (2 * N if HW >= 4 else 0)
    got = sharp.view.cpu().numpy().reshape(N, 2)
    print("part_usage", shape, "rel", (np.abs(got - want_s) / np.maximum(terms, 1e-300)).max(axis=0))
    assert np.isfinite(got).all(), "an output was not written"
    assert (np.abs(got[:, 0] - want_s[:, 0]) <= V.sharp_rtol(HW) * terms[:, 0]).all()
    assert (np.abs(got[:, 1] - want_s[:, 1]) <= V.sharp_rtol(HW * P) * terms[:, 1]).all()
    for g in (counts, invalid, sharp, scratch):
        assert g.intact(), "wrote outside an output or the scratch"
    rc, _, _, again, _ = _part_usage(L, dev, soft, pred, P)
    assert rc == 0 and torch.equal(again.view, sharp.view)


def test_part_usage_above_the_table_and_the_host_route(dev, caplog):
    L, ops, E = _mods()
    N, HW, P = 2, 40, 33
    soft, pred = V.soft_maps(np.random.RandomState(33), N, HW, P)
    rc, counts, invalid, sharp, scratch = _part_usage(L, dev, soft, pred, P)
    assert rc == E_UNSUPPORTED
    assert int(counts.view.abs().sum()) == 0 and bool(torch.isnan(sharp.view).all()) and counts.intact() and sharp.intact()
    ts, tp = torch.from_numpy(soft).to(dev), torch.from_numpy(pred).to(dev)
    with pytest.raises(L.UpsError):
        ops.part_usage(ts, tp)
    assert _part_usage(L, dev, soft, pred, 0)[0] == E_ARG
    # the evaluator computes the same quantities on the host, and says so once
    want_c, want_bad, want_s, terms = V.part_usage(soft, pred, P)
    import logging
    with caplog.at_level(logging.INFO, logger="upsparts"):
        ev = E.PartUsageEvaluator(dev, P)
    assert sum("on the host" in r.getMessage() for r in caplog.records) == 1
    ev.update(ts, tp)
    c, s, bad = ev.sums()
    assert np.array_equal(c, want_c) and bad == want_bad == 2 * N
    assert (np.abs(s[:, 0] - want_s[:, 0]) <= V.sharp_rtol(HW) * terms[:, 0]).all()
    assert (np.abs(s[:, 1] - want_s[:, 1]) <= V.sharp_rtol(HW * P) * terms[:, 1]).all()
    with pytest.raises(L.UpsError, match=str(2 * N)):
        ev.result()
    ok = np.where((pred < 0) | (pred >= P), 0, pred)
    ev.reset()
    ev.update(ts, torch.from_numpy(ok).to(dev))
    want = V.usage_from_counts(V.part_usage(soft, ok, P)[0], want_s, HW, 0.005)
    got = ev.result()
    assert got["part_area"] == want["part_area"] and got["parts_active"] == want["parts_active"]
    assert abs(got["entropy"] - want["entropy"]) <= V.sharp_rtol(HW * P) * terms[:, 1].sum() / (N * HW)


# ---------------------------------------------------------------------------------------------- wrappers / evaluators
def test_evaluators_accumulate_rows_on_the_device(dev):
    """Two updates of 40 images: 80 rows, so both buffers grow past their first 64 rows and keep what they held."""
    _, ops, E = _mods()
    rng = np.random.RandomState(4)
    a, b = V.image_pair(rng, 80, 11, 13, 8, 3)
    ta, tb, a, b = _operands(dev, a, b, "bf16x8_f32x3")
    rec = E.ReconstructionEvaluator(dev)
    rec.update(ta[:40], tb[:40])
    rec.update(ta[40:], tb[40:], valid=39)
    want = V.image_metrics(a[:79], b[:79])
    rows = rec.rows()
    assert rec.n == 79 and rows.shape == (79, 3)
    n = 3 * 11 * 13
    assert (np.abs(rows[:, :2] - want[:, :2]) <= V.sum_rtol(n) * want[:, :2]).all()
    assert (np.abs(rows[:, 2] - want[:, 2]) / (3 * 1 * 3) <= V.SSIM_ATOL).all()
    got, ref = rec.result(), V.reconstruction_from_sums(want, 11, 13)
    assert abs(got["mse"] - ref["mse"]) <= V.sum_rtol(n) * ref["mse"] and abs(got["ssim"] - ref["ssim"]) <= V.SSIM_ATOL
    # the wrapper alone, on identical fp32 operands
    one = ops.image_metrics(tb[:3], tb[:3].clone()).cpu().numpy()
    assert (one[:, :2] == 0).all() and np.abs(one[:, 2] / 9 - 1.0).max() <= 1e-10
    with pytest.raises(ValueError):
        rec.update(ta[:2, :, :12].contiguous(), tb[:2, :, :12].contiguous())
    soft, pred = V.soft_maps(rng, 80, 7, 3)
    pred = np.where((pred < 0) | (pred >= 3), 1, pred)
    ts, tp = torch.from_numpy(soft).to(dev), torch.from_numpy(pred).to(dev)
    use = E.PartUsageEvaluator(dev, 3, 0.005)
    use.update(ts[:40], tp[:40])
    use.update(ts[40:], tp[40:], valid=39)
    want_c, _, want_s, terms = V.part_usage(soft[:79], pred[:79], 3)
    c, s, bad = use.sums()
    assert bad == 0 and np.array_equal(c, want_c) and c.dtype == np.int32
    assert (np.abs(s[:, 0] - want_s[:, 0]) <= V.sharp_rtol(7) * terms[:, 0]).all()
    assert (np.abs(s[:, 1] - want_s[:, 1]) <= V.sharp_rtol(7 * 3) * terms[:, 1]).all()
    assert use.result()["part_area"] == V.usage_from_counts(want_c, want_s, 7, 0.005)["part_area"]
    rec.reset()
    use.reset()
    assert rec.n == 0 and use.n == 0
    with pytest.raises(ValueError):
        rec.result()


# ---------------------------------------------------------------------------------------------- trainer: `val_metrics`
def _expected_on_pairs(trainer):
    """The restatement on the tensors of one forward per chunk of the trainer's pair set, under the current weights."""
    model, pairs = trainer.model, trainer._val["pairs"]
    rows, counts, sharps, terms, recs = [], [], [], [], []
    P = model.n_parts
    for ci in range(pairs.chunks()):
        chunk = pairs.chunk_views(ci, trainer.device)
        out = model.forward(chunk, noise=None)
        gen = model.generated_act
        rows.append(V.image_metrics(gen[..., :3].float().cpu().numpy(), chunk["view0"].cpu().numpy()))
        c, bad, s, t = V.part_usage(out["out_parts_soft"].cpu().numpy().reshape(gen.shape[0], -1, P), out["out_parts_hard"].cpu().numpy(), P)
        assert bad == 0
        counts.append(c), sharps.append(s), terms.append(t)
        with torch.no_grad():
            recs.append(float(trainer.vgg.loss(chunk["view0"].contiguous(), gen, model.act_dtype, gram_weight=trainer.gram_weight).double()))
    return {"rows": np.concatenate(rows), "counts": np.concatenate(counts), "sharp": np.concatenate(sharps),
            "terms": np.concatenate(terms), "rec": float(np.mean(np.asarray(recs, dtype=np.float64)))}


def _train(cfg, dev, steps, hook=False):
    import upsparts_amd  # noqa: F401
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
            if hook and trainer.global_step in (2, 4):
                expected[trainer.global_step] = _expected_on_pairs(trainer)
    trainer.iterate(feed(), num_steps=steps, log_fn=lines.append)
    rng = np.random.RandomState(0)
    sample = {}
    for name in sorted(model.variables):
        flat = model.variables[name].detach().reshape(-1)
        idx = torch.from_numpy(rng.randint(0, flat.numel(), min(16, flat.numel()))).to(flat.device)
        sample[name] = flat[idx].cpu()
    return trainer, losses[:steps], sample, lines, expected


def _val_blocks(lines):
    logged, block, order = {}, {}, []
    for ln in lines:
        m = re.match(r"\[INFO\] \[LoggingHook\]: (val/\S+): (\S+)", ln)
        if m:
            block[m.group(1)] = float(m.group(2))
            order.append(m.group(1))
            if m.group(1) == "val/steps_done":
                logged.setdefault(int(block["val/steps_done"]), (block, order))
                block, order = {}, []
    return logged


def test_val_metrics_report_and_leave_the_trajectory_alone(dev, tmp_path):
    from oracle import configs
    base = copy.deepcopy(configs.tiny_config())
    base.update({"precision": "bf16", "vgg_widths": VGG_W, "ckpt_freq": 0, "log_freq": 250})
    B, S, P = base["batch_size"], base["spatial_size"], base["n_parts"]
    assert (B, S, P) == (2, 16, 3)
    ds = write_label_dataset(tmp_path, n=5, S=S, seed=4, name="val")
    ds.pop("data_gt_segmentation_column")                               # no label column in the config
    cfg = dict(base, **ds)
    cfg.update({"val_freq": 2, "val_csv": cfg.pop("data_csv"), "val_metrics": ["reconstruction", "parts"]})
    # A: plain
    _, plain_losses, plain_sample, plain_lines, _ = _train(copy.deepcopy(base), dev, 4)
    assert not any("val/" in ln for ln in plain_lines)
    # B: the keys set -- the same four steps, bit for bit
    trainer_b, losses, sample, lines_b, _ = _train(copy.deepcopy(cfg), dev, 4)
    assert len(losses) == len(plain_losses) == 4
    for s in range(4):
        assert losses[s] == plain_losses[s], s
    for name in plain_sample:
        assert torch.equal(sample[name], plain_sample[name]), name
    assert sorted(_val_blocks(lines_b)) == [2, 4]
    # C: the keys and a hook that runs the same forward passes after steps 2 and 4
    trainer, _, _, lines, expected = _train(copy.deepcopy(cfg), dev, 4, hook=True)
    assert len(trainer._val["pairs"]) == 4 and trainer._val["pairs"].chunks() == 2 and trainer._val["rec"].n == 4
    assert trainer._val["usage"].n == 4 and "evaluator" not in trainer._val
    logged = _val_blocks(lines)
    assert sorted(expected) == [2, 4] and sorted(logged) == [2, 4]
    names = sorted(["val/mse", "val/l1", "val/psnr", "val/ssim", "val/rec", "val/parts_active", "val/confidence", "val/entropy"]
                   + ["val/part_area_{}".format(p) for p in range(P)])
    n, HW = 3 * S * S, S * S
    for step in (2, 4):
        got, order = logged[step]
        assert order == names + ["val/steps_done"], order            # sorted, val/steps_done closes the block
        e = expected[step]
        rec = V.reconstruction_from_sums(e["rows"], S, S)
        use = V.usage_from_counts(e["counts"], e["sharp"], HW, 0.005)
        print("val step", step, {k: (got["val/" + k], rec[k]) for k in rec}, got["val/rec"], e["rec"])
        for p in range(P):
            assert got["val/part_area_{}".format(p)] == use["part_area"][p], (step, p)
        assert got["val/parts_active"] == use["parts_active"]
        assert abs(got["val/mse"] - rec["mse"]) <= V.sum_rtol(n) * rec["mse"]
        assert abs(got["val/l1"] - rec["l1"]) <= V.sum_rtol(n) * rec["l1"]
        # psnr = -10 log10(mse): d psnr = (10 / ln 10) d mse / mse, plus the roundings of log10, the division and the mean
        assert abs(got["val/psnr"] - rec["psnr"]) <= 10.0 / math.log(10.0) * V.sum_rtol(n) + 8 * 2.0 ** -53 * abs(rec["psnr"])
        assert abs(got["val/ssim"] - rec["ssim"]) <= V.SSIM_ATOL
        assert abs(got["val/confidence"] - use["confidence"]) <= V.sharp_rtol(HW) * e["terms"][:, 0].sum() / (4 * HW)
        assert abs(got["val/entropy"] - use["entropy"]) <= V.sharp_rtol(HW * P) * e["terms"][:, 1].sum() / (4 * HW)
        assert got["val/rec"] == e["rec"], step
    last = trainer.fetch_logs()
    assert last["val/steps_done"] == 4 and last["val/rec"] == expected[4]["rec"] and last["val/mse"] == logged[4][0]["val/mse"]


# ---------------------------------------------------------------------------------------------- runner: `eval_metrics`
def test_runner_eval_metrics_writes_metrics_yml(dev, tmp_path):
    """`-e` over five images at batch 2 (a ragged last batch) with and without eval_metrics: metrics.yml holds the restatement's numbers
    on the pickled outputs, every other file is byte-identical."""
    import os
    import pickle
    import yaml
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(write_label_dataset(tmp_path, n=5, S=cfg["spatial_size"]))
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W)})
    S, P = cfg["spatial_size"], cfg["n_parts"]
    ypath = tmp_path / "eval.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    runner.main(["-e", str(ypath), "-p", str(tmp_path / "plain"), "--strict-dataset"])
    runner.main(["-e", str(ypath), "-p", str(tmp_path / "metrics"), "--strict-dataset", "--set", "eval_metrics=[reconstruction, parts]"])
    pdir, mdir = tmp_path / "plain" / "eval" / "0", tmp_path / "metrics" / "eval" / "0"
    assert sorted(os.listdir(str(mdir))) == sorted(os.listdir(str(pdir)) + ["metrics.yml"])
    for f in os.listdir(str(pdir)):
        assert (pdir / f).read_bytes() == (mdir / f).read_bytes(), f
    data = pickle.loads((mdir / "model_outputs.p").read_bytes())
    gen, v0 = data["outputs"]["generated"], data["inputs"]["view0"]
    assert gen.shape == (5, S, S, 3)
    rec = V.reconstruction_from_sums(V.image_metrics(gen, v0), S, S)
    c, bad, s, terms = V.part_usage(data["outputs"]["out_parts_soft"].reshape(5, S * S, P), data["outputs"]["out_parts_hard"], P)
    use = V.usage_from_counts(c, s, S * S, 0.005)
    got = yaml.safe_load((mdir / "metrics.yml").read_text())
    assert sorted(got) == sorted(["mse", "l1", "psnr", "ssim", "parts_active", "confidence", "entropy"] + ["part_area_{}".format(p) for p in range(P)])
    n = 3 * S * S
    assert bad == 0 and got["parts_active"] == use["parts_active"]
    for p in range(P):
        assert got["part_area_{}".format(p)] == use["part_area"][p]
    assert abs(got["mse"] - rec["mse"]) <= V.sum_rtol(n) * rec["mse"] and abs(got["l1"] - rec["l1"]) <= V.sum_rtol(n) * rec["l1"]
    assert abs(got["psnr"] - rec["psnr"]) <= 10.0 / math.log(10.0) * V.sum_rtol(n) + 8 * 2.0 ** -53 * abs(rec["psnr"])
    assert abs(got["ssim"] - rec["ssim"]) <= V.SSIM_ATOL
    assert abs(got["confidence"] - use["confidence"]) <= V.sharp_rtol(S * S) * terms[:, 0].sum() / (5 * S * S)
    assert abs(got["entropy"] - use["entropy"]) <= V.sharp_rtol(S * S * P) * terms[:, 1].sum() / (5 * S * S)
