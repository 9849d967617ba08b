"""GPU tests of the segmentation export: ups_segment_render (csrc/segexport.hip, through the C ABI) against the NumPy float64
restatement of segexport_ref.py, its memory contract and refusals, ``TrainModel.segment_soft`` / ``export_segments`` and
``upsparts-run --segment``.  Everything compares with ==: the kernel decides in fp64, operation for operation as the restatement."""
import copy
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

import segexport_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements in front of and behind every output that must keep the sentinel
BSENT = 0xA5                     # also what the alignment gaps between packed images must still hold
ISENT = -0x5A5A5A5B
VGG_W = (8, 8, 16, 16, 16)
E_ARG, E_UNSUPPORTED = -1, -2
ALL = ("labels", "overlay", "confidence", "counts")


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


class _Guarded(object):
    """`n` elements inside a sentinel-filled buffer with GUARD elements on each side (the pattern of test_gpu_valmetrics.py).
    uint8 planes start as the sentinel inside as well: the kernel writes the pixels of the images and nothing else."""

    def __init__(self, dev, n, dtype=torch.uint8, inside=None):
        self.sent = BSENT if dtype == torch.uint8 else ISENT
        self.buf = torch.full((GUARD + n + GUARD,), self.sent, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n]
        if inside is not None:
            self.view.fill_(inside)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())


def _sizes(S):
    """The mixed launch of the issue, an image of several chunks whose pixel count is no multiple of 4, one-chunk images behind it."""
    return [(S, S), (2 * S, 2 * S), (3 * S + 1, 2 * S - 3), (1, 1), (1, 37), (S // 2, S // 2), (5, 4 * S),
            (45, 47), (3, 3), (2, 5), (7, 1), (S, S)]


def _inputs(seed, S, P, sizes, kind="random"):
    rng = np.random.RandomState(seed)
    soft = R.soft_maps(rng, len(sizes), S, P, kind)
    colors = rng.randint(0, 256, size=(P, 3)).astype(np.uint8)
    srcs = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    return soft, colors, srcs


def _launch(dev, soft, sizes, colors, srcs, alpha, which=ALL, counts_init=0, table=None, total=None, n=None, P=None, S=None):
    """One ups_segment_render call on guarded outputs -> (rc, {name: _Guarded}).  `table` / `total` / n / P / S override what the
    sizes give (the refusals)."""
    L, ops = _mods()
    lib = L.load()
    tab, tot = ops.segment_table(sizes)
    if table is not None:
        tab = np.ascontiguousarray(table, dtype=np.int32)
    ts = torch.from_numpy(soft).to(dev)
    td = torch.from_numpy(tab).to(dev)
    tc = None if colors is None else torch.from_numpy(colors).to(dev)
    tsrc = None if srcs is None else ops.segment_pack_sources(srcs, ops.segment_table(sizes)[0], tot).to(dev)
    out = {"labels": _Guarded(dev, tot), "overlay": _Guarded(dev, 3 * tot), "confidence": _Guarded(dev, tot),
           "counts": _Guarded(dev, soft.shape[0] * soft.shape[3], torch.int32, counts_init)}
    p = {k: (out[k].ptr() if k in which else None) for k in ALL}
    rc = lib.ups_segment_render(L.ptr(ts), soft.shape[0] if n is None else n, soft.shape[1] if S is None else S,
                                soft.shape[3] if P is None else P, tab.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(td),
                                tot if total is None else total, L.ptr(tsrc), L.ptr(tc), float(alpha), p["labels"], p["overlay"],
                                p["confidence"], p["counts"], L.stream())
    torch.cuda.synchronize(dev)
    return rc, out


def _check(out, want, which, counts_init=0):
    """Every wanted plane equals the restatement's packed plane byte for byte, the alignment gaps (which the restatement fills with
    the sentinel) included; every other plane is untouched; the guard bands are intact."""
    for k in ALL:
        assert out[k].intact(), "wrote outside " + k
        got = out[k].view.cpu().numpy()
        if k not in which:
            assert (got == (counts_init if k == "counts" else BSENT)).all(), k + " was not asked for and was written"
        elif k == "counts":
            assert (got.reshape(want[k].shape) == want[k] + counts_init).all(), "counts differ"
        else:
            ref = want[k].reshape(-1)
            bad = np.nonzero(got != ref)[0]
            assert bad.size == 0, "{}: {} of {} bytes differ, first at {} (got {}, want {})".format(
                k, bad.size, ref.size, bad[:1], got[bad[:1]], ref[bad[:1]])


@pytest.mark.parametrize("P", [1, 2, 10, 33])
@pytest.mark.parametrize("S", [4, 16])
def test_kernel_equals_the_restatement(S, P, dev):
    L, ops = _mods()
    assert ops.SEGMENT_CHUNK == R.CHUNK == L.load().ups_segment_chunk()
    sizes = _sizes(S)
    assert 45 * 47 > 2 * R.CHUNK and (45 * 47) % 4 == 3
    soft, colors, srcs = _inputs(100 * S + P, S, P, sizes)
    want = R.render_packed(soft, sizes, colors, srcs, 0.5, fill=BSENT)
    assert (np.diff(want["table"][:, 0]) > (want["table"][:-1, 1] * want["table"][:-1, 2])).any(), "no alignment gap in this launch"
    rc, out = _launch(dev, soft, sizes, colors, srcs, 0.5)
    assert rc == 0, L.load().ups_last_error().decode()
    _check(out, want, ALL)
    if P > 1:
        assert (want["counts"] > 0).sum() > len(sizes), "the maps are not varied enough to test anything"
    # the model-size images are the arg-max of the map itself
    lab = out["labels"].view.cpu().numpy()
    for i in (0, len(sizes) - 1):
        o = int(want["table"][i, 0])
        assert (lab[o:o + S * S].reshape(S, S) == np.argmax(soft[i], axis=2)).all()


@pytest.mark.parametrize("kind", ["ties", "onehot"])
def test_tie_and_one_hot_maps(kind, dev):
    S, P = 16, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(7, S, P, sizes, kind)
    want = R.render_packed(soft, sizes, colors, srcs, 0.5, fill=BSENT)
    if kind == "ties":           # the first of two equal maxima, at every model-size pixel
        v = soft[0].astype(np.float64)
        assert ((v == v.max(axis=2, keepdims=True)).sum(axis=2) >= 2).all()
    rc, out = _launch(dev, soft, sizes, colors, srcs, 0.5)
    assert rc == 0
    _check(out, want, ALL)


@pytest.mark.parametrize("with_src", [True, False], ids=["src", "nosrc"])
@pytest.mark.parametrize("which", [("labels",), ("overlay",), ("confidence",), ("counts",), ALL], ids=["labels", "overlay", "confidence",
                                                                                                       "counts", "all"])
def test_each_output_alone_and_all_together(which, with_src, dev):
    S, P = 4, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(11, S, P, sizes)
    want = R.render_packed(soft, sizes, colors, srcs if with_src else None, 0.5, fill=BSENT)
    if not with_src:
        o, (h, w) = int(want["table"][2, 0]), sizes[2]
        assert (want["overlay"][o:o + h * w] == colors[want["labels"][o:o + h * w]]).all()
    rc, out = _launch(dev, soft, sizes, colors, srcs if with_src else None, 0.5, which)
    assert rc == 0
    _check(out, want, which)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_overlay_alpha(alpha, dev):
    S, P = 4, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(13, S, P, sizes)
    want = R.render_packed(soft, sizes, colors, srcs, alpha, fill=BSENT)
    rc, out = _launch(dev, soft, sizes, colors, srcs, alpha)
    assert rc == 0
    _check(out, want, ALL)
    got = out["overlay"].view.cpu().numpy().reshape(-1, 3)
    o, (h, w) = int(want["table"][2, 0]), sizes[2]
    if alpha == 0.0:
        assert (got[o:o + h * w] == srcs[2].reshape(-1, 3)).all()
    if alpha == 1.0:
        assert (got[o:o + h * w] == colors[want["labels"][o:o + h * w]]).all()


def test_counts_are_added_to(dev):
    """The contract of `counts` is ups_part_confusion's: the kernel ADDS (caller-zeroed, or earlier launches' counts)."""
    S, P = 4, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(17, S, P, sizes)
    want = R.render_packed(soft, sizes, colors, srcs, 0.5, fill=BSENT)
    rc, out = _launch(dev, soft, sizes, colors, srcs, 0.5, ("counts", "labels"), counts_init=7)
    assert rc == 0
    _check(out, want, ("counts", "labels"), counts_init=7)
    assert want["counts"].sum(axis=1).tolist() == [h * w for h, w in sizes]


def test_refusals_launch_nothing(dev):
    L, ops = _mods()
    S, P = 4, 3
    sizes = [(4, 4), (5, 7), (2, 2)]
    soft, colors, srcs = _inputs(19, S, P, sizes)
    tab, tot = ops.segment_table(sizes)

    def refused(code, **kw):
        which = kw.pop("which", ALL)
        col = kw.pop("colors", colors)
        rc, out = _launch(dev, soft, sizes, col, srcs, kw.pop("alpha", 0.5), which, **kw)
        assert rc == code, (rc, code, kw, L.load().ups_last_error().decode())
        for k in ALL:
            got = out[k].view.cpu().numpy()
            assert (got == (0 if k == "counts" else BSENT)).all() and out[k].intact(), "a refused call wrote " + k

    def edited(row, col, value):
        t = tab.copy()
        t[row, col] = value
        return t
    refused(E_ARG, P=0)
    refused(E_UNSUPPORTED, P=256)
    refused(E_ARG, n=0)
    refused(E_ARG, table=edited(1, 1, 0))               # h = 0
    refused(E_ARG, table=edited(1, 2, 0))               # w = 0
    refused(E_ARG, table=edited(1, 2, -3))
    refused(E_ARG, table=edited(1, 0, tab[1, 0] + 4))   # a misaligned offset
    refused(E_ARG, table=edited(2, 0, tab[1, 0]))       # overlapping images
    refused(E_ARG, table=edited(2, 3, 5))               # a first_block that is not the prefix sum
    refused(E_ARG, total=tot - 16)                      # the last image ends behind the planes
    refused(E_ARG, which=())                            # all four outputs null
    refused(E_ARG, colors=None)                         # an overlay without a colour table
    refused(E_ARG, alpha=1.5)
    refused(E_ARG, alpha=float("nan"))


def test_ops_segment_render(dev):
    L, ops = _mods()
    S, P = 16, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(23, S, P, sizes)
    want = R.render_packed(soft, sizes, colors, srcs, 0.25, fill=0)
    ts = torch.from_numpy(soft).to(dev)
    res = ops.segment_render(ts, sizes, src=srcs, colors=colors, alpha=0.25, want=ALL)
    assert (res["table"] == want["table"]).all() and res["total"] == want["total"]
    for k in ALL:
        assert (res[k].cpu().numpy().reshape(want[k].shape) == want[k]).all(), k
    for i, (h, w) in enumerate(sizes):
        one = R.render(soft[i], h, w, colors, srcs[i], 0.25)
        assert tuple(res["views"]["labels"][i].shape) == (h, w) and tuple(res["views"]["overlay"][i].shape) == (h, w, 3)
        for k in ("labels", "overlay", "confidence"):
            assert (res["views"][k][i].cpu().numpy() == one[k]).all()
    # planes handed back in are reused, counts added to
    again = ops.segment_render(ts, sizes, want=("labels", "counts"), out={"labels": res["labels"], "counts": res["counts"]})
    assert again["labels"] is res["labels"] and (again["counts"].cpu().numpy() == 2 * want["counts"]).all()
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes, want=("overlay",))
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes[:-1])
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes, want=("masks",))


# ---------------------------------------------------------------------------------------------- the model
def _model(precision, dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel
    from oracle import configs, ref_model
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(precision=precision, vgg_widths=VGG_W)
    return cfg, TrainModel(cfg, device=dev, seed=0), ref_model


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_segment_soft_and_export_segments(precision, dev):
    cfg, model, RM = _model(precision, dev)
    B, S, P = cfg["batch_size"], cfg["spatial_size"], cfg["n_parts"]
    views = RM.synthetic_views(cfg)
    a, b = views["view0"], views["view1"]
    fwd = model.forward({"view0": a, "view1": b})
    f_soft, f_hard = fwd["out_parts_soft"].clone(), fwd["out_parts_hard"].clone()
    gen = torch.Generator().manual_seed(3)
    v = torch.cat([a, b, torch.rand(1, S, S, 3, generator=gen) * 2 - 1], 0)        # a whole pass and a ragged one
    n = v.shape[0]
    seg = model.segment(v)
    hard, soft = model.segment_soft(v)
    assert soft.dtype == torch.float32 and tuple(soft.shape) == (n, S, S, P) and soft.device.type == "cuda"
    assert torch.equal(hard, seg) and (np.argmax(soft.cpu().numpy(), axis=3) == seg.cpu().numpy()).all()      # (NumPy: the first maximum)
    # the batch composition segment's docstring names: the first B maps of a pass of 2B are forward's
    assert torch.equal(soft[:B], f_soft) and torch.equal(hard[:B], f_hard)
    assert torch.equal(model.segment(v), seg), "segment() changed after segment_soft()"
    res = model.export_segments(v, [(S, S)] * n, outputs=("labels", "confidence"))
    res["ready"].synchronize()
    seg_h, soft_h = seg.cpu().numpy(), soft.cpu().numpy()
    for i in range(n):
        assert (res["views"]["labels"][i].numpy() == seg_h[i]).all()
        assert (res["views"]["confidence"][i].numpy() == R.render(soft_h[i], S, S)["confidence"]).all()
    assert (res["host"]["counts"].numpy() == np.stack([np.bincount(seg_h[i].reshape(-1), minlength=P) for i in range(n)])).all()
    assert torch.equal(res["soft"], soft)
    # at other sizes, with sources: the restatement on segment_soft's output
    sizes = [(37, 50), (S, S), (5, 3), (2 * S + 1, S - 1), (1, 1)]
    rng = np.random.RandomState(4)
    srcs = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    colors = rng.randint(0, 256, size=(P, 3)).astype(np.uint8)
    res = model.export_segments(v, sizes, sources=srcs, outputs=("labels", "overlay", "confidence"), alpha=0.3, colors=colors)
    res["ready"].synchronize()
    for i, (h, w) in enumerate(sizes):
        one = R.render(soft_h[i], h, w, colors, srcs[i], 0.3)
        for k in ("labels", "overlay", "confidence"):
            assert (res["views"][k][i].numpy() == one[k]).all(), (k, i)
        assert (res["host"]["counts"][i].numpy() == one["counts"]).all()


# ---------------------------------------------------------------------------------------------- the runner
def test_runner_segment_end_to_end(dev, tmp_path, caplog):
    import logging
    import yaml
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import imglog as IL, runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    S, P = cfg["spatial_size"], cfg["n_parts"]
    data_root = tmp_path / "images"
    rng = np.random.RandomState(6)
    files = [("a/one.png", (37, 46)), ("a/two.png", (S, S)), ("b/three.png", (21, 13)), ("four.png", (60, 90)), ("b/c/five.png", (9, 48))]
    for rel, (h, w) in files:
        os.makedirs(os.path.dirname(str(data_root / rel)), exist_ok=True)
        # smooth images (a few random blocks, enlarged): resizing them is not all noise
        small = rng.randint(0, 256, size=(4, 5, 3)).astype(np.uint8)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(str(data_root / rel))
    csv_path = tmp_path / "list.csv"
    csv_path.write_text("\n".join(rel for rel, _ in files) + "\n")
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(data_root), "segment_csv": str(csv_path),
                "segment_max_side": 48, "segment_outputs": ["labels", "overlay", "confidence"], "segment_alpha": 0.5})
    ypath = tmp_path / "segment.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    with caplog.at_level(logging.WARNING, logger="upsparts"):
        res = runner.main(["--segment", str(ypath), "-p", str(tmp_path / "run")])
    assert caplog.text.count("segment_max_side") == 1, "the scaling is logged once per run"
    odir = str(tmp_path / "run" / "segment" / "0")
    assert res["dir"] == odir
    # the restatement on segment_soft's output of the same model, from the files decoded as the runner decodes them
    imgs = [Image.open(str(data_root / rel)).convert("RGB") for rel, _ in files]
    views = np.stack([np.asarray(im.resize((S, S), Image.BILINEAR), dtype=np.float32) / 127.5 - 1.0 for im in imgs])
    _, soft = res["model"].segment_soft(torch.from_numpy(views))
    soft = soft.cpu().numpy()
    palette = IL.mask_color_bytes(IL.mask_colors01(P))
    with open(os.path.join(odir, "index.csv"), newline="") as f:
        index = list(csv.reader(f))
    assert index[0] == ["file", "h", "w"] + ["area_{}".format(p) for p in range(P)] and len(index) == 1 + len(files)
    for i, (rel, (h, w)) in enumerate(files):
        oh, ow = (32, 48) if rel == "four.png" else (h, w)         # 60 x 90 is larger than segment_max_side = 48
        src = np.asarray(imgs[i] if (oh, ow) == (h, w) else imgs[i].resize((ow, oh), Image.BILINEAR), dtype=np.uint8)
        one = R.render(soft[i], oh, ow, palette, src, 0.5)
        lab = Image.open(os.path.join(odir, "labels", rel + ".png"))
        assert lab.mode == "P" and lab.size == (ow, oh)
        assert (np.asarray(lab) == one["labels"]).all(), rel
        assert (np.asarray(lab.getpalette()[:3 * P], dtype=np.uint8).reshape(P, 3) == palette).all()
        assert (np.asarray(Image.open(os.path.join(odir, "overlay", rel + ".png"))) == one["overlay"]).all(), rel
        assert (np.asarray(Image.open(os.path.join(odir, "confidence", rel + ".png"))) == one["confidence"]).all(), rel
        assert index[1 + i][:3] == [rel, str(oh), str(ow)]
        assert [float(x) for x in index[1 + i][3:]] == [c / float(oh * ow) for c in one["counts"]]
    # a missing file raises; nothing synthetic stands in
    csv_path.write_text("a/one.png\nnot/there.png\n")
    with pytest.raises(FileNotFoundError):
        runner.main(["--segment", str(ypath), "-p", str(tmp_path / "run2")])
    assert not os.path.exists(str(tmp_path / "run2" / "segment"))
