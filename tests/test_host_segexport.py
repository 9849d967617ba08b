"""CPU tests of the segmentation export: properties of the NumPy float64 restatement (segexport_ref.py) that the kernel is held to,
the packing table of ops.segment_table, the palette PNG and index.csv writers, and the runner's argument handling.  Nothing here
launches a kernel."""
import csv
import os

import numpy as np
import pytest

import segexport_ref as R


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import imglog, lib, ops, runner
    return lib, ops, imglog, runner


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("S,P", [(4, 1), (4, 2), (16, 10), (8, 33)])
def test_model_size_labels_are_the_argmax_of_the_map(S, P):
    soft = R.soft_maps(np.random.RandomState(S + P), 1, S, P)[0]
    y0, y1, f = R.source_coords(S, S)
    assert (y0 == np.arange(S)).all() and (f == 0).all()                        # the weights are exactly 1 and 0
    r = R.render(soft, S, S)
    assert (r["labels"] == np.argmax(soft, axis=2)).all()
    assert (R.resample(soft, S, S) == soft.astype(np.float64)).all()
    assert (r["confidence"] == np.clip(np.floor(soft.max(axis=2).astype(np.float64) * 255.0 + 0.5), 0, 255)).all()


@pytest.mark.parametrize("hw", [(1, 1), (3, 50), (37, 5), (8, 8)])
def test_constant_map_gives_a_constant_label(hw):
    S, P = 8, 5
    soft = np.zeros((S, S, P), np.float32)
    soft[..., 3] = 0.75
    soft[..., 1] = 0.25
    r = R.render(soft, *hw)
    assert (r["labels"] == 3).all() and (r["confidence"] == 191).all()          # floor(0.75 * 255 + 0.5)
    assert r["counts"].tolist() == [0, 0, 0, hw[0] * hw[1], 0]


def test_equal_channels_resolve_to_the_lower_index():
    S, P = 4, 4
    soft = np.full((S, S, P), 0.125, np.float32)
    soft[..., 1] = soft[..., 3] = 0.375
    for hw in [(4, 4), (9, 7), (2, 2)]:
        assert (R.render(soft, *hw)["labels"] == 1).all()
    ties = R.soft_maps(np.random.RandomState(0), 2, 4, 6, "ties")
    v = R.resample(ties[0], 4, 4)
    assert ((v == v.max(axis=2, keepdims=True)).sum(axis=2) >= 2).all()
    lab = R.render(ties[0], 4, 4)["labels"]
    assert (lab == np.argmax(ties[0], axis=2)).all()


@pytest.mark.parametrize("hw", [(1, 1), (1, 37), (13, 5), (33, 31), (2, 2)])
def test_counts_sum_to_the_pixels(hw):
    soft = R.soft_maps(np.random.RandomState(3), 1, 4, 10)[0]
    r = R.render(soft, *hw)
    assert r["counts"].sum() == hw[0] * hw[1] and (r["counts"] == np.bincount(r["labels"].reshape(-1), minlength=10)).all()
    assert r["labels"].shape == hw and r["labels"].max() < 10


def test_alpha_zero_is_the_source_and_alpha_one_the_colour():
    rng = np.random.RandomState(5)
    S, P, h, w = 4, 3, 9, 6
    soft = R.soft_maps(rng, 1, S, P)[0]
    colors = rng.randint(0, 256, size=(P, 3)).astype(np.uint8)
    src = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    src[0, 0], src[0, 1] = 0, 255
    lab = R.render(soft, h, w)["labels"]
    assert (R.render(soft, h, w, colors, src, 0.0)["overlay"] == src).all()
    assert (R.render(soft, h, w, colors, src, 1.0)["overlay"] == colors[lab]).all()
    assert (R.render(soft, h, w, colors, None, 0.3)["overlay"] == colors[lab]).all()
    half = R.render(soft, h, w, colors, src, 0.5)["overlay"].astype(np.int64)
    assert (half == (colors[lab].astype(np.int64) + src + 1) // 2).all()          # 0.5 a + 0.5 b + 0.5, floored: exact in float64


def test_downsampling_uses_the_same_formula_without_antialiasing():
    S, P = 8, 2
    soft = np.zeros((S, S, P), np.float32)
    soft[::2, :, 0] = 1.0
    soft[1::2, :, 1] = 1.0
    # h = S / 2: sy = 2 y + 0.5 -> rows 2y and 2y + 1 with weight one half each: a tie, the lower index
    assert (R.render(soft, S // 2, S // 2)["labels"] == 0).all()
    assert (R.render(soft, S // 2, S // 2)["confidence"] == 128).all()


# ---------------------------------------------------------------------------------------------- the packing table
SIZES = [(4, 4), (8, 8), (13, 5), (1, 1), (1, 37), (2, 2), (5, 16), (40, 30), (16, 16)]


def test_packing_table():
    lib, ops, _, _ = _mods()
    tab, total = ops.segment_table(SIZES)
    ref_tab, ref_total = R.table(SIZES)
    assert tab.dtype == np.int32 and tab.shape == (len(SIZES), 4) and (tab == ref_tab).all() and total == ref_total
    assert R.CHUNK == ops.SEGMENT_CHUNK == lib.load().ups_segment_chunk() and lib.load().ups_segment_table_words() == 4
    assert R.ALIGN == ops.SEGMENT_ALIGN == 16
    off, h, w, blk = tab.T.astype(np.int64)
    assert (off % 16 == 0).all() and off[0] == 0 and total % 16 == 0
    assert (off[1:] >= off[:-1] + (h * w)[:-1]).all(), "two images overlap"
    assert (off[1:] - (off[:-1] + (h * w)[:-1]) < 16).all(), "a gap wider than the alignment needs"
    assert off[-1] + h[-1] * w[-1] <= total < off[-1] + h[-1] * w[-1] + 16
    assert [tuple(r) for r in np.stack([h, w], 1)] == SIZES
    assert blk.tolist() == np.concatenate([[0], np.cumsum(-(-(h * w) // ops.SEGMENT_CHUNK))[:-1]]).tolist()
    assert blk[-2] == len(SIZES) - 2 and blk[-1] == blk[-2] + 2                # 40 x 30 = 1200 pixels: two chunks
    with pytest.raises(lib.UpsError):
        ops.segment_table([(4, 0)])
    with pytest.raises(lib.UpsError):
        ops.segment_table([])
    for name in ("ups_segment_render", "ups_segment_chunk", "ups_segment_table_words"):
        assert name in lib.EXPORTS
    assert lib.ABI_VERSION == 6


def test_packed_sources_and_views():
    import torch
    _, ops, _, _ = _mods()
    rng = np.random.RandomState(1)
    srcs = [rng.randint(1, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SIZES]
    tab, total = ops.segment_table(SIZES)
    packed = ops.segment_pack_sources(srcs, tab, total)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (total, 3)
    views = ops.segment_views(packed, tab)
    covered = np.zeros(total, bool)
    for v, s, (o, h, w, _) in zip(views, srcs, tab.tolist()):
        assert (v.numpy() == s).all()
        covered[o:o + h * w] = True
    assert (packed.numpy()[~covered] == 0).all()


# ---------------------------------------------------------------------------------------------- writers
def test_palette_png_round_trip(tmp_path):
    from PIL import Image
    _, _, IL, runner = _mods()
    P = 10
    palette = IL.mask_color_bytes(IL.mask_colors01(P))
    assert palette.shape == (P, 3) and palette.dtype == np.uint8
    lab = np.random.RandomState(2).randint(0, P, size=(13, 7)).astype(np.uint8)
    w = IL.ImageWriter(str(tmp_path), path_fn=runner.segment_png_path)
    w.submit(40, {("labels", "sub/dir/bird_01.jpg"): IL.Paletted(lab, palette), ("confidence", "sub/dir/bird_01.jpg"): lab * 20})
    w.close()
    path = runner.segment_png_path(str(tmp_path), ("labels", "sub/dir/bird_01.jpg"), 40)
    assert path == os.path.join(str(tmp_path), "segment", "40", "labels", "sub/dir/bird_01.jpg.png") and w.written[0] == path
    img = Image.open(path)
    assert img.mode == "P" and img.size == (7, 13)
    assert (np.asarray(img) == lab).all(), "the bytes of a palette PNG are the part ids"
    assert (np.asarray(img.getpalette()[:3 * P], dtype=np.uint8).reshape(P, 3) == palette).all()
    assert (np.asarray(img.convert("RGB")) == palette[lab]).all()
    conf = Image.open(runner.segment_png_path(str(tmp_path), ("confidence", "sub/dir/bird_01.jpg"), 40))
    assert conf.mode == "L" and (np.asarray(conf) == lab * 20).all()


def test_index_csv_round_trip(tmp_path):
    _, _, _, runner = _mods()
    rows = [("a/x.png", 3, 5, [15, 0, 0]), ("b.jpg", 7, 3, [1, 13, 7])]
    path = str(tmp_path / "index.csv")
    runner.write_segment_index(path, rows, 3)
    with open(path, newline="") as f:
        got = list(csv.reader(f))
    assert got[0] == ["file", "h", "w", "area_0", "area_1", "area_2"]
    for line, (rel, h, w, c) in zip(got[1:], rows):
        assert line[:3] == [rel, str(h), str(w)]
        assert [float(v) for v in line[3:]] == [k / float(h * w) for k in c]       # repr round-trips a float64


# ---------------------------------------------------------------------------------------------- runner arguments
def test_runner_requires_exactly_one_route(tmp_path, capsys):
    _, _, _, runner = _mods()
    y = str(tmp_path / "x.yaml")
    for argv in ([], ["--segment", y, "-t", y], ["--segment", y, "-e", y], ["--segment", y, "--transfer", y]):
        with pytest.raises(SystemExit):
            runner.main(argv)
        assert "exactly one of -t / -e / --transfer / --segment" in capsys.readouterr().err


def test_segment_options_and_sizes(tmp_path):
    import yaml
    _, _, _, runner = _mods()
    base = {"segment_csv": "list.csv"}
    opt = runner.segment_options(base)
    assert opt == {"csv": "list.csv", "size": "source", "max_side": 1024, "outputs": ("labels", "overlay"), "alpha": 0.5}
    for bad in ({}, {"segment_size": "big"}, {"segment_size": [3]}, {"segment_size": [0, 4]}, {"segment_max_side": 0},
                {"segment_max_side": "1k"}, {"segment_outputs": []}, {"segment_outputs": ["labels", "masks"]},
                {"segment_outputs": ["labels", "labels"]}, {"segment_alpha": 1.5}, {"segment_alpha": "half"}):
        with pytest.raises(ValueError):
            runner.segment_options(dict(base, **bad) if bad else {})
    assert runner.segment_options(dict(base, segment_size=[30, 40], segment_outputs="confidence", segment_alpha=1))["size"] == (30, 40)
    assert runner.segment_output_size(375, 500, opt, 128) == (375, 500, False)
    assert runner.segment_output_size(375, 500, dict(opt, size="model"), 128) == (128, 128, False)
    assert runner.segment_output_size(375, 500, dict(opt, size=(30, 40)), 128) == (30, 40, False)
    assert runner.segment_output_size(1500, 2048, opt, 128) == (750, 1024, True)
    assert runner.segment_output_size(40, 25, dict(opt, max_side=16), 128) == (16, 10, True)
    assert runner.segment_output_size(1000, 1, dict(opt, max_side=10), 128) == (10, 1, True)
    # a yaml without segment_csv, and one without data_root, fail before any device is touched
    ypath = tmp_path / "seg.yaml"
    ypath.write_text(yaml.safe_dump({"batch_size": 2}))
    with pytest.raises(ValueError, match="segment_csv"):
        runner.main(["--segment", str(ypath)])
    ypath.write_text(yaml.safe_dump({"batch_size": 2, "segment_csv": "x.csv"}))
    with pytest.raises(ValueError, match="data_root"):
        runner.main(["--segment", str(ypath)])
