"""GPU tests of the edge-aware refinement of the segmentation export: ups_segment_guide and ups_segment_render_guided
(csrc/segexport.hip, through the C ABI) against the NumPy restatement of segrefine_ref.py, their memory contract and refusals,
``ops.segment_render(refine=...)`` and ``upsparts-run --segment`` with ``segment_refine: bilateral``.  Everything compares with == on
every byte: the guide is integer arithmetic and the guided kernel decides in fp64, operation for operation as the restatement."""
import copy
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

import segexport_ref as R0
import segrefine_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements in front of and behind every output that must keep the sentinel
BSENT = 0xA5                     # also what the alignment gaps between packed images must still hold
ISENT = -0x5A5A5A5B
VGG_W = (8, 8, 16, 16, 16)
E_ARG, E_UNSUPPORTED = -1, -2
ALL = ("labels", "overlay", "confidence", "counts")
TABLES = {"ones": np.ones(R.RANGE), "sigma16": R.range_table(16.0), "sigma1": R.range_table(1.0)}      # sigma1: most entries the floor


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


class _Guarded(object):
    """`n` elements inside a sentinel-filled buffer with GUARD elements on each side (the pattern of test_gpu_segexport.py)."""

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
    """The mixed launch of test_gpu_segexport.py, restated: model-size images, an image of several chunks whose pixel count is no
    multiple of 4, 1 x 1, 1 x 37, 7 x 1, shrunk images, and alignment gaps behind most of them."""
    return [(S, S), (2 * S, 2 * S), (3 * S + 1, 2 * S - 3), (1, 1), (1, 37), (S // 2, S // 2), (5, 4 * S),
            (45, 47), (3, 3), (2, 5), (7, 1), (S, S)]


def _sources(rng, sizes, kind="noise"):
    if kind == "noise":
        return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    srcs = []                    # two-tone: a vertical edge at a column of its own in every image
    for h, w in sizes:
        s = np.empty((h, w, 3), np.uint8)
        e = rng.randint(0, w + 1)
        s[:, :e] = (40, 60, 80)
        s[:, e:] = (200, 180, 160)
        srcs.append(s)
    return srcs


def _inputs(seed, S, P, sizes, kind="random", src_kind="noise"):
    rng = np.random.RandomState(seed)
    soft = R.soft_maps(rng, len(sizes), S, P, kind)
    colors = rng.randint(0, 256, size=(P, 3)).astype(np.uint8)
    return soft, colors, _sources(rng, sizes, src_kind)


def _guide(dev, srcs, sizes, S, table=None, n=None, with_src=True, with_out=True):
    """One ups_segment_guide call on a guarded output -> (rc, _Guarded, the packed sources on the device)."""
    L, ops = _mods()
    tab, tot = ops.segment_table(sizes)
    packed = ops.segment_pack_sources(srcs, tab, tot).to(dev)
    if table is not None:
        tab = np.ascontiguousarray(table, dtype=np.int32)
    td = torch.from_numpy(tab).to(dev)
    g = _Guarded(dev, len(sizes) * S * S * 3)
    rc = L.load().ups_segment_guide(L.ptr(packed) if with_src else None, len(sizes) if n is None else n, S,
                                    tab.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(td), tot, g.ptr() if with_out else None, L.stream())
    torch.cuda.synchronize(dev)
    return rc, g, packed


def _launch(dev, soft, sizes, colors, srcs, wr, radius, alpha=0.5, which=ALL, counts_init=0, table=None, P=None, drop=()):
    """The guide launch and one ups_segment_render_guided call on guarded outputs -> (rc, {name: _Guarded}).  `table` / P override
    what the inputs give and `drop` names required pointers passed as NULL (the refusals)."""
    L, ops = _mods()
    lib = L.load()
    S = soft.shape[1]
    rc, guide, packed = _guide(dev, srcs, sizes, S)
    assert rc == 0 and guide.intact(), lib.ups_last_error().decode()
    tab, tot = ops.segment_table(sizes)
    if table is not None:
        tab = np.ascontiguousarray(table, dtype=np.int32)
    ts = torch.from_numpy(soft).to(dev)
    td = torch.from_numpy(tab).to(dev)
    tc = None if colors is None else torch.from_numpy(colors).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(wr, dtype=np.float64)).to(dev)
    out = {"labels": _Guarded(dev, tot), "overlay": _Guarded(dev, 3 * tot), "confidence": _Guarded(dev, tot),
           "counts": _Guarded(dev, soft.shape[0] * soft.shape[3], torch.int32, counts_init)}
    p = {k: (out[k].ptr() if k in which else None) for k in ALL}
    rc = lib.ups_segment_render_guided(L.ptr(ts), soft.shape[0], S, soft.shape[3] if P is None else P,
                                       tab.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(td), tot,
                                       None if "src" in drop else L.ptr(packed), None if "guide" in drop else guide.ptr(),
                                       None if "range_w" in drop else L.ptr(tw), radius, L.ptr(tc), float(alpha), p["labels"],
                                       p["overlay"], p["confidence"], p["counts"], L.stream())
    torch.cuda.synchronize(dev)
    out["guide"] = guide
    return rc, out


def _check(out, want, which, counts_init=0):
    """Every wanted plane equals the restatement's packed plane byte for byte, the alignment gaps (which the restatement fills with
    the sentinel) included; every other plane is untouched; the guard bands are intact; the guide is the restatement's."""
    assert out["guide"].intact(), "wrote outside the guide"
    assert (out["guide"].view.cpu().numpy() == want["guide"].reshape(-1)).all(), "the guide differs"
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


# ---------------------------------------------------------------------------------------------- the guide kernel
@pytest.mark.parametrize("S", [4, 16])
def test_guide_kernel_equals_the_restatement(S, dev):
    sizes = _sizes(S)
    for kind in ("noise", "two-tone"):
        srcs = _sources(np.random.RandomState(S), sizes, kind)
        rc, g, _ = _guide(dev, srcs, sizes, S)
        assert rc == 0 and g.intact()
        got = g.view.cpu().numpy().reshape(len(sizes), S, S, 3)
        for i, s in enumerate(srcs):
            assert (got[i] == R.guide(s, S)).all(), (kind, i, sizes[i])
    assert (got[0] == srcs[0]).all() and (got[3] == srcs[3][0, 0]).all()       # S x S: the source itself; 1 x 1: its one pixel


def test_guide_kernel_on_more_taps_than_one_tile(dev):
    """S = 300 > the 256 taps a block sums at a time, enlarged, shrunk and mixed images."""
    S, sizes = 300, [(7, 650), (3, 299), (301, 5), (2, 1201)]
    srcs = _sources(np.random.RandomState(9), sizes)
    rc, g, _ = _guide(dev, srcs, sizes, S)
    assert rc == 0 and g.intact()
    got = g.view.cpu().numpy().reshape(len(sizes), S, S, 3)
    for i, s in enumerate(srcs):
        assert (got[i] == R.guide(s, S)).all(), sizes[i]


# ---------------------------------------------------------------------------------------------- the guided kernel
@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("P", [1, 2, 10, 33])
@pytest.mark.parametrize("S", [4, 16])
def test_guided_kernel_equals_the_restatement(S, P, radius, dev):
    sizes = _sizes(S)
    assert 45 * 47 > 2 * R0.CHUNK and (45 * 47) % 4 == 3
    if S == 4 and radius == 3:
        assert 2 * radius + 2 > S, "a window larger than the map"
    soft, colors, srcs = _inputs(100 * S + 10 * P + radius, S, P, sizes)
    for name in ("ones", "sigma16", "sigma1"):
        want = R.render_packed_guided(soft, sizes, srcs, TABLES[name], radius, colors, 0.5, fill=BSENT)
        assert (np.diff(want["table"][:, 0]) > (want["table"][:-1, 1] * want["table"][:-1, 2])).any(), "no alignment gap in this launch"
        rc, out = _launch(dev, soft, sizes, colors, srcs, TABLES[name], radius)
        assert rc == 0, (name, _mods()[0].load().ups_last_error().decode())
        _check(out, want, ALL)
        if P > 1:
            assert (want["counts"] > 0).sum() > len(sizes), "the maps are not varied enough to test anything"


@pytest.mark.parametrize("src_kind", ["noise", "two-tone"])
@pytest.mark.parametrize("kind", ["random", "onehot", "ties"])
def test_map_kinds_and_two_tone_sources(kind, src_kind, dev):
    S, P = 16, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(7, S, P, sizes, kind, src_kind)
    for name, radius in (("sigma16", 1), ("sigma1", 3), ("ones", 0)):
        want = R.render_packed_guided(soft, sizes, srcs, TABLES[name], radius, colors, 0.5, fill=BSENT)
        rc, out = _launch(dev, soft, sizes, colors, srcs, TABLES[name], radius)
        assert rc == 0
        _check(out, want, ALL)


@pytest.mark.parametrize("which", [("labels",), ("overlay",), ("confidence",), ("counts",), ALL], ids=["labels", "overlay", "confidence",
                                                                                                       "counts", "all"])
def test_each_output_alone_and_counts_are_added_to(which, dev):
    S, P = 4, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(11, S, P, sizes)
    want = R.render_packed_guided(soft, sizes, srcs, TABLES["sigma16"], 1, colors, 0.25, fill=BSENT)
    rc, out = _launch(dev, soft, sizes, colors, srcs, TABLES["sigma16"], 1, 0.25, which, counts_init=7)
    assert rc == 0
    _check(out, want, which, counts_init=7)
    assert want["counts"].sum(axis=1).tolist() == [h * w for h, w in sizes]


def test_refusals_launch_nothing(dev):
    L, ops = _mods()
    S, P = 4, 3
    sizes = [(4, 4), (5, 7), (2, 2)]
    soft, colors, srcs = _inputs(19, S, P, sizes)
    tab, tot = ops.segment_table(sizes)

    def refused(code, radius=1, **kw):
        rc, out = _launch(dev, soft, sizes, colors, srcs, TABLES["sigma16"], radius, **kw)
        assert rc == code, (rc, code, kw, L.load().ups_last_error().decode())
        for k in ALL:
            got = out[k].view.cpu().numpy()
            assert (got == (0 if k == "counts" else BSENT)).all() and out[k].intact(), "a refused call wrote " + k

    def edited(row, col, value):
        t = tab.copy()
        t[row, col] = value
        return t
    refused(E_ARG, drop=("src",))
    refused(E_ARG, drop=("guide",))
    refused(E_ARG, drop=("range_w",))
    refused(E_ARG, radius=-1)
    refused(E_ARG, radius=4)
    refused(E_ARG, table=edited(2, 3, 5))               # a first_block that is not the prefix sum
    refused(E_ARG, table=edited(1, 0, tab[1, 0] + 4))   # a misaligned offset
    refused(E_UNSUPPORTED, P=256)
    refused(E_ARG, P=0)
    refused(E_ARG, which=())                            # all four outputs null
    # the guide launch makes the same table checks
    for kw in ({"table": edited(2, 3, 5)}, {"table": edited(1, 2, 0)}, {"n": 0}, {"with_src": False}, {"with_out": False}):
        rc, g, _ = _guide(dev, srcs, sizes, S, **kw)
        assert rc == E_ARG and g.intact() and (g.view.cpu().numpy() == BSENT).all(), kw


# ---------------------------------------------------------------------------------------------- ops
def test_ops_segment_render_with_and_without_refine(dev):
    L, ops = _mods()
    S, P = 16, 10
    sizes = _sizes(S)
    soft, colors, srcs = _inputs(23, S, P, sizes)
    ts = torch.from_numpy(soft).to(dev)
    want = R.render_packed_guided(soft, sizes, srcs, R.range_table(12.5), 2, colors, 0.25, fill=0)
    res = ops.segment_render(ts, sizes, src=srcs, colors=colors, alpha=0.25, want=ALL, refine={"radius": 2, "sigma": 12.5})
    assert (res["table"] == want["table"]).all() and res["total"] == want["total"]
    for k in ALL + ("guide",):
        assert (res[k].cpu().numpy().reshape(want[k].shape) == want[k]).all(), k
    assert tuple(res["views"]["labels"][2].shape) == sizes[2]
    # refine=None is today's call: the bilinear restatement's bytes, and no guide
    plain = R0.render_packed(soft, sizes, colors, srcs, 0.25, fill=0)
    res = ops.segment_render(ts, sizes, src=srcs, colors=colors, alpha=0.25, want=ALL, refine=None)
    assert "guide" not in res
    for k in ALL:
        assert (res[k].cpu().numpy().reshape(plain[k].shape) == plain[k]).all(), k
    assert (plain["labels"] != want["labels"]).any(), "the refinement changed nothing: the case tests nothing"
    # the guide alone
    tab, tot = ops.segment_table(sizes)
    g = ops.segment_guide(ops.segment_pack_sources(srcs, tab, tot).to(dev), tab, tot, S)
    assert g.dtype == torch.uint8 and tuple(g.shape) == (len(sizes), S, S, 3) and (g.cpu().numpy() == want["guide"]).all()
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes, refine={"radius": 1, "sigma": 16.0})                       # no src
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes, src=srcs, refine={"radius": 4, "sigma": 16.0})
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes, src=srcs, refine={"radius": 1, "sigma": 0.0})
    with pytest.raises(L.UpsError):
        ops.segment_render(ts, sizes, src=srcs, refine={"radius": 1})


def test_an_image_edge_moves_the_label_boundary_on_the_device(dev):
    """The two-tone property of test_host_segrefine.py, for R = 1: the label boundary of a half / half map follows the image edge."""
    _, ops = _mods()
    S = 8
    soft = np.zeros((2, S, S, 2), np.float32)
    soft[:, :, :S // 2, 0] = 1.0
    soft[:, :, S // 2:, 1] = 1.0
    srcs = []
    for edge in (18, 13):
        s = np.empty((32, 32, 3), np.uint8)
        s[:, :edge] = (40, 60, 80)
        s[:, edge:] = (200, 180, 160)
        srcs.append(s)
    ts = torch.from_numpy(soft).to(dev)
    res = ops.segment_render(ts, [(32, 32)] * 2, src=srcs, want=("labels",), refine={"radius": 1, "sigma": 16.0})
    plain = ops.segment_render(ts, [(32, 32)] * 2, want=("labels",))
    for i, edge in enumerate((18, 13)):
        for r, at in ((res, edge), (plain, 16)):
            lab = r["views"]["labels"][i].cpu().numpy()
            assert (lab == lab[:1]).all() and (np.diff(lab[0].astype(np.int64)) >= 0).all()
            assert lab[0, 0] == 0 and lab[0, -1] == 1 and int(np.argmax(lab[0])) == at


# ---------------------------------------------------------------------------------------------- the runner
def test_runner_segment_refine_end_to_end(dev, tmp_path, caplog):
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
    files = [("a/one.png", (37, 46)), ("two.png", (S, S)), ("b/three.png", (21, 13)), ("four.png", (60, 90)), ("b/c/five.png", (9, 48))]
    for rel, (h, w) in files:
        os.makedirs(os.path.dirname(str(data_root / rel)), exist_ok=True)
        small = rng.randint(0, 256, size=(4, 5, 3)).astype(np.uint8)
        Image.fromarray(small).resize((w, h), Image.NEAREST).save(str(data_root / rel))          # blocks with sharp edges
    csv_path = tmp_path / "list.csv"
    csv_path.write_text("\n".join(rel for rel, _ in files) + "\n")
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(data_root), "segment_csv": str(csv_path),
                "segment_max_side": 48, "segment_outputs": ["labels", "confidence"]})
    plain_yaml, fine_yaml = tmp_path / "plain.yaml", tmp_path / "fine.yaml"
    plain_yaml.write_text(yaml.safe_dump(cfg))
    fine_yaml.write_text(yaml.safe_dump(dict(cfg, segment_refine="bilateral", segment_refine_radius=2, segment_refine_sigma=20.0)))
    with caplog.at_level(logging.INFO, logger="upsparts"):
        res = runner.main(["--segment", str(fine_yaml), "-p", str(tmp_path / "fine")])
    assert caplog.text.count("segment_refine = bilateral") == 1, "the mode is logged once"
    again = runner.main(["--segment", str(fine_yaml), "-p", str(tmp_path / "again")])
    plain = runner.main(["--segment", str(plain_yaml), "-p", str(tmp_path / "plain")])
    imgs = [Image.open(str(data_root / rel)).convert("RGB") for rel, _ in files]
    views = np.stack([np.asarray(im.resize((S, S), Image.BILINEAR), dtype=np.float32) / 127.5 - 1.0 for im in imgs])
    _, soft = res["model"].segment_soft(torch.from_numpy(views))
    soft = soft.cpu().numpy()
    palette = IL.mask_color_bytes(IL.mask_colors01(P))
    wr = R.range_table(20.0)

    def index_of(run):
        with open(os.path.join(run["dir"], "index.csv"), newline="") as f:
            return list(csv.reader(f))
    fine_index, plain_index = index_of(res), index_of(plain)
    assert fine_index[0] == ["file", "h", "w"] + ["area_{}".format(p) for p in range(P)] and len(fine_index) == 1 + len(files)
    moved = 0
    for i, (rel, (h, w)) in enumerate(files):
        oh, ow = (32, 48) if rel == "four.png" else (h, w)         # segment_max_side applies first
        src = np.asarray(imgs[i] if (oh, ow) == (h, w) else imgs[i].resize((ow, oh), Image.BILINEAR), dtype=np.uint8)
        fine, base = R.render_guided(soft[i], src, wr, 2), R0.render(soft[i], oh, ow, palette, src, 0.5)
        lab = Image.open(os.path.join(res["dir"], "labels", rel + ".png"))
        assert lab.mode == "P" and lab.size == (ow, oh)
        assert (np.asarray(lab) == fine["labels"]).all(), rel
        assert (np.asarray(Image.open(os.path.join(res["dir"], "confidence", rel + ".png"))) == fine["confidence"]).all(), rel
        assert fine_index[1 + i][:3] == [rel, str(oh), str(ow)]
        assert [float(x) for x in fine_index[1 + i][3:]] == [c / float(oh * ow) for c in fine["counts"]]
        # the key unset: the bilinear route's files, as before
        assert (np.asarray(Image.open(os.path.join(plain["dir"], "labels", rel + ".png"))) == base["labels"]).all(), rel
        assert (np.asarray(Image.open(os.path.join(plain["dir"], "confidence", rel + ".png"))) == base["confidence"]).all(), rel
        assert [float(x) for x in plain_index[1 + i][3:]] == [c / float(oh * ow) for c in base["counts"]]
        moved += int((fine["labels"] != base["labels"]).sum())
        # two runs give equal bytes
        for kind in ("labels", "confidence"):
            with open(os.path.join(res["dir"], kind, rel + ".png"), "rb") as f0, open(os.path.join(again["dir"], kind, rel + ".png"), "rb") as f1:
                assert f0.read() == f1.read(), (kind, rel)
    assert not os.path.exists(os.path.join(res["dir"], "overlay")), "an output that was not asked for was written"
    with open(os.path.join(res["dir"], "index.csv"), "rb") as f0, open(os.path.join(again["dir"], "index.csv"), "rb") as f1:
        assert f0.read() == f1.read()
    assert moved > 0, "the refinement changed no label: the case tests nothing"
