"""GPU tests of the run-length annotations: ups_segment_rle_count / ups_segment_rle_write (csrc/segrle.hip) through ops.segment_rle
and through the C ABI against the two restatements of segrle_ref.py, the memory contract and the refusals,
``TrainModel.export_segments(rle=True)`` and ``upsparts-run --segment`` with `segment_annotations: coco`.  Everything is an integer:
every comparison is ==."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import segrle_ref as R

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)
E_ARG, E_UNSUPPORTED = -1, -2
CASES = R.host_cases()
_EXPECTED = {}


@pytest.fixture(autouse=True)
def _keep_rng_state(dev):
    """Building a model seeds torch's generators; later test files draw unseeded device tensors.  They see the state they saw before
    this file existed."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu, dev)


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _expected(name, maps, P):
    """The reference of a case, computed once (NumPy restatement) and never changed."""
    if name not in _EXPECTED:
        _EXPECTED[name] = R.encode_all(maps, P)
        for v in _EXPECTED[name].values():
            v.setflags(write=False)
    return _EXPECTED[name]


def _encode(ops, dev, maps, P, fill=0):
    plane, table, total = R.pack(maps, fill)
    t = torch.from_numpy(plane).to(dev)
    res = ops.segment_rle(t, P, table=(table, torch.from_numpy(table).to(dev), total))
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, exp):
    for k in ("offsets", "area", "bbox", "counts"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (k, got[k].dtype, got[k].shape, exp[k].shape)
        assert np.array_equal(got[k], exp[k]), k


def test_chunk_is_the_render_chunk(dev):
    L, ops = _mods()
    assert L.load().ups_segment_rle_chunk() == R.CHUNK == ops.SEGMENT_RLE_CHUNK
    assert L.load().ups_segment_rle_scratch_bytes(1, 16, 1) >= 8 + 8 and L.load().ups_segment_rle_scratch_bytes(0, 16, 1) == 0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_single_images(dev, case):
    """Every size and pattern of the list in segrle_ref.host_cases: the sizes around the chunk, maps that are constant, begin with a
    one, alternate every pixel, change exactly at a chunk's first and last position, carry invalid bytes, and P = 1, 10, 255."""
    _, ops = _mods()
    name, m, P = case
    exp = _expected(name, [m], P)
    got = _encode(ops, dev, [m], P)
    _same(got, exp)
    again = _encode(ops, dev, [m], P)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_longest_lists(dev):
    """A one-pixel checkerboard of ODD height alternates at every position of the column-major order (with an even height a column
    begins with the label the previous one ended with): h w + 1 entries for the part of pixel 0 and h w for the other."""
    _, ops = _mods()
    for h, w in ((37, 29), (71, 49), (1, R.CHUNK + 1)):
        got = _encode(ops, dev, [R.checkerboard(h, w)], 2)
        assert got["offsets"].tolist() == [0, h * w + 1, 2 * h * w + 1]
        assert got["counts"].tolist() == [0] + [1] * (2 * h * w)


def test_constant_map_lists(dev):
    _, ops = _mods()
    got = _encode(ops, dev, [np.full((70, 50), 1, dtype=np.uint8)], 3)
    assert got["counts"].tolist() == [3500, 0, 3500, 3500] and got["offsets"].tolist() == [0, 1, 3, 4]
    assert got["area"].tolist() == [[0, 3500, 0]] and got["bbox"].tolist() == [[[0, 0, 0, 0], [0, 0, 50, 70], [0, 0, 0, 0]]]


def test_pass_of_nine_images_with_filled_gaps(dev):
    """Nine images of different sizes in one launch, the alignment gaps filled with a valid label: a kernel that reads a gap, or that
    carries m[k-1] from one image into the next, gives other counts.  Two launches give the same bytes."""
    _, ops = _mods()
    maps, P = R.pass_of_nine()
    exp = _expected("nine", maps, P)
    for fill in (0, 3, 1):
        got = _encode(ops, dev, maps, P, fill=fill)
        _same(got, exp)
    # every image ends with the label its successor begins with, and the gap carries it too
    ones = [np.full(m.shape, 2, dtype=np.uint8) for m in maps]
    got = _encode(ops, dev, ones, P, fill=2)
    _same(got, R.encode_all(ones, P))
    lists = ops.rle_lists(got["offsets"], got["counts"], len(maps), P)
    assert all(lists[i][2] == [0, m.size] and lists[i][0] == [m.size] for i, m in enumerate(maps))


def test_many_images_scan_over_several_blocks(dev):
    """n P = 300 x 3 lists: the scan of the list lengths runs over four blocks of 256."""
    _, ops = _mods()
    maps = [R.noise_map(3 + i % 5, 2 + i % 7, 3, 500 + i) for i in range(300)]
    _same(_encode(ops, dev, maps, 3, fill=1), R.encode_all(maps, 3))


def test_regular_batch_through_ops(dev):
    L, ops = _mods()
    maps = [R.blocks_map(37, 29, 5, 40 + i) for i in range(3)]              # 37 x 29 is no multiple of 16: packed by the wrapper
    t = torch.from_numpy(np.stack(maps)).to(dev)
    res = {k: v.cpu().numpy() for k, v in ops.segment_rle(t, 5).items()}
    _same(res, R.encode_all(maps, 5))
    for bad in (lambda: ops.segment_rle(t.long(), 5), lambda: ops.segment_rle(t, 0), lambda: ops.segment_rle(t, 256),
                lambda: ops.segment_rle(t.cpu(), 5), lambda: ops.segment_rle(t.view(-1), 5), lambda: ops.segment_rle(t, True)):
        with pytest.raises(L.UpsError):
            bad()


# ---------------------------------------------------------------------------------------------- the C entries
def _raw(dev, maps, P):
    L, ops = _mods()
    plane, table, total = R.pack(maps)
    n = len(maps)
    return {"L": L, "lib": L.load(), "n": n, "P": P, "total": total, "table": table,
            "th": table.ctypes.data_as(C.POINTER(C.c_int32)), "td": torch.from_numpy(table).to(dev),
            "lab": torch.from_numpy(plane).to(dev), "offsets": torch.full((n * P + 1,), -7, dtype=torch.int64, device=dev),
            "area": torch.full((n, P), -7, dtype=torch.int32, device=dev), "bbox": torch.full((n, P, 4), -7, dtype=torch.int32, device=dev),
            "scratch": torch.zeros(L.load().ups_segment_rle_scratch_bytes(n, total, P) // 8 + 1, dtype=torch.int64, device=dev)}


def test_capacity_one_too_small_writes_nothing(dev):
    maps = [R.noise_map(37, 29, 3, 21), R.blocks_map(70, 50, 3, 22)]
    r = _raw(dev, maps, 3)
    L, lib, s = r["L"], r["lib"], r["L"].stream()
    exp = R.encode_all(maps, 3)
    assert lib.ups_segment_rle_count(L.ptr(r["lab"]), r["n"], r["th"], L.ptr(r["td"]), r["total"], 3, L.ptr(r["offsets"]), L.ptr(r["area"]),
                                     L.ptr(r["bbox"]), L.ptr(r["scratch"]), s) == 0
    total = int(r["offsets"][-1].item())
    assert total == exp["counts"].size and np.array_equal(r["offsets"].cpu().numpy(), exp["offsets"])
    assert np.array_equal(r["area"].cpu().numpy(), exp["area"]) and np.array_equal(r["bbox"].cpu().numpy(), exp["bbox"])      # written
    counts = torch.full((total + 8,), -5, dtype=torch.int32, device=dev)

    def write(capacity, n_counts=total):
        return lib.ups_segment_rle_write(L.ptr(r["lab"]), r["n"], r["th"], L.ptr(r["td"]), r["total"], 3, L.ptr(r["offsets"]),
                                         L.ptr(r["scratch"]), L.ptr(counts), capacity, n_counts, s)

    assert write(total - 1) == E_ARG and write(0) == E_ARG and write(total, 0) == E_ARG
    torch.cuda.synchronize(dev)
    assert (counts == -5).all(), "a refused call wrote"
    assert write(total) == 0
    got = counts.cpu().numpy()
    assert np.array_equal(got[:total], exp["counts"]) and (got[total:] == -5).all(), "the guard band behind the lists"
    # the second launch of the pair gives the same bytes
    assert write(total + 8) == 0
    assert np.array_equal(counts.cpu().numpy(), got)


def test_refusals_launch_nothing(dev):
    maps = [R.noise_map(4, 4, 2, 1)]
    r = _raw(dev, maps, 2)
    L, lib, s = r["L"], r["lib"], r["L"].stream()
    counts = torch.full((64,), -5, dtype=torch.int32, device=dev)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)

    def count(P=2, n=1, th=r["th"], tot=r["total"], lab=p(r["lab"]), td=p(r["td"]), offsets=p(r["offsets"]), area=p(r["area"]),
              bbox=p(r["bbox"]), scratch=p(r["scratch"])):
        return lib.ups_segment_rle_count(lab, n, th, td, tot, P, offsets, area, bbox, scratch, s)

    def write(P=2, n=1, th=r["th"], tot=r["total"], lab=p(r["lab"]), td=p(r["td"]), offsets=p(r["offsets"]), scratch=p(r["scratch"]),
              cnt=p(counts), capacity=64, n_counts=64):
        return lib.ups_segment_rle_write(lab, n, th, td, tot, P, offsets, scratch, cnt, capacity, n_counts, s)

    big, _ = R.table_of([(1025, 1024)])
    bad_off = r["table"].copy()
    bad_off[0, 0] = 8                                                        # an offset that is no multiple of 16
    bad_blk = r["table"].copy()
    bad_blk[0, 3] = 1                                                        # first_block is not the prefix sum
    as_c = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    for fn in (count, write):
        assert fn(P=256) == E_UNSUPPORTED and fn(P=0) == E_ARG and fn(n=0) == E_ARG and fn(n=65536) == E_ARG
        assert fn(lab=None) == E_ARG and fn(td=None) == E_ARG and fn(th=None) == E_ARG and fn(offsets=None) == E_ARG
        assert fn(scratch=None) == E_ARG
        assert fn(th=as_c(big), tot=1025 * 1024) == E_ARG                    # h w > 2^20
        assert fn(th=as_c(bad_off)) == E_ARG and fn(th=as_c(bad_blk)) == E_ARG and fn(tot=15) == E_ARG
        assert fn(offsets=p(r["offsets"], 4)) == E_ARG and fn(scratch=p(r["scratch"], 4)) == E_ARG
    assert count(area=None) == E_ARG and count(bbox=None) == E_ARG
    assert count(area=p(r["area"], 2)) == E_ARG and count(bbox=p(r["bbox"], 1)) == E_ARG
    assert write(cnt=None) == E_ARG and write(cnt=p(counts, 2)) == E_ARG and write(capacity=63) == E_ARG
    torch.cuda.synchronize(dev)
    assert (r["offsets"] == -7).all() and (r["area"] == -7).all() and (r["bbox"] == -7).all() and (counts == -5).all()
    assert (r["scratch"] == 0).all(), "a refused call launched something"
    assert count() == 0


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("clean", (None, {"min_area": 40, "rounds": 2, "connectivity": 4}), ids=("plain", "clean"))
def test_export_segments_rle(dev, clean):
    """The decoded masks of export_segments(rle=True) tile the host copy of the FINAL labels plane -- after the clean-up when it is
    on -- and area / bbox are its; with outputs empty the encoding is the same and no plane is copied."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import ops
    from upsparts_amd.model import TrainModel
    from oracle import configs, ref_model
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(precision="bf16", vgg_widths=VGG_W)
    model = TrainModel(cfg, device=dev, seed=0)
    S, P = cfg["spatial_size"], cfg["n_parts"]
    views = ref_model.synthetic_views(cfg)
    gen = torch.Generator().manual_seed(3)
    v = torch.cat([views["view0"], views["view1"], torch.rand(1, S, S, 3, generator=gen) * 2 - 1], 0)[:5]   # a whole pass and a ragged one
    sizes = [(37, 50), (S, S), (5, 3), (2 * S + 1, S - 1), (1, 1)]
    extra = {} if clean is None else {"clean": clean}
    plain = model.export_segments(v, sizes, outputs=("labels",), **extra)
    res = model.export_segments(v, sizes, outputs=("labels",), rle=True, **extra)
    only = model.export_segments(v, sizes, outputs=(), rle=True, **extra)
    for r in (plain, res, only):
        r["ready"].synchronize()
    assert set(plain["host"]) == {"labels", "counts"} and set(only["host"]) == {"counts", "rle_offsets", "rle_counts", "area", "bbox"}
    assert only["views"] == {}
    assert torch.equal(plain["host"]["labels"], res["host"]["labels"]) and plain["relabelled"] == res["relabelled"] == only["relabelled"]
    for k in ("rle_offsets", "rle_counts", "area", "bbox", "counts"):
        assert torch.equal(res["host"][k], only["host"][k]), k
    assert res["host"]["rle_offsets"].dtype == torch.int64 and res["host"]["rle_counts"].dtype == torch.int32
    lists = ops.rle_lists(res["host"]["rle_offsets"], res["host"]["rle_counts"], len(sizes), P)
    assert torch.equal(res["host"]["area"], res["host"]["counts"])
    for i, (h, w) in enumerate(sizes):
        lab = res["views"]["labels"][i].numpy()
        seen = np.zeros((h, w), dtype=np.int32)
        for p in range(P):
            mask = R.decode(lists[i][p], h, w)
            assert np.array_equal(mask, lab == p), (i, p)
            assert lists[i][p] == R.encode_loop(lab, p)
            area, bbox = R.area_bbox(lab, p)
            assert int(res["host"]["area"][i, p]) == area and tuple(res["host"]["bbox"][i, p].tolist()) == bbox
            seen += mask
        assert (seen == 1).all(), "the masks tile the image"


# ---------------------------------------------------------------------------------------------- the runner
def _file_bytes(odir):
    out = {}
    for base, _, names in os.walk(odir):
        for n in names:
            with open(os.path.join(base, n), "rb") as f:
                out[os.path.relpath(os.path.join(base, n), odir)] = f.read()
    return out


def test_runner_segment_annotations_end_to_end(dev, tmp_path):
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
        small = rng.randint(0, 256, size=(4, 5, 3)).astype(np.uint8)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(str(data_root / rel))
    csv_path = tmp_path / "list.csv"
    csv_path.write_text("\n".join(rel for rel, _ in files) + "\n")
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(data_root), "segment_csv": str(csv_path),
                "segment_max_side": 48, "segment_outputs": ["labels"], "segment_alpha": 0.5})

    def run(name, **keys):
        ypath = tmp_path / (name + ".yaml")
        ypath.write_text(yaml.safe_dump(dict(cfg, **keys)))
        runner.main(["--segment", str(ypath), "-p", str(tmp_path / name)])
        return str(tmp_path / name / "segment" / "0")

    plain = _file_bytes(run("plain"))
    both = _file_bytes(run("both", segment_annotations="coco", segment_annotation_min_area=0))
    assert sorted(both) == sorted(list(plain) + ["annotations.json"])
    assert all(both[k] == plain[k] for k in plain), "the PNG files and index.csv of a run without the key"
    doc = json.loads(both["annotations.json"].decode())
    assert list(doc) == ["images", "categories", "annotations"]
    palette = IL.mask_color_bytes(IL.mask_colors01(P))
    assert doc["categories"] == [{"id": p + 1, "name": "part_{}".format(p), "color": [int(c) for c in palette[p]]} for p in range(P)]
    assert len(doc["annotations"]) == len(files) * P                         # min_area 0: every part of every image
    odir = str(tmp_path / "both" / "segment" / "0")
    for i, (rel, (h, w)) in enumerate(files):
        oh, ow = (32, 48) if rel == "four.png" else (h, w)                   # 60 x 90 is larger than segment_max_side = 48
        assert doc["images"][i] == {"id": i + 1, "file_name": rel, "height": oh, "width": ow}
        lab = np.asarray(Image.open(os.path.join(odir, "labels", rel + ".png")))
        for p in range(P):
            a = doc["annotations"][i * P + p]
            assert list(a) == ["id", "image_id", "category_id", "segmentation", "area", "bbox", "iscrowd"]
            assert (a["id"], a["image_id"], a["category_id"], a["iscrowd"]) == (i * P + p + 1, i + 1, p + 1, 1)
            assert a["segmentation"]["size"] == [oh, ow]
            assert np.array_equal(R.decode(a["segmentation"]["counts"], oh, ow), lab == p), (rel, p)
            assert a["segmentation"]["counts"] == R.encode_loop(lab, p)
            area, bbox = R.area_bbox(lab, p)
            assert a["area"] == area and a["bbox"] == list(bbox)
    # annotations alone: the same bytes, index.csv as before, and not one PNG or PNG directory
    alone = _file_bytes(run("alone", segment_annotations="coco", segment_annotation_min_area=0, segment_outputs=[]))
    assert sorted(alone) == ["annotations.json", "index.csv"]
    assert alone["annotations.json"] == both["annotations.json"] and alone["index.csv"] == plain["index.csv"]
    assert sorted(os.listdir(str(tmp_path / "alone" / "segment" / "0"))) == ["annotations.json", "index.csv"]
    # the default threshold drops the parts without a pixel; the path key moves the file
    elsewhere = tmp_path / "out" / "parts.json"
    moved = _file_bytes(run("moved", segment_annotations="coco", segment_outputs=[], segment_annotation_path=str(elsewhere)))
    assert sorted(moved) == ["index.csv"]
    kept = json.loads(elsewhere.read_text())["annotations"]
    want = [a for a in doc["annotations"] if a["area"] >= 1]
    assert [dict(a, id=0) for a in kept] == [dict(a, id=0) for a in want] and [a["id"] for a in kept] == list(range(1, len(want) + 1))
    with pytest.raises(ValueError):
        run("refused", segment_outputs=[])
    assert not os.path.exists(str(tmp_path / "refused" / "segment"))
