"""CPU tests of the run-length annotations: the two restatements of segrle_ref.py agree on every case the GPU tests run, decode and
encode round-trip, the counts' invariants, the parsing and the refusals of the new yaml keys, ops.rle_lists, and the JSON writer on
a hand-written map.  Nothing here launches a kernel."""
import json

import numpy as np
import pytest

import segrle_ref as R

CASES = R.host_cases()


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, runner
    return lib, ops, runner


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatements_agree_and_round_trip(case):
    _, m, P = case
    h, w = m.shape
    union = np.zeros((h, w), dtype=bool)
    for p in range(P):
        a, b = R.encode_numpy(m, p), R.encode_loop(m, p)
        assert a == b, p
        assert sum(a) == h * w and all(c > 0 for c in a[1:]) and a[0] >= 0
        mask = R.decode(a, h, w)
        assert np.array_equal(mask, m == p)
        assert R.encode_numpy(np.where(mask, p, 255), p) == a           # decode, then encode again
        area, bbox = R.area_bbox(m, p)
        assert area == sum(a[1::2]) == int(mask.sum())
        if area:
            x, y, bw, bh = bbox
            assert mask[y:y + bh, x:x + bw].sum() == area and mask[y, x:x + bw].any() and mask[y + bh - 1, x:x + bw].any()
            assert mask[y:y + bh, x].any() and mask[y:y + bh, x + bw - 1].any()
        else:
            assert bbox == (0, 0, 0, 0) and a == [h * w]
        union |= mask
    assert np.array_equal(union, m < P)


def test_counts_by_hand():
    m = np.array([[0, 1],
                  [0, 1],
                  [1, 1]], dtype=np.uint8)                              # column-major: 0 0 1 | 1 1 1
    assert R.encode_numpy(m, 0) == R.encode_loop(m, 0) == [0, 2, 4]
    assert R.encode_numpy(m, 1) == R.encode_loop(m, 1) == [2, 4]
    assert R.encode_numpy(m, 2) == R.encode_loop(m, 2) == [6]
    assert R.area_bbox(m, 0) == (2, (0, 0, 1, 2)) and R.area_bbox(m, 1) == (4, (0, 0, 2, 3)) and R.area_bbox(m, 2) == (0, (0, 0, 0, 0))
    assert R.encode_numpy(R.checkerboard(37, 29), 0) == [0] + [1] * (37 * 29)         # h w + 1 counts over both parts: the longest
    assert R.encode_numpy(R.checkerboard(37, 29), 1) == [1] * (37 * 29)
    assert R.encode_numpy(np.full((4, 5), 1, dtype=np.uint8), 1) == [0, 20] and R.encode_numpy(np.full((4, 5), 1, dtype=np.uint8), 0) == [20]
    all_ = R.encode_all([m, m[:, ::-1]], 3, R.encode_loop)
    assert all_["offsets"].tolist() == [0, 3, 5, 6, 9, 13, 14] and all_["counts"].tolist() == [0, 2, 4, 2, 4, 6, 3, 2, 1, 0, 3, 2, 1, 6]
    plane, table, total = R.pack([m, m], fill=7)
    assert total == 32 and table.tolist() == [[0, 3, 2, 0], [16, 3, 2, 1]] and plane[6:16].tolist() == [7] * 10


def test_rle_lists_splits_and_refuses():
    _, ops, _ = _mods()
    from upsparts_amd import lib as L
    ref = R.encode_all([R.noise_map(5, 4, 3, 1), R.blocks_map(6, 7, 3, 2, cell=2)], 3)
    lists = ops.rle_lists(ref["offsets"], ref["counts"], 2, 3)
    assert lists[1][2] == R.encode_loop(R.blocks_map(6, 7, 3, 2, cell=2), 2) and all(isinstance(v, int) for v in lists[0][0])
    assert sum(len(l) for img in lists for l in img) == ref["counts"].size
    for bad in ((ref["offsets"][:-1], ref["counts"]), (ref["offsets"], ref["counts"][:-1]), (ref["offsets"] + 1, ref["counts"])):
        with pytest.raises(L.UpsError):
            ops.rle_lists(bad[0], bad[1], 2, 3)


def test_library_exports_the_new_symbols():
    lib, ops, _ = _mods()
    for name in ("ups_segment_rle_chunk", "ups_segment_rle_scratch_bytes", "ups_segment_rle_count", "ups_segment_rle_write"):
        assert name in lib.EXPORTS
    assert ops.SEGMENT_RLE_CHUNK == R.CHUNK == ops.SEGMENT_CHUNK


def test_segment_options_annotation_keys():
    _, _, runner = _mods()
    base = {"segment_csv": "list.csv"}
    assert "annotations" not in runner.segment_options(base)
    assert "annotations" not in runner.segment_options(dict(base, segment_annotations="none", segment_annotation_min_area=7))
    assert runner.segment_options(dict(base, segment_annotations="coco"))["annotations"] == {"min_area": 1, "path": None}
    opt = runner.segment_options(dict(base, segment_annotations="coco", segment_annotation_min_area=0, segment_annotation_path="a/b.json"))
    assert opt["annotations"] == {"min_area": 0, "path": "a/b.json"} and opt["outputs"] == ("labels", "overlay")
    for bad in ({"segment_annotations": "voc"}, {"segment_annotations": True}, {"segment_annotations": None},
                {"segment_annotations": ["coco"]}, {"segment_annotation_min_area": -1}, {"segment_annotation_min_area": 1.5},
                {"segment_annotation_min_area": True}, {"segment_annotation_min_area": "3"}, {"segment_annotation_path": ""},
                {"segment_annotation_path": 3}):
        with pytest.raises(ValueError):
            runner.segment_options(dict(base, **bad))
        if "segment_annotations" not in bad:
            with pytest.raises(ValueError):
                runner.segment_options(dict(base, segment_annotations="coco", **bad))
    # an empty list of outputs: only with the annotations
    for cfg in (dict(base, segment_outputs=[]), dict(base, segment_outputs=[], segment_annotations="none")):
        with pytest.raises(ValueError):
            runner.segment_options(cfg)
    opt = runner.segment_options(dict(base, segment_outputs=[], segment_annotations="coco"))
    assert opt["outputs"] == () and opt["annotations"] == {"min_area": 1, "path": None}
    with pytest.raises(ValueError):
        runner.segment_options(dict(base, segment_outputs=["masks"], segment_annotations="coco"))


EXPECTED_JSON = (
    '{"images":[{"id":1,"file_name":"a/one.png","height":3,"width":2}],'
    '"categories":[{"id":1,"name":"part_0","color":[10,20,30]},{"id":2,"name":"part_1","color":[40,50,60]},'
    '{"id":3,"name":"part_2","color":[70,80,90]}],'
    '"annotations":[{"id":1,"image_id":1,"category_id":1,"segmentation":{"size":[3,2],"counts":[0,2,4]},"area":2,"bbox":[0,0,1,2],'
    '"iscrowd":1},'
    '{"id":2,"image_id":1,"category_id":2,"segmentation":{"size":[3,2],"counts":[2,4]},"area":4,"bbox":[0,0,2,3],"iscrowd":1}]}\n')


def test_json_writer_on_a_hand_written_map(tmp_path):
    _, _, runner = _mods()
    m = np.array([[0, 1],
                  [0, 1],
                  [1, 1]], dtype=np.uint8)
    palette = [[10, 20, 30], [40, 50, 60], [70, 80, 90]]
    masks = [[(R.encode_loop(m, p),) + R.area_bbox(m, p) for p in range(3)]]
    path = tmp_path / "deep" / "annotations.json"
    runner.write_coco_annotations(str(path), [("a/one.png", 3, 2)], masks, palette, min_area=1)
    assert path.read_text() == EXPECTED_JSON
    doc = json.loads(path.read_text())
    assert list(doc) == ["images", "categories", "annotations"]
    for a in doc["annotations"]:
        h, w = a["segmentation"]["size"]
        assert np.array_equal(R.decode(a["segmentation"]["counts"], h, w), m == a["category_id"] - 1)
    # min_area 0 keeps the empty part (its mask is one run of zeros), 3 drops the part of two pixels; ids stay 1-based and dense
    doc0 = runner.coco_annotations([("a/one.png", 3, 2)], masks, palette, min_area=0)
    assert [a["category_id"] for a in doc0["annotations"]] == [1, 2, 3] and doc0["annotations"][2]["segmentation"]["counts"] == [6]
    assert doc0["annotations"][2]["bbox"] == [0, 0, 0, 0] and doc0["annotations"][2]["area"] == 0
    doc3 = runner.coco_annotations([("a/one.png", 3, 2)], masks, palette, min_area=3)
    assert [(a["id"], a["category_id"]) for a in doc3["annotations"]] == [(1, 2)]
    with pytest.raises(ValueError):
        runner.coco_annotations([("a/one.png", 3, 2)], [masks[0][:2]], palette)
