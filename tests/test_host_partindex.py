"""Host tests of the part-appearance index: the NumPy restatement (partindex_ref.py) against brute force, Lloyd's monotone inertia, the
seeding as a pure function of the seed, the library's exports, PartIndex's files and the `index_*` refusals of the runner."""
import os
import re

import numpy as np
import pytest

import partindex_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, partindex, runner
    return lib, ops, partindex, runner


# ---------------------------------------------------------------------------------------------- the restatement
def test_distance_is_the_ascending_channel_loop():
    rng = np.random.RandomState(0)
    x, y = rng.standard_normal((5, 7)).astype(np.float32), rng.standard_normal((3, 7)).astype(np.float32)
    d = R.distance(x[:, None], y[None])
    assert d.shape == (5, 3) and d.dtype == np.float64
    for i in range(5):
        for j in range(3):
            acc = 0.0
            for a in range(7):
                t = float(x[i, a]) - float(y[j, a])
                acc = acc + t * t
            assert d[i, j] == acc
    assert np.abs(d - ((x[:, None].astype(np.float64) - y[None]) ** 2).sum(-1)).max() <= 1e-13


@pytest.mark.parametrize("bank", ["float", "lattice"])
def test_knn_equals_a_brute_force_sort(bank):
    rng = np.random.RandomState(1)
    N, P, A, K = 23, 3, 5, 6
    feat, valid = R.float_bank(rng, N, P, A) if bank == "float" else R.lattice_bank(rng, N, P, A, 2)
    feat[10:17] = feat[0:7]                      # exact duplicates: ties in d, broken by the index
    valid[:, 2] = 0
    valid[:4, 2] = 1                             # three eligible neighbours < K: padding
    idx, dist = R.knn(feat, valid, feat, valid, K, True)
    for p in range(P):
        for n in range(N):
            if not valid[n, p]:
                assert (idx[n, p] == -1).all() and np.isinf(dist[n, p]).all()
                continue
            pairs = sorted((float(R.distance(feat[n, p], feat[g, p])), g) for g in range(N) if valid[g, p] and g != n)[:K]
            assert idx[n, p, :len(pairs)].tolist() == [g for _, g in pairs]
            assert dist[n, p, :len(pairs)].tolist() == [d for d, _ in pairs]
            assert (idx[n, p, len(pairs):] == -1).all() and np.isinf(dist[n, p, len(pairs):]).all()
    assert (idx[:4, 2, 3:] == -1).all() and (idx[:4, 2, :3] >= 0).all()
    d0 = dist[0, 0][np.isfinite(dist[0, 0])]
    assert (np.diff(d0) >= 0).all()
    same, _ = R.knn(feat, valid, feat, valid, K, False)
    for v in np.flatnonzero(valid[:, 0]):        # with itself eligible: itself or an earlier valid copy
        assert same[v, 0, 0] == min(g for g in range(N) if valid[g, 0] and (feat[g, 0] == feat[v, 0]).all())


def test_kmeans_step_by_hand():
    feat = np.array([[[0.0, 0.0]], [[1.0, 0.0]], [[10.0, 0.0]], [[11.0, 0.0]], [[5.5, 0.0]], [[99.0, 0.0]]], dtype=np.float32)
    valid = np.array([[1], [1], [1], [1], [1], [0]], dtype=np.uint8)
    cent = np.array([[[0.0, 0.0], [11.0, 0.0], [500.0, 0.0]]])
    prev = np.array([[0], [0], [0], [1], [1], [-1]], dtype=np.int32)
    r = R.kmeans_step(feat, valid, cent, prev)
    assert r["label"][:, 0].tolist() == [0, 0, 1, 1, 0, -1]            # 5.5 is equally far from both: the first
    assert r["mind"][:, 0].tolist() == [0.0, 1.0, 1.0, 0.0, 30.25, np.inf]
    assert r["counts"].tolist() == [[3, 2, 0]] and r["changed"] == 2 and r["inertia"].tolist() == [32.25]
    assert r["sums"][0].tolist() == [[6.5, 0.0], [21.0, 0.0], [0.0, 0.0]]
    new = R.update_centroids(cent, r["sums"], r["counts"])
    assert new[0].tolist() == [[6.5 / 3, 0.0], [10.5, 0.0], [500.0, 0.0]]          # the empty cluster keeps its centroid


@pytest.mark.parametrize("init", ["kmeans++", "random"])
def test_lloyd_inertia_does_not_increase(init):
    rng = np.random.RandomState(2)
    feat, valid = R.float_bank(rng, 120, 2, 4)
    feat[:60] += 3.0
    r = R.lloyd(feat, valid, 4, seed=3, init=init)
    trace = np.stack(r["inertia_trace"])
    assert r["iterations"] == len(trace) >= 2
    assert (np.diff(trace, axis=0) <= 1e-12 * trace[:-1]).all()
    assert r["labels"].shape == (2, 120) and r["labels"].dtype == np.int32 and r["clusters"].shape == (2, 4, 4)
    assert ((r["labels"] == -1) == (valid.T == 0)).all()
    assert r["counts"].sum(axis=1).tolist() == valid.sum(axis=0).tolist()


def test_seeding_is_a_pure_function_of_the_seed():
    rng = np.random.RandomState(3)
    feat, valid = R.lattice_bank(rng, 60, 3, 4, 3)
    for init in ("kmeans++", "random"):
        a, b = R.seed_centres(feat, valid, 4, 5, init), R.seed_centres(feat.copy(), valid.copy(), 4, 5, init)
        assert np.array_equal(a, b) and a.shape == (3, 4, 4) and a.dtype == np.float64
        assert not np.array_equal(a, R.seed_centres(feat, valid, 4, 6, init))
        for p in range(3):                       # every centre is a valid item of its part
            items = feat[valid[:, p] != 0, p].astype(np.float64)
            for j in range(4):
                assert (items == a[p, j]).all(axis=1).any()
    # the random init of the product is host logic alone: the same centres
    _, _, PI, _ = _mods()
    assert np.array_equal(PI.PartIndex(feat, valid).seed_centres(4, 5, "random"), R.seed_centres(feat, valid, 4, 5, "random"))
    valid[:, 1] = 0
    valid[:3, 1] = 1
    with pytest.raises(ValueError, match="part 1"):
        R.seed_centres(feat, valid, 4, 5)
    with pytest.raises(ValueError, match="part 1"):
        PI.PartIndex(feat, valid).seed_centres(4, 5, "random")


def test_normalize_restated_alike():
    _, _, PI, _ = _mods()
    rng = np.random.RandomState(4)
    feat, valid = R.float_bank(rng, 9, 2, 5)
    feat[3, 1] = 0.0
    valid[3, 1] = 1
    want_f, want_v = R.normalize(feat, valid)
    idx = PI.PartIndex(feat, valid, normalize=True)
    assert np.array_equal(idx.feat, want_f) and np.array_equal(idx.valid != 0, want_v) and not idx.valid[3, 1] and idx.normalized
    n = np.sqrt((idx.feat.astype(np.float64) ** 2).sum(-1))
    assert np.abs(n[np.arange(9) != 3] - 1.0).max() <= 1e-6


# ---------------------------------------------------------------------------------------------- library and files
def test_library_exports_the_index_entries():
    lib, ops, _, _ = _mods()
    names = ("ups_part_knn_tile", "ups_part_kmeans_chunk", "ups_part_knn", "ups_part_kmeans_scratch_bytes", "ups_part_kmeans_step")
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    for name in names:
        assert name in lib.EXPORTS and re.search(r"\b{}\s*\(".format(name), hdr)
    assert lib.ABI_VERSION == 6 and "#define UPS_ABI_VERSION 6" in hdr
    flags = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "flags.sh")).read()
    assert "partindex" in re.search(r'UPS_SOURCES="([^"]*)"', flags).group(1).split()
    h = lib.load()
    T, C = h.ups_part_knn_tile(), h.ups_part_kmeans_chunk()
    assert T >= 2 and C >= 2
    # per block of C items and part: k * A partial feature sums and one partial inertia
    assert h.ups_part_kmeans_scratch_bytes(C + 1, 3, 5, 7) == 3 * 2 * (7 * 5 + 1) * 8
    assert h.ups_part_kmeans_scratch_bytes(1, 1, 1, 1) == 2 * 8
    for bad in ((0, 3, 5, 7), (4, 0, 5, 7), (4, 3, 0, 7), (4, 3, 5, 0), (4, 3, 513, 7), (4, 3, 5, 65), (2 ** 31 - 1, 64, 512, 64)):
        assert h.ups_part_kmeans_scratch_bytes(*bad) == 0
    assert (ops.PART_KNN_MAX_K, ops.PART_KMEANS_MAX_K) == (32, 64)


def test_kmeans_step_refuses_a_bad_changed_counter():
    """`changed` is written as one int32: another dtype or size is refused by name, before any device pointer is formed."""
    import torch
    lib, ops, _, _ = _mods()
    feat, valid, cent = torch.zeros((4, 2, 3)), torch.ones((4, 2), dtype=torch.uint8), torch.zeros((2, 2, 3), dtype=torch.float64)
    for changed in (torch.zeros(1, dtype=torch.float32), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(lib.UpsError, match="changed"):
            ops.part_kmeans_step(feat, valid, cent, accumulate=False, changed=changed)


def test_part_index_save_load_round_trip(tmp_path):
    _, _, PI, _ = _mods()
    rng = np.random.RandomState(5)
    feat, valid = R.float_bank(rng, 11, 3, 5)
    area = rng.randint(0, 256, size=(11, 3)).astype(np.int32)
    files = ["a/{}.png".format(i) for i in range(11)]
    idx = PI.PartIndex(feat, valid, files=files, area=area, normalize=True)
    idx.save(str(tmp_path / "one"))
    assert sorted(os.listdir(str(tmp_path / "one"))) == ["features.npz", "index.csv"]
    back = PI.PartIndex.load(str(tmp_path / "one"))
    assert np.array_equal(back.feat, idx.feat) and back.feat.dtype == np.float32
    assert np.array_equal(back.valid, idx.valid) and back.valid.dtype == np.uint8
    assert np.array_equal(back.area, area) and back.files == files and back.normalized
    assert (back.N, back.P, back.A) == (11, 3, 5)
    with np.load(str(tmp_path / "one" / "features.npz")) as z:
        assert sorted(z.files) == ["area", "feat", "normalized", "valid"]
    lines = open(str(tmp_path / "one" / "index.csv")).read().splitlines()
    assert lines[0] == "file,area_0,area_1,area_2" and lines[1] == "a/0.png," + ",".join(str(a) for a in area[0])
    # written twice: the same bytes; without names and areas: the arrays alone
    back.save(str(tmp_path / "two"))
    for name in ("features.npz", "index.csv"):
        assert open(str(tmp_path / "one" / name), "rb").read() == open(str(tmp_path / "two" / name), "rb").read()
    PI.PartIndex(feat, valid).save(str(tmp_path / "three"))
    bare = PI.PartIndex.load(str(tmp_path / "three"))
    assert os.listdir(str(tmp_path / "three")) == ["features.npz"] and bare.files is None and bare.area is None and not bare.normalized
    for bad in ((feat[0], valid), (feat, valid[:5]), (np.full_like(feat, np.nan), valid)):
        with pytest.raises(ValueError):
            PI.PartIndex(*bad)
    with pytest.raises(ValueError):
        PI.PartIndex(feat, valid, files=files[:3])


def test_sheet_geometry():
    _, _, PI, _ = _mods()
    rng = np.random.RandomState(6)
    S, N, P, K = 4, 5, 2, 3
    views = rng.randint(1, 256, size=(N, S, S, 3)).astype(np.uint8)
    labels = rng.randint(0, P, size=(N, S, S)).astype(np.uint8)
    crop = PI.part_crop(views[1], labels[1], 1)
    assert (crop[labels[1] == 1] == views[1][labels[1] == 1]).all() and (crop[labels[1] != 1] == 0).all()
    valid = np.array([[1, 1], [0, 1], [1, 1], [1, 0], [1, 1]], dtype=np.uint8)
    idx = np.full((N, P, K), -1, dtype=np.int32)
    idx[0, 0] = [2, 4, -1]
    sheet = PI.neighbour_sheet(views, labels, valid, views, labels, idx, 0, 3)
    assert sheet.shape == (3 * S, (K + 1) * S, 3) and sheet.dtype == np.uint8          # queries 0, 2, 3 of part 0
    assert (sheet[:S, :S] == PI.part_crop(views[0], labels[0], 0)).all()
    assert (sheet[:S, S:2 * S] == PI.part_crop(views[2], labels[2], 0)).all() and (sheet[:S, 3 * S:] == 0).all()
    assert (sheet[S:2 * S, :S] == PI.part_crop(views[2], labels[2], 0)).all()
    one = PI.cluster_sheet(views, labels, np.array([4, 1]), 1, 6)
    assert one.shape == (S, 6 * S, 3) and (one[:, S:2 * S] == PI.part_crop(views[1], labels[1], 1)).all() and (one[:, 2 * S:] == 0).all()


# ---------------------------------------------------------------------------------------------- the runner's keys
def test_index_options_defaults_and_refusals(tmp_path):
    import yaml
    _, _, PI, runner = _mods()
    base = {"index_csv": "list.csv"}
    assert PI.index_options(base) == {"csv": "list.csv", "query_csv": None, "neighbours": 8, "clusters": 0, "min_part_area": 0.005,
                                      "normalize": False, "init": "kmeans++", "seed": 1, "max_iter": 100, "sheets": True, "n_vis": 20}
    assert PI.index_options(dict(base, index_clusters=2, index_init="random", index_query_csv="q.csv"))["clusters"] == 2
    assert PI.min_area_pixels(0.005, 16) == 2 and PI.min_area_pixels(0.005, 128) == 82 and PI.min_area_pixels(0.0, 16) == 0
    assert PI.min_area_pixels(0.005, 16) == R.part_area_threshold(0.005, 16)
    bads = [{"index_csv": None}, {"index_csv": 3}, {"index_query_csv": 5}, {"index_query_csv": ""}, {"index_neighbours": -1},
            {"index_neighbours": 33}, {"index_neighbours": 2.5}, {"index_neighbours": True}, {"index_clusters": -1},
            {"index_clusters": 65}, {"index_clusters": "two"}, {"index_min_part_area": -0.1}, {"index_min_part_area": 1.5},
            {"index_min_part_area": "small"}, {"index_normalize": "yes"}, {"index_normalize": 1}, {"index_init": "pca"},
            {"index_seed": -1}, {"index_seed": 1.5}, {"index_max_iter": 0}, {"index_max_iter": "many"}, {"index_sheets": "no"},
            {"index_n_vis": 0}, {"index_n_vis": 2.0}, {"index_neigbours": 4},
            {"index_neighbours": 0, "index_clusters": 0, "index_sheets": False}]
    for bad in bads:
        with pytest.raises(ValueError):
            PI.index_options(dict(base, **bad))
    # through the runner: before a model is built (no device here), and before data_root is asked for
    ypath = tmp_path / "index.yaml"
    for bad in [{}] + [dict(base, **b) for b in bads[2:]]:
        ypath.write_text(yaml.safe_dump(dict({"batch_size": 2}, **bad)))
        with pytest.raises(ValueError, match="index"):
            runner.main(["--index", str(ypath)])
    ypath.write_text(yaml.safe_dump(dict({"batch_size": 2}, **base)))
    with pytest.raises(ValueError, match="data_root"):
        runner.main(["--index", str(ypath)])


def test_runner_counts_index_among_the_routes(tmp_path, capsys):
    _, _, _, runner = _mods()
    y = str(tmp_path / "x.yaml")
    for argv in (["--index", y, "-t", y], ["--index", y, "--segment", y]):
        with pytest.raises(SystemExit):
            runner.main(argv)
        assert "--index" in capsys.readouterr().err
