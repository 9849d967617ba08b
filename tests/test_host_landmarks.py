"""Host tests of the landmark regression evaluation: the NumPy restatement (landmarks_ref.py) against independent formulas -- moments
against np.einsum, the solve on a planted problem -- the keypoint csv and its normalisation, the `landmark_*` refusals of the runner,
the PCK and mean arithmetic on a hand-made d2, the regressor's files and the library's exports."""
import os
import re

import numpy as np
import pytest

import landmarks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, landmarks, runner
    return lib, ops, landmarks, runner


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", [(16, 16, 3), (5, 51, 10), (1, 257, 1), (12, 12, 32)], ids=lambda s: "x".join(map(str, s)))
def test_moments_restatement_against_einsum(shape):
    h, w, P = shape
    rng = np.random.RandomState(sum(shape))
    soft = rng.rand(3, h, w, P).astype(np.float32)
    soft /= soft.sum(-1, keepdims=True)
    pred = soft.argmax(-1).astype(np.int64)
    pred[0, 0, 0], pred[1, -1, -1] = -1, P                   # out of range: counted, no sum touched
    r = R.part_moments(soft, pred, min_mass=0.0)
    s = soft.reshape(3, h * w, P).astype(np.float64)
    ux, uy, ix, iy = R.pixel_units(h, w)
    assert ux.min() == (1.0 - w) / w and ux.max() == (w - 1.0) / w and uy.min() == (1.0 - h) / h      # pixel centres on [-1, 1]
    want = np.stack([np.einsum("npk->nk", s), np.einsum("npk,p->nk", s, ux), np.einsum("npk,p->nk", s, uy)], axis=-1)
    bound = R.reordered_sum_bound(h * w, r["terms"])
    assert (np.abs(r["sums"] - want) <= bound).all()
    assert (r["valid"] == 1).all()
    assert np.array_equal(r["centre"], r["sums"][..., 1:] / r["sums"][..., :1])
    assert np.abs(r["mass"].sum(-1) - h * w).max() <= 1e-3                                           # a soft-max: masses add up to the pixels
    # the integer sums against a plain loop
    hard = np.zeros((3, P, 3), dtype=np.int64)
    bad = 0
    for n in range(3):
        for y in range(h):
            for x in range(w):
                p = pred[n, y, x]
                if 0 <= p < P:
                    hard[n, p] += (1, 2 * x + 1 - w, 2 * y + 1 - h)
                else:
                    bad += 1
    assert np.array_equal(r["hard"], hard) and r["hard"].dtype == np.int32 and r["invalid"] == bad == 2
    c, cnt, ok = R.hard_centres(r["hard"], h, w, 1)
    m = cnt > 0
    assert (np.abs(c[m]) < 1).all() and (c[~m] == 0).all() and np.array_equal(ok != 0, m)


def test_moments_restatement_is_exact_on_a_lattice_and_honours_min_mass():
    rng = np.random.RandomState(3)
    soft = (rng.randint(0, 257, size=(2, 16, 16, 3)) / 256.0).astype(np.float32)
    soft[1, :, :, 2] = 0
    soft[1, 0, 0, 2] = 0.25                                  # mass 0.25
    soft[0, :, :, 1] = 0                                     # mass 0: never valid, also at min_mass 0
    r = R.part_moments(soft, None, min_mass=0.5)
    s = soft.reshape(2, 256, 3).astype(np.float64)
    ux, uy, _, _ = R.pixel_units(16, 16)
    assert np.array_equal(r["sums"][..., 0], s.sum(1)) and np.array_equal(r["sums"][..., 1], (s * ux[None, :, None]).sum(1))
    assert r["valid"].tolist() == [[1, 0, 1], [1, 1, 0]] and (r["centre"][1, 2] == 0).all() and (r["centre"][0, 1] == 0).all()
    assert r["mass"][1, 2] == 0.25 and r["hard"] is None
    assert R.part_moments(soft, None, min_mass=0.0)["valid"].tolist() == [[1, 0, 1], [1, 1, 1]]
    assert R.part_moments(soft, None, min_mass=0.0)["centre"][1, 2].tolist() == [-15.0 / 16.0, -15.0 / 16.0]


@pytest.mark.parametrize("P", [3, 10, 32])
def test_solve_restatement_recovers_a_planted_map(P):
    """Features on a 1/64 lattice, regressors multiples of 1/8, 70 % visible, ridge 0: the targets are exact in float64, so the
    normal equations hold the planted W exactly and the sequential Cholesky returns it to within its own rounding."""
    rng = np.random.RandomState(P)
    N, K = 400, 5
    feat = rng.randint(-64, 65, size=(N, 2 * P)) / 64.0
    planted = rng.randint(-16, 17, size=(K, 2 * P + 1, 2)) / 8.0
    vis = (rng.rand(N, K) < 0.7).astype(np.uint8)
    target = np.einsum("nd,kdc->nkc", R.with_one(feat), planted)
    target[vis == 0] = np.nan                                # never read
    G, Rr, cnt = R.gram(feat, target, vis)
    assert np.array_equal(G, G.transpose(0, 2, 1)) and np.array_equal(cnt, vis.sum(0)) and np.isfinite(Rr).all()
    f1 = R.with_one(feat)
    assert np.array_equal(G[2], np.einsum("na,nb->ab", f1[vis[:, 2] != 0], f1[vis[:, 2] != 0]))     # lattice data: exact in any order
    W, bad = R.solve(G, Rr, cnt, 0.0)
    err = np.abs(W - planted).max()
    print("planted solve, P =", P, "max |W - planted| =", err, "cond(G_0) =", np.linalg.cond(G[0]))
    assert not bad.any() and err <= 1e-12
    pred, d2 = R.predict(feat, W, target, vis)
    assert (d2[vis == 0] == -1).all() and d2[vis != 0].max() <= 1e-24 and np.abs(pred - np.einsum("nd,kdc->nkc", f1, W)).max() <= 1e-13


def test_solve_restatement_singular_cases():
    rng = np.random.RandomState(9)
    N, P, K = 50, 3, 3
    feat = rng.randint(-64, 65, size=(N, 2 * P)) / 64.0
    feat[:, 2:4] = 0.0                                       # an always-absent part: two zero columns
    target = rng.rand(N, K, 2) * 2 - 1
    vis = np.ones((N, K), dtype=np.uint8)
    vis[:, 1] = 0                                            # a keypoint that is never visible
    G, Rr, cnt = R.gram(feat, target, vis)
    assert cnt.tolist() == [N, 0, N] and (G[1] == 0).all() and (Rr[1] == 0).all()
    W0, bad0 = R.solve(G, Rr, cnt, 0.0)
    assert bad0.all() and (W0 == 0).all()                    # the zero columns: a zero pivot without the ridge
    W, bad = R.solve(G, Rr, cnt, 1e-6)
    assert bad.tolist() == [False, True, False] and (W[1] == 0).all() and (W[0, 2:4] == 0).all() and np.abs(W[0]).max() > 0
    A = G[0] + 1e-6 * np.diag([1.0] * (2 * P) + [0.0])
    assert np.abs(W[0] - np.linalg.solve(A, Rr[0])).max() <= 1e-9


# ---------------------------------------------------------------------------------------------- csv, options, metrics, files
def test_keypoint_csv_and_normalisation(tmp_path):
    _, _, LM, _ = _mods()
    path = tmp_path / "kp.csv"
    path.write_text("a/0.png, 0, 0, 1, 9.5, 4, 0\n\nb/1.png,19,9,1,nan,nan,0\n")
    files, xy, vis = LM.read_landmark_csv(str(path))
    assert files == ["a/0.png", "b/1.png"] and xy.shape == (2, 2, 2) and xy.dtype == np.float64
    assert vis.tolist() == [[1, 0], [1, 0]] and vis.dtype == np.uint8 and xy[0, 1].tolist() == [9.5, 4.0]
    t = LM.normalise_targets(xy, [(10, 20), (10, 20)])
    assert t[0, 0].tolist() == [1.0 / 20 - 1, 1.0 / 10 - 1] and t[1, 0].tolist() == [39.0 / 20 - 1, 19.0 / 10 - 1]   # first and last pixel centre
    assert np.abs(LM.to_source_pixels(t, [(10, 20), (10, 20)])[:, 0] - xy[:, 0]).max() <= 1e-12
    for text in ("a.png,1,2\n", "a.png,1,2,1\nb.png,1,2,1,3,4,1\n", "a.png,1,x,1\n", "a.png,inf,2,1\n", "\n"):
        path.write_text(text)
        with pytest.raises(ValueError):
            LM.read_landmark_csv(str(path))
    with pytest.raises(FileNotFoundError):
        LM.read_landmark_csv(str(tmp_path / "nope.csv"))


def test_landmark_options_defaults_and_refusals(tmp_path):
    import yaml
    _, _, LM, runner = _mods()
    base = {"landmark_fit_csv": "fit.csv"}
    assert LM.landmark_options(base) == {"fit_csv": "fit.csv", "test_csv": None, "source": "soft", "min_part_area": 0.005,
                                         "ridge": 1e-6, "pck": [0.05, 0.1], "names": None}
    assert sorted(LM.LANDMARK_DEFAULTS) == ["landmark_min_part_area", "landmark_names", "landmark_pck", "landmark_ridge",
                                            "landmark_source", "landmark_test_csv"]
    o = LM.landmark_options(dict(base, landmark_test_csv="t.csv", landmark_source="hard", landmark_ridge=0, landmark_pck=[0.2],
                                 landmark_names=["beak", "tail"]))
    assert (o["test_csv"], o["source"], o["ridge"], o["pck"], o["names"]) == ("t.csv", "hard", 0.0, [0.2], ["beak", "tail"])
    bads = [{"landmark_fit_csv": None}, {"landmark_fit_csv": 3}, {"landmark_test_csv": 5}, {"landmark_test_csv": ""},
            {"landmark_source": "mean"}, {"landmark_min_part_area": -0.1}, {"landmark_min_part_area": 1.5},
            {"landmark_min_part_area": "small"}, {"landmark_min_part_area": True}, {"landmark_ridge": -1e-6}, {"landmark_ridge": "tiny"},
            {"landmark_ridge": float("inf")}, {"landmark_pck": []}, {"landmark_pck": 0.1}, {"landmark_pck": [0.0]}, {"landmark_pck": [1.5]},
            {"landmark_pck": [0.1, 0.1]}, {"landmark_pck": ["a"]}, {"landmark_names": "beak"}, {"landmark_names": [1, 2]},
            {"landmark_names": []}, {"landmark_rigde": 1e-3}]
    for bad in bads:
        with pytest.raises(ValueError):
            LM.landmark_options(dict(base, **bad))
    # through the runner: before a model is built (no device here), and before data_root is asked for
    ypath = tmp_path / "lm.yaml"
    for bad in [{}] + [dict(base, **b) for b in bads[2:]]:
        ypath.write_text(yaml.safe_dump(dict({"batch_size": 2}, **bad)))
        with pytest.raises(ValueError, match="landmark"):
            runner.main(["--landmarks", str(ypath)])
    ypath.write_text(yaml.safe_dump(dict({"batch_size": 2}, **base)))
    with pytest.raises(ValueError, match="data_root"):
        runner.main(["--landmarks", str(ypath)])


def test_runner_counts_landmarks_among_the_routes(tmp_path, capsys):
    _, _, _, runner = _mods()
    y = str(tmp_path / "x.yaml")
    for argv in (["--landmarks", y, "-t", y], ["--landmarks", y, "--index", y], []):
        with pytest.raises(SystemExit):
            runner.main(argv)
        assert "--landmarks" in capsys.readouterr().err


def test_metrics_on_a_hand_made_d2():
    _, _, LM, _ = _mods()
    # errors (sqrt(d2) / 2): keypoint 0: 0.05, 0.1, 0.2; keypoint 1: 0.0 and two invisible; keypoint 2: never visible
    d2 = np.array([[0.01, 0.0, -1.0], [0.04, -1.0, -1.0], [0.16, -1.0, -1.0]])
    m = LM.metrics_from_d2(d2, [0.05, 0.1], n_singular=1)
    k0, k1, k2 = m["keypoints"]
    e0 = np.sqrt(np.array([0.01, 0.04, 0.16])) / 2.0
    assert k0 == {"n_visible": 3, "mean_error": float(e0.mean()), "pck@0.05": float((e0 <= 0.05).mean()), "pck@0.1": float((e0 <= 0.1).mean())}
    assert abs(k0["mean_error"] - 0.35 / 3) <= 1e-15 and k0["pck@0.1"] in (1.0 / 3, 2.0 / 3)          # (0.1 itself: as the rounding falls)
    assert k1 == {"n_visible": 1, "mean_error": 0.0, "pck@0.05": 1.0, "pck@0.1": 1.0}
    assert k2 == {"n_visible": 0, "mean_error": None, "pck@0.05": None, "pck@0.1": None}
    assert m["n_visible"] == 4 and m["n_singular"] == 1
    assert m["mean_error"] == float(np.mean([k0["mean_error"], 0.0])) and m["mean_error_instances"] == float(np.append(e0, 0.0).mean())
    assert m["pck@0.05"] == float(np.mean([k0["pck@0.05"], 1.0]))
    r = R.metrics(d2, [0.05, 0.1])
    assert r["mean_error"] == m["mean_error"] and r["mean_error_instances"] == m["mean_error_instances"]
    assert r["n_visible"].tolist() == [3, 1, 0] and r["pck@0.1"][0] == k0["pck@0.1"]
    none = LM.metrics_from_d2(np.full((2, 2), -1.0), [0.1])
    assert none["mean_error"] is None and none["mean_error_instances"] is None and none["pck@0.1"] is None and none["n_visible"] == 0


def test_regressor_save_load_round_trip(tmp_path):
    lib, _, LM, _ = _mods()
    rng = np.random.RandomState(4)
    W, cnt = rng.standard_normal((4, 7, 2)), np.array([5, 0, 9, 9], dtype=np.int32)
    reg = LM.LandmarkRegressor(W, cnt, n_singular=1, options={"ridge": 1e-6, "source": "soft", "pck": [0.05, 0.1]})
    reg.save(str(tmp_path / "one.npz"))
    back = LM.LandmarkRegressor.load(str(tmp_path / "one.npz"))
    assert np.array_equal(back.W.view(np.int64), W.view(np.int64)) and np.array_equal(back.cnt, cnt) and back.cnt.dtype == np.int32
    assert back.n_singular == 1 and back.options == reg.options
    with np.load(str(tmp_path / "one.npz")) as z:
        assert sorted(z.files) == ["W", "cnt", "options", "singular"]
    back.save(str(tmp_path / "two.npz"))
    assert open(str(tmp_path / "one.npz"), "rb").read() == open(str(tmp_path / "two.npz"), "rb").read()
    with pytest.raises(ValueError):
        LM.LandmarkRegressor().save(str(tmp_path / "three.npz"))
    import torch
    if not torch.cuda.is_available():                        # no host route: the kernels are the product
        with pytest.raises(lib.UpsError):
            back.predict(np.zeros((2, 3, 2)), np.ones((2, 3), dtype=np.uint8))


def test_library_exports_the_landmark_entries():
    lib, ops, _, _ = _mods()
    names = ("ups_part_moments_chunk", "ups_part_moments_scratch_bytes", "ups_part_moments", "ups_landmark_chunk",
             "ups_landmark_gram_scratch_bytes", "ups_landmark_gram", "ups_landmark_solve", "ups_landmark_predict")
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    h = lib.load()
    for name in names:
        assert name in lib.EXPORTS and re.search(r"\b{}\s*\(".format(name), hdr) and hasattr(h, name), name
    assert lib.ABI_VERSION == 6 and "#define UPS_ABI_VERSION 6" in hdr
    flags = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "flags.sh")).read()
    assert "landmarks" in re.search(r'UPS_SOURCES="([^"]*)"', flags).group(1).split()
    assert (h.ups_part_moments_chunk(), h.ups_landmark_chunk()) == (R.MOMENTS_CHUNK, R.LANDMARK_CHUNK)
    # one partial of 3 P doubles per block of MOMENTS_CHUNK pixels; D D + 2 D + 1 doubles per block of LANDMARK_CHUNK items and keypoint
    assert h.ups_part_moments_scratch_bytes(3, 1, 257, 10) == 3 * 2 * 3 * 10 * 8
    assert h.ups_part_moments_scratch_bytes(1, 16, 16, 1) == 3 * 8
    for bad in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3), (1, 4, 4, 0), (1, 4, 4, 33), (1, 1024, 1025, 3), (1, 1, 1 << 17, 3)):
        assert h.ups_part_moments_scratch_bytes(*bad) == 0, bad
    assert h.ups_landmark_gram_scratch_bytes(R.LANDMARK_CHUNK + 1, 7, 4) == 2 * 4 * (49 + 14 + 1) * 8
    for bad in ((0, 7, 4), (5, 0, 4), (5, 7, 0), (5, 66, 4), (5, 7, 33)):
        assert h.ups_landmark_gram_scratch_bytes(*bad) == 0, bad
    assert (ops.PART_MOMENTS_MAX_P, ops.LANDMARK_MAX_D, ops.LANDMARK_MAX_K) == (32, 65, 32)
