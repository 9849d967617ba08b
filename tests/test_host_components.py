"""CPU tests of the part-coherence feature: the two NumPy restatements of components_ref.py agree on every pattern the GPU tests
run, evalutil.coherence_from_stats on hand-computed tables, evalutil.coherence_host against the restatement, the parsing and the
refusals of the new keys, and the wrapper's error path.  Nothing here launches a kernel."""
import os

import numpy as np
import pytest
import torch

import components_ref as R

SIZES = ((1, 1), (1, 7), (7, 1), (19, 33), (33, 19), (64, 64))


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil, lib, model, ops, runner
    return lib, ops, evalutil, model, runner


# ---------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "{}x{}".format(*s))
def test_restatements_agree(size):
    h, w = size
    maps = R.patterns(h, w) + [("invalid", R.with_invalid(R.noise(h, w, 5, 3), 5, (-1, 5, 1 << 40), 4), 5)]
    for name, m, P in maps:
        for conn in (4, 8):
            a, b = R.components_flood(m, P, conn), R.components_unionfind(m, P, conn)
            assert np.array_equal(a, b), (name, conn)
            valid = (m >= 0) & (m < P)
            assert ((a >= 0) == valid).all()
            flat = a.reshape(-1)
            roots = flat[flat >= 0]
            assert (roots <= np.nonzero(flat >= 0)[0]).all() and (flat[roots] == roots).all()      # the minimum, and a fixed point


def test_known_component_counts():
    n = lambda m, P, conn: len(np.unique(R.components_flood(m, P, conn)))
    assert n(R.checkerboard(6, 7), 2, 4) == 42 and n(R.checkerboard(6, 7), 2, 8) == 2
    assert n(R.diagonals(5, 5), 3, 4) == 25 and n(R.diagonals(5, 5), 3, 8) == 9        # x + y = 0 .. 8: one diagonal each
    assert n(R.filled(7, 3), 1, 4) == 1
    for side in (19, 64, 128):
        m = R.spiral(side, side)
        assert n(m, 2, 4) == 2 and m.sum() > side * side // 2 - 2 * side                 # one long chain of each part
    assert n(R.serpentine(9, 8), 2, 4) == 1 + 4 and n(R.combs(9, 9), 2, 4) == 1 + 4


def test_stats_and_clean_restatement_by_hand():
    m = np.array([[0, 0, 1, 1],
                  [0, 2, 1, 1],
                  [0, 0, 1, 0]])
    comp = R.components_flood(m, 3, 4)
    area, st, inv = R.stats(m, comp, 3, 2)
    assert np.array_equal(comp, [[0, 0, 2, 2], [0, 5, 2, 2], [0, 0, 2, 11]]) and inv == 0
    assert np.array_equal(area, [[5, 5, 5, 5], [5, 1, 5, 5], [5, 5, 5, 1]])
    assert st.tolist() == [[6, 2, 5, 1], [5, 1, 5, 0], [1, 1, 1, 1]]
    out, changed = R.clean_round(m, 3, 4, 2)
    # (1, 1): three neighbours of part 0, one of part 1 -> 0;  (2, 3): two neighbours, both part 1 -> 1
    assert changed == 2 and out[1, 1] == 0 and out[2, 3] == 1 and (out != m).sum() == 2
    prev = np.array([[1, 1, 9, 1]] * 3)
    assert R.accumulate_stats(prev, st).tolist() == [[7, 3, 9, 2], [6, 2, 9, 1], [2, 2, 9, 2]]


# ---------------------------------------------------------------------------------------------- evalutil
def test_coherence_from_stats_by_hand():
    _, _, E, _, _ = _mods()
    # two images of 10 pixels, three parts: part 2 is present nowhere
    stats = np.array([[[6, 2, 5, 1], [4, 1, 4, 0], [0, 0, 0, 0]],
                      [[10, 1, 10, 0], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=np.int32)
    r = E.coherence_from_stats(stats, 10)
    assert r["components_0"] == 1.5 and r["components_1"] == 1.0 and r["components_2"] == -1.0
    assert r["fragmentation_0"] == 1.0 - 15 / 16 and r["fragmentation_1"] == 0.0 and r["fragmentation_2"] == -1.0
    assert r["fragmentation"] == 1.0 - 19 / 20 and r["specks"] == 0.5
    assert sorted(r) == sorted(["components_0", "components_1", "components_2", "fragmentation_0", "fragmentation_1",
                                "fragmentation_2", "fragmentation", "specks"])
    with pytest.raises(ValueError):
        E.coherence_from_stats(stats, 9)
    with pytest.raises(ValueError):
        E.coherence_from_stats(np.zeros((0, 3, 4), np.int32), 10)
    logs = E.validation_logs(coherence=r)
    assert logs["val/fragmentation"] == r["fragmentation"] and logs["val/components_1"] == 1.0 and logs["val/specks"] == 0.5
    assert all(k < "val/steps_done" for k in logs)


@pytest.mark.parametrize("conn", (4, 8))
def test_coherence_host_equals_the_restatement(conn):
    _, _, E, _, _ = _mods()
    maps = [m for _, m, _ in R.patterns(19, 33)] + [R.with_invalid(R.noise(19, 33, 25, 5), 25, (-1, 25, 1 << 40), 6)]
    P, small = 25, 4
    got, invalid = E.coherence_host(np.stack(maps), P, conn, small)
    bad = 0
    for i, m in enumerate(maps):
        _, st, inv = R.stats(m, R.components_flood(m, P, conn), P, small)
        assert np.array_equal(got[i], st), i
        bad += inv
    assert invalid == bad > 0 and got.dtype == np.int32
    big, _ = E.coherence_host(R.spiral(64, 64)[None], 2, conn, 0)
    assert big[0, :, 1].tolist() == [1, 1]


def test_evaluator_host_route_and_refusals():
    _, _, E, _, _ = _mods()
    ev = E.CoherenceEvaluator(torch.device("cpu"), 300, conn=4, speck_area=3)          # P > 255: the host route, no kernel
    assert not ev.on_device
    m = R.noise(8, 8, 300, 7)
    ev.update(torch.from_numpy(np.stack([m, m, m])), valid=2)
    stats, invalid = ev.sums()
    assert stats.shape == (2, 300, 4) and invalid == 0 and ev.n == 2 and ev.HW == 64
    want, _ = E.coherence_host(np.stack([m, m]), 300, 4, 3)
    assert np.array_equal(stats, want)
    assert ev.result() == E.coherence_from_stats(want, 64)
    ev.reset()
    with pytest.raises(ValueError):
        ev.result()
    for bad in ((0, 8, 0), (3, 6, 0), (3, 8, -1)):
        with pytest.raises(ValueError):
            E.CoherenceEvaluator(torch.device("cpu"), *bad)


# ---------------------------------------------------------------------------------------------- keys
def test_metric_names():
    _, _, _, M, _ = _mods()
    assert M.VAL_METRICS == ("iou", "reconstruction", "parts", "equivariance")
    assert M.VAL_METRICS_MORE == ("coherence",)
    assert M.validation_metrics({"val_metrics": ["coherence", "parts"]}) == ["parts", "coherence"]
    assert M.validation_metrics({"eval_metrics": ["coherence"]}, "eval_metrics", ()) == ["coherence"]
    assert M.validation_metrics({}) == ["iou"]
    with pytest.raises(ValueError) as e:
        M.validation_metrics({"val_metrics": ["coherent"]})
    assert "coherence" in str(e.value) and "equivariance" in str(e.value)


def test_coherence_keys_and_refusals():
    _, _, _, M, _ = _mods()
    assert M.coherence_config({"spatial_size": 128}) == (8, 17)                        # ceil(0.001 * 128^2) = ceil(16.384)
    assert M.coherence_config({"spatial_size": 100, "val_speck_area": 0.001, "val_coherence_connectivity": 4}) == (4, 10)
    assert M.coherence_config({"spatial_size": 128, "val_speck_area": 0}) == (8, 0)
    for bad in ({"val_coherence_connectivity": 6}, {"val_coherence_connectivity": True}, {"val_speck_area": -0.1},
                {"val_speck_area": 1.5}, {"val_speck_area": "small"}):
        with pytest.raises(ValueError):
            M.coherence_config(dict(bad, spatial_size=128))
    base = {"val_freq": 10, "val_csv": "val.csv", "val_metrics": ["coherence"], "precision": "bf16", "hip_graph": False,
            "spatial_size": 128}
    M.check_validation_config(base)                                                    # no label column is needed
    for extra in ({"precision": "fp8"}, {"hip_graph": True}, {"val_csv": None}, {"val_coherence_connectivity": 5}):
        with pytest.raises(ValueError):
            M.check_validation_config(dict(base, **extra))


def test_segment_clean_keys():
    _, _, _, _, RUN = _mods()
    base = {"segment_csv": "list.csv"}
    assert "clean" not in RUN.segment_options(base) and "clean" not in RUN.segment_options(dict(base, segment_clean_min_area=0))
    assert "clean" not in RUN.segment_options(dict(base, segment_clean_min_area=0, segment_clean_rounds=3))
    assert RUN.segment_options(dict(base, segment_clean_min_area=6))["clean"] == {"min_area": 6, "rounds": 1, "connectivity": 8}
    assert RUN.segment_options(dict(base, segment_clean_min_area=6, segment_clean_rounds=4, segment_clean_connectivity=4))["clean"] == {
        "min_area": 6, "rounds": 4, "connectivity": 4}
    for bad in ({"segment_clean_min_area": -1}, {"segment_clean_min_area": 2.5}, {"segment_clean_min_area": True},
                {"segment_clean_rounds": 0}, {"segment_clean_rounds": 5}, {"segment_clean_connectivity": 6}):
        with pytest.raises(ValueError):
            RUN.segment_options(dict(base, **bad))


class _Ready(object):
    def synchronize(self):
        pass


class _OldModel(object):
    """A model whose export_segments is the one from before the clean-up existed: it takes no `clean`."""
    n_parts, device = 3, torch.device("cpu")

    def __init__(self):
        self.calls = 0

    def export_segments(self, views, sizes, sources=None, outputs=("labels",), alpha=0.5, colors=None, maps=None, after_launch=None,
                        refine=None):
        self.calls += 1
        planes = {"labels": [torch.full((h, w), i % 3, dtype=torch.uint8) for i, (h, w) in enumerate(sizes)]}
        counts = torch.zeros((len(sizes), 3), dtype=torch.int32)
        for i, (h, w) in enumerate(sizes):
            counts[i, i % 3] = h * w
        return {"views": planes, "host": {"counts": counts}, "ready": _Ready()}


def test_clean_off_takes_no_new_path(tmp_path, monkeypatch):
    """`segment_clean_min_area: 0` (and the key unset): export_segments is called exactly as before -- no `clean` argument -- and no
    component kernel wrapper is reached."""
    from PIL import Image
    _, ops, _, _, RUN = _mods()

    def refuse(*a, **k):
        raise AssertionError("a component wrapper was reached with the clean-up off")
    for name in ("label_components", "label_component_stats", "label_components_clean"):
        monkeypatch.setattr(ops, name, refuse)
    rng = np.random.RandomState(0)
    for i, (h, w) in enumerate(((9, 12), (7, 7), (16, 5))):
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(tmp_path / "im{}.png".format(i)))
    (tmp_path / "list.csv").write_text("".join("im{}.png\n".format(i) for i in range(3)))
    for extra in ({}, {"segment_clean_min_area": 0}):
        cfg = dict({"segment_csv": str(tmp_path / "list.csv"), "data_root": str(tmp_path), "spatial_size": 8, "batch_size": 2,
                    "segment_outputs": ["labels"]}, **extra)
        model = _OldModel()
        rows = RUN.segment_files(model, cfg, str(tmp_path / "out{}".format(len(extra))), 0)
        assert model.calls == 1 and [r[0] for r in rows] == ["im0.png", "im1.png", "im2.png"]
        assert os.path.isfile(str(tmp_path / "out{}".format(len(extra)) / "segment" / "0" / "labels" / "im1.png.png"))


# ---------------------------------------------------------------------------------------------- the wrapper's error path
def test_bounded_loop_flag_raises():
    """The kernels' bounded loops raise a device flag; the wrapper turns a set flag into L.UpsError (and a clear one into nothing)."""
    L, ops, _, _, _ = _mods()
    ops.components_check(torch.zeros(1, dtype=torch.int32))
    with pytest.raises(L.UpsError) as e:
        ops.components_check(torch.ones(1, dtype=torch.int32))
    assert "bound" in str(e.value)


def test_wrappers_refuse_before_the_library_is_touched():
    L, ops, _, _, _ = _mods()
    t = torch.zeros((2, 4, 4), dtype=torch.int64)
    for bad in (lambda: ops.label_components(t, 0), lambda: ops.label_components(t, 256), lambda: ops.label_components(t, True),
                lambda: ops.label_component_stats(t, t, 0), lambda: ops.label_components_clean(t, t, t, 300, 1)):
        with pytest.raises(L.UpsError):
            bad()
