"""CPU tests of the edge-aware refinement of the segmentation export: properties of the NumPy restatement (segrefine_ref.py) that the
kernels are held to, the guide's integer box means, the runner's three `segment_refine*` keys and the new entry points' declarations.
Nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest

import segexport_ref as R0
import segrefine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ups_segment_guide", "ups_segment_render_guided")


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, runner
    return lib, ops, runner


# ---------------------------------------------------------------------------------------------- the restatement
def two_tone(edge, h=32, w=32, left=(40, 60, 80), right=(200, 180, 160)):
    src = np.empty((h, w, 3), np.uint8)
    src[:, :edge] = left
    src[:, edge:] = right
    return src


def half_map(S=8):
    """One-hot: part 0 for taps tx < S / 2, part 1 otherwise."""
    soft = np.zeros((S, S, 2), np.float32)
    soft[:, :S // 2, 0] = 1.0
    soft[:, S // 2:, 1] = 1.0
    return soft


def boundary(labels):
    """The column at which every row of a label map steps from 0 to 1 (rows equal and monotone, asserted)."""
    assert (labels == labels[:1]).all(), "the rows differ"
    row = labels[0].astype(np.int64)
    assert (np.diff(row) >= 0).all() and row[0] == 0 and row[-1] == 1, row
    return int(np.argmax(row))


@pytest.mark.parametrize("edge,radii", [(18, (0, 1, 2)), (13, (1, 2))])
def test_an_image_edge_moves_the_label_boundary(edge, radii):
    soft, src, wr = half_map(), two_tone(edge), R.range_table(16.0)
    assert boundary(R0.render(soft, 32, 32)["labels"]) == 16            # the bilinear route: the map's boundary, enlarged
    for rad in radii:
        assert boundary(R.render_guided(soft, src, wr, rad)["labels"]) == edge, rad


def test_radius_zero_with_a_table_of_ones_is_the_bilinear_route_on_random_maps():
    """An observation, not a guarantee (the factoring differs): 0 differing labels and confidences in 19 x 23 from S = 8, P = 10."""
    rng = np.random.RandomState(0)
    soft = R.soft_maps(rng, 1, 8, 10)[0]
    src = rng.randint(0, 256, size=(19, 23, 3)).astype(np.uint8)
    a, b = R.render_guided(soft, src, np.ones(R.RANGE), 0), R0.render(soft, 19, 23)
    assert (a["labels"] == b["labels"]).all() and (a["confidence"] == b["confidence"]).all()


def test_denominators_stay_positive_on_noise_at_sigma_one():
    rng = np.random.RandomState(1)
    wr = R.range_table(1.0)
    assert wr[0] == 1.0 and wr.min() == R.FLOOR == 2.0 ** -64 and (np.diff(wr) <= 0).all() and wr.shape == (766,)
    lows = []
    for S, (h, w), rad in [(8, (19, 23), 1), (4, (9, 40), 3), (16, (5, 5), 0)]:
        src = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        r = R.render_guided(R.soft_maps(rng, 1, S, 3)[0], src, wr, rad)
        assert (r["den"] > 0).all() and np.isfinite(r["den"]).all()
        lows.append(r["den"].min())
    assert min(lows) < 1e-15, "no denominator came near the floor: the case tests nothing"


def test_ties_resolve_to_the_first_maximal_index_on_a_constant_source():
    S, P = 8, 6
    ties = R.soft_maps(np.random.RandomState(2), 1, S, P, "ties")[0]
    src = np.full((S, S, 3), 77, np.uint8)
    for rad in (0, 1, 3):
        r = R.render_guided(ties, src, R.range_table(16.0), rad)
        num, _ = R.refine(ties, src, r["guide"], R.range_table(16.0), rad)
        assert ((num == num.max(axis=2, keepdims=True)).sum(axis=2) >= 2).any()
        first = np.argmax(num == num.max(axis=2, keepdims=True), axis=2)
        assert (r["labels"] == first).all()
    # at the model's size with radius 0 the only tap of weight > 0 is the pixel's own: the first maximum of the map itself
    assert (R.render_guided(ties, src, R.range_table(16.0), 0)["labels"] == np.argmax(ties, axis=2)).all()


def test_range_table_is_the_packages():
    _, ops, _ = _mods()
    for sigma in (1.0, 16.0, 0.37, 200.0):
        assert (ops.segment_range_table(sigma) == R.range_table(sigma)).all()
    assert ops.segment_range_table(16.0).dtype == np.float64 and ops.SEGMENT_RANGE == R.RANGE


# ---------------------------------------------------------------------------------------------- the guide
def test_guide_of_a_constant_image_is_the_constant():
    for h, w, S in [(32, 32, 8), (5, 7, 4), (3, 50, 16), (1, 1, 4)]:
        src = np.full((h, w, 3), (7, 130, 255), np.uint8)
        assert (R.guide(src, S) == np.asarray((7, 130, 255), np.uint8)).all()


def test_guide_at_the_models_size_is_the_source():
    src = np.random.RandomState(3).randint(0, 256, size=(8, 8, 3)).astype(np.uint8)
    assert (R.guide(src, 8) == src).all()


def test_guide_ranges_are_never_empty_and_the_mean_is_rounded():
    for n, S in [(1, 4), (3, 8), (7, 8), (8, 8), (9, 8), (37, 16), (500, 128)]:
        a, b = R.tap_ranges(n, S)
        assert (b > a).all() and a[0] == 0 and b[-1] == n and (a >= 0).all() and (b <= n).all()
        if n >= S:
            assert (a[1:] == b[:-1]).all(), "the ranges partition the axis"
    src = np.random.RandomState(4).randint(0, 256, size=(3, 5, 3)).astype(np.uint8)        # h, w < S
    g = R.guide(src, 8)
    ya, _ = R.tap_ranges(3, 8)
    xa, _ = R.tap_ranges(5, 8)
    assert (g == src[ya][:, xa]).all()                                                      # every tap is one source pixel
    src = np.random.RandomState(5).randint(0, 256, size=(9, 10, 3)).astype(np.uint8)
    g = R.guide(src, 4)
    blk = src[2:4, 5:7].reshape(-1, 3).astype(np.float64)                                   # tap (1, 2): rows [2, 4), columns [5, 7)
    assert (g[1, 2] == np.floor(blk.mean(axis=0) + 0.5)).all()


# ---------------------------------------------------------------------------------------------- options and ABI
def test_segment_options_accepts_the_refine_keys():
    _, _, runner = _mods()
    base = {"segment_csv": "list.csv"}
    assert "refine" not in runner.segment_options(base)
    assert "refine" not in runner.segment_options(dict(base, segment_refine="none", segment_refine_radius=2, segment_refine_sigma=3))
    assert runner.segment_options(dict(base, segment_refine="bilateral"))["refine"] == {"radius": 1, "sigma": 16.0}
    opt = runner.segment_options(dict(base, segment_refine="bilateral", segment_refine_radius=3, segment_refine_sigma=4))
    assert opt["refine"] == {"radius": 3, "sigma": 4.0}
    assert runner.segment_options(dict(base, segment_refine="bilateral", segment_refine_radius=0))["refine"]["radius"] == 0
    for bad in ({"segment_refine": "joint"}, {"segment_refine": True}, {"segment_refine": None}, {"segment_refine_radius": -1},
                {"segment_refine_radius": 4}, {"segment_refine_radius": 1.0}, {"segment_refine_radius": True},
                {"segment_refine_radius": "1"}, {"segment_refine_sigma": 0}, {"segment_refine_sigma": -2.0},
                {"segment_refine_sigma": "16"}, {"segment_refine_sigma": float("nan")}, {"segment_refine_sigma": float("inf")},
                {"segment_refine_sigma": True}):
        with pytest.raises(ValueError, match=list(bad)[0]):
            runner.segment_options(dict(base, segment_refine="bilateral", **bad) if "segment_refine" not in bad else dict(base, **bad))
        if "segment_refine" not in bad:          # a bad value is refused also while the route is off
            with pytest.raises(ValueError):
                runner.segment_options(dict(base, **bad))


def test_library_exports_the_new_symbols():
    import ctypes as C
    lib, ops, _ = _mods()
    handle = lib.load()
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    declared = set(re.findall(r"\b(ups_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in lib.EXPORTS and name in declared and hasattr(handle, name), name
    assert lib.ABI_VERSION == 6, "the entry points are added by name, without a new ABI number"
    assert len(lib._SIGS["ups_segment_guide"][0]) == 8 and len(lib._SIGS["ups_segment_render_guided"][0]) == 18
    assert lib._SIGS["ups_segment_render_guided"][0][12] is C.c_double                       # alpha
    assert ops.SEGMENT_MAX_RADIUS == 3


def test_ops_refuses_a_bad_refine_before_touching_a_device():
    lib, ops, _ = _mods()
    with pytest.raises(lib.UpsError):
        ops.segment_range_table(0.0)
    with pytest.raises(lib.UpsError):
        ops.segment_range_table(float("nan"))
