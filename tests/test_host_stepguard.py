"""Host tests of the guarded optimizer step: the NumPy restatement (stepguard_ref.py) against independent formulas -- its fixed-order sum
against math.fsum of the exact squares, the non-finite count, the clip scale, the record's transitions -- the config validation (no
GPU) and the header's declarations."""
import math
import os
import re

import numpy as np
import pytest

import stepguard_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("count", [1, 255, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 10 * R.CHUNK + 3, 300 * R.CHUNK + 17])
@pytest.mark.parametrize("mag", [1e-20, 1.0, 1e18])
def test_fixed_order_sum_against_fsum(count, mag):
    """Every addition of non-negative terms loses at most 2^-53 relative, and a term passes through min(count - 1, 8 + 10 + chunks / 256
    + 8) of them (a lone element through none that rounds): |sum - exact| <= count 2^-52 |exact| with room to spare.  The exact sum:
    math.fsum of the squares, which are exact in fp64."""
    rng = np.random.RandomState(count % 9973)
    x = (rng.standard_normal(count) * mag).astype(np.float32)
    exact = math.fsum(float(v) * float(v) for v in x.astype(np.float64))
    got = float(R.sumsq(x))
    assert abs(got - exact) <= count * 2.0 ** -52 * exact
    assert R.chunk_partials(x).size == (count + R.CHUNK - 1) // R.CHUNK


def test_sum_is_exact_on_integers_and_empty():
    x = np.arange(1, 3 * R.CHUNK + 5, dtype=np.float32) % 97
    assert float(R.sumsq(x)) == float(np.sum((x.astype(np.int64)) ** 2))
    assert float(R.sumsq(np.zeros(0, np.float32))) == 0.0
    r = R.grad_guard(np.zeros(0, np.float32), 1.0, 2.0, True)
    assert (r["skip"], float(r["scale"]), float(r["norm"])) == (0, 1.0, 0.0)


def test_nonfinite_count():
    den = np.array([1, 0x7fffff, 0x80000001], dtype=np.uint32).view(np.float32)          # denormals: finite
    x = np.concatenate([np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.4e38, -1e-38], np.float32), den,
                        np.array([0xffc00001, 0x7f800001], dtype=np.uint32).view(np.float32)])  # a negative quiet and a signalling NaN
    assert R.nonfinite_count(x) == 5
    assert R.nonfinite_count(den) == 0
    assert R.nonfinite_count(np.zeros(0, np.float32)) == 0


def test_clip_scale_below_at_and_above():
    assert R.clip_scale(0.5, 2.0) == np.float32(1.0)
    assert R.clip_scale(2.0, 2.0) == np.float32(1.0)
    assert R.clip_scale(8.0, 2.0) == np.float32(0.25)
    assert R.clip_scale(3.0, 2.0) == np.float32(2.0 / 3.0)
    assert R.clip_scale(0.0, 2.0) == np.float32(1.0)
    assert R.clip_scale(1e300, 0.0) == np.float32(1.0)           # clipping off
    assert R.clip_scale(np.inf, 2.0) == np.float32(0.0)
    assert np.isnan(R.clip_scale(np.nan, 2.0))
    assert R.clip_scale(np.nan, 0.0) == np.float32(1.0)


def test_record_transitions():
    clean = np.ones(10, np.float32)
    bad = clean.copy()
    bad[3] = np.nan
    r = R.grad_guard(bad, 1.0, 0.0, True)
    assert (r["skip"], r["consecutive"], r["skipped"], r["clipped"], r["nonfinite"]) == (1, 1, 1, 0, 1)
    r = R.grad_guard(clean, 1.0, 0.0, True, r)
    assert (r["skip"], r["consecutive"], r["skipped"], r["clipped"]) == (0, 0, 1, 0)
    r = R.grad_guard(bad, 1.0, 0.0, True, r)
    assert (r["skip"], r["consecutive"], r["skipped"]) == (1, 1, 2)
    r = R.grad_guard(bad, 1.0, 0.0, True, r)
    assert (r["consecutive"], r["skipped"]) == (2, 3)
    r = R.grad_guard(clean, 0.5, 1.0, True, r)                   # norm = sqrt(10) / 2 > 1: clipped
    assert (r["skip"], r["consecutive"], r["skipped"], r["clipped"]) == (0, 0, 3, 1)
    assert float(r["norm"]) == math.sqrt(10.0) * 0.5 and r["scale"] == np.float32(1.0 / (math.sqrt(10.0) * 0.5))
    r = R.grad_guard(bad, 1.0, 1.0, False, r)                    # skip_nonfinite off: nothing is skipped, the formulas run on NaN
    assert (r["skip"], r["consecutive"], r["nonfinite"]) == (0, 0, 1) and np.isnan(r["norm"]) and np.isnan(r["scale"])
    assert R.state_guard(np.array([0, 1, 2, np.inf, 4, 5], np.float32), (3, 1)) == (True, (4, 2))
    assert R.state_guard(np.arange(6, dtype=np.float32), (3, 1)) == (False, (3, 0))


def test_config_validation_needs_no_gpu():
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import step_guard_config
    assert step_guard_config({}) == (0.0, False, 10)
    assert step_guard_config({"grad_clip_norm": 2, "skip_nonfinite": True, "nonfinite_max_consecutive": 1}) == (2.0, True, 1)
    for bad in ({"grad_clip_norm": -1.0}, {"grad_clip_norm": float("nan")}, {"grad_clip_norm": "1"}, {"nonfinite_max_consecutive": 0},
                {"nonfinite_max_consecutive": -3}, {"nonfinite_max_consecutive": 2.5}, {"skip_nonfinite": "yes"}):
        with pytest.raises(ValueError):
            step_guard_config(bad)


def test_header_and_binding_declare_the_entry_points():
    import ctypes as C
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    for name in ("ups_step_guard_bytes", "ups_grad_guard_chunk", "ups_grad_guard_scratch_bytes", "ups_grad_guard", "ups_adam_guarded",
                 "ups_state_update_guarded"):
        assert re.search(r"\b{}\s*\(".format(name), hdr), name
        assert name in lib._SIGS, name
    assert "typedef struct ups_step_guard" in hdr
    assert C.sizeof(lib.StepGuard) == R.RECORD_BYTES
    handle = lib.load()
    assert handle.ups_step_guard_bytes() == R.RECORD_BYTES
    assert handle.ups_grad_guard_chunk() == R.CHUNK
    nc = lambda n: (n + R.CHUNK - 1) // R.CHUNK
    for n in (0, 1, R.CHUNK, R.CHUNK + 1, 14313472):
        assert handle.ups_grad_guard_scratch_bytes(n) >= nc(n) * 12 and handle.ups_grad_guard_scratch_bytes(n) % 8 == 0
    assert handle.ups_grad_guard_scratch_bytes(-1) == 0
