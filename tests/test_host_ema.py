"""Host tests of the weight EMA: the NumPy restatement (ema_ref.py) against what its definition implies, the config validation and the
checkpoint refusals (no GPU), the TensorFlow bundle's shadow names, and the header's declarations."""
import math
import os
import re

import numpy as np
import pytest

import ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import model
    return model


def test_warmup_rule_crosses_over_at_eight_updates():
    """decay 0.5 with warm-up: (1 + n) / (10 + n) for n = 0 .. 7, then 0.5 ((1 + 8) / (10 + 8) is exactly 0.5)."""
    for n in range(8):
        assert R.effective_decay(0.5, True, n) == (1.0 + n) / (10.0 + n) < 0.5
        assert R.one_minus_decay(0.5, True, n) == np.float32(1.0 - (1.0 + n) / (10.0 + n))
    for n in (8, 9, 100, 10 ** 9):
        assert R.effective_decay(0.5, True, n) == 0.5
    assert all(R.effective_decay(0.5, False, n) == 0.5 for n in range(12))
    assert R.effective_decay(0.0, True, 5) == 0.0 and R.one_minus_decay(0.0, True, 5) == np.float32(1.0)


def test_shadow_converges_to_a_constant_weight():
    rng = np.random.RandomState(3)
    w = rng.standard_normal(1000).astype(np.float32)
    s, n = np.zeros_like(w), 0
    for _ in range(80):
        s, n = R.update(s, w, 0.5, False, n)
    # the distance halves per update until it is one ulp: half an ulp off s then rounds to even, which may be s itself
    assert n == 80 and bool(np.all(np.abs(s - w) <= np.spacing(np.abs(w))))
    s_next, _ = R.update(s, w, 0.5, False, n)
    assert np.array_equal(R.bits(s_next), R.bits(s))          # a fixed point
    # one update by hand: s - (s - w) * (1 - d)
    s1, n1 = R.update(np.float32([2.0]), np.float32([1.0]), 0.75, False, 0)
    assert n1 == 1 and s1[0] == np.float32(1.75)
    # decay 0: the shadow IS the weight after one update whenever s - (s - w) is exact
    s2, _ = R.update(np.float32([4.0]), np.float32([3.0]), 0.0, False, 0)
    assert s2[0] == np.float32(3.0)


def test_a_skipped_update_leaves_shadow_and_count():
    s = np.array([1.0, np.nan, -0.0, np.inf, 1e-45], dtype=np.float32)
    w = np.full(5, np.nan, dtype=np.float32)
    out, n = R.update(s, w, 0.9, True, 7, skip=True)
    assert n == 7 and np.array_equal(R.bits(out), R.bits(s)) and out is not s


def test_canon_maps_every_nan_to_one_and_nothing_else():
    x = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345, 0x7f800000, 0xff800000, 0, 0x80000000, 1], dtype=np.uint32)
    got = R.canon(x.view(np.float32))
    assert got.tolist() == [0x7fc00000] * 4 + x[4:].tolist()


@pytest.mark.parametrize("bad", [1.0, -0.1, float("nan"), 1.5, "0.5", True])
def test_ema_decay_outside_the_half_open_interval_is_refused(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        _model().ema_config({"ema_decay": bad})


def test_ema_config_defaults_and_refusals():
    M = _model()
    assert M.ema_config({}) == (0.0, True, False, False)
    assert M.ema_config({"ema_decay": 0.999, "ema_warmup": False, "val_use_ema": True, "use_ema": True}) == (0.999, False, True, True)
    assert M.ema_config({"ema_decay": 0}) [0] == 0.0
    with pytest.raises(ValueError, match="ema_foo"):
        M.ema_config({"ema_decay": 0.5, "ema_foo": 1})
    with pytest.raises(ValueError, match="ema_start"):
        M.ema_config({"ema_start": 100})
    with pytest.raises(ValueError, match="ema_warmup"):
        M.ema_config({"ema_decay": 0.5, "ema_warmup": 1})
    with pytest.raises(ValueError, match="val_use_ema"):
        M.ema_config({"val_use_ema": True})
    with pytest.raises(ValueError, match="use_ema"):
        M.ema_config({"use_ema": "yes"})


def test_unknown_ema_key_is_refused_before_the_model_is_built():
    """TrainModel checks the keys first: the refusal needs no device."""
    M = _model()
    with pytest.raises(ValueError, match="ema_foo"):
        M.TrainModel({"ema_foo": 1})


def test_use_ema_needs_a_checkpoint_with_shadows():
    M = _model()
    with pytest.raises(ValueError, match="holds no shadow weights"):
        M.checkpoint_shadows({"params": {}, "global_step": 3}, True, "model.ckpt-3")
    with pytest.raises(ValueError, match="holds no shadow weights"):
        M.checkpoint_shadows({"params": {}, "ema": {"params": {}, "n": {}}}, True, "model.ckpt-3")
    assert M.checkpoint_shadows({"params": {}}, False, "x") is None
    ema = {"params": {"a/V": np.zeros(2, np.float32)}, "n": {"a": 1}}
    assert M.checkpoint_shadows({"ema": ema}, True, "x") is ema and M.checkpoint_shadows({"ema": ema}, False, "x") is ema


def test_validate_runs_inside_the_scope_under_val_use_ema():
    """`val_use_ema`: the metrics are computed between the swap in and the swap out; without the key no swap happens."""
    import contextlib
    M = _model()

    class Stub(object):
        _val = {"metrics": []}

        def __init__(self, use):
            self.val_use_ema, self.events = use, []

        @contextlib.contextmanager
        def ema_weights(self):
            self.events.append("in")
            yield self
            self.events.append("out")

        def _validate(self):
            self.events.append("validate")
            return {"val/steps_done": 4}

    on, off = Stub(True), Stub(False)
    assert M.Trainer.validate(on) == {"val/steps_done": 4} and on.events == ["in", "validate", "out"]
    assert M.Trainer.validate(off) == {"val/steps_done": 4} and off.events == ["validate"]


def test_bundle_round_trip_with_shadow_names(tmp_path):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import tfckpt
    rng = np.random.RandomState(5)
    v = rng.standard_normal((3, 3, 2, 4)).astype(np.float32)
    sh = rng.standard_normal((3, 3, 2, 4)).astype(np.float32)
    plain = {"x/V": v, "x/V/Adam": v * 2, "x/V/Adam_1": v * v, "global_step": np.asarray(7, dtype=np.int64),
             "Variable": np.asarray(1.5, dtype=np.float32)}
    with_ema = dict(plain)
    with_ema["x/V/ExponentialMovingAverage"] = sh
    tfckpt.write_bundle(str(tmp_path / "a.ckpt-7"), with_ema)
    tfckpt.write_bundle(str(tmp_path / "b.ckpt-7"), plain)
    got = tfckpt.read_bundle(str(tmp_path / "a.ckpt-7"))
    assert sorted(got) == sorted(with_ema)
    assert np.array_equal(R.bits(got["x/V/ExponentialMovingAverage"]), R.bits(sh)) and np.array_equal(R.bits(got["x/V"]), R.bits(v))
    params, m, vv, other = tfckpt.to_trainer_state(got)
    assert sorted(params) == ["x/V"] and sorted(m) == ["x/V"] and sorted(vv) == ["x/V"]
    shadows = tfckpt.pop_shadows(other)
    assert sorted(shadows) == ["x/V"] and np.array_equal(R.bits(shadows["x/V"]), R.bits(sh))
    assert sorted(other) == ["Variable", "global_step"]
    # a bundle without shadow names: to_trainer_state's results are what they were, and there is nothing to take out
    p2, m2, v2, o2 = tfckpt.to_trainer_state(tfckpt.read_bundle(str(tmp_path / "b.ckpt-7")))
    assert sorted(p2) == ["x/V"] and sorted(m2) == ["x/V"] and sorted(v2) == ["x/V"] and sorted(o2) == ["Variable", "global_step"]
    assert np.array_equal(p2["x/V"], v) and np.array_equal(m2["x/V"], v * 2) and np.array_equal(v2["x/V"], v * v)
    assert tfckpt.pop_shadows(o2) == {} and sorted(o2) == ["Variable", "global_step"]


def test_header_binding_and_build_list_name_the_entries():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    text = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    for name in ("ups_ema_item_bytes", "ups_ema_update", "ups_ema_swap"):
        assert re.search(r"\b{}\(".format(name), text), name
        assert name in lib.EXPORTS
    assert re.search(r"#define\s+UPS_EMA_MAX_ITEMS\s+16\b", text) and lib.EMA_MAX_ITEMS == 16
    import ctypes
    assert ctypes.sizeof(lib.EmaItem) == 32
    flags = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "flags.sh")).read()
    assert re.search(r'UPS_SOURCES="[^"]*\bema\b', flags)
    assert math.isfinite(lib.ABI_VERSION) and "UPS_ABI_VERSION {}".format(lib.ABI_VERSION) in text
