"""GPU tests of the device-resident data path: ups_gather_views (csrc/dataset.hip, through the C ABI) bit for bit against the NumPy
restatement of devdata_ref.py, the device iterator against the host iterator, and a training run fed by it through the runner."""
import copy
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from devdata_ref import gather_ref, write_dataset

pytestmark = pytest.mark.gpu

GUARD = 64          # floats in front of and behind every output view that must stay NaN
PLAN = [[0, 6, 0], [6, 0, 1], [3, 3, 2], [2, 5, 3], [4, 1, 1]]     # all four flip combinations, i0 == i1, lowest and highest index


def _L():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    return lib


class _Out(object):
    """An output view [B,S,S,3] inside a larger NaN-filled buffer: GUARD floats in front (+ `shift`, to break the 16-byte
    alignment) and GUARD behind."""

    def __init__(self, dev, B, S, shift=0):
        n = B * S * S * 3
        self.buf = torch.full((GUARD + shift + n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD + shift:GUARD + shift + n].view(B, S, S, 3)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _gather(L, dev, store, plan, S, with_target, shift=0):
    B = len(plan)
    images = torch.from_numpy(store).to(dev)
    plan_d = torch.tensor(plan, dtype=torch.int32, device=dev)
    outs = {k: _Out(dev, B, S, shift) for k in (("view0", "view1", "view0_target") if with_target else ("view0", "view1"))}
    L.call("ups_gather_views", L.ptr(images), store.shape[0], L.ptr(plan_d), B, S, L.ptr(outs["view0"].view), L.ptr(outs["view1"].view),
           L.ptr(outs["view0_target"].view) if with_target else None, L.stream())
    torch.cuda.synchronize(dev)
    return outs


@pytest.mark.parametrize("S", [16, 10], ids=["vector", "scalar"])
def test_lut_equals_numpy_on_all_256_bytes(S, dev):
    """float(u) / 127.5f - 1.0f in the kernel against np.float32(u) / 127.5 - 1.0, bit for bit, for every byte value, in both
    forms of the kernel (16 * 16 * 3 = 768 and 10 * 10 * 3 = 300 bytes: every value occurs)."""
    L = _L()
    store = (np.arange(S * S * 3) % 256).astype(np.uint8).reshape(1, S, S, 3)
    assert len(np.unique(store)) == 256
    outs = _gather(L, dev, store, [[0, 0, 0]], S, True)
    want = torch.from_numpy(store.astype(np.float32) / 127.5 - 1.0)
    for k in ("view0", "view1", "view0_target"):
        assert torch.equal(outs[k].view.cpu(), want), k
    lut = np.arange(256, dtype=np.uint8).astype(np.float32) / 127.5 - 1.0
    assert np.array_equal(outs["view0"].view.cpu().numpy().reshape(-1)[:256].view(np.uint32), lut.view(np.uint32))


@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no_target"])
@pytest.mark.parametrize("S,shift", [(16, 0), (12, 0), (10, 0), (5, 0), (16, 1)],
                         ids=["S16_vector", "S12_vector", "S10_scalar", "S5_scalar", "S16_unaligned_scalar"])
def test_gather_equals_numpy_restatement(S, shift, with_target, dev):
    """7 random images, 5 items.  S = 16, 12: four pixels per lane; S = 10, 5: one pixel per lane (3 S is no multiple of 4); S = 16
    with outputs one float off 16-byte alignment: the launcher must fall back to one pixel per lane.  Outputs bit-equal to the
    restatement, and the 64 floats on either side of every view still NaN."""
    L = _L()
    store = np.random.RandomState(100 + S).randint(0, 256, (7, S, S, 3), dtype=np.uint8)
    ref = gather_ref(store, PLAN, with_target)
    outs = _gather(L, dev, store, PLAN, S, with_target, shift)
    assert set(outs) == set(ref)
    for k, o in outs.items():
        assert torch.equal(o.view.cpu(), torch.from_numpy(ref[k])), k
        assert o.guards_intact(), k + ": wrote outside its view"


def test_entry_point_refusals(dev):
    """B = 0, S = 0, a NULL view (and an empty store): non-zero status, nothing launched, outputs untouched."""
    L = _L()
    fn = L.load().ups_gather_views
    S, B = 8, 2
    images = torch.zeros((3, S, S, 3), dtype=torch.uint8, device=dev)
    plan = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    outs = [_Out(dev, B, S) for _ in range(3)]
    v0, v1, vt = (L.ptr(o.view) for o in outs)
    st = L.stream()
    assert fn(L.ptr(images), 3, L.ptr(plan), 0, S, v0, v1, vt, st) != 0
    assert "argument check failed" in L.load().ups_last_error().decode()
    assert fn(L.ptr(images), 3, L.ptr(plan), B, 0, v0, v1, vt, st) != 0
    assert fn(L.ptr(images), 3, L.ptr(plan), B, S, None, v1, vt, st) != 0
    assert fn(L.ptr(images), 3, L.ptr(plan), B, S, v0, None, vt, st) != 0
    assert fn(None, 3, L.ptr(plan), B, S, v0, v1, vt, st) != 0
    assert fn(L.ptr(images), 3, None, B, S, v0, v1, vt, st) != 0
    assert fn(L.ptr(images), 0, L.ptr(plan), B, S, v0, v1, vt, st) != 0
    torch.cuda.synchronize(dev)
    assert all(o.untouched() for o in outs)
    assert fn(L.ptr(images), 3, L.ptr(plan), B, S, v0, v1, None, st) == 0      # target alone may be NULL
    torch.cuda.synchronize(dev)
    assert bool((outs[0].view == -1.0).all()) and bool((outs[1].view == -1.0).all()) and outs[2].untouched()


@pytest.mark.parametrize("cls", ["AugmentedPair2", "StochasticPairs"])
def test_device_iterator_equals_host_iterator(cls, dev, tmp_path):
    """device_batches against batches(workers=1): batch 4, two epochs, both flips on -- the same number of batches, the same keys,
    torch.equal on every tensor; the device tensors are float32 on the device and fresh per batch."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import data
    cfg = write_dataset(tmp_path, n=9)           # 9 images, batch 4: one is dropped per epoch
    host = list(data.batches(getattr(data, cls)(cfg), 4, workers=1, seed=5, epochs=2))
    devb = list(data.device_batches(getattr(data, cls)(cfg), 4, dev, seed=5, epochs=2))
    assert len(host) == len(devb) == 4
    ptrs = set()
    for h, d in zip(host, devb):
        assert set(h) == set(d) == ({"view0", "view1", "view0_target"} if cls == "AugmentedPair2" else {"view0", "view1"})
        for k in h:
            assert d[k].device == dev and d[k].dtype == torch.float32 and d[k].is_contiguous()
            assert torch.equal(d[k].cpu(), h[k]), k
            ptrs.add(d[k].data_ptr())
    assert len(ptrs) == sum(len(d) for d in devb)          # (all batches are alive here: no tensor may be handed out twice)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hip_graph"])
def test_runner_trains_from_the_device_iterator(graph, dev, tmp_path):
    """The csv config of test_runner_end_to_end_with_csv_dataset_and_checkpoint with data_on_device: 3 steps, finite logged losses.
    Once more with hip_graph: True and 4 steps -- and without the in-graph TPS, with which the trainer does not capture at all: two
    eager warm-up steps, the capture, and steps 2 and 3 replayed on batches of the device iterator."""
    import yaml
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    from oracle import configs
    rng = np.random.RandomState(0)
    rows = ["character_id,relative_file_path_,foo,category"]
    for i in range(8):
        Image.fromarray(rng.randint(0, 255, (24, 24, 3), dtype=np.uint8)).save(str(tmp_path / "im{}.png".format(i)))
        rows.append("{},im{}.png,x,bird".format(i // 2, i))
    (tmp_path / "train.csv").write_text("\n".join(rows) + "\n")
    steps = 4 if graph else 3
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"dataset": "src.data.data.AugmentedPair2", "data_root": str(tmp_path), "data_csv": str(tmp_path / "train.csv"),
                "data_csv_columns": ["character_id", "relative_file_path_", "foo", "category"], "data_csv_has_header": True,
                "data_avoid_identity": False, "precision": "bf16", "vgg_widths": [8, 8, 16, 16, 16], "use_tps": not graph,
                "ckpt_freq": 2, "log_freq": 250, "num_steps": steps, "data_on_device": True, "hip_graph": graph,
                "data_cache": str(tmp_path / "cache" / "u8")})
    ypath = tmp_path / "train.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    root = tmp_path / "run"
    it = runner.main(["-t", str(ypath), "-p", str(root), "--strict-dataset"])
    assert it.global_step == steps
    assert (tmp_path / "cache" / "u8.npy").exists() and (tmp_path / "cache" / "u8.json").exists()
    if graph:
        assert it._graph_enabled and it.graph is not None and it.graph.graphs, "no step was replayed"
    log = (root / "train" / "log.txt").read_text()
    assert "SYNTHETIC" not in log
    losses = re.findall(r"\[LoggingHook\]: (loss_[a-z0-9_]+): (\S+)", log)
    assert len(losses) >= 2 * 7 and "[INFO] [LoggingHook]: global_step: 2\n" in log
    for name, value in losses:
        assert math.isfinite(float(value)), (name, value)
