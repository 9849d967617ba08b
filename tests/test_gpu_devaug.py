"""GPU tests of the device-side augmentation: ups_augment_views / ups_augment_field (csrc/augment.hip, through the C ABI) bit for bit
against the NumPy executor of devaug_ref.py, the augmented route of data.device_batches against the executor and the host iterator,
the sync rules of AugmentedPair2, the entry points' refusals, and a training run fed by it through the runner."""
import copy
import math
import re

import numpy as np
import pytest
import torch

import devaug_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64          # floats in front of and behind every output view that must stay NaN
TAIL = 4096         # bytes behind the images of each scratch buffer that must keep their fill
FILL = 0xA5
KEYS = ("view0", "view1", "view0_target")


def _L():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    return lib


class _Out(object):
    """An output view [B,S,S,3] inside a larger NaN-filled buffer (as test_gpu_devdata.py's): GUARD floats in front and behind."""

    def __init__(self, dev, B, S):
        n = B * S * S * 3
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD:GUARD + n].view(B, S, S, 3)
        self.lo, self.hi = GUARD, GUARD + n

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _field(L, dev, noise):
    """ups_augment_field on noise float32 [n,2,S,S] (NumPy) -> the field tensor on the device."""
    D = R._pkg()[1]
    n, S = noise.shape[0], noise.shape[-1]
    noise_d = torch.from_numpy(np.ascontiguousarray(noise)).to(dev)
    weights = torch.from_numpy(D.gauss_weights()).to(dev)
    tmp, field = torch.full_like(noise_d, float("nan")), torch.full_like(noise_d, float("nan"))
    L.call("ups_augment_field", L.ptr(noise_d), L.ptr(weights), n, S, L.ptr(tmp), L.ptr(field), L.stream())
    return field


def _run(L, dev, store, recs, noise, n_fields):
    """ups_augment_views on records int32 [R,B,REC_WORDS] (R = 3: with a target, 2: without) -> ({key: _Out}, the two scratch
    buffers' tails intact?)."""
    D = R._pkg()[1]
    roles, B, S = recs.shape[0], recs.shape[1], store.shape[1]
    images = torch.from_numpy(store).to(dev)
    recs_d = torch.from_numpy(np.ascontiguousarray(recs)).to(dev)
    luts = torch.from_numpy(D.aug_luts()).to(dev)
    field = _field(L, dev, noise[:n_fields]) if n_fields else None
    nbytes = roles * B * S * S * 3
    scratch = [torch.full((nbytes + TAIL,), FILL, dtype=torch.uint8, device=dev) for _ in range(2)]
    outs = {k: _Out(dev, B, S) for k in KEYS[:roles]}
    L.call("ups_augment_views", L.ptr(images), store.shape[0], L.ptr(recs_d), L.ptr(luts), L.ptr(field), n_fields, B, S,
           L.ptr(scratch[0]), L.ptr(scratch[1]), L.ptr(outs["view0"].view), L.ptr(outs["view1"].view),
           L.ptr(outs["view0_target"].view) if roles == 3 else None, 7, L.stream())
    torch.cuda.synchronize(dev)
    return outs, all(bool((s[nbytes:] == FILL).all()) for s in scratch)


def _bit_equal(got, want):
    return torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))


@pytest.mark.parametrize("mid", [0, 1], ids=["one_pipeline", "both_pipelines"])
def test_all_256_bytes_through_an_op_free_pipeline(mid, dev):
    """A pipeline that is on but drew no op still casts to uint8 and back (twice when both are on): all 256 byte values equal the
    host's round trip(s) bit for bit, in every view."""
    A, D = R._pkg()
    L = _L()
    S = 16
    store = (np.arange(S * S * 3) % 256).astype(np.uint8).reshape(1, S, S, 3)
    assert len(np.unique(store)) == 256
    recs = np.zeros((3, 1, D.REC_WORDS), dtype=np.int32)
    recs[:, :, D.REC_MID] = mid
    outs, tails = _run(L, dev, store, recs, None, 0)
    want = A._from_u8(A._to_u8(store[0].astype(np.float32) / 127.5 - 1.0))
    if mid:
        want = A._from_u8(A._to_u8(want))
    assert want.dtype == np.float32 and tails
    for k in KEYS:
        assert _bit_equal(outs[k].view[0], want), k
        assert outs[k].guards_intact(), k
    assert not np.array_equal(want, store[0].astype(np.float32) / 127.5 - 1.0)       # (the round trip does lose levels)


def _hand_records(kind, B, S, rng):
    """Per item one appearance list and one shape list of hand-written records holding `kind` alone, or the full chain."""
    app, shp = [], []
    for b in range(B):
        inv = np.float32([[1.1, 0.2 - 0.1 * b, -1.5 + b], [-0.15 * b, 0.9, 0.7 * b]])
        a = {"median": [("median",)], "box": [("box",)], "gray": [("gray",)], "perm": [("perm", [(b + 1) % 3, (b + 2) % 3, b % 3])],
             "bc": [("bc", np.clip(np.arange(256) * (0.8 + 0.1 * b) + 10 * b - 20, 0, 255).astype(np.uint8))],
             "rgb": [("rgb", [20 - 10 * b, 5 * b, -20 + 7 * b])], "hsv": [("hsv", -20 + 10 * b, 30 - 15 * b, -20 + 9 * b)]}
        s = {"hflip": [("hflip",)], "affine": [("affine", inv)],
             "grid": [("grid", (rng.randn(4, 4) * 0.05 * S).astype(np.float32), (rng.randn(4, 4) * 0.05 * S).astype(np.float32))],
             "elastic": [("elastic", inv[::-1].copy() if b % 2 else inv, None, None)]}
        if kind == "chain":
            app.append(a["box" if b % 2 else "median"] + a["hsv"] + a["bc"] + a["rgb"] + a["gray"] * (b == 3) + a["perm"])
            shp.append(s["hflip"] * (b != 1) + s["affine"] + s["elastic" if b % 2 else "grid"])
        elif kind == "hsv3":
            app.append([("hsv", 7 * b - 20, 11 * b - 30, 20 - 6 * b), ("hsv", 20 - 9 * b, -30 + 13 * b, 3 * b), ("hsv", b, -b, 2 * b)])
            shp.append([])
        else:
            app.append(a.get(kind, []))
            shp.append(s.get(kind, []))
    return app, shp


@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no_target"])
@pytest.mark.parametrize("S", [16, 10, 5])
def test_hand_written_records_equal_the_executor(S, with_target, dev):
    """7 random images, B = 5 items with all four plan flips: every op kind alone, three hsv ops in a row, and the full chain with
    both round trips.  Outputs bit-equal to the executor, guard bands intact, the scratch untouched behind its 3 B (2 B) images."""
    D = R._pkg()[1]
    L = _L()
    B, roles = 5, 3 if with_target else 2
    rng = np.random.RandomState(300 + S)
    store = rng.randint(0, 256, (7, S, S, 3), dtype=np.uint8)
    store[3] = np.kron(rng.randint(0, 256, (-(-S // 4), -(-S // 4), 3), dtype=np.uint8), np.ones((4, 4, 1), np.uint8))[:S, :S]
    for kind in sorted(R.ALL_KINDS) + ["hsv3", "chain"]:
        app, shp = _hand_records(kind, B, S, rng)
        recs = np.zeros((roles, B, D.REC_WORDS), dtype=np.int32)
        noise = (rng.rand(2 * B, 2, S, S).astype(np.float32) * 2 - 1) * (30.0 if S > 5 else 5.0)      # (large: the field must move pixels)
        for b in range(B):
            recs[:, b, D.REC_SRC] = ([0, 6, 3][b % 3], [6, 3, 2, 5, 1][b], [0, 6, 3][b % 3])[:roles]
            recs[:, b, D.REC_FLIP] = b % 4
            recs[:, b, D.REC_MID] = int(kind == "chain")
            for r in range(roles):              # view1 takes its neighbour's realisations; field 2 b is item b's S3, 2 b + 1 its S4
                D.write_appearance(recs[r, b], app[b] if r != 1 else app[(b + 1) % B])
                D.write_shape(recs[r, b], shp[b] if r != 1 else shp[(b + 1) % B], 2 * b + (r == 1))
        n_fields = 2 * B if (recs[:, :, D.REC_WARP] == 2).any() else 0
        if kind in R.ALL_KINDS:
            assert all(R.record_kinds(recs[r, b]) == {kind} for r in range(roles) for b in range(B)), kind
        want = R.execute(store, recs, noise, n_fields)
        outs, tails = _run(L, dev, store, recs, noise, n_fields)
        assert set(outs) == set(want) == set(KEYS[:roles])
        for k, o in outs.items():
            assert not np.isnan(want[k]).any()
            assert _bit_equal(o.view, want[k]), (kind, k, int((o.view.cpu() != torch.from_numpy(want[k])).sum()))
            assert o.guards_intact(), (kind, k)
        assert tails, kind + ": scratch written behind its images"
        if kind in ("affine", "grid", "elastic", "median", "box", "hsv"):         # (the op is not a no-op on these inputs)
            plain = R.execute(store, np.where(np.arange(D.REC_WORDS) < D.REC_FILTER, recs, 0).astype(np.int32), noise, 0)
            assert not np.array_equal(plain["view0"], want["view0"]), kind


@pytest.mark.parametrize("S", [10, 16, 128])
def test_field_kernel_equals_the_executor(S, dev):
    """The separable Gaussian alone, 3 noise pairs: radius 200 reflects up to 20 times inside a 10-pixel image and less than twice
    inside a 128-pixel one.  Bit-equal to the float32 NumPy restatement (same tap order, no contraction)."""
    D = R._pkg()[1]
    L = _L()
    noise = np.random.RandomState(S).rand(3, 2, S, S).astype(np.float32) * 2 - 1
    want = R.gauss_field(noise, D.gauss_weights())
    got = _field(L, dev, noise)
    torch.cuda.synchronize(dev)
    assert want.dtype == np.float32 and _bit_equal(got, want)
    assert float(np.abs(want).max()) < 0.5 and float(np.abs(want).max()) > 0       # (smoothed, not copied)


def test_device_iterator_against_executor_and_host(dev, tmp_path):
    """device_batches (9 images, batch 4, two epochs, both switches): bit-equal to the executor's batches from a twin dataset's plan;
    against batches(workers=1) no value more than 2 levels off and at most 1e-3 of them differing (the bound of
    test_host_devaug.py); items whose records hold no gray and no warp bit-equal to the host; tensors fresh per batch."""
    D = R._pkg()[1]
    cfg = R.write_aug_dataset(tmp_path, 9, 16)
    host = list(D.batches(D.AugmentedPair2(cfg), 4, workers=1, seed=5, epochs=2))
    devb = list(D.device_batches(D.AugmentedPair2(cfg), 4, dev, seed=5, epochs=2))
    torch.cuda.synchronize(dev)
    twin = D.AugmentedPair2(cfg)
    store = D.build_u8_store(twin)
    rng = np.random.RandomState(5)
    assert len(host) == len(devb) == 4
    ptrs, k = set(), 0
    total = differing = exact_items = 0
    for _ in range(2):
        order = rng.permutation(9)
        for b in range(2):
            recs, noise = np.zeros((3, 4, D.REC_WORDS), dtype=np.int32), np.zeros((8, 2, 16, 16), dtype=np.float32)
            n_el = D.fill_aug_plan(twin, order[4 * b:4 * b + 4], recs, noise)
            want = R.execute(store, recs, noise, n_el)
            h, d = host[k], devb[k]
            k += 1
            assert set(h) == set(d) == set(KEYS)
            for key in KEYS:
                assert d[key].device == dev and d[key].dtype == torch.float32 and d[key].is_contiguous()
                assert _bit_equal(d[key], want[key]), key
                ptrs.add(d[key].data_ptr())
                diff = np.abs(R.levels(d[key].cpu().numpy()) - R.levels(h[key].numpy()))
                assert int(diff.max()) <= 2
                total += diff.size
                differing += int((diff > 0).sum())
            for item in range(4):
                if not any(R.record_kinds(recs[r, item]) & R.INEXACT_KINDS for r in range(3)):
                    exact_items += 1
                    for key in KEYS:
                        assert torch.equal(d[key][item].cpu(), h[key][item]), (key, item)
    assert exact_items > 0 and differing <= 1e-3 * total, (differing, total)
    assert len(ptrs) == 12          # (all batches are alive here: no tensor may be handed out twice)


def test_sync_rules(dev, tmp_path):
    """Shape only: the target is view0 (one shape realisation, no appearance).  Appearance only on single-image characters with
    data_avoid_identity False (the partner is the image itself): the target is view1 (one appearance realisation)."""
    D = R._pkg()[1]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    cfg = dict(R.write_aug_dataset(tmp_path / "a", 9, 16), data_augment_appearance=False)
    n = moved = 0
    for batch in D.device_batches(D.AugmentedPair2(cfg), 4, dev, seed=3, epochs=3):
        assert torch.equal(batch["view0_target"], batch["view0"])
        n += 1
    cfg = dict(R.write_aug_dataset(tmp_path / "b", 9, 16, singles=True), data_augment_shape=False)
    for batch in D.device_batches(D.AugmentedPair2(cfg), 4, dev, seed=3, epochs=3):
        assert torch.equal(batch["view0_target"], batch["view1"])
        moved += int(not torch.equal(batch["view0"], batch["view1"]))
        n += 1
    assert n == 12 and moved > 0        # (view0 has a realisation of its own)


def test_entry_point_refusals_and_unknown_op_code(dev):
    """B = 0, S = 0, NULL pointers, passes = 0: non-zero status, nothing launched, outputs untouched.  A record with an unknown op code,
    a source image or a field index out of range gives a NaN image and leaves the other images alone."""
    D = R._pkg()[1]
    L = _L()
    S, B = 8, 2
    images = torch.zeros((3, S, S, 3), dtype=torch.uint8, device=dev)
    recs = torch.zeros((3, B, D.REC_WORDS), dtype=torch.int32, device=dev)
    luts = torch.from_numpy(D.aug_luts()).to(dev)
    sa, sb = (torch.zeros((3 * B, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    noise = torch.zeros((1, 2, S, S), dtype=torch.float32, device=dev)
    weights = torch.from_numpy(D.gauss_weights()).to(dev)
    outs = [_Out(dev, B, S) for _ in range(3)]
    v0, v1, vt = (L.ptr(o.view) for o in outs)
    st = L.stream()
    fn, ff = L.load().ups_augment_views, L.load().ups_augment_field
    p = L.ptr
    assert fn(p(images), 3, p(recs), p(luts), None, 0, 0, S, p(sa), p(sb), v0, v1, vt, 7, st) != 0
    assert "argument check failed" in L.load().ups_last_error().decode()
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, 0, p(sa), p(sb), v0, v1, vt, 7, st) != 0
    assert fn(None, 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, vt, 7, st) != 0
    assert fn(p(images), 3, None, p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, vt, 7, st) != 0
    assert fn(p(images), 3, p(recs), None, None, 0, B, S, p(sa), p(sb), v0, v1, vt, 7, st) != 0
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, None, p(sb), v0, v1, vt, 7, st) != 0
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), None, v0, v1, vt, 7, st) != 0
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), None, v1, vt, 7, st) != 0
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, None, vt, 7, st) != 0
    assert fn(p(images), 0, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, vt, 7, st) != 0
    assert fn(p(images), 3, p(recs), p(luts), None, 1, B, S, p(sa), p(sb), v0, v1, vt, 7, st) != 0       # fields announced, none given
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, vt, 0, st) != 0
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, vt, 8, st) != 0
    assert ff(p(noise), p(weights), 0, S, p(noise), p(noise), st) != 0
    assert ff(p(noise), p(weights), 1, 0, p(noise), p(noise), st) != 0
    assert ff(None, p(weights), 1, S, p(noise), p(noise), st) != 0
    assert ff(p(noise), None, 1, S, p(noise), p(noise), st) != 0
    assert ff(p(noise), p(weights), 1, S, None, p(noise), st) != 0
    assert ff(p(noise), p(weights), 1, S, p(noise), None, st) != 0
    torch.cuda.synchronize(dev)
    assert all(o.untouched() for o in outs)
    # unknown codes: (role, item) -> (word, value); every other image is the op-free -1.0 (T_in[0] = 0)
    bad = {(0, 0): (D.REC_FILTER, 3), (1, 1): (D.REC_COLOR + 2, 4), (2, 0): (D.REC_WARP, 3), (2, 1): (D.REC_PIDX + 1, 3)}
    host = np.zeros((3, B, D.REC_WORDS), dtype=np.int32)
    for (r, b), (w, v) in bad.items():
        host[r, b, w] = v
    recs.copy_(torch.from_numpy(host))
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, vt, 7, st) == 0
    torch.cuda.synchronize(dev)
    for r in range(3):
        for b in range(B):
            img = outs[r].view[b]
            assert bool(torch.isnan(img).all()) if (r, b) in bad else bool((img == -1.0).all()), (r, b)
        assert outs[r].guards_intact()
    # a source image and a field index out of range, a negative flag; and the target may be NULL
    host[:] = 0
    host[0, 0, D.REC_SRC], host[0, 1, D.REC_SRC], host[1, 0, D.REC_WARP], host[1, 0, D.REC_FIELD], host[1, 1, D.REC_GRAY] = 3, -1, 2, 0, -1
    recs.copy_(torch.from_numpy(host))
    outs = [_Out(dev, B, S) for _ in range(3)]
    v0, v1, vt = (L.ptr(o.view) for o in outs)
    assert fn(p(images), 3, p(recs), p(luts), None, 0, B, S, p(sa), p(sb), v0, v1, None, 7, st) == 0
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(outs[0].view).all()) and bool(torch.isnan(outs[1].view).all()) and outs[2].untouched()
    assert outs[0].guards_intact() and outs[1].guards_intact()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hip_graph"])
def test_runner_trains_from_the_augmented_device_iterator(graph, dev, tmp_path):
    """The csv config of test_gpu_devdata.py's runner test with all three keys on: 3 steps eager, 4 steps with hip_graph: True and
    without the in-graph TPS (two eager warm-up steps, the capture, two replays).  Finite losses, no SYNTHETIC line."""
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
                "data_augment_on_device": True, "data_augment_appearance": True, "data_augment_shape": True})
    ypath = tmp_path / "train.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    root = tmp_path / "run"
    it = runner.main(["-t", str(ypath), "-p", str(root), "--strict-dataset"])
    assert it.global_step == steps
    if graph:
        assert it._graph_enabled and it.graph is not None and it.graph.graphs, "no step was replayed"
    log = (root / "train" / "log.txt").read_text()
    assert "SYNTHETIC" not in log
    losses = re.findall(r"\[LoggingHook\]: (loss_[a-z0-9_]+): (\S+)", log)
    assert len(losses) >= 2 * 7 and "[INFO] [LoggingHook]: global_step: 2\n" in log
    for name, value in losses:
        assert math.isfinite(float(value)), (name, value)
