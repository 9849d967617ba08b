"""CPU tests of the device-resident data path's host side (upsparts_amd.data): the uint8 store and its cache, the plan
(``plan_example``) against the examples the host path decodes, and the refusals.  The gather itself is the NumPy restatement of
devdata_ref.py here; tests/test_gpu_devdata.py holds the kernel to the same restatement."""
import os
import re

import numpy as np
import pytest
import torch

from devdata_ref import gather_ref, write_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("view0", "view1", "view0_target")


def _data():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import data
    return data


def _get_example_before(ds, i):
    """StochasticPairs / AugmentedPair2.get_example as it stood before decisions and decoding were split (no augmentations, no
    label maps): ONE generator per example, partner first, then the horizontal draw only when data_flip_h is set, then the vertical
    one only when data_flip_v is set; float32 decode, flips as array views."""
    from PIL import Image

    def decode(path):
        img = Image.open(path).convert("RGB").resize((ds.size, ds.size), Image.BILINEAR)
        return np.asarray(img, dtype=np.float32) / 127.5 - 1.0
    rng = ds._rng(i)
    j = ds.pick_partner(i, rng)
    view0, view1 = decode(ds.labels["file_path_"][i]), decode(ds.labels["file_path_"][j])
    flip_h = ds.flip_h and rng.rand() < 0.5
    flip_v = ds.flip_v and rng.rand() < 0.5
    if flip_h:
        view0, view1 = view0[:, ::-1].copy(), view1[:, ::-1].copy()
    if flip_v:
        view0, view1 = view0[::-1].copy(), view1[::-1].copy()
    return {"view0": view0, "view1": view1, "view0_target": view0.copy()}


def test_surface_is_declared_everywhere():
    """One entry point, in the header (test_host.py compares header, binding and library), the binding's table and the build's source
    list; the yaml keys have their defaults in configs.py."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import configs, lib
    assert "ups_gather_views" in lib.EXPORTS
    flags = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "flags.sh")).read()
    assert "dataset" in re.search(r'UPS_SOURCES="([^"]*)"', flags).group(1).split()
    assert configs.DATA_ON_DEVICE == {"data_on_device": False, "data_cache": None, "data_on_device_max_gb": 16}


def test_preprocess_u8_is_what_preprocess_image_normalises(tmp_path):
    data = _data()
    ds = data.AugmentedPair2(write_dataset(tmp_path))
    for path in ds.labels["file_path_"]:
        u8 = ds.preprocess_u8(path)
        assert u8.dtype == np.uint8 and u8.shape == (16, 16, 3)
        f = ds.preprocess_image(path)
        assert f.dtype == np.float32 and np.array_equal(f, u8.astype(np.float32) / 127.5 - 1.0)


@pytest.mark.parametrize("flips", [(True, True), (True, False), (False, True), (False, False)], ids=["hv", "h", "v", "none"])
def test_plan_and_store_give_the_host_examples(flips, tmp_path):
    """Three passes over all indices: get_example, its restatement from before the split, and plan_example + the uint8 store + the
    NumPy gather, each on its own dataset object (own draw counters), give the same arrays -- so the draws come in the same order
    whichever flips are configured."""
    data = _data()
    cfg = dict(write_dataset(tmp_path), data_flip_h=flips[0], data_flip_v=flips[1])
    host, before, planned = data.AugmentedPair2(cfg), data.AugmentedPair2(cfg), data.AugmentedPair2(cfg)
    store = data.build_u8_store(planned)
    assert store.dtype == np.uint8 and store.shape == (8, 16, 16, 3)
    seen = set()
    for _ in range(3):
        for i in range(len(host)):
            ex, old = host.get_example(i), _get_example_before(before, i)
            i0, j, fh, fv = planned.plan_example(i)
            assert i0 == i and planned.labels["character_id"][j] == planned.labels["character_id"][i] and j != i
            assert (flips[0] or not fh) and (flips[1] or not fv)
            seen.add((fh, fv))
            ref = gather_ref(store, [[i0, j, int(fh) | (int(fv) << 1)]])
            assert set(ex) == set(KEYS)
            for k in KEYS:
                assert ex[k].dtype == np.float32
                assert np.array_equal(ex[k], old[k]), (i, k, "get_example changed")
                assert np.array_equal(ex[k], ref[k][0]), (i, k, "plan + store + gather")
    assert seen == {(h, v) for h in ((False, True) if flips[0] else (False,)) for v in ((False, True) if flips[1] else (False,))}


def test_batches_yield_the_examples_drawn_directly(tmp_path):
    """batches(workers=1): the permutation of RandomState(seed) per epoch, the ragged last batch dropped, get_example per index in
    order -- the tensors of the examples drawn directly (by the restatement from before the split) on a second dataset object."""
    data = _data()
    cfg = write_dataset(tmp_path, n=7)            # 7 images, batch 3: one image per epoch is dropped
    a, b = data.AugmentedPair2(cfg), data.AugmentedPair2(cfg)
    got = list(data.batches(a, 3, workers=1, seed=5, epochs=2))
    rng = np.random.RandomState(5)
    want = []
    for _ in range(2):
        order = rng.permutation(7)
        for k in range(2):
            exs = [_get_example_before(b, i) for i in order[3 * k:3 * k + 3]]
            want.append({key: torch.from_numpy(np.stack([e[key] for e in exs])) for key in KEYS})
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert set(g) == set(KEYS)
        for k in KEYS:
            assert g[k].dtype == torch.float32 and g[k].shape == (3, 16, 16, 3) and torch.equal(g[k], w[k])


def test_fill_plan_layout_and_index_check(tmp_path):
    data = _data()
    cfg = write_dataset(tmp_path)
    ds, twin = data.StochasticPairs(cfg), data.StochasticPairs(cfg)
    plan = np.full((4, 3), -7, dtype=np.int32)
    data.fill_plan(ds, [5, 0, 7, 2], plan)
    for row, i in zip(plan, [5, 0, 7, 2]):
        i0, j, fh, fv = twin.plan_example(i)
        assert list(row) == [i0, j, int(fh) | 2 * int(fv)]
    ds.labels["choices"][3] = np.array([8])       # a partner beyond the store: refused on the host, before anything is copied
    with pytest.raises(ValueError, match="outside the store of 8 images"):
        data.fill_plan(ds, [3], plan)


def test_store_cache(tmp_path, monkeypatch):
    """data_cache: <path>.npy + <path>.json {N, spatial_size, sha1 of the path column}.  A matching cache is loaded without opening
    an image (the PNGs are deleted first); another csv or another spatial_size rebuilds."""
    import hashlib
    import json
    data = _data()
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    cfg = write_dataset(imgs)
    cache = str(tmp_path / "cache" / "store")
    decoded = []
    orig = data.StochasticPairs.preprocess_u8
    monkeypatch.setattr(data.StochasticPairs, "preprocess_u8", lambda self, path: decoded.append(path) or orig(self, path))

    def build(c):
        del decoded[:]
        return data.build_u8_store(data.AugmentedPair2(c), cache=cache, workers=64), len(decoded)
    first, n = build(cfg)
    assert n == 8 and os.path.exists(cache + ".npy")
    side = json.load(open(cache + ".json"))
    paths = "\n".join("im{}.png".format(i) for i in range(8))
    assert side == {"N": 8, "spatial_size": 16, "sha1": hashlib.sha1(paths.encode()).hexdigest()}
    again, n = build(cfg)
    assert n == 0 and np.array_equal(again, first)
    other, n = build(dict(cfg, spatial_size=12))                  # another size: rebuilt, and the sidecar now says 12
    assert n == 8 and other.shape == (8, 12, 12, 3) and json.load(open(cache + ".json"))["spatial_size"] == 12
    back, n = build(cfg)
    assert n == 8 and np.array_equal(back, first)
    rows = (imgs / "train.csv").read_text().splitlines()
    (imgs / "short.csv").write_text("\n".join(rows[:1] + rows[2:]) + "\n")          # another csv: the first image is gone
    short, n = build(dict(cfg, data_csv=str(imgs / "short.csv")))
    assert n == 7 and np.array_equal(short, first[1:])
    (imgs / "swapped.csv").write_text("\n".join(rows[:1] + [rows[2], rows[1]] + rows[3:]) + "\n")   # same rows, another order
    swapped, n = build(dict(cfg, data_csv=str(imgs / "swapped.csv")))
    assert n == 8 and np.array_equal(swapped[0], first[1]) and np.array_equal(swapped[1], first[0])
    back, n = build(cfg)
    assert n == 8
    for i in range(8):
        os.remove(str(imgs / "im{}.png".format(i)))
    cached, n = build(cfg)
    assert n == 0 and np.array_equal(cached, first)
    with pytest.raises(FileNotFoundError):                        # a cache that does not match is never used
        build(dict(cfg, spatial_size=12))
    np.save(cache + ".npy", first[:5])                            # an array that is not what the sidecar describes: rebuilt (and the images are gone)
    with open(cache + ".json", "w") as f:
        json.dump(side, f)
    with pytest.raises(FileNotFoundError):
        build(cfg)


def test_store_workers_are_capped():
    data = _data()
    assert data.MAX_STORE_WORKERS == 16
    src = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "data.py")).read()
    assert "cpu_count" not in src


def test_refusals(tmp_path):
    """data_on_device together with a host-only transform, or with a store above data_on_device_max_gb: ValueError at
    construction, naming the keys / both numbers -- before a device is touched (this test has none)."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    data = _data()
    cfg = write_dataset(tmp_path)
    for key in ("data_augment_appearance", "data_augment_shape"):
        with pytest.raises(ValueError, match="data_on_device.*" + key):
            data.device_batches(data.AugmentedPair2(dict(cfg, **{key: True})), 4, "cuda:0")
    with pytest.raises(ValueError, match=r"6\.144e-06 GB.*data_on_device_max_gb = 1e-06 GB"):      # 8 * 16 * 16 * 3 = 6 144 bytes
        data.device_batches(data.AugmentedPair2(dict(cfg, data_on_device_max_gb=1e-6)), 4, "cuda:0")
    data.check_on_device(data.AugmentedPair2(cfg))                # default limit (16 GB): nothing to refuse
    # through the runner: a ValueError is not "the data is not there" -- no synthetic fall-back, strict or not
    ycfg = dict(cfg, dataset="src.data.data.AugmentedPair2", data_on_device=True, data_augment_shape=True)
    for strict in (False, True):
        with pytest.raises(ValueError, match="data_augment_shape"):
            runner.make_dataset(ycfg, rank=0, strict=strict, device="cuda:0")
    # ... and a csv that is not there still is (the store is never reached)
    gone = dict(cfg, dataset="src.data.data.AugmentedPair2", data_on_device=True, data_csv=str(tmp_path / "nope.csv"))
    ds, why = runner.make_dataset(gone, rank=0, strict=False, device="cuda:0")
    assert isinstance(ds, runner.SyntheticPairs) and "FileNotFoundError" in why
    with pytest.raises(FileNotFoundError):
        runner.make_dataset(gone, rank=0, strict=True, device="cuda:0")
