"""CPU tests of the device-side augmentation's host half: augment.py's draw / build split against the draw code from before the
split, the records of data.fill_aug_plan executed in NumPy (devaug_ref.py) against AugmentedPair2.get_example, and the refusals and
acceptances of `data_augment_on_device`.  tests/test_gpu_devaug.py holds the kernels to the same executor bit for bit."""
import os
import re

import numpy as np
import pytest

import devaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("view0", "view1", "view0_target")


def _state_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_surface_is_declared_everywhere():
    A, D = R._pkg()
    from upsparts_amd import configs, lib
    assert {"ups_augment_views", "ups_augment_field", "ups_augment_record_words"} <= set(lib.EXPORTS)
    flags = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "flags.sh")).read()
    assert "augment" in re.search(r'UPS_SOURCES="([^"]*)"', flags).group(1).split()
    assert configs.DATA_AUGMENT_ON_DEVICE == {"data_augment_on_device": False}
    assert lib.load().ups_augment_record_words() == D.REC_WORDS
    src = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "augment.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    w = D.gauss_weights()
    assert w.dtype == np.float32 and w.shape == (401,) and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    luts = D.aug_luts()
    u = np.arange(256, dtype=np.uint8)
    assert luts.dtype == np.uint8 and luts.shape == (2, 256)
    # the truncating casts lose a level on some byte values (never more than one), and T_mid keeps a value it has produced
    assert 0 < int((luts[0] != u).sum()) < 128 and int((u.astype(int) - luts[0]).max()) == 1 and int((u.astype(int) - luts[0]).min()) == 0
    assert np.array_equal(luts[0], A._to_u8(u.astype(np.float32) / 127.5 - 1.0))


def test_split_draws_equal_the_draw_code_before_the_split():
    """200 seeds: appearance_ops / shape_ops (= build(draw(rng))) give the same arrays as the code from before the split and leave the
    generator in the same state; so does a bare draw_*."""
    A, _ = R._pkg()
    imgs = [np.random.RandomState(1).randint(0, 256, (16, 16, 3), dtype=np.uint8),
            np.random.RandomState(2).randint(0, 256, (12, 20, 3), dtype=np.uint8)]
    n_ops = 0
    for seed in range(200):
        for img in imgs:
            h, w = img.shape[:2]
            for new, old, draw in ((A.appearance_ops, R.appearance_ops_before, A.draw_appearance),
                                   (lambda r: A.shape_ops(r, h, w), lambda r: R.shape_ops_before(r, h, w), lambda r: A.draw_shape(r, h, w))):
                ra, rb, rc = (np.random.RandomState(seed) for _ in range(3))
                ops_new, ops_old, recs = new(ra), old(rb), draw(rc)
                assert len(ops_new) == len(ops_old) == len(recs)
                assert _state_equal(ra, rb) and _state_equal(ra, rc), seed
                a = b = img
                for f, g in zip(ops_new, ops_old):
                    a, b = f(a), g(b)
                    assert a.dtype == np.uint8 and np.array_equal(a, b), seed
                n_ops += len(recs)
    assert n_ops > 1000


def _compare_with_host(tmp_path, S, n, rounds):
    """Executor (plan + store + records) against get_example on a twin dataset, all indices `rounds` times."""
    _, D = R._pkg()
    cfg = R.write_aug_dataset(tmp_path, n, S)
    host, planned = D.AugmentedPair2(cfg), D.AugmentedPair2(cfg)
    D.check_on_device(planned)
    store = D.build_u8_store(planned)
    recs = np.zeros((3, 1, D.REC_WORDS), dtype=np.int32)
    noise = np.zeros((2, 2, S, S), dtype=np.float32)
    seen = {k: set() for k in KEYS}
    total = differing = 0
    worst = 0
    exact_examples = 0
    for _ in range(rounds):
        for i in range(n):
            ex = host.get_example(i)
            n_el = D.fill_aug_plan(planned, [i], recs, noise)
            got = R.execute(store, recs, noise, n_el)
            kinds = [R.record_kinds(recs[r, 0]) for r in range(3)]
            for k, ks in zip(KEYS, kinds):
                seen[k] |= ks
            exact = not any(ks & R.INEXACT_KINDS for ks in kinds)
            exact_examples += exact
            for k in KEYS:
                assert got[k].dtype == np.float32 and got[k].shape == (1, S, S, 3)
                if exact:
                    assert np.array_equal(got[k][0], ex[k]), (i, k, kinds)
                d = np.abs(R.levels(got[k][0]) - R.levels(ex[k]))
                total += d.size
                differing += int((d > 0).sum())
                worst = max(worst, int(d.max()))
    for k in KEYS:
        assert seen[k] == R.ALL_KINDS, (k, R.ALL_KINDS - seen[k])
    share = differing / total
    print("S = {}: {} examples, {} exact by kind, {} of {} values differ ({:.3g}), worst {} level(s)".format(
        S, rounds * n, exact_examples, differing, total, share, worst))
    assert exact_examples > 0
    assert worst <= 2, worst
    assert share <= 1e-3, share


def test_executor_against_get_example_S16(tmp_path):
    """S = 16, 240 examples, both switches on, noise and 4 x 4-block PNGs: every record kind in every view role; examples with neither
    a gray nor a warp record exactly equal; over all values no difference above 2 levels and at most 1e-3 of them differing."""
    _compare_with_host(tmp_path, 16, 10, 24)


def test_executor_against_get_example_S128(tmp_path):
    """S = 128, 60 examples: the same conditions (the radius-200 Gaussian reflects inside the image here, the bilinear warps see
    long rows)."""
    _compare_with_host(tmp_path, 128, 6, 10)


def test_fill_aug_plan_layout_and_sync(tmp_path):
    """view1 and the target share the appearance words, view0 and the target the shape words; the elastic noise of S3 is stored once;
    only the switched-on kind is drawn; an index outside the store is refused on the host."""
    _, D = R._pkg()
    cfg = R.write_aug_dataset(tmp_path, 8, 16)
    app = slice(D.REC_FILTER, D.REC_HFLIP)
    for a_on, s_on in ((True, True), (True, False), (False, True)):
        ds = D.AugmentedPair2(dict(cfg, data_augment_appearance=a_on, data_augment_shape=s_on))
        recs = np.full((3, 8, D.REC_WORDS), -1, dtype=np.int32)
        noise = np.zeros((16, 2, 16, 16), dtype=np.float32)
        n_el = 0
        for _ in range(6):
            n_el += D.fill_aug_plan(ds, range(8), recs, noise)
            assert np.array_equal(recs[1, :, app], recs[2, :, app]) and np.array_equal(recs[1, :, D.REC_BC:], recs[2, :, D.REC_BC:])
            assert np.array_equal(recs[0, :, D.REC_HFLIP:D.REC_BC], recs[2, :, D.REC_HFLIP:D.REC_BC])
            assert np.array_equal(recs[0, :, :2], recs[2, :, :2]) and (recs[:, :, D.REC_MID] == int(a_on and s_on)).all()
            if not a_on:
                assert not recs[:, :, app].any() and not recs[:, :, D.REC_BC:].any()
            if not s_on:
                assert not recs[:, :, D.REC_HFLIP:D.REC_BC].any()
        assert (n_el > 0) == s_on
    ds.labels["choices"][3] = np.array([8])
    with pytest.raises(ValueError, match="outside the store of 8 images"):
        D.fill_aug_plan(ds, [3], recs, noise)


def test_refusals_and_acceptances(tmp_path):
    """`data_augment_on_device` lifts the refusal of the two augmentation keys on an AugmentedPair2 and of nothing else; alone, or on
    another dataset, it is a ValueError naming both keys.  No device is touched."""
    _, D = R._pkg()
    from upsparts_amd import runner
    cfg = R.write_aug_dataset(tmp_path, 8, 16)
    D.check_on_device(D.AugmentedPair2(cfg))
    for key in ("data_augment_appearance", "data_augment_shape"):
        D.check_on_device(D.AugmentedPair2(dict(dict(cfg, data_augment_appearance=False, data_augment_shape=False), **{key: True})))
        with pytest.raises(ValueError, match="data_on_device.*" + key):          # the key off: today's refusal, today's message
            D.check_on_device(D.AugmentedPair2(dict(cfg, data_augment_on_device=False)))
    with pytest.raises(ValueError, match="data_on_device cannot be combined with data_gt_segmentation_column:"):
        D.check_on_device(D.AugmentedPair2(dict(cfg, data_gt_segmentation_column="foo")))
    with pytest.raises(ValueError, match=r"data_on_device_max_gb = 1e-06 GB"):
        D.check_on_device(D.AugmentedPair2(dict(cfg, data_on_device_max_gb=1e-6)))
    plain = dict(cfg, data_augment_appearance=False, data_augment_shape=False)
    with pytest.raises(ValueError, match="data_augment_on_device.*data_on_device.*StochasticPairs"):
        D.check_on_device(D.StochasticPairs(plain))
    with pytest.raises(ValueError, match="data_augment_on_device.*data_on_device"):
        D.device_batches(D.StochasticPairs(plain), 4, "cuda:0")
    for strict in (False, True):
        for name in ("src.data.data.AugmentedPair2", "eddata.stochastic_pair.StochasticPairs"):
            if name not in runner.DATA_ALIASES:
                continue
            with pytest.raises(ValueError, match="data_augment_on_device needs data_on_device"):
                runner.make_dataset(dict(cfg, dataset=name, data_on_device=False), rank=0, strict=strict, device="cuda:0")
        with pytest.raises(ValueError, match="data_augment_on_device.*data_on_device.*StochasticPairs"):
            runner.make_dataset(dict(plain, dataset="eddata.stochastic_pair.StochasticPairs"), rank=0, strict=strict, device="cuda:0")
