"""What the device-resident data path (yaml `data_on_device`; data.device_batches + csrc/dataset.hip) costs and buys.

The tool writes its OWN dataset into a temporary directory: `--images` (512) PNG files of 375 x 500, smooth content plus noise, three
per character_id.  SYNTHETIC PNGs ARE NOT CUB JPEGs: decoding cost, and so every host-fed figure below, depends on the files; the
device-fed figures do not.

(a) kernel   event time of ups_gather_views at (B, S) = (64, 128) and (16, 256), view0 + view1 + target: microseconds per launch, the
             minimum of `--repeats` readings of `--iters` launches (all readings are printed).  Output sets rotate over more than the
             Infinity Cache (`--sets-mib`, as tools/hbm_roofline.py does) and the plans draw from a store larger than it, so that the
             bytes come from and go to HBM; bytes moved (uint8 in, fp32 out, the plan) over time as a fraction of 8 TB/s.
(b) batches  batches per second of data.batches (8 decoding threads, the default) against data.device_batches alone, at batch 64 and
             128 x 128, nothing consuming them; the one-off cost of building the store is reported beside it.
(c) training images per second of Trainer.iterate on the CUB 128 x 128 config at batch 64, bf16, `--repeats` alternated readings each,
             fed by the host iterator, by the device iterator, and by ONE fixed device-resident batch (the ceiling: what bench.py
             measures).  Every reading goes through the same iterate() -- its logging steps synchronise in all three alike.
Prints one JSON line per row.

    python tools/bench_data.py [--images 512] [--repeats 3] [--skip-model] > profiles/bench_data.jsonl

`--augment` measures the device-side augmentation instead (yaml `data_augment_on_device`; csrc/augment.hip), with the same PNGs and
rules, and its rows are APPENDED to the file:
(d) aug_kernel    event time per launch of each of the three passes of ups_augment_views and of ups_augment_field at (B, S) = (64, 128)
                  and (16, 256): records drawn by data.fill_aug_plan with both switches on (the mix of ops a training batch has),
                  rotating record / output sets;
(e) aug_plan      host time of data.fill_aug_plan per batch (it runs in the iterator's thread);
(f) aug_batches   batches per second of data.batches (8 workers) with both switches on -- the only route without the switch --
                  against data.device_batches' augmented route;
(g) aug_training  Trainer.iterate img/s at batch 64, bf16, alternated readings, fed by the host iterator with augmentation, the device
                  iterator with augmentation and the device iterator without.

    python tools/bench_data.py --augment [--images 512] [--repeats 3] [--skip-model] >> profiles/bench_data.jsonl
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
NOTE = "synthetic PNGs (375x500, smooth + noise), not CUB JPEGs: host-fed figures depend on the files"


def emit(row):
    print(json.dumps(row), flush=True)


def write_pngs(root, n):
    import concurrent.futures as cf
    from PIL import Image
    yy, xx = np.mgrid[0:375, 0:500].astype(np.float32)

    def one(i):
        rng = np.random.RandomState(i)
        f = rng.uniform(0.005, 0.03, 6)
        smooth = np.stack([np.sin(f[2 * c] * xx + i) * np.cos(f[2 * c + 1] * yy) for c in range(3)], -1) * 90 + 128
        img = np.clip(smooth + rng.normal(0, 12, smooth.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "im{:04}.png".format(i)), compress_level=1)
    with cf.ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(one, range(n)))
    rows = ["character_id,relative_file_path_"] + ["{},im{:04}.png".format(i // 3, i) for i in range(n)]
    with open(os.path.join(root, "train.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    return {"data_root": root, "data_csv": os.path.join(root, "train.csv"), "data_csv_has_header": True,
            "data_csv_columns": ["character_id", "relative_file_path_"], "data_avoid_identity": True, "data_flip_h": True}


def kernel_rows(iters, repeats, sets_mib, store_mib):
    from upsparts_amd import lib as L
    dev = torch.device("cuda:0")
    for B, S in ((64, 128), (16, 256)):
        img_bytes = S * S * 3
        N = max(B, store_mib * (1 << 20) // img_bytes)
        g = torch.Generator(device=dev).manual_seed(S)
        store = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
        out_bytes = 3 * B * img_bytes * 4
        nsets = max(3, -(-sets_mib * (1 << 20) // out_bytes))
        sets = []
        for k in range(nsets):
            plan = torch.stack([torch.randint(0, N, (B,), generator=g, device=dev), torch.randint(0, N, (B,), generator=g, device=dev),
                                torch.randint(0, 4, (B,), generator=g, device=dev)], 1).to(torch.int32).contiguous()
            sets.append((plan, [torch.empty((B, S, S, 3), dtype=torch.float32, device=dev) for _ in range(3)]))

        def launch(k):
            plan, (v0, v1, vt) = sets[k % nsets]
            L.call("ups_gather_views", L.ptr(store), N, L.ptr(plan), B, S, L.ptr(v0), L.ptr(v1), L.ptr(vt), L.stream())
        for k in range(nsets):
            launch(k)
        torch.cuda.synchronize()
        n = max(iters, 2 * nsets)
        ts = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n):
                launch(k)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / n)
        moved = 2 * B * img_bytes + out_bytes + B * 12
        emit({"row": "kernel", "launch": "ups_gather_views view0+view1+target", "B": B, "S": S, "store_images": N,
              "store_MB": round(N * img_bytes / 1e6, 1), "output_sets": nsets, "output_sets_MB": round(nsets * out_bytes / 1e6, 1),
              "launches_per_reading": n, "bytes_moved": moved, "us": round(min(ts), 2), "us_all": [round(t, 2) for t in ts],
              "GBps": round(moved / min(ts) * 1e-3, 1), "fraction_of_8TBs": round(moved / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4)})
        del sets, store
        torch.cuda.empty_cache()


def batch_rows(dcfg, repeats, n_host, n_dev):
    from upsparts_amd import data
    dev = torch.device("cuda:0")
    cfg = dict(dcfg, spatial_size=128, batch_size=64)
    t0 = time.perf_counter()
    store = data.build_u8_store(data.AugmentedPair2(cfg))
    build_s = time.perf_counter() - t0
    emit({"row": "store", "images": int(store.shape[0]), "spatial_size": 128, "store_MB": round(store.nbytes / 1e6, 2),
          "build_s": round(build_s, 2), "images_per_s": round(store.shape[0] / build_s, 1), "decode_threads": 8, "note": NOTE})
    host, devr = [], []
    for _ in range(repeats):
        it = data.batches(data.AugmentedPair2(cfg), 64)
        next(it)
        t0 = time.perf_counter()
        for _ in range(n_host):
            next(it)
        host.append(n_host / (time.perf_counter() - t0))
        del it
    it = data.device_batches(data.AugmentedPair2(cfg), 64, dev)
    for _ in range(8):
        next(it)
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_dev):
            next(it)
        torch.cuda.synchronize()
        devr.append(n_dev / (time.perf_counter() - t0))
    emit({"row": "batches", "B": 64, "S": 128, "host_batches_per_s": round(max(host), 2), "host_all": [round(v, 2) for v in host],
          "host_workers": 8, "host_batches_per_reading": n_host, "device_batches_per_s": round(max(devr), 1),
          "device_all": [round(v, 1) for v in devr], "device_batches_per_reading": n_dev,
          "device_ms_per_batch": round(1e3 / max(devr), 3), "note": NOTE})


def training_rows(dcfg, repeats, steps_host, steps_dev):
    from upsparts_amd import configs, data
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    B, S = 64, 128
    cfg = configs.BENCH_CONFIGS["cub128p10"][0](B)
    cfg["precision"] = "bf16"
    cfg.update(dcfg)
    model = TrainModel(cfg, device=dev, seed=0)
    tr = Trainer(cfg, None, model)
    g = torch.Generator().manual_seed(1234)
    fixed = {k: (torch.rand(B, S, S, 3, generator=g) * 2 - 1).to(dev) for k in ("view0", "view1", "view0_target")}
    feeds = {"host": (data.batches(data.AugmentedPair2(cfg), B), steps_host),
             "device": (data.device_batches(data.AugmentedPair2(cfg), B, dev), steps_dev),
             "fixed": (itertools.repeat(fixed), steps_dev)}
    quiet = lambda line: None
    tr.iterate(itertools.islice(itertools.repeat(fixed), 8), num_steps=tr.global_step + 8, log_fn=quiet)          # warm-up
    rates = {k: [] for k in feeds}
    for _ in range(repeats):
        for name, (it, n) in feeds.items():                  # alternated: host, device, fixed, host, ...
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.iterate(itertools.islice(it, n), num_steps=tr.global_step + n, log_fn=quiet)   # (islice: exactly n batches are drawn)
            torch.cuda.synchronize()
            rates[name].append(n * B / (time.perf_counter() - t0))
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    spread = {k: max(v) - min(v) for k, v in rates.items()}
    row = {"row": "training", "config": "cub128p10", "B": B, "S": S, "precision": "bf16",
           "steps_per_reading": {k: n for k, (_, n) in feeds.items()}}
    for k in feeds:
        row[k + "_img_per_s"] = round(mean[k], 1)
        row[k + "_all"] = [round(v, 1) for v in rates[k]]
        row[k + "_spread"] = round(spread[k], 1)
        row[k + "_ms_per_step"] = round(1e3 * B / mean[k], 2)
    row["device_minus_host"] = round(mean["device"] - mean["host"], 1)
    row["device_not_below_host_by_more_than_spread"] = bool(mean["device"] >= mean["host"] - max(spread["host"], spread["device"]))
    row["ceiling_minus_device"] = round(mean["fixed"] - mean["device"], 1)
    row["gap_to_ceiling_exceeds_ceiling_spread"] = bool(mean["fixed"] - mean["device"] > spread["fixed"])
    row["note"] = NOTE
    emit(row)


AUG = {"data_augment_appearance": True, "data_augment_shape": True, "data_on_device": True, "data_augment_on_device": True}


def _event_us(launch, n, repeats):
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(n):
            launch(k)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    return ts


def aug_kernel_rows(dcfg, iters, repeats, sets_mib):
    from upsparts_amd import data, lib as L
    dev = torch.device("cuda:0")
    for B, S in ((64, 128), (16, 256)):
        ds = data.AugmentedPair2(dict(dcfg, spatial_size=S, batch_size=B, **AUG))
        N = len(ds)
        store = torch.from_numpy(data.build_u8_store(ds)).to(dev)
        luts, weights = torch.from_numpy(data.aug_luts()).to(dev), torch.from_numpy(data.gauss_weights()).to(dev)
        out_bytes = 3 * B * S * S * 3 * 4
        nsets = max(3, -(-sets_mib * (1 << 20) // out_bytes))
        rng = np.random.RandomState(S)
        sets, plan_s, n_els = [], [], []
        for k in range(nsets):
            recs, noise = np.zeros((3, B, data.REC_WORDS), dtype=np.int32), np.zeros((2 * B, 2, S, S), dtype=np.float32)
            t0 = time.perf_counter()
            n_el = data.fill_aug_plan(ds, rng.permutation(N)[:B], recs, noise)
            plan_s.append(time.perf_counter() - t0)
            n_els.append(n_el)
            fld = torch.from_numpy(noise[:max(n_el, 1)]).to(dev)
            sets.append((torch.from_numpy(recs).to(dev), n_el, fld, torch.empty_like(fld), torch.empty_like(fld),
                         torch.empty((2, 3 * B, S, S, 3), dtype=torch.uint8, device=dev),
                         [torch.empty((B, S, S, 3), dtype=torch.float32, device=dev) for _ in range(3)]))

        def views(k, passes):
            recs, n_el, _, _, fld, scr, (v0, v1, vt) = sets[k % nsets]
            L.call("ups_augment_views", L.ptr(store), N, L.ptr(recs), L.ptr(luts), L.ptr(fld), n_el, B, S, L.ptr(scr[0]), L.ptr(scr[1]),
                   L.ptr(v0), L.ptr(v1), L.ptr(vt), passes, L.stream())

        def field(k):
            _, n_el, noise, tmp, fld, _, _ = sets[k % nsets]
            if n_el:
                L.call("ups_augment_field", L.ptr(noise), L.ptr(weights), n_el, S, L.ptr(tmp), L.ptr(fld), L.stream())
        for k in range(nsets):
            field(k)
            views(k, 7)
        torch.cuda.synchronize()
        n = max(iters, 2 * nsets)
        common = {"B": B, "S": S, "store_images": N, "record_sets": nsets, "launches_per_reading": n,
                  "elastic_fields_per_batch_mean": round(float(np.mean(n_els)), 2), "note": NOTE}
        for name, fn in (("pass 1: gather + T_in + filter + colour chain", lambda k: views(k, 1)),
                         ("pass 2: T_mid + hflip + affine", lambda k: views(k, 2)),
                         ("pass 3: grid / elastic warp + normalise", lambda k: views(k, 4)),
                         ("ups_augment_views, all three passes", lambda k: views(k, 7)),
                         ("ups_augment_field (both axes; sets without an elastic record launch nothing)", field)):
            ts = _event_us(fn, n, repeats)
            emit(dict(common, row="aug_kernel", launch=name, us=round(min(ts), 2), us_all=[round(t, 2) for t in ts]))
        emit(dict(common, row="aug_plan", what="host time of data.fill_aug_plan per batch, both switches on",
                  ms=round(1e3 * min(plan_s), 3), ms_mean=round(1e3 * float(np.mean(plan_s)), 3), ms_max=round(1e3 * max(plan_s), 3)))
        del sets, store
        torch.cuda.empty_cache()


def aug_batch_rows(dcfg, repeats, n_host, n_dev):
    from upsparts_amd import data
    dev = torch.device("cuda:0")
    cfg = dict(dcfg, spatial_size=128, batch_size=64, **AUG)
    host, devr = [], []
    for _ in range(repeats):
        it = data.batches(data.AugmentedPair2(cfg), 64)
        next(it)
        t0 = time.perf_counter()
        for _ in range(n_host):
            next(it)
        host.append(n_host / (time.perf_counter() - t0))
        del it
    it = data.device_batches(data.AugmentedPair2(cfg), 64, dev)
    for _ in range(8):
        next(it)
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_dev):
            next(it)
        torch.cuda.synchronize()
        devr.append(n_dev / (time.perf_counter() - t0))
    emit({"row": "aug_batches", "B": 64, "S": 128, "augment": "appearance + shape", "host_batches_per_s": round(max(host), 2),
          "host_all": [round(v, 2) for v in host], "host_workers": 8, "host_batches_per_reading": n_host,
          "device_batches_per_s": round(max(devr), 1), "device_all": [round(v, 1) for v in devr], "device_batches_per_reading": n_dev,
          "device_ms_per_batch": round(1e3 / max(devr), 3), "note": NOTE})


def aug_training_rows(dcfg, repeats, steps_host, steps_dev):
    from upsparts_amd import configs, data
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    B, S = 64, 128
    cfg = configs.BENCH_CONFIGS["cub128p10"][0](B)
    cfg["precision"] = "bf16"
    cfg.update(dcfg)
    model = TrainModel(cfg, device=dev, seed=0)
    tr = Trainer(cfg, None, model)
    g = torch.Generator().manual_seed(1234)
    fixed = {k: (torch.rand(B, S, S, 3, generator=g) * 2 - 1).to(dev) for k in ("view0", "view1", "view0_target")}
    aug = dict(cfg, **AUG)
    feeds = {"host_augmented": (data.batches(data.AugmentedPair2(aug), B), steps_host),
             "device_augmented": (data.device_batches(data.AugmentedPair2(aug), B, dev), steps_dev),
             "device_plain": (data.device_batches(data.AugmentedPair2(cfg), B, dev), steps_dev)}
    quiet = lambda line: None
    tr.iterate(itertools.islice(itertools.repeat(fixed), 8), num_steps=tr.global_step + 8, log_fn=quiet)          # warm-up
    rates = {k: [] for k in feeds}
    for _ in range(repeats):
        for name, (it, n) in feeds.items():                  # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.iterate(itertools.islice(it, n), num_steps=tr.global_step + n, log_fn=quiet)
            torch.cuda.synchronize()
            rates[name].append(n * B / (time.perf_counter() - t0))
    row = {"row": "aug_training", "config": "cub128p10", "B": B, "S": S, "precision": "bf16",
           "steps_per_reading": {k: n for k, (_, n) in feeds.items()}}
    for k, v in rates.items():
        row[k + "_img_per_s"] = round(sum(v) / len(v), 1)
        row[k + "_all"] = [round(x, 1) for x in v]
        row[k + "_spread"] = round(max(v) - min(v), 1)
    row["note"] = NOTE
    emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets-mib", type=int, default=800, help="rotate output sets until they sum to at least this (>> 256 MiB)")
    ap.add_argument("--store-mib", type=int, default=384, help="size of the random store the kernel rows gather from (> 256 MiB)")
    ap.add_argument("--host-batches", type=int, default=6)
    ap.add_argument("--device-batches", type=int, default=400)
    ap.add_argument("--steps-host", type=int, default=12)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--augment", action="store_true", help="the rows of the device-side augmentation (appended to the file) instead")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_data.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    if args.augment:
        emit({"row": "about", "rows": "augment", "device": torch.cuda.get_device_name(0), "images": args.images, "note": NOTE})
        with tempfile.TemporaryDirectory() as tmp:
            dcfg = write_pngs(tmp, args.images)
            aug_kernel_rows(dcfg, args.iters, max(args.repeats, 5), args.sets_mib)
            aug_batch_rows(dcfg, args.repeats, args.host_batches, args.device_batches)
            if not args.skip_model:
                aug_training_rows(dcfg, args.repeats, args.steps_host, args.steps)
        return
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "images": args.images, "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 5), args.sets_mib, args.store_mib)
    with tempfile.TemporaryDirectory() as tmp:
        dcfg = write_pngs(tmp, args.images)
        batch_rows(dcfg, args.repeats, args.host_batches, args.device_batches)
        if not args.skip_model:
            training_rows(dcfg, args.repeats, args.steps_host, args.steps)


if __name__ == "__main__":
    main()
