"""What the part-IoU evaluation costs the slow way and on the device (yaml `eval_on_device`; evalutil.PartEvaluator, TrainModel.segment,
csrc/evalparts.hip).

The workload is the reduced evaluation of the CUB config: `--images` (512) SYNTHETIC 128 x 128 views (U(-1, 1) noise) with label maps
of 8 x 8 blocks, P = 10 parts, G = 5 labels, batch 64, bf16, seeded weights.  The masks of an untrained model on noise are not the
masks of a trained one: the model time does not depend on them, the host scoring time and the kernel's run lengths do.

(a) parent   the route of `-e` without the key: TrainModel.forward per batch, the four fetched outputs copied to the host as fp32,
             evalutil.evaluate_parts over the collected maps (the pickle is NOT written: the figure flatters this leg).
(b) device   runner.evaluate_on_device over the same host batches: segment + ups_part_confusion, one copy of the counts,
             evalutil.evaluate_from_counts.  The result dict is compared with (a)'s: `equal` in the row.
(c) kernel   event time of ups_part_confusion at [128, 128 x 128, 10, 5] on block-constant maps and on noise (a key change at almost
             every pixel), input sets rotated over more than the Infinity Cache: microseconds per launch (minimum of `--repeats`
             readings of `--iters` launches, all printed) and the share of 8 TB/s on the 9 bytes per pixel it must read.
Wall-clock legs are the minimum of `--repeats` alternated readings after one warm-up of each.  Prints one JSON line per row.

    python tools/bench_parteval.py [--images 512] [--repeats 3] > profiles/bench_parteval.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
NOTE = "synthetic noise views, seeded weights, block label maps: not CUB images and not a trained model's masks"


def emit(row):
    print(json.dumps(row), flush=True)


def block_maps(rng, n, S, values, block):
    small = rng.randint(0, values, (n, S // block, S // block))
    return np.repeat(np.repeat(small, block, axis=1), block, axis=2)


def kernel_rows(iters, repeats, sets_mib):
    from upsparts_amd import lib as L
    dev = torch.device("cuda:0")
    N, S, P, G = 128, 128, 10, 5
    set_bytes = N * S * S * 9
    nsets = max(3, -(-sets_mib * (1 << 20) // set_bytes))
    for kind in ("blocks", "noise"):
        rng = np.random.RandomState(1)
        sets = []
        for k in range(nsets):
            if kind == "blocks":
                pred, gt = block_maps(rng, N, S, P, 16), block_maps(rng, N, S, G, 8)
            else:
                pred, gt = rng.randint(0, P, (N, S, S)), rng.randint(0, G, (N, S, S))
            sets.append((torch.from_numpy(pred.astype(np.int64)).to(dev), torch.from_numpy(gt.astype(np.uint8)).to(dev)))
        counts = torch.zeros((N, P, G), dtype=torch.int32, device=dev)
        invalid = torch.zeros(1, dtype=torch.int32, device=dev)

        def launch(k):
            pred, gt = sets[k % nsets]
            L.call("ups_part_confusion", L.ptr(pred), L.ptr(gt), None, N, S * S, P, G, L.ptr(counts), L.ptr(invalid), L.stream())
        for k in range(nsets):
            launch(k)
        torch.cuda.synchronize()
        n = max(iters, 2 * nsets)
        ts = []
        for _ in range(repeats):
            counts.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n):
                launch(k)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / n)
        assert int(invalid) == 0 and int(counts.sum()) == n * N * S * S
        emit({"row": "kernel", "launch": "ups_part_confusion", "keys": kind, "N": N, "HW": S * S, "P": P, "G": G, "input_sets": nsets,
              "input_sets_MB": round(nsets * set_bytes / 1e6, 1), "launches_per_reading": n, "bytes_read": set_bytes,
              "us": round(min(ts), 2), "us_all": [round(t, 2) for t in ts], "GBps": round(set_bytes / min(ts) * 1e-3, 1),
              "fraction_of_8TBs": round(set_bytes / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4)})
        del sets
        torch.cuda.empty_cache()


def route_rows(n_images, repeats):
    from upsparts_amd import configs, evalutil, runner
    from upsparts_amd.model import TrainModel
    dev = torch.device("cuda:0")
    B, S, G = 64, 128, 5
    cfg = configs.BENCH_CONFIGS["cub128p10"][0](B)
    cfg.update({"precision": "bf16", "test_mode": True, "eval_n_labels": G})
    model = TrainModel(cfg, device=dev, seed=0)
    g = torch.Generator().manual_seed(1234)
    rng = np.random.RandomState(5)
    n_batches = n_images // B
    batches = [{"view0": torch.rand(B, S, S, 3, generator=g) * 2 - 1, "view1": torch.rand(B, S, S, 3, generator=g) * 2 - 1,
                "gt_segmentation": torch.from_numpy(block_maps(rng, B, S, G, 8).astype(np.int64))} for _ in range(n_batches)]
    keys = ["out_parts_hard", "out_parts_soft", "generated", "m0_sample"]

    def parent():
        t0 = time.perf_counter()
        outs, gts = {k: [] for k in keys}, []
        for batch in batches:
            o = model.forward({"view0": batch["view0"], "view1": batch["view1"]})
            for k in keys:
                outs[k].append(o[k].detach().float().cpu().numpy() if o[k].dtype.is_floating_point else o[k].cpu().numpy())
            gts.append(np.asarray(batch["gt_segmentation"]))
        t1 = time.perf_counter()
        res = evalutil.evaluate_parts(np.concatenate(outs["out_parts_hard"]), np.concatenate(gts))
        return res, time.perf_counter() - t0, t1 - t0

    def device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = runner.evaluate_on_device(model, iter(batches), cfg)
        return res, time.perf_counter() - t0

    parent()
    device()
    ta, tfw, tb, ra, rb = [], [], [], None, None
    for _ in range(repeats):
        ra, t, tf = parent()
        ta.append(t)
        tfw.append(tf)
        rb, t = device()
        tb.append(t)
    common = {"images": n_batches * B, "S": S, "P": cfg["n_parts"], "G": G, "B": B, "precision": "bf16", "config": "cub128p10", "note": NOTE}
    emit(dict(common, row="parent", route="forward per batch, outputs to host, evaluate_parts", s=round(min(ta), 3),
              s_all=[round(t, 3) for t in ta], forward_and_copies_s=round(min(tfw), 3), host_scoring_s=round(min(ta) - min(tfw), 3),
              images_per_s=round(n_batches * B / min(ta), 1)))
    emit(dict(common, row="device", route="segment + ups_part_confusion, evaluate_from_counts", s=round(min(tb), 3),
              s_all=[round(t, 3) for t in tb], images_per_s=round(n_batches * B / min(tb), 1),
              speedup_over_parent=round(min(ta) / min(tb), 2), faster_than_parent=bool(min(tb) < min(ta)),
              equal=bool(ra["mapping"] == rb["mapping"] and ra["iou"] == rb["iou"] and ra["per_image"] == rb["per_image"]
                         and ra["pooled"] == rb["pooled"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets-mib", type=int, default=400, help="rotate input sets until they sum to at least this (> 256 MiB)")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_parteval.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "images": args.images, "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 5), args.sets_mib)
    if not args.skip_model:
        route_rows(args.images, args.repeats)


if __name__ == "__main__":
    main()
