"""What the part-equivariance metric costs (yaml `val_metrics: [equivariance]`; csrc/equivariance.hip, evalutil.EquivarianceEvaluator).

(a) kernel      event time of ups_part_equivariance at 128 maps of 128 x 128, P = 10 and 25, on NOISE maps (a seeded soft-max per pixel) and
                on BLOCK-CONSTANT maps (one-hot in 16 x 16 blocks: the histogram's worst case, every lane of a wave on one bin), operand
                sets rotated over more than the Infinity Cache: microseconds per call (minimum of `--repeats` readings of `--iters`
                calls, all printed; a call is the kernel and its partial-sum pass) and the share of 8 TB/s on the bytes that must move
                (N HW (2 * 4 P + 8 + 8): both soft maps once, pred_b and the grid).  ups_tps_grid at the same size likewise (bytes: the
                8 N HW it writes -- the kernel is arithmetic, K = 9 logf per pixel).
(b) composition what the kernel replaces, on the same operands: ups_tps_warp on the soft map + torch argmax + ups_part_confusion (pred_b
                already cast to uint8 outside the timed region).  It has no inside rule, decides on fp32 clamped-corner weights and gives
                no distance; `agreement_diff` in the row is how far its agreement lies from the kernel's.
(c) validate    Trainer.validate() over 512 synthetic images at batch 64 (cub128p10, bf16, seeded weights, U8 noise images) with
                `val_metrics` [equivariance], [reconstruction, parts] and all three: wall clock of the whole call.
Prints one JSON line per row.

    python tools/bench_equivariance.py [--pairs 512] [--repeats 3] > profiles/bench_equivariance.jsonl
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
NOTE = "synthetic maps and noise images, seeded weights: not CUB images and not a trained model's masks"


def emit(row):
    print(json.dumps(row), flush=True)


def event_us(fn, n, repeats):
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(n):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    return ts


def make_maps(kind, N, S, P, g, dev):
    """(soft [N,S,S,P] float32, pred [N,S,S] int64)."""
    if kind == "noise":
        soft = torch.softmax(4 * torch.randn((N, S, S, P), generator=g, device=dev), dim=3).contiguous()
        return soft, soft.argmax(dim=3)
    blocks = torch.randint(0, P, (N, S // 16, S // 16), generator=g, device=dev)
    pred = blocks.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2).contiguous()
    return torch.nn.functional.one_hot(pred, P).float().contiguous(), pred


def kernel_rows(iters, repeats, sets_mib):
    from upsparts_amd import configs, evalutil, ops, tps
    dev = torch.device("cuda:0")
    N, S = 128, 128
    g = torch.Generator(device=dev).manual_seed(1)
    for P in (10, 25):
        for kind in ("noise", "block-constant"):
            set_bytes = N * S * S * (2 * 4 * P + 8 + 8)
            nsets = max(3, -(-sets_mib * (1 << 20) // set_bytes))
            sets = []
            for k in range(nsets):
                u = evalutil.equivariance_uniforms(N, 100 + k).to(dev)
                coord, _, T = tps.tps_system(u, configs.TPS_PARAMETERS)
                soft_a, _ = make_maps(kind, N, S, P, g, dev)
                soft_b, pred_b = make_maps(kind, N, S, P, g, dev)
                sets.append((soft_a, soft_b, pred_b, ops.tps_grid(T, coord, S, S), T, coord, pred_b.to(torch.uint8)))
            counts = torch.zeros((N, P, P), dtype=torch.int32, device=dev)
            invalid = torch.zeros(1, dtype=torch.int32, device=dev)
            tv = torch.empty((N,), dtype=torch.float64, device=dev)
            n = max(iters, 2 * nsets)
            run = lambda k: ops.part_equivariance(*sets[k % nsets][:4], counts=counts, invalid=invalid, tv=tv)
            for k in range(nsets):
                run(k)
            torch.cuda.synchronize()
            ts = event_us(run, n, repeats)
            counts.zero_()
            run(0)
            res = evalutil.equivariance_from_counts(counts.cpu().numpy(), tv.cpu().numpy(), S * S)
            assert int(invalid) == 0
            common = {"N": N, "H": S, "W": S, "P": P, "maps": kind, "input_sets": nsets, "input_sets_MB": round(nsets * set_bytes / 1e6, 1),
                      "calls_per_reading": n, "bytes_moved": set_bytes}
            emit(dict(common, row="kernel", launch="ups_part_equivariance", us=round(min(ts), 2), us_all=[round(t, 2) for t in ts],
                      GBps=round(set_bytes / min(ts) * 1e-3, 1), fraction_of_8TBs=round(set_bytes / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4),
                      valid=res["valid"], agreement=res["agreement"], tv=res["tv"]))
            # the composition the kernel replaces
            cc = torch.zeros((N, P, P), dtype=torch.int32, device=dev)

            def composed(k):
                soft_a, _, _, _, T, coord, pb8 = sets[k % nsets]
                ops.part_confusion(tps._warp(soft_a, T, coord).argmax(dim=3), pb8, P, P, counts=cc, invalid=invalid)
            for k in range(nsets):
                composed(k)
            torch.cuda.synchronize()
            tc = event_us(composed, n, repeats)
            cc.zero_()
            composed(0)
            c = cc.cpu().numpy().astype(np.int64)
            agree = float(np.trace(c.sum(axis=0)) / c.sum())
            emit(dict(common, row="composition", launch="ups_tps_warp + torch argmax + ups_part_confusion", us=round(min(tc), 2),
                      us_all=[round(t, 2) for t in tc], fused_over_composition=round(min(ts) / min(tc), 3), agreement=agree,
                      agreement_diff=agree - res["agreement"], pixels_counted=int(c.sum()), fused_pixels_counted=int(counts.sum())))
            if kind == "noise":
                grid = torch.empty((N, S, S, 2), dtype=torch.float32, device=dev)
                from upsparts_amd import lib as L
                K = sets[0][5].shape[1]

                def grid_only(k):
                    _, _, _, _, T, coord, _ = sets[k % nsets]
                    L.call("ups_tps_grid", L.ptr(T), L.ptr(coord), L.ptr(grid), N, S, S, K, L.stream())
                grid_only(0)
                tg = event_us(grid_only, n, repeats)
                gb = N * S * S * 8
                emit({"row": "kernel", "launch": "ups_tps_grid", "N": N, "H": S, "W": S, "K": K, "calls_per_reading": n, "bytes_moved": gb,
                      "us": round(min(tg), 2), "us_all": [round(t, 2) for t in tg], "GBps": round(gb / min(tg) * 1e-3, 1),
                      "fraction_of_8TBs": round(gb / (min(tg) * 1e-6) / HBM_BYTES_PER_S, 4)})
            del sets
            torch.cuda.empty_cache()


def validate_rows(n_pairs, repeats):
    from upsparts_amd import configs, data, evalutil
    from upsparts_amd.model import TrainModel, Trainer, equivariance_tps_parameters
    dev = torch.device("cuda:0")
    B, S = 64, 128
    cfg = configs.BENCH_CONFIGS["cub128p10"][0](B)
    cfg.update({"precision": "bf16"})
    model = TrainModel(cfg, device=dev, seed=0)
    trainer = Trainer(cfg, None, model)
    # a pair set of noise images without files: the fields ValidationPairs.__init__ fills
    rng = np.random.RandomState(3)
    n = n_pairs // B * B
    pairs = data.ValidationPairs.__new__(data.ValidationPairs)
    pairs.batch_size, pairs._dev = B, None
    pairs.rows = pairs.pairs = np.stack([np.arange(n), rng.permutation(n)], 1).astype(np.int32)
    pairs.store = torch.from_numpy(rng.randint(0, 256, (n, S, S, 3), dtype=np.uint8))
    trainer._tps_singular = torch.zeros(1, dtype=torch.int32, device=dev)
    everything = {"pairs": pairs, "rec": evalutil.ReconstructionEvaluator(dev), "usage": evalutil.PartUsageEvaluator(dev, model.n_parts, 0.005),
                  "equiv": evalutil.EquivarianceEvaluator(dev, model.n_parts, equivariance_tps_parameters(cfg), n_singular=trainer._tps_singular),
                  "equiv_uniforms": evalutil.equivariance_uniforms(n, 1).to(dev)}
    for metrics, keys in ((["equivariance"], ("equiv", "equiv_uniforms")), (["reconstruction", "parts"], ("rec", "usage")),
                          (["reconstruction", "parts", "equivariance"], ("rec", "usage", "equiv", "equiv_uniforms"))):
        trainer._val = dict({"metrics": metrics, "pairs": pairs}, **{k: everything[k] for k in keys})
        logs = dict(trainer.validate())
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.validate()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        emit({"row": "validate", "val_metrics": metrics, "images": n, "B": B, "S": S, "P": model.n_parts, "config": "cub128p10",
              "precision": "bf16", "chunks": pairs.chunks(), "validate_s": round(min(ts), 4), "validate_s_all": [round(t, 4) for t in ts],
              "images_per_s": round(n / min(ts), 1), "values": {k: float(v) for k, v in logs.items() if "equiv" in k}, "note": NOTE})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets-mib", type=int, default=400, help="rotate operand sets until they sum to at least this (> 256 MiB)")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_equivariance.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "images": args.pairs, "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 5), args.sets_mib)
    if not args.skip_model:
        validate_rows(args.pairs, args.repeats)


if __name__ == "__main__":
    main()
