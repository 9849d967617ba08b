"""What the label-free validation metrics cost (yaml `val_metrics: [reconstruction, parts]`; csrc/valmetrics.hip, evalutil, Trainer.validate).

(a) kernel   event time of ups_image_metrics at [128, 128 x 128, 3] fp32 against fp32 and of ups_part_usage at [128, 128 x 128, 10], input
             sets rotated over more than the Infinity Cache: microseconds per call (minimum of `--repeats` readings of `--iters` calls,
             all printed; a call is the kernel and its partial-sum pass) and the share of 8 TB/s on the bytes it must read
             (2 N H W 3 4 for the images; N HW (4 P + 8) for the parts).
(b) torch    the same quantities with torch ops on the device in float64 (two depth-wise conv2d passes per filtered map, bincount, log),
             on the same rotated inputs; `max_rel_diff` against the kernel's sums is in the row.
(c) validate Trainer.validate() over 512 synthetic pairs at batch 64 (cub128p10, bf16, seeded weights, U8 noise images): wall clock of the
             whole call, of the forward passes alone, of the perceptual term alone and event time of the two metric kernels alone.
Wall-clock legs are the minimum of `--repeats` readings after one warm-up.  Prints one JSON line per row.

    python tools/bench_valmetrics.py [--pairs 512] [--repeats 3] > profiles/bench_valmetrics.jsonl
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
NOTE = "synthetic noise images, seeded weights: not CUB images and not a trained model's reconstructions or masks"


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


def torch_image_metrics(a, b, w):
    """ups_image_metrics with torch ops: float64, valid depth-wise convolutions along W then H."""
    import torch.nn.functional as F
    x = ((a[..., :3].double() + 1) / 2).clamp(0, 1).permute(0, 3, 1, 2)
    y = ((b[..., :3].double() + 1) / 2).clamp(0, 1).permute(0, 3, 1, 2)
    kw, kh = w.view(1, 1, 1, -1).repeat(3, 1, 1, 1), w.view(1, 1, -1, 1).repeat(3, 1, 1, 1)

    def f(t):
        return F.conv2d(F.conv2d(t, kw, groups=3), kh, groups=3)
    mx, my = f(x), f(y)
    vx, vy, cxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    d = x - y
    return torch.stack([(d * d).sum(dim=(1, 2, 3)), d.abs().sum(dim=(1, 2, 3)), ssim.sum(dim=(1, 2, 3))], 1)


def torch_part_usage(soft, pred, P):
    N = soft.shape[0]
    s = soft.double().view(N, -1, P)
    key = pred.view(N, -1) + P * torch.arange(N, device=pred.device)[:, None]
    counts = torch.bincount(key.reshape(-1), minlength=N * P).view(N, P)
    ent = -(torch.where(s > 0, s * torch.log(torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))).sum(dim=(1, 2))
    return counts, torch.stack([s.max(dim=2).values.sum(dim=1), ent], 1)


def kernel_rows(iters, repeats, sets_mib):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    N, S, P = 128, 128, 10
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.from_numpy(ops.ssim_weights()).to(dev)
    # ---- ups_image_metrics
    set_bytes = 2 * N * S * S * 3 * 4
    nsets = max(3, -(-sets_mib * (1 << 20) // set_bytes))
    sets = []
    for _ in range(nsets):
        a = torch.rand((N, S, S, 3), generator=g, device=dev) * 2.4 - 1.2
        sets.append((a, (0.7 * a + (torch.rand((N, S, S, 3), generator=g, device=dev) - 0.5) * 0.8).contiguous()))
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    n = max(iters, 2 * nsets)
    for k in range(nsets):
        ops.image_metrics(*sets[k], out=out)
    torch.cuda.synchronize()
    ts = event_us(lambda k: ops.image_metrics(*sets[k % nsets], out=out), n, repeats)
    ref = torch_image_metrics(*sets[(n - 1) % nsets], w)
    diff = float(((out - ref).abs() / ref.abs()).max())
    common = {"N": N, "H": S, "W": S, "operands": "fp32 ld 3 x fp32 ld 3", "input_sets": nsets, "input_sets_MB": round(nsets * set_bytes / 1e6, 1),
              "calls_per_reading": n, "bytes_read": set_bytes}
    emit(dict(common, row="kernel", launch="ups_image_metrics", us=round(min(ts), 2), us_all=[round(t, 2) for t in ts],
              GBps=round(set_bytes / min(ts) * 1e-3, 1), fraction_of_8TBs=round(set_bytes / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4)))
    nt = max(10, n // 10)
    tt = event_us(lambda k: torch_image_metrics(*sets[k % nsets], w), nt, repeats)
    emit(dict(common, row="torch", launch="torch ops, float64", calls_per_reading=nt, us=round(min(tt), 2), us_all=[round(t, 2) for t in tt],
              kernel_speedup=round(min(tt) / min(ts), 2), max_rel_diff=diff))
    del sets
    torch.cuda.empty_cache()
    # ---- ups_part_usage
    set_bytes = N * S * S * (4 * P + 8)
    nsets = max(3, -(-sets_mib * (1 << 20) // set_bytes))
    sets = []
    for _ in range(nsets):
        soft = torch.softmax(4 * torch.randn((N, S * S, P), generator=g, device=dev), dim=2).contiguous()
        sets.append((soft, soft.argmax(dim=2)))
    counts = torch.zeros((N, P), dtype=torch.int32, device=dev)
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    sharp = torch.empty((N, 2), dtype=torch.float64, device=dev)
    n = max(iters, 2 * nsets)
    for k in range(nsets):
        ops.part_usage(*sets[k], counts=counts, invalid=invalid, sharp=sharp)
    torch.cuda.synchronize()
    ts = event_us(lambda k: ops.part_usage(*sets[k % nsets], counts=counts, invalid=invalid, sharp=sharp), n, repeats)
    counts.zero_()
    ops.part_usage(*sets[0], counts=counts, invalid=invalid, sharp=sharp)
    rc, rs = torch_part_usage(*sets[0], P)
    assert int(invalid) == 0 and torch.equal(counts.long(), rc)
    diff = float(((sharp - rs).abs() / rs.abs()).max())
    common = {"N": N, "HW": S * S, "P": P, "input_sets": nsets, "input_sets_MB": round(nsets * set_bytes / 1e6, 1), "calls_per_reading": n,
              "bytes_read": set_bytes}
    emit(dict(common, row="kernel", launch="ups_part_usage", us=round(min(ts), 2), us_all=[round(t, 2) for t in ts],
              GBps=round(set_bytes / min(ts) * 1e-3, 1), fraction_of_8TBs=round(set_bytes / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4)))
    nt = max(10, n // 10)
    tt = event_us(lambda k: torch_part_usage(*sets[k % nsets], P), nt, repeats)
    emit(dict(common, row="torch", launch="torch ops, float64", calls_per_reading=nt, us=round(min(tt), 2), us_all=[round(t, 2) for t in tt],
              kernel_speedup=round(min(tt) / min(ts), 2), max_rel_diff=diff))
    del sets
    torch.cuda.empty_cache()


def validate_rows(n_pairs, repeats):
    from upsparts_amd import configs, data, evalutil, ops
    from upsparts_amd.model import TrainModel, Trainer
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
    trainer._val = {"metrics": ["reconstruction", "parts"], "pairs": pairs, "rec": evalutil.ReconstructionEvaluator(dev),
                    "usage": evalutil.PartUsageEvaluator(dev, model.n_parts, 0.005)}

    def wall(fn):
        fn()
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts
    logs = {}

    def whole():
        logs.update(trainer.validate())

    def forwards():
        for c in range(pairs.chunks()):
            model.forward(pairs.chunk_views(c, dev), noise=None)

    chunk = pairs.chunk_views(0, dev)
    out = model.forward(chunk, noise=None)
    gen, soft, hard = model.generated_act, out["out_parts_soft"], out["out_parts_hard"]

    pc = trainer._validation_perceptual()

    def rec_terms():
        with torch.no_grad():
            for c in range(pairs.chunks()):
                tgt = chunk["view0"] if pc.pmode == "native" else trainer._perceptual_view(pc, model.to_act(chunk["view0"]))
                trainer.vgg.loss(tgt.contiguous(), trainer._perceptual_view(pc, gen), model.act_dtype, gram_weight=trainer.gram_weight)
    tw, tf, tr = wall(whole), wall(forwards), wall(rec_terms)
    rows = torch.empty((B, 3), dtype=torch.float64, device=dev)

    def metrics(k):
        ops.image_metrics(gen, chunk["view0"], out=rows)
        ops.part_usage(soft, hard)
    metrics(0)
    tk = event_us(metrics, 50, max(repeats, 3))
    emit({"row": "validate", "pairs": n, "B": B, "S": S, "P": model.n_parts, "config": "cub128p10", "precision": "bf16",
          "chunks": pairs.chunks(), "validate_s": round(min(tw), 4), "validate_s_all": [round(t, 4) for t in tw],
          "forward_passes_s": round(min(tf), 4), "perceptual_term_s": round(min(tr), 4),
          "metric_kernels_s": round(min(tk) * 1e-6 * pairs.chunks(), 6), "metric_kernels_us_per_chunk": round(min(tk), 2),
          "pairs_per_s": round(n / min(tw), 1), "values": {k: float(v) for k, v in logs.items()}, "note": NOTE})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets-mib", type=int, default=400, help="rotate input sets until they sum to at least this (> 256 MiB)")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_valmetrics.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "pairs": args.pairs, "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 5), args.sets_mib)
    if not args.skip_model:
        validate_rows(args.pairs, args.repeats)


if __name__ == "__main__":
    main()
