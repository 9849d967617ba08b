"""Timing of the Gram-matrix perceptual terms (`gram_weight`, csrc/gram.hip).

Per feature map of the trunk (bf16, relu maps; input_1 with 3 channels): forward (ups_gram_l1_fwd, split-K reduce included) and
backward (ups_gram_l1_bwd) in microseconds from device events, TFLOP/s on full-square counts (forward 2 n c^2 2hw, backward
2 n hw c^2), effective GB/s for reading each tensor once (forward: a and b; backward: b and gb read, gb written), and the same terms
through torch.bmm in fp32 for comparison (here only: the product path has no torch fallback).  Then whole training steps, eager,
with gram_weight 0 and 0.1.  Prints one JSON line per row.

    python tools/bench_gram.py [--iters 50] [--steps 10] [--warmup 3] [--skip-steps]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAPS = {   # (c, h, w, relu) of the six compared maps
    "cub128": [(3, 128, 128, False), (64, 128, 128, True), (128, 64, 64, True), (256, 32, 32, True), (512, 16, 16, True),
               (512, 8, 8, True)],
    "crop224": [(3, 224, 224, False), (64, 224, 224, True), (128, 112, 112, True), (256, 56, 56, True), (512, 28, 28, True),
                (512, 14, 14, True)],
}
NAMES = ["input_1", "block1_conv2", "block2_conv2", "block3_conv2", "block4_conv2", "block5_conv2"]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def per_map(n, iters):
    from upsparts_amd import lib as L, ops
    dev = torch.device("cuda:0")
    g = torch.tensor(1.0, device=dev)
    for setting, maps in MAPS.items():
        tot = {"fwd_us": 0.0, "bwd_us": 0.0, "torch_fwd_us": 0.0, "torch_bwd_us": 0.0}
        for name, (c, h, w, relu) in zip(NAMES, maps):
            ld, hw = ops.round8(c), h * w
            gen = torch.Generator().manual_seed(c + h)
            a = torch.randn((n, h, w, ld), generator=gen).bfloat16().to(dev)
            b = torch.randn((n, h, w, ld), generator=gen).bfloat16().to(dev)
            gb = torch.zeros_like(b)
            act = L.ACT_RELU if relu else L.ACT_NONE
            _, npart, nws, nsign = ops.gram_plan(n, hw, c, L.BF16)
            splits = ops.gram_plan(n, hw, c, L.BF16)[0]
            part = torch.empty(npart, dtype=torch.float32, device=dev)
            sign = torch.empty(nsign, dtype=torch.int8, device=dev)
            ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws else None
            out = torch.empty((), dtype=torch.float32, device=dev)

            def fwd():
                L.call("ups_gram_l1_fwd", L.ptr(a), L.ptr(b), L.BF16, n, hw, c, ld, act, L.ptr(part), L.ptr(sign), L.ptr(ws), L.stream())
                L.call("ups_sum_scale", L.ptr(part), npart, 1.0, L.ptr(out), 0, L.stream())

            def bwd():
                L.call("ups_gram_l1_bwd", L.ptr(b), L.ptr(sign), L.ptr(gb), L.BF16, n, hw, c, ld, act, L.ptr(g), 1e-9, L.stream())
            tf, tb = timed(fwd, iters), timed(bwd, iters)
            # torch fp32 reference path (tool only)
            fa = a[..., :c].float().reshape(n, hw, c)
            fb = b[..., :c].float().reshape(n, hw, c)
            if relu:
                fa, fb = fa.relu(), fb.relu()
            S = torch.sign(fb.transpose(1, 2).bmm(fb) - fa.transpose(1, 2).bmm(fa))

            def tfwd():
                return (fb.transpose(1, 2).bmm(fb) - fa.transpose(1, 2).bmm(fa)).abs().mean()

            def tbwd():
                return fb.bmm(S)
            ttf, ttb = timed(tfwd, max(iters // 5, 5)), timed(tbwd, max(iters // 5, 5))
            fl_f, fl_b = 2.0 * n * c * c * 2 * hw, 2.0 * n * hw * c * c
            by_f, by_b = 2.0 * n * hw * ld * 2, 3.0 * n * hw * ld * 2
            row = {"setting": setting, "n": n, "map": name, "c": c, "hw": hw, "splits": splits,
                   "fwd_us": round(tf, 1), "fwd_tflops": round(fl_f / tf * 1e-6, 1), "fwd_gbs": round(by_f / tf * 1e-3, 0),
                   "bwd_us": round(tb, 1), "bwd_tflops": round(fl_b / tb * 1e-6, 1), "bwd_gbs": round(by_b / tb * 1e-3, 0),
                   "torch_fp32_fwd_us": round(ttf, 1), "torch_fp32_bwd_us": round(ttb, 1)}
            print(json.dumps(row), flush=True)
            tot["fwd_us"] += tf
            tot["bwd_us"] += tb
            tot["torch_fwd_us"] += ttf
            tot["torch_bwd_us"] += ttb
            del a, b, gb, fa, fb, S, sign, ws
        print(json.dumps(dict({"setting": setting, "n": n, "map": "all six"}, **{k: round(v, 1) for k, v in tot.items()})), flush=True)


def steps(nsteps, warmup):
    from upsparts_amd import configs
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    for cname in ("cub128p10", "deepfashion256p16"):
        build, S, P, B0, prec0, _, _ = configs.BENCH_CONFIGS[cname]
        res = {}
        for gw in (0.0, 0.1, 0.0, 0.1):         # alternated: the spread shows in the two readings of each
            cfg = build(B0)
            cfg["precision"] = "bf16"
            cfg["gram_weight"] = gw
            model = TrainModel(cfg, device=dev, seed=0)
            tr = Trainer(cfg, None, model)
            g = torch.Generator().manual_seed(1234)
            batch = {k: (torch.rand(B0, S, S, 3, generator=g) * 2 - 1).to(dev) for k in model.inputs}
            for _ in range(warmup):
                tr.train_step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(nsteps):
                tr.train_step(batch)
            torch.cuda.synchronize()
            res.setdefault(gw, []).append((time.perf_counter() - t0) * 1e3 / nsteps)
            del tr, model, batch
            torch.cuda.empty_cache()
        base, gram = min(res[0.0]), min(res[0.1])
        print(json.dumps({"setting": cname, "batch": B0, "precision": "bf16", "step_ms_gram0": [round(v, 2) for v in res[0.0]],
                          "step_ms_gram0.1": [round(v, 2) for v in res[0.1]],
                          "overhead_pct": round(100.0 * (gram - base) / base, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gram.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    per_map(args.n, args.iters)
    if not args.skip_steps:
        steps(args.steps, args.warmup)


if __name__ == "__main__":
    main()
