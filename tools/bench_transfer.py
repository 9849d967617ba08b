"""Timing of appearance transfer (csrc/partpath.hip: ups_unpool_mix_fwd; TrainModel.transfer_matrix).

(a) The mixed unpool against the way the same tensor is made without it -- index_select of the hard masks, a gathered [K,P,F] feature
    tensor, then ups_unpool_fwd -- in the same process: full 16 x 16 matrices (K = 256), bf16, at CUB-128 (P = 10, A = 64) and at
    256 x 256 with P = 20.  Microseconds from device events, the minimum of `--repeats` readings of `--iters` launches each (all
    readings are printed), and effective GB/s on output-written-once plus inputs-read-once.
(b) A 16 x 16 transfer_matrix against the same 256 (pose, appearance) pairs through ``forward`` at batch_size 64 (the headline CUB-128
    model, bf16): images per second for both and their ratio, from device events around one whole call per reading.
Prints one JSON line per row.

    python tools/bench_transfer.py [--iters 20] [--repeats 5] [--skip-model]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cub128 P10 A64": (128, 10, 64), "256x256 P20 A64": (256, 20, 64)}
N = 16                                  # rows = columns of the matrix


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


def kernel_rows(iters, repeats):
    from upsparts_amd import lib as L, ops
    from upsparts_amd.model import transfer_indices
    dev = torch.device("cuda:0")
    for name, (S, P, F) in SHAPES.items():
        hw, K, ldo = S * S, N * N, ops.round8(F + P)
        gen = torch.Generator().manual_seed(S + P)
        hard = torch.nn.functional.one_hot(torch.randint(0, P, (N, hw), generator=gen), P).float().to(dev)
        feat = torch.randn(N, P, F, generator=gen).to(dev)
        pi, ai = transfer_indices(N, N, P)
        pd, ad = pi.to(torch.int32).to(dev), ai.reshape(-1).to(torch.int32).to(dev)
        pl, al, pr = pi.to(dev), ai.to(dev), torch.arange(P, device=dev)[None, :]
        out = torch.empty((K, hw, ldo), dtype=torch.bfloat16, device=dev)
        ref = torch.empty_like(out)

        def mix():
            L.call("ups_unpool_mix_fwd", L.ptr(hard), L.ptr(feat), L.ptr(pd), L.ptr(ad), L.ptr(out), L.BF16, K, N, N, hw, P, F, ldo,
                   L.stream())

        def gathered():
            hg = hard.index_select(0, pl)
            fg = feat[al, pr].contiguous()
            L.call("ups_unpool_fwd", L.ptr(hg), L.ptr(fg), L.ptr(ref), L.BF16, K, hw, P, F, ldo, L.stream())
        mix(); gathered()
        same = bool(torch.equal(out, ref))
        tm, tg = [], []
        for _ in range(repeats):            # alternated readings
            tg.append(timed(gathered, iters))
            tm.append(timed(mix, iters))
        by = K * hw * ldo * 2 + N * hw * P * 4 + N * P * F * 4 + (K + K * P) * 4
        print(json.dumps({"row": "unpool_mix", "shape": name, "K": K, "hw": hw, "P": P, "F": F, "dtype": "bf16", "bit_identical": same,
                          "mix_us": round(min(tm), 1), "mix_us_all": [round(v, 1) for v in tm],
                          "gather_unpool_us": round(min(tg), 1), "gather_unpool_us_all": [round(v, 1) for v in tg],
                          "gather_unpool_spread_us": round(max(tg) - min(tg), 1),
                          "mix_gbs": round(by / min(tm) * 1e-3, 0), "speedup": round(min(tg) / min(tm), 3)}), flush=True)
        del hard, feat, out, ref


def matrix_rows(repeats):
    from upsparts_amd import configs
    from upsparts_amd.model import TrainModel
    dev = torch.device("cuda:0")
    build, S, P, _, _, _, _ = configs.BENCH_CONFIGS["cub128p10"]
    B = 64
    cfg = build(B)
    cfg["precision"] = "bf16"
    model = TrainModel(cfg, device=dev, seed=0)
    g = torch.Generator().manual_seed(1234)
    rows = (torch.rand(N, S, S, 3, generator=g) * 2 - 1).to(dev)
    cols = (torch.rand(N, S, S, 3, generator=g) * 2 - 1).to(dev)
    v0 = rows.repeat_interleave(N, 0)           # pair k = (row k // N, column k % N)
    v1 = cols.repeat(N, 1, 1, 1)

    def matrix():
        return model.transfer_matrix(rows, cols)["generated"]

    def pairs():
        return torch.cat([model.forward({"view0": v0[b:b + B], "view1": v1[b:b + B]})["generated"].clone() for b in range(0, N * N, B)])
    res = {"matrix": [], "pairs": []}
    a, b = matrix().view(N * N, S, S, 3), pairs()
    for _ in range(repeats):
        for name, fn in (("pairs", pairs), ("matrix", matrix)):
            res[name].append(timed(fn, 1) * 1e-6)          # device events, one whole call per reading (after timed()'s warm-up calls)
    ips = {k: N * N / min(v) for k, v in res.items()}
    print(json.dumps({"row": "transfer_matrix 16x16", "config": "cub128p10", "precision": "bf16", "batch_size": B,
                      # (the pairs run the pose path on batches of 2B repeated views, the matrix on its 2N images once: the generic
                      #  convolution plans split-K by the batch, so the images are not the same bits: the largest difference is reported)
                      "same_images": bool(torch.equal(a, b)), "max_abs_diff": round(float((a - b).abs().max()), 6),
                      "matrix_ms_all": [round(v * 1e3, 2) for v in res["matrix"]], "pairs_ms_all": [round(v * 1e3, 2) for v in res["pairs"]],
                      "matrix_img_s": round(ips["matrix"], 0), "pairs_forward_img_s": round(ips["pairs"], 0),
                      "ratio": round(ips["matrix"] / ips["pairs"], 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_transfer.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    kernel_rows(args.iters, args.repeats)
    if not args.skip_model:
        matrix_rows(args.repeats)


if __name__ == "__main__":
    main()
