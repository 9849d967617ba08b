"""Micro-benchmark of `upsample: conv_transposed` (weight-normalised deconv2d, csrc/deconv3x3_s2.hip) on the deconvolution layers of a
CUB 128x128 / B=64 step with the method in `final_hour` and in every level of `dv`: forward, input gradient (dx) and weight
gradient (dW: the swapped-role weight-gradient kernel + db / coordinate rows + the normalisation backward), in us and TFLOP/s, for
the one-launch forward kernel and the four per-class launches of the convolution engine.  One JSON line per layer.
Usage (GPU box): python tools/bench_deconv.py [--reps N] [--only name,...]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import upsparts_amd  # noqa: E402,F401
from upsparts_amd import ops, lib  # noqa: E402

CASES = [
    # name, images, input size, C_in, nf, coords, fp16 forward (the mask decoder's scope)
    ("dd_up", 64, 64, 64, 32, False, False),
    ("dv_up4", 128, 4, 256, 128, True, True),
    ("dv_up8", 128, 8, 128, 128, True, True),
    ("dv_up16", 128, 16, 128, 32, True, True),
    ("dv_up32", 128, 32, 32, 32, True, True),
    ("dv_up64", 128, 64, 32, 16, True, True),
]


def _time(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else None
    ops.Streams.enabled = False
    for name, n, h, cin, nf, coords, f16 in CASES:
        if only and name not in only:
            continue
        gen = torch.Generator().manual_seed(0)
        V = (torch.randn((3, 3, nf, cin + (2 if coords else 0)), generator=gen) * 0.05).to(dev)
        g, b = torch.ones(nf, device=dev), torch.zeros(nf, device=dev)
        lay = ops.DeconvLayer("bench/deconv2d_0", V, g, b, coords)
        lay.f16 = f16
        fmt = lib.F16 if f16 else None
        x = torch.randn((n, h, h, ops.round8(cin)), generator=gen)
        x = (x.half().view(torch.bfloat16) if f16 else x.bfloat16()).to(dev)
        gy = torch.randn((n, 2 * h, 2 * h, ops.round8(nf)), generator=gen).bfloat16().to(dev)
        ops.deconv_forward(x, lay, fmt=fmt)
        flops = 2.0 * n * h * h * 9 * cin * nf
        res = {"layer": name, "n": n, "h": h, "cin": cin, "nf": nf, "coords": coords, "fp16_fwd": f16}
        for form, one in (("one_launch", True), ("four_launch", False)):
            us = _time(lambda: ops.deconv_forward(x, lay, fmt=fmt, one_launch=one), a.reps)
            res["fwd_us_" + form], res["fwd_tflops_" + form] = round(us, 2), round(flops / us * 1e-6, 2)
        rc = lib.load().ups_deconv3x3_s2_fwd(lib.ptr(x), fmt or lib.BF16, n, h, h, ops.round8(cin), x.shape[-1],
                                             lib.ptr(ops._deconv_ent(lay, x, fmt)["w_fwd"]), None, None, nf, ops.round8(nf),
                                             lib.ptr(torch.empty((n, 2 * h, 2 * h, ops.round8(nf)), dtype=torch.bfloat16, device=dev)),
                                             lib.stream())
        res["one_launch_takes_shape"] = rc == 0
        us = _time(lambda: ops.deconv_dgrad(gy, x, lay, fmt=fmt), a.reps)
        res["dx_us"], res["dx_tflops"] = round(us, 2), round(flops / us * 1e-6, 2)
        us = _time(lambda: ops.deconv_wgrad(gy, x, lay, fmt=fmt), a.reps)
        res["dw_us"], res["dw_tflops"] = round(us, 2), round(flops / us * 1e-6, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
