"""Timing of the training image logs (csrc/canvas.hip; Trainer.train_step(images=True)) at the headline shape (CUB 128 x 128, P = 10,
B = 64) and at BASELINE config #5's shape (256 x 256, P = 20, B = 16).

(a) Every canvas launch on synthetic sources: microseconds from device events, the minimum of `--repeats` readings of `--iters`
    launches each (all readings are printed), the bytes the launch writes, and the fraction of 8 TB/s those bytes reach.
(b) One image step against a plain step of the same trainer (bf16; config #5 runs in bf16 here as well, because `cross` is not
    rendered under fp8): milliseconds from device events around whole steps, the image step measured to the end of its canvases
    on the side stream.  The extra time is split into the `cross` decoding (launching stream) and the canvases (side stream).
(c) PNG encoding of every canvas of that step on the writer's thread: milliseconds per canvas and in total.
Prints one JSON line per row.

    python tools/bench_imglog.py [--iters 20] [--repeats 5] [--skip-model]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cub128 P10 B64": (128, 10, 64, "cub128p10"), "256x256 P20 B16": (256, 20, 16, "cub256p20")}
HBM_BYTES_PER_S = 8e12


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
    from upsparts_amd import imglog as IL, ops
    dev = torch.device("cuda:0")
    for name, (S, P, B, _) in SHAPES.items():
        g = torch.Generator().manual_seed(S + P)
        views = [(torch.rand(B, S, S, 3, generator=g) * 2 - 1).to(dev) for _ in range(2)]
        gen = (torch.rand(B, S, S, 8, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        m = torch.softmax(3 * torch.randn(2 * B, S, S, P, generator=g), -1).to(dev)
        am = m.argmax(-1)
        hard = torch.nn.functional.one_hot(am, P).float()
        bits = (1 << am).to(torch.int32)
        colors = torch.from_numpy(IL.mask_color_bytes(IL.mask_colors01(P))).to(dev)
        table = torch.from_numpy(IL.viridis_bytes()).to(dev)
        launches = {
            "images fp32 ld3": lambda: ops.canvas_images(views[0]),
            "images bf16 ld8": lambda: ops.canvas_images(gen),
            "mask_rgb argmax": lambda: ops.canvas_mask_rgb(colors, mask=m[:B]),
            "mask_rgb one-hot row": lambda: ops.canvas_mask_rgb(colors, mask=hard[:B], one_hot=True, cols=B),
            "mask_rgb bits row": lambda: ops.canvas_mask_rgb(colors, bits=bits[:B], n_parts=P, cols=B),
            "assigned_parts fp32 masks": lambda: ops.canvas_assigned_parts(views[0], views[1], hard0=hard[:B], hard1=hard[B:]),
            "assigned_parts bits": lambda: ops.canvas_assigned_parts(views[0], views[1], bits0=bits[:B], bits1=bits[B:], n_parts=P),
            "first_item bits": lambda: ops.canvas_first_item(m[0], table, bits=bits[0]),
        }
        for what, fn in launches.items():
            out = fn()
            written = sum(o.numel() for o in out) if isinstance(out, tuple) else out.numel()
            del out
            ts = [timed(fn, iters) for _ in range(repeats)]
            print(json.dumps({"row": "canvas", "shape": name, "launch": what, "bytes_written": written, "us": round(min(ts), 1),
                              "us_all": [round(t, 1) for t in ts], "write_gbs": round(written / min(ts) * 1e-3, 1),
                              "fraction_of_8TBs": round(written / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4)}), flush=True)
        del views, gen, m, hard, bits


def step_rows(repeats):
    from upsparts_amd import configs, imglog as IL
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    for name, (S, P, B, key) in SHAPES.items():
        cfg = configs.BENCH_CONFIGS[key][0](B)
        cfg["precision"] = "bf16"
        cfg["log_images"] = True
        model = TrainModel(cfg, device=dev, seed=0)
        tr = Trainer(cfg, None, model)
        g = torch.Generator().manual_seed(1234)
        batch = {k: (torch.rand(B, S, S, 3, generator=g) * 2 - 1).to(dev) for k in ("view0", "view1", "view0_target")}
        for _ in range(4):
            tr.train_step(batch)
        tr.train_step(batch, images=True)
        torch.cuda.synchronize()

        def one(images):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            tr.train_step(batch, images=images)
            e[1].record()                               # launching stream: the step (+ the `cross` decoding of an image step)
            if images:
                with torch.cuda.stream(tr._img["stream"]):
                    e[2].record()                       # side stream: the canvases
            torch.cuda.synchronize()
            return e[0].elapsed_time(e[1]), (e[0].elapsed_time(e[2]) if images else None)
        plain, img_main, img_all = [], [], []
        for _ in range(repeats):                        # alternated readings
            plain.append(one(False)[0])
            a, b = one(True)
            img_main.append(a); img_all.append(b)
            plain.append(one(False)[0])                 # (the step after an image step waits for its canvases: counted as plain)
        print(json.dumps({"row": "step", "shape": name, "precision": "bf16", "plain_ms": round(min(plain), 2),
                          "plain_ms_all": [round(v, 2) for v in plain], "image_step_launching_stream_ms": round(min(img_main), 2),
                          "image_step_with_canvases_ms": round(min(img_all), 2), "image_ms_all": [round(v, 2) for v in img_all],
                          "extra_cross_decoding_ms": round(min(img_main) - min(plain), 2),
                          "extra_canvases_ms": round(min(img_all) - min(img_main), 2)}), flush=True)
        imgs = tr.fetch_images()
        if IL.have_pil():
            with tempfile.TemporaryDirectory() as tmp:
                w, per = IL.ImageWriter(tmp), {}

                def encode(path, a, _enc=IL.encode_png):
                    t0 = time.perf_counter()
                    _enc(path, a)
                    per[os.path.basename(path)] = round((time.perf_counter() - t0) * 1e3, 2)
                w.encode = encode
                w.submit(0, imgs)
                w.close()
            print(json.dumps({"row": "png", "shape": name, "canvas_MB": round(sum(v.size for v in imgs.values()) / 1e6, 2),
                              "encode_ms_total": round(sum(per.values()), 1), "encode_ms": per}), flush=True)
        del tr, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_imglog.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    kernel_rows(args.iters, args.repeats)
    if not args.skip_model:
        step_rows(args.repeats)


if __name__ == "__main__":
    main()
