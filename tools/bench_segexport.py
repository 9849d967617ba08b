"""What the segmentation export costs (`upsparts-run --segment`; csrc/segexport.hip, ops.segment_render, runner.segment_files).

(a) kernel   event time of ups_segment_render at n = 128 maps [128 x 128, P = 10], every image rendered at 375 x 500 with labels, overlay
             and counts, input sets (soft maps and source images) rotated over more than the Infinity Cache: microseconds per call
             (minimum of `--repeats` readings of `--iters` calls, all printed) and the share of 8 TB/s on the bytes it must move
             (3 read + 4 written per pixel, plus `soft` once).
(a') guided  the edge-aware route in the SAME run and on the same rotated inputs: ups_segment_guide alone, and
             ups_segment_render_guided (sigma = 16) for R = 0, 1, 2 with its ratio to the plain kernel row above.
(b) torch    the same result with torch ops on the device, per image: interpolate(bilinear, align_corners=False) in float64, arg-max,
             colour gather, blend, bincount; the share of label and overlay bytes that differ from the kernel's is in the row.
(c) export   runner.segment_files over `--images` synthetic PNG files of 375 x 500 (cub128p10, bf16, seeded weights, batch 64): wall
             clock of the whole call, and -- from a second, phase-synchronised call -- its split into decode, model passes, packing
             and upload of the source images, kernel, copies and PNG encode.
Prints one JSON line per row.

    python tools/bench_segexport.py [--images 512] [--repeats 3] > profiles/bench_segexport.jsonl
"""
import argparse
import ctypes as C
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
NOTE = "synthetic images (enlarged noise blocks) and seeded weights: not CUB photographs and not a trained model's masks"


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


def torch_render(soft, views, colors, alpha, P):
    """The kernel's result by torch ops, image by image.  views: the per-image source views [h,w,3] uint8 of the packed plane."""
    import torch.nn.functional as F
    labels, overlays, counts = [], [], []
    for i, src in enumerate(views):
        h, w = src.shape[:2]
        v = F.interpolate(soft[i].permute(2, 0, 1)[None].double(), size=(h, w), mode="bilinear", align_corners=False)[0]
        lab = v.argmax(dim=0)
        col = colors[lab]
        overlays.append(torch.floor(alpha * col.double() + (1.0 - alpha) * src.double() + 0.5).clamp_(0, 255).to(torch.uint8))
        labels.append(lab.to(torch.uint8))
        counts.append(torch.bincount(lab.reshape(-1), minlength=P))
    return labels, overlays, torch.stack(counts)


def kernel_rows(iters, repeats, sets_mib):
    from upsparts_amd import imglog as IL, lib as L, ops
    dev = torch.device("cuda:0")
    n, S, P, H, W, alpha = 128, 128, 10, 375, 500, 0.5
    sizes = [(H, W)] * n
    table, total = ops.segment_table(sizes)
    table_dev = torch.from_numpy(table).to(dev)
    colors = torch.from_numpy(IL.mask_color_bytes(IL.mask_colors01(P))).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    set_bytes = n * S * S * P * 4 + total * 3
    nsets = max(3, -(-sets_mib * (1 << 20) // set_bytes))
    sets = []
    for _ in range(nsets):
        # smooth maps (a soft-max of enlarged noise): piecewise-constant labels, as a trained model's
        z = torch.nn.functional.interpolate(torch.randn((n, P, 8, 8), generator=g, device=dev) * 4, size=(S, S), mode="bilinear")
        soft = torch.softmax(z.permute(0, 2, 3, 1), dim=3).contiguous()
        sets.append((soft, torch.randint(0, 256, (total, 3), generator=g, device=dev, dtype=torch.uint8)))
    labels = torch.zeros(total, dtype=torch.uint8, device=dev)
    overlay = torch.zeros((total, 3), dtype=torch.uint8, device=dev)
    counts = torch.zeros((n, P), dtype=torch.int32, device=dev)
    tp = table.ctypes.data_as(C.POINTER(C.c_int32))

    def launch(k):
        soft, src = sets[k % nsets]
        L.call("ups_segment_render", L.ptr(soft), n, S, P, tp, L.ptr(table_dev), total, L.ptr(src), L.ptr(colors), alpha, L.ptr(labels),
               L.ptr(overlay), None, L.ptr(counts), L.stream())
    nk = max(iters, 2 * nsets)
    for k in range(nsets):
        launch(k)
    torch.cuda.synchronize()
    ts = event_us(launch, nk, repeats)
    pixels = n * H * W
    moved = 7 * pixels + n * S * S * P * 4
    common = {"n": n, "S": S, "P": P, "h": H, "w": W, "outputs": "labels + overlay + counts", "input_sets": nsets,
              "input_sets_MB": round(nsets * set_bytes / 1e6, 1), "bytes_to_move": moved}
    emit(dict(common, row="kernel", launch="ups_segment_render", calls_per_reading=nk, us=round(min(ts), 2), us_all=[round(t, 2) for t in ts],
              GBps=round(moved / min(ts) * 1e-3, 1), fraction_of_8TBs=round(moved / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4),
              Mpixels_per_s=round(pixels / min(ts), 1)))
    # the edge-aware route on the same rotated inputs: the guide launch alone, then the guided kernel per radius (the guide of set k
    # is made once, outside the timed calls)
    guides = [torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(nsets)]
    range_w = torch.from_numpy(ops.segment_range_table(16.0)).to(dev)

    def launch_guide(k):
        L.call("ups_segment_guide", L.ptr(sets[k % nsets][1]), n, S, tp, L.ptr(table_dev), total, L.ptr(guides[k % nsets]), L.stream())
    for k in range(nsets):
        launch_guide(k)
    torch.cuda.synchronize()
    tg = event_us(launch_guide, nk, repeats)
    gmoved = 3 * pixels + 3 * n * S * S
    emit(dict(common, row="guide", launch="ups_segment_guide", outputs="guide", bytes_to_move=gmoved, calls_per_reading=nk,
              us=round(min(tg), 2), us_all=[round(t, 2) for t in tg], GBps=round(gmoved / min(tg) * 1e-3, 1)))
    for radius in (0, 1, 2):
        def launch_guided(k, radius=radius):
            soft, src = sets[k % nsets]
            L.call("ups_segment_render_guided", L.ptr(soft), n, S, P, tp, L.ptr(table_dev), total, L.ptr(src), L.ptr(guides[k % nsets]),
                   L.ptr(range_w), radius, L.ptr(colors), alpha, L.ptr(labels), L.ptr(overlay), None, L.ptr(counts), L.stream())
        for k in range(nsets):
            launch_guided(k)
        torch.cuda.synchronize()
        tr = event_us(launch_guided, nk, repeats)
        emit(dict(common, row="guided", launch="ups_segment_render_guided", radius=radius, sigma=16.0, taps=(2 * radius + 2) ** 2,
                  calls_per_reading=nk, us=round(min(tr), 2), us_all=[round(t, 2) for t in tr],
                  ratio_to_plain_kernel=round(min(tr) / min(ts), 2), Mpixels_per_s=round(pixels / min(tr), 1)))
    del guides
    # the torch composition on set 0, and how its bytes compare
    soft, src = sets[0]
    views = ops.segment_views(src, table)
    counts.zero_()
    launch(0)
    tl, to, tc = torch_render(soft, views, colors, alpha, P)
    kl, ko = ops.segment_views(labels, table), ops.segment_views(overlay, table)
    dl = sum(int((a != b).sum()) for a, b in zip(tl, kl))
    do = sum(int((a != b).sum()) for a, b in zip(to, ko))
    dc = int((tc != counts.long()).sum())
    nt = max(2, nk // 20)
    tt = event_us(lambda k: torch_render(sets[k % nsets][0], ops.segment_views(sets[k % nsets][1], table), colors, alpha, P), nt,
                  min(repeats, 3))
    emit(dict(common, row="torch", launch="torch ops per image, float64 interpolate", calls_per_reading=nt, us=round(min(tt), 2),
              us_all=[round(t, 2) for t in tt], kernel_speedup=round(min(tt) / min(ts), 2),
              differing_label_bytes=dl, differing_overlay_bytes=do, differing_counts=dc,
              differing_byte_share=(dl + do) / float(4 * pixels)))
    del sets
    torch.cuda.empty_cache()


def export_rows(n_images, repeats, refine=False):
    from PIL import Image
    from upsparts_amd import configs, runner
    from upsparts_amd.model import TrainModel
    dev = torch.device("cuda:0")
    B, H, W = 64, 375, 500
    cfg = configs.BENCH_CONFIGS["cub128p10"][0](B)
    cfg.update({"precision": "bf16"})
    model = TrainModel(cfg, device=dev, seed=0)
    rng = np.random.RandomState(3)
    with tempfile.TemporaryDirectory() as tmp:
        droot = os.path.join(tmp, "images")
        os.makedirs(droot)
        rels = []
        for i in range(n_images):
            rel = "img_{:04d}.png".format(i)
            Image.fromarray(rng.randint(0, 256, size=(12, 16, 3)).astype(np.uint8)).resize((W, H), Image.BILINEAR).save(os.path.join(droot, rel))
            rels.append(rel)
        with open(os.path.join(tmp, "list.csv"), "w") as f:
            f.write("\n".join(rels) + "\n")
        cfg.update({"data_root": droot, "segment_csv": os.path.join(tmp, "list.csv")})
        if refine:
            cfg.update({"segment_refine": "bilateral"})
        runner.segment_files(model, cfg, os.path.join(tmp, "warm"), 0)
        walls = []
        for r in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.segment_files(model, cfg, os.path.join(tmp, "run{}".format(r)), 0)
            walls.append(time.perf_counter() - t0)
        split = {}
        t0 = time.perf_counter()
        runner.segment_files(model, cfg, os.path.join(tmp, "split"), 0, profile=split)
        tsplit = time.perf_counter() - t0
    emit({"row": "export_refine" if refine else "export", "segment_refine": "bilateral (radius 1, sigma 16)" if refine else "none",
          "images": n_images, "h": H, "w": W, "B": B, "S": 128, "P": model.n_parts, "config": "cub128p10", "precision": "bf16",
          "outputs": "labels + overlay", "export_s": round(min(walls), 3), "export_s_all": [round(t, 3) for t in walls],
          "images_per_s": round(n_images / min(walls), 1), "phase_synchronised_s": round(tsplit, 3),
          "split_s": {k: round(v, 4) for k, v in split.items()}, "note": NOTE})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets-mib", type=int, default=400, help="rotate input sets until they sum to at least this (> 256 MiB)")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segexport.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "images": args.images, "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 5), args.sets_mib)
    if not args.skip_model:
        export_rows(args.images, args.repeats)
        export_rows(args.images, args.repeats, refine=True)


if __name__ == "__main__":
    main()
