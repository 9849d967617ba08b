"""What the part-coherence kernels cost (csrc/components.hip; ops.label_components / label_component_stats / label_components_clean,
evalutil.CoherenceEvaluator, the runner's `segment_clean_min_area`).

(a) kernel    event time of the three entries at 128 maps of 128 x 128 int64 (P = 10: the part maps of validation) on block-constant
              maps, on seeded noise (the worst realistic case: every pixel its own tile-local root) and on the 256 x 256 spiral
              (the adversarial case: one chain across every tile border), and at 128 planes of 375 x 500 uint8 (the export's shape).
              Operand sets are rotated; a reading is `--iters` calls between two events, the minimum of `--repeats` readings is
              reported and all are printed.  `fraction_of_8TBs` is the share of 8 TB/s on the bytes that MUST move (labels read, comp
              written; labels + comp read, area written; labels + comp + area read, out written).  A propagation kernel chases
              dependent loads and sits far below that roof: the rows say so, nothing here was tuned for it.
(b) host      the same components on the host for comparison: scipy.ndimage.label per image and part when scipy is importable,
              otherwise evalutil.coherence_host (NumPy min-propagation) on a subset of 8 maps, stated as such.
(c) validate  Trainer.validate() over 512 synthetic pairs at batch 64 (cub128p10, bf16, seeded weights, noise images) with
              val_metrics [parts] -- the code path as it was before the metric existed -- and [parts, coherence], in the same run.
(d) export    runner.segment_files over 256 synthetic 375 x 500 PNG files without the clean-up (the path as it was) and with
              segment_clean_min_area = 64, in the same run.
Synthetic inputs throughout: what a trained checkpoint's maps cost or score is not measured.  Prints one JSON line per row.

    python tools/bench_components.py > profiles/bench_components.jsonl
"""
import argparse
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
NOTE = "synthetic maps (block-constant, seeded noise, a spiral), seeded weights, noise images: not a trained model's part maps"


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


def spiral(side):
    """A one-pixel-wide spiral of part 1 in part 0 with one-pixel gaps (the generator of tests/components_ref.py, restated)."""
    m = np.zeros((side, side), dtype=np.int64)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = turns = 0
    m[0, 0] = 1
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ok = 0 <= ny < side and 0 <= nx < side and m[ny, nx] == 0 and (not (0 <= ay < side and 0 <= ax < side) or m[ay, ax] == 0)
        if ok:
            for sy, sx in ((dx, dy), (-dx, -dy)):
                ty, tx = ny + sy, nx + sx
                ok = ok and not (0 <= ty < side and 0 <= tx < side and m[ty, tx] == 1)
        if ok:
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def make_maps(kind, g, dev, N, h, w, P, dtype):
    if kind == "blocks":          # block-constant: 16 x 16 blocks of one part each
        small = torch.randint(0, P, (N, -(-h // 16), -(-w // 16)), generator=g, device=dev)
        m = small.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :h, :w]
    elif kind == "noise":
        m = torch.randint(0, P, (N, h, w), generator=g, device=dev)
    else:
        m = torch.from_numpy(spiral(h)).to(dev)[None].expand(N, h, w)
    return m.to(dtype).contiguous()


def kernel_rows(iters, repeats):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    P = 10
    for shape_name, N, h, w, dtype, kinds in (("validation", 128, 128, 128, torch.int64, ("blocks", "noise")),
                                              ("validation_256", 32, 256, 256, torch.int64, ("spiral",)),
                                              ("export", 128, 375, 500, torch.uint8, ("blocks", "noise"))):
        lb = 1 if dtype == torch.uint8 else 8
        for kind in kinds:
            nsets = 1 if kind == "spiral" else 3
            if shape_name == "export":          # packed planes, as the export holds them
                sizes = [(h, w)] * N
                tab, total = ops.segment_table(sizes)
                table = (tab, torch.from_numpy(tab).to(dev), total)
                stride = total // N
                sets = []
                for _ in range(nsets):
                    plane = torch.zeros(total, dtype=dtype, device=dev)
                    plane.view(N, stride)[:, :h * w] = make_maps(kind, g, dev, N, h, w, P, dtype).view(N, h * w)
                    sets.append(plane)
                kw = {"table": table}
            else:
                sets = [make_maps(kind, g, dev, N, h, w, P, dtype) for _ in range(nsets)]
                kw = {}
            px = N * h * w
            comps, areas = [], []
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            for s in sets:
                c, _ = ops.label_components(s, P, conn=8, err=err, **kw)
                a, st, _ = ops.label_component_stats(s, c, P, small=16, **kw)
                ops.label_components_clean(s, c, a, P, 16, **kw)
                comps.append(c), areas.append(a)
            ops.components_check(err)
            n_comp = int(st[:, :, 1].sum())
            common = {"shape": shape_name, "N": N, "h": h, "w": w, "P": P, "label_bytes": lb, "conn": 8, "maps": kind, "input_sets": nsets,
                      "calls_per_reading": iters, "components_in_last_set": n_comp}
            for launch, fn, nbytes in (
                    ("ups_label_components (3 launches)", lambda k: ops.label_components(sets[k % nsets], P, conn=8, err=err, **kw),
                     px * (lb + 4)),
                    ("ups_label_component_stats (memset + 2 launches)",
                     lambda k: ops.label_component_stats(sets[k % nsets], comps[k % nsets], P, small=16, **kw), px * (lb + 4 + 4)),
                    ("ups_label_components_clean (2 P + 2 launches)",
                     lambda k: ops.label_components_clean(sets[k % nsets], comps[k % nsets], areas[k % nsets], P, 16, **kw),
                     px * (lb + 4 + 4 + lb))):
                ts = event_us(fn, iters, repeats)
                emit(dict(common, row="kernel", launch=launch, us=round(min(ts), 1), us_all=[round(t, 1) for t in ts],
                          bytes_that_must_move=nbytes, GBps=round(nbytes / min(ts) * 1e-3, 1),
                          fraction_of_8TBs=round(nbytes / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4),
                          note="includes the wrapper's allocations; a propagation kernel chases dependent loads: far below the roof, not tuned"))
            if shape_name == "validation" or kind == "spiral":
                host_row(sets[0], P, common)
            del sets, comps, areas
            torch.cuda.empty_cache()


def host_row(maps, P, common):
    from upsparts_amd import evalutil
    m = maps.cpu().numpy()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        eight = np.ones((3, 3), dtype=np.int64)
        t0 = time.perf_counter()
        for i in range(m.shape[0]):
            for p in range(P):
                ndimage.label(m[i] == p, structure=eight)
        dt = time.perf_counter() - t0
        emit(dict(common, row="host", route="scipy.ndimage.label per image and part (labelling only, maps already on the host)",
                  maps_timed=int(m.shape[0]), s=round(dt, 4), us_per_map=round(dt / m.shape[0] * 1e6, 1)))
    else:
        k = min(8, m.shape[0])
        t0 = time.perf_counter()
        evalutil.coherence_host(m[:k], P, 8, 16)
        dt = time.perf_counter() - t0
        emit(dict(common, row="host", route="evalutil.coherence_host (NumPy min-propagation with pointer jumping) on a SUBSET of the maps; "
                  "scipy is not importable here", maps_timed=k, s=round(dt, 4), us_per_map=round(dt / k * 1e6, 1)))


def wall(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def validate_rows(n_pairs, repeats):
    from upsparts_amd import configs, data, evalutil
    from upsparts_amd.model import TrainModel, Trainer, coherence_config
    dev = torch.device("cuda:0")
    B, S = 64, 128
    cfg = configs.BENCH_CONFIGS["cub128p10"][0](B)
    cfg.update({"precision": "bf16"})
    model = TrainModel(cfg, device=dev, seed=0)
    trainer = Trainer(cfg, None, model)
    rng = np.random.RandomState(3)
    n = n_pairs // B * B
    pairs = data.ValidationPairs.__new__(data.ValidationPairs)          # a pair set of noise images without files
    pairs.batch_size, pairs._dev = B, None
    pairs.rows = pairs.pairs = np.stack([np.arange(n), rng.permutation(n)], 1).astype(np.int32)
    pairs.store = torch.from_numpy(rng.randint(0, 256, (n, S, S, 3), dtype=np.uint8))
    conn, speck = coherence_config(cfg)
    logs = {}
    res = {}
    for name, metrics in (("parts", ["parts"]), ("parts+coherence", ["parts", "coherence"])):
        trainer._val = {"metrics": metrics, "pairs": pairs, "usage": evalutil.PartUsageEvaluator(dev, model.n_parts, 0.005)}
        if "coherence" in metrics:
            trainer._val["coherence"] = evalutil.CoherenceEvaluator(dev, model.n_parts, conn, speck)
        res[name] = wall(lambda: logs.update(trainer.validate()), repeats)
    a, b = min(res["parts"]), min(res["parts+coherence"])
    emit({"row": "validate", "pairs": n, "B": B, "S": S, "P": model.n_parts, "config": "cub128p10", "precision": "bf16",
          "conn": conn, "speck_area_px": speck,
          "validate_parts_s": round(a, 4), "validate_parts_s_all": [round(t, 4) for t in res["parts"]],
          "validate_parts_coherence_s": round(b, 4), "validate_parts_coherence_s_all": [round(t, 4) for t in res["parts+coherence"]],
          "added_s": round(b - a, 4), "added_share": round((b - a) / a, 4),
          "values": {k: float(v) for k, v in logs.items() if "fragmentation" in k or "specks" in k or "components" in k},
          "note": NOTE + "; [parts] alone is the call as it was before the metric existed, timed in the same run"})


def export_rows(n_images, repeats):
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
        res = {}
        for name, keys in (("plain", {}), ("clean", {"segment_clean_min_area": 64})):
            c = dict(cfg, **keys)
            runner.segment_files(model, c, os.path.join(tmp, "warm_" + name), 0)
            walls = []
            for r in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runner.segment_files(model, c, os.path.join(tmp, "{}{}".format(name, r)), 0)
                walls.append(time.perf_counter() - t0)
            res[name] = walls
    a, b = min(res["plain"]), min(res["clean"])
    emit({"row": "export", "images": n_images, "h": H, "w": W, "B": B, "S": 128, "P": model.n_parts, "config": "cub128p10",
          "precision": "bf16", "outputs": "labels + overlay", "segment_clean_min_area": 64, "rounds": 1, "conn": 8,
          "export_plain_s": round(a, 3), "export_plain_s_all": [round(t, 3) for t in res["plain"]],
          "export_clean_s": round(b, 3), "export_clean_s_all": [round(t, 3) for t in res["clean"]],
          "added_s": round(b - a, 3), "added_share": round((b - a) / a, 4),
          "note": NOTE + "; the plain export is the path as it was before the key existed, timed in the same run"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_components.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 3))
    if not args.skip_model:
        validate_rows(args.pairs, args.repeats)
        export_rows(args.images, args.repeats)


if __name__ == "__main__":
    main()
