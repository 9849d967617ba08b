"""What the run-length annotations cost (csrc/segrle.hip; ops.segment_rle, TrainModel.export_segments(rle=True), the runner's
`segment_annotations: coco`).

(a) kernel    event time of ups_segment_rle_count (5 launches) and ups_segment_rle_write (1 launch) at the export's shape, 128
              planes of 375 x 500 uint8, P = 10, on block-constant labels and on seeded noise (the worst case: about one transition
              per pixel and 8 bytes written per byte read).  Three operand sets are rotated; a reading is `--iters` calls between two
              events, the minimum of `--repeats` readings is reported and all are printed.  `fraction_of_8TBs` is the share of 8 TB/s
              on the bytes that MUST move (count: the plane read, offsets / area / bbox written; write: the plane read, the counts
              written).  ops.segment_rle as a whole (both calls, the read of the total and the allocations) is timed with a host clock.
(b) host      the NumPy restatement (labels.T.ravel, np.diff, np.flatnonzero per part) on the host, including the device-to-host copy
              of the plane it needs, on the same labels -- on a SUBSET of the planes, stated in the row, and scaled to the whole.
(c) export    runner.segment_files over 256 synthetic 375 x 500 PNG files: `segment_outputs: [labels]` without annotations (the PNG
              route as it was), `segment_outputs: []` with `segment_annotations: coco` (annotations alone), and both, in the same run.
Synthetic inputs throughout: what a trained checkpoint's maps cost is not measured.  Prints one JSON line per row.

    python tools/bench_rle.py > profiles/bench_rle.jsonl
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
NOTE = "synthetic labels (block-constant, seeded noise), seeded weights, enlarged noise images: not a trained model's part maps"


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


def make_plane(kind, g, dev, N, h, w, P, total):
    if kind == "blocks":          # block-constant: 16 x 16 blocks of one part each
        small = torch.randint(0, P, (N, -(-h // 16), -(-w // 16)), generator=g, device=dev)
        m = small.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :h, :w]
    else:
        m = torch.randint(0, P, (N, h, w), generator=g, device=dev)
    plane = torch.zeros(total, dtype=torch.uint8, device=dev)
    plane.view(N, total // N)[:, :h * w] = m.to(torch.uint8).reshape(N, h * w)
    return plane


def host_encode(plane_dev, table, P, images):
    """The restatement on the host: the copy of the plane, then per image and part transpose, diff, flatnonzero, diff."""
    t0 = time.perf_counter()
    plane = plane_dev.cpu().numpy()
    t_copy = time.perf_counter() - t0
    n_counts = 0
    t0 = time.perf_counter()
    for off, h, w, _ in table[:images].tolist():
        col = plane[off:off + h * w].reshape(h, w).T.ravel()
        for p in range(P):
            m = (col == p).astype(np.int8)
            T = np.flatnonzero(np.diff(np.concatenate([[0], m])))
            n_counts += np.diff(np.concatenate([[0], T, [m.size]])).size
    return t_copy, time.perf_counter() - t0, n_counts


def kernel_rows(iters, repeats, host_images):
    import ctypes as C
    from upsparts_amd import lib as L, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    N, h, w, P, nsets = 128, 375, 500, 10, 3
    tab, total = ops.segment_table([(h, w)] * N)
    td = torch.from_numpy(tab).to(dev)
    th = tab.ctypes.data_as(C.POINTER(C.c_int32))
    lib = L.load()
    px = N * h * w
    for kind in ("blocks", "noise"):
        sets = [make_plane(kind, g, dev, N, h, w, P, total) for _ in range(nsets)]
        offsets = [torch.empty(N * P + 1, dtype=torch.int64, device=dev) for _ in range(nsets)]
        area = torch.empty((N, P), dtype=torch.int32, device=dev)
        bbox = torch.empty((N, P, 4), dtype=torch.int32, device=dev)
        scratch = [torch.empty(lib.ups_segment_rle_scratch_bytes(N, total, P) // 8 + 1, dtype=torch.int64, device=dev) for _ in range(nsets)]

        def count(k):
            j = k % nsets
            L.call("ups_segment_rle_count", L.ptr(sets[j]), N, th, L.ptr(td), total, P, L.ptr(offsets[j]), L.ptr(area), L.ptr(bbox),
                   L.ptr(scratch[j]), L.stream())

        for j in range(nsets):
            count(j)
        totals = [int(o[-1].item()) for o in offsets]
        counts = [torch.empty(t, dtype=torch.int32, device=dev) for t in totals]

        def write(k):
            j = k % nsets
            L.call("ups_segment_rle_write", L.ptr(sets[j]), N, th, L.ptr(td), total, P, L.ptr(offsets[j]), L.ptr(scratch[j]),
                   L.ptr(counts[j]), totals[j], totals[j], L.stream())

        for j in range(nsets):
            write(j)
        # the wrapper's result on the first set is the launches' (and the reference's on the first images, below)
        whole = ops.segment_rle(sets[0], P, table=(tab, td, total))
        assert torch.equal(whole["counts"], counts[0]) and torch.equal(whole["offsets"], offsets[0])
        common = {"shape": "export", "N": N, "h": h, "w": w, "P": P, "labels": kind, "input_sets": nsets, "calls_per_reading": iters,
                  "counts_per_pixel": round(totals[0] / px, 4)}
        for launch, fn, nbytes in (("ups_segment_rle_count (5 launches)", count, px + (N * P + 1) * 8 + N * P * 20),
                                   ("ups_segment_rle_write (1 launch)", write, px + totals[0] * 4)):
            for k in range(2 * nsets):
                fn(k)
            ts = event_us(fn, iters, repeats)
            emit(dict(common, row="kernel", launch=launch, us=round(min(ts), 1), us_all=[round(t, 1) for t in ts],
                      bytes_that_must_move=nbytes, GBps=round(nbytes / min(ts) * 1e-3, 1),
                      fraction_of_8TBs=round(nbytes / (min(ts) * 1e-6) / HBM_BYTES_PER_S, 4),
                      note="not tuned; the reads follow columns of a row-major plane, the noise map writes 8 bytes per byte read"))
        walls = []
        for k in range(2 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.segment_rle(sets[k % nsets], P, table=(tab, td, total))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        walls = walls[2:]
        emit(dict(common, row="wrapper", route="ops.segment_rle: both calls, the read of the total, the allocations (host clock)",
                  s=round(min(walls), 5), s_all=[round(t, 5) for t in walls]))
        t_copy, t_enc, n_counts = host_encode(sets[0], tab, P, host_images)
        ref = whole["offsets"][host_images * P].item()
        assert n_counts == ref, (n_counts, ref)
        emit(dict(common, row="host", route="NumPy restatement per image and part on a SUBSET of the planes, after the device-to-host copy "
                  "of the whole plane", images_timed=host_images, copy_s=round(t_copy, 5), encode_s=round(t_enc, 4),
                  encode_s_scaled_to_all=round(t_enc * N / host_images, 3),
                  total_s_scaled_to_all=round(t_copy + t_enc * N / host_images, 3)))
        del sets, counts, scratch, whole
        torch.cuda.empty_cache()


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
    routes = (("png_labels", {"segment_outputs": ["labels"]}),
              ("annotations_only", {"segment_outputs": [], "segment_annotations": "coco"}),
              ("png_labels+annotations", {"segment_outputs": ["labels"], "segment_annotations": "coco"}))
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
        res, phases, sizes = {}, {}, {}
        for name, keys in routes:
            runner.segment_files(model, dict(cfg, **keys), os.path.join(tmp, "warm_" + name), 0)
        for r in range(repeats):                    # the routes alternate inside one run
            for name, keys in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runner.segment_files(model, dict(cfg, **keys), os.path.join(tmp, "{}{}".format(name, r)), 0)
                res.setdefault(name, []).append(time.perf_counter() - t0)
        for name, keys in routes:                   # where the time goes: one profiled (synchronised) run each
            prof = {}
            root = os.path.join(tmp, "prof_" + name)
            runner.segment_files(model, dict(cfg, **keys), root, 0, profile=prof)
            phases[name] = {k: round(v, 4) for k, v in prof.items()}
            ann = os.path.join(root, "segment", "0", "annotations.json")
            sizes[name] = os.path.getsize(ann) if os.path.exists(ann) else 0
    best = {k: min(v) for k, v in res.items()}
    emit({"row": "export", "images": n_images, "h": H, "w": W, "B": B, "S": 128, "P": model.n_parts, "config": "cub128p10",
          "precision": "bf16", "seconds": {k: round(v, 3) for k, v in best.items()},
          "seconds_all": {k: [round(t, 3) for t in v] for k, v in res.items()},
          "annotations_only_over_png": round(best["annotations_only"] / best["png_labels"], 4),
          "annotations_added_to_png_s": round(best["png_labels+annotations"] - best["png_labels"], 3),
          "phases_of_a_synchronised_run": phases, "annotations_json_bytes": sizes,
          "note": NOTE + "; png_labels is the export as it was before the keys existed, timed in the same run"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-images", type=int, default=8)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rle.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "note": NOTE})
    kernel_rows(args.iters, max(args.repeats, 3), args.host_images)
    if not args.skip_model:
        export_rows(args.images, args.repeats)


if __name__ == "__main__":
    main()
