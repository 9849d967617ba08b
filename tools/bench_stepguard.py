"""What the guarded optimizer step (csrc/stepguard.hip) costs.

(a) guard     ups_grad_guard (both launches) over the flat gradient bucket of every optimizer key of cub128p10, at the bucket's real size:
              device-event microseconds per call and the share of 8 TB/s its one read of the bucket reaches.  The calls ROTATE over
              operand sets whose bytes sum to `--sets-mib` (well above the 256 MiB Infinity Cache, as tools/hbm_roofline.py rotates):
              every call reads from HBM.  `--repeats` readings, all printed.
(b) adam      ups_adam_guarded against ups_adam_dev at the same sizes, rotated the same way (a set: p, g, m, v); 28 bytes per element
              move (p, m, v read and written, g read).
(c) step      Trainer.train_step on cub128p10 in img/s: batch 64 eager and batch 8 under hip_graph, bf16, one fixed device-resident
              batch, the trainer's own noise; `keys_off` (no key of the guard set: the step's launches are the earlier ones) against
              `keys_on` (skip_nonfinite: True, grad_clip_norm: 100), alternated readings.  `--tree DIR` imports the package from another
              checkout of this project (with its library built) instead of this one -- a checkout from before the guard knows no keys:
              `--variants keys_off` -- and `--label` names the tree in the rows, so that one session can put both side by side.
Appends one JSON line per row.

    python tools/bench_stepguard.py [--repeats 3] [--steps 40] >> profiles/bench_stepguard.jsonl
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 8.0


def emit(row):
    print(json.dumps(row), flush=True)


def _event_us(fns, calls):
    """Mean device time per call of `calls` calls that walk round-robin over fns (one per operand set)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def bucket_sizes(dev):
    """{optimizer key: elements of its flat bucket} of cub128p10 (the model is built once and dropped)."""
    from upsparts_amd import configs
    from upsparts_amd.model import TrainModel
    cfg = configs.cub_config(10, 8)
    cfg["precision"] = "bf16"
    model = TrainModel(cfg, device=dev, seed=0)
    sizes = {k: int(g["flat"]["g"].numel()) for k, g in model.bank.groups.items()}
    del model
    torch.cuda.empty_cache()
    return sizes


def _stats(vals):
    return {"mean": round(sum(vals) / len(vals), 2), "all": [round(v, 2) for v in vals], "spread": round(max(vals) - min(vals), 2)}


def guard_rows(sizes, sets_mib, repeats, label):
    from upsparts_amd import lib as L, ops
    dev = torch.device("cuda:0")
    for key, n in sizes.items():
        nsets = max(3, -(-sets_mib * (1 << 20) // (4 * n)))
        nsets = min(nsets, 4096)
        bufs = [torch.randn(n, dtype=torch.float32, device=dev) for _ in range(nsets)]
        recs = ops.guard_records(nsets, dev)
        fns = [(lambda g=g, r=recs[i]: ops.grad_guard(g, r, 1.0, 1.0, True)) for i, g in enumerate(bufs)]
        calls = max(2 * nsets, 60)
        _event_us(fns, calls)                   # warm-up: every set touched
        us = [_event_us(fns, calls) for _ in range(repeats)]
        mean = sum(us) / len(us)
        emit({"row": "guard", "tree": label, "key": key, "elements": n, "bucket_mb": round(4 * n / 1e6, 2), "operand_sets": nsets,
              "rotated_mib": round(nsets * 4 * n / (1 << 20), 1), "calls_per_reading": calls, "chunk": L.load().ups_grad_guard_chunk(),
              "us": _stats(us), "gb_per_s": round(4 * n / mean / 1e3, 1), "share_of_8_tb_s": round(4 * n / mean / 1e6 / HBM_TBS, 3)})
        del bufs, fns


def adam_rows(sizes, sets_mib, repeats, label):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    lr = torch.tensor([1e-4], dtype=torch.float32, device=dev)
    for key, n in sizes.items():
        nsets = min(max(3, -(-sets_mib * (1 << 20) // (16 * n))), 1024)
        sets = [[torch.randn(n, dtype=torch.float32, device=dev) for _ in range(3)] + [torch.rand(n, dtype=torch.float32, device=dev)]
                for _ in range(nsets)]
        recs = ops.guard_records(nsets, dev)
        for i, s in enumerate(sets):            # (scale 1 or below, skip 0: the guarded kernel does the whole update)
            ops.grad_guard(s[1], recs[i], 1.0, 1e9, True)
        routes = {"ups_adam_dev": [(lambda s=s: ops.adam_step(s[0], s[1], s[2], s[3], lr, 0.5, 0.9, 1e-8, 1.0)) for s in sets],
                  "ups_adam_guarded": [(lambda s=s, r=recs[i]: ops.adam_step(s[0], s[1], s[2], s[3], lr, 0.5, 0.9, 1e-8, 1.0, guard=r))
                                       for i, s in enumerate(sets)]}
        calls = max(2 * nsets, 40)
        us = {k: [] for k in routes}
        for fns in routes.values():
            _event_us(fns, calls)
        for _ in range(repeats):                # alternated
            for k, fns in routes.items():
                us[k].append(_event_us(fns, calls))
        row = {"row": "adam", "tree": label, "key": key, "elements": n, "operand_sets": nsets,
               "rotated_mib": round(nsets * 16 * n / (1 << 20), 1), "calls_per_reading": calls}
        for k in routes:
            mean = sum(us[k]) / len(us[k])
            row[k + "_us"] = _stats(us[k])
            row[k + "_share_of_8_tb_s"] = round(28 * n / mean / 1e6 / HBM_TBS, 3)
        row["guarded_over_dev"] = round(row["ups_adam_guarded_us"]["mean"] / row["ups_adam_dev_us"]["mean"], 3)
        emit(row)
        del sets, routes


def step_rows(steps, repeats, label, variants):
    from upsparts_amd import configs
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    keys = {"keys_off": {}, "keys_on": {"skip_nonfinite": True, "grad_clip_norm": 100.0}}
    for B, graph in ((64, False), (8, True)):
        g = torch.Generator().manual_seed(1234)
        batch = {k: (torch.rand(B, 128, 128, 3, generator=g) * 2 - 1).to(dev) for k in ("view0", "view1", "view0_target")}
        trainers = {}
        for name in variants:
            cfg = configs.cub_config(10, B)
            cfg.update(precision="bf16", hip_graph=graph)
            cfg.update(keys[name])
            trainers[name] = Trainer(cfg, None, TrainModel(cfg, device=dev, seed=0))

        def run(name, n):
            for _ in range(n):
                trainers[name].train_step(batch)
            torch.cuda.synchronize()
        for name in variants:                   # warm-up: kernel attributes, allocator pools, the capture
            run(name, 8)
        rates = {k: [] for k in variants}
        for _ in range(repeats):
            for name in variants:               # alternated
                t0 = time.perf_counter()
                run(name, steps)
                rates[name].append(steps * B / (time.perf_counter() - t0))
        row = {"row": "step", "tree": label, "config": "cub128p10", "batch": B, "hip_graph": graph, "precision": "bf16",
               "steps_per_reading": steps, "readings": repeats}
        for name in variants:
            row[name + "_img_per_s"] = _stats(rates[name])
            row[name + "_ms_per_step"] = round(1e3 * B / (sum(rates[name]) / len(rates[name])), 3)
            row[name + "_captured"] = bool(trainers[name].graph is not None and trainers[name].graph.graphs)
        if "keys_on" in variants:
            rep = trainers["keys_on"].guard_report()
            row["keys_on_skipped"] = sum(r["skipped"] for r in rep.values())
            row["keys_on_grad_norms"] = {k: round(r["norm"], 4) for k, r in rep.items() if k != "state"}
            if "keys_off" in variants:
                row["keys_on_over_keys_off"] = round(row["keys_on_img_per_s"]["mean"] / row["keys_off_img_per_s"]["mean"], 4)
        emit(row)
        del trainers
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--sets-mib", type=int, default=800, help="rotate operand sets until their bytes sum to at least this (>> 256 MiB)")
    ap.add_argument("--rows", default="guard,adam,step")
    ap.add_argument("--variants", default="keys_off,keys_on")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    assert torch.cuda.is_available(), "bench_stepguard.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    rows = args.rows.split(",")
    emit({"row": "about", "tree": args.label, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": rows})
    dev = torch.device("cuda:0")
    if "guard" in rows or "adam" in rows:
        sizes = bucket_sizes(dev)
    if "guard" in rows:
        guard_rows(sizes, args.sets_mib, max(args.repeats, 3), args.label)
    if "adam" in rows:
        adam_rows(sizes, args.sets_mib, max(args.repeats, 3), args.label)
    if "step" in rows:
        step_rows(args.steps, max(args.repeats, 3), args.label, args.variants.split(","))


if __name__ == "__main__":
    main()
