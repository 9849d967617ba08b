"""What the weight EMA (csrc/ema.hip) costs.

(i)   update    ups_ema_update (both launches) over the flat buckets of ALL optimizer keys of cub128p10 in ONE call, at their real sizes:
                device-event microseconds per call and the share of 8 TB/s that 12 bytes per parameter (shadow read and written, weights
                read) reach.  The calls ROTATE over operand sets whose bytes sum to `--sets-mib` (well above the 256 MiB Infinity Cache,
                as tools/hbm_roofline.py rotates): every call reads from HBM.  `--repeats` readings, all printed.  The swap (16 bytes
                per parameter) is timed the same way.
(ii)  the same for cub256p20's sizes.
(iii) step      Trainer.train_step on cub128p10 in img/s: batch 64 eager and batch 8 under hip_graph, bf16, one fixed device-resident
                batch of synthetic views, seeded weights, the trainer's own noise; `ema_off` (the key unset: the step's launches are the
                earlier ones) against `ema_on` (ema_decay: 0.999), alternated readings.
Appends one JSON line per row.

    python tools/bench_ema.py [--repeats 3] [--steps 40] >> profiles/bench_ema.jsonl
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


def _stats(vals):
    return {"mean": round(sum(vals) / len(vals), 2), "all": [round(v, 2) for v in vals], "spread": round(max(vals) - min(vals), 2)}


def bucket_sizes(cfg, dev):
    """{optimizer key: elements of its flat bucket} of the config's model (built once and dropped)."""
    from upsparts_amd.model import TrainModel
    cfg = dict(cfg, precision="bf16")
    model = TrainModel(cfg, device=dev, seed=0)
    sizes = {k: int(g["flat"]["p"].numel()) for k, g in model.bank.groups.items()}
    del model
    torch.cuda.empty_cache()
    return sizes


def update_rows(name, sizes, sets_mib, repeats):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    total = sum(sizes.values())
    nsets = min(max(3, -(-sets_mib * (1 << 20) // (8 * total))), 256)
    sets = []
    for _ in range(nsets):
        triples = [(torch.randn(n, dtype=torch.float32, device=dev), torch.randn(n, dtype=torch.float32, device=dev), None)
                   for n in sizes.values()]
        sets.append(ops.EmaItems(triples))
    n_upd = torch.zeros(len(sizes), dtype=torch.int64, device=dev)
    omd = torch.zeros(len(sizes), dtype=torch.float32, device=dev)
    routes = {"update": ([(lambda it=it: ops.ema_update(it, n_upd, omd, 0.999, True)) for it in sets], 12),
              "swap": ([(lambda it=it: ops.ema_swap(it)) for it in sets], 16)}
    calls = max(2 * nsets, 40)
    for what, (fns, bytes_per) in routes.items():
        _event_us(fns, calls)                   # warm-up: every set touched
        us = [_event_us(fns, calls) for _ in range(repeats)]
        mean = sum(us) / len(us)
        emit({"row": what, "config": name, "keys": len(sizes), "elements": total, "largest_bucket": max(sizes.values()),
              "smallest_bucket": min(sizes.values()), "mb_moved": round(bytes_per * total / 1e6, 2), "bytes_per_parameter": bytes_per,
              "operand_sets": nsets, "rotated_mib": round(nsets * 8 * total / (1 << 20), 1), "calls_per_reading": calls,
              "launches_per_call": 2 if what == "update" else 1, "us": _stats(us),
              "gb_per_s": round(bytes_per * total / mean / 1e3, 1), "share_of_8_tb_s": round(bytes_per * total / mean / 1e6 / HBM_TBS, 3)})
    del sets, routes


def step_rows(steps, repeats, variants):
    from upsparts_amd import configs
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    keys = {"ema_off": {}, "ema_on": {"ema_decay": 0.999}}
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
        row = {"row": "step", "config": "cub128p10", "batch": B, "hip_graph": graph, "precision": "bf16", "data": "synthetic views, seeded weights",
               "steps_per_reading": steps, "readings": repeats}
        for name in variants:
            row[name + "_img_per_s"] = _stats(rates[name])
            row[name + "_ms_per_step"] = round(1e3 * B / (sum(rates[name]) / len(rates[name])), 3)
            row[name + "_captured"] = bool(trainers[name].graph is not None and trainers[name].graph.graphs)
        if "ema_on" in variants:
            row["ema_on_updates"] = dict(trainers["ema_on"].ema_report())
            if "ema_off" in variants:
                row["ema_on_over_ema_off"] = round(row["ema_on_img_per_s"]["mean"] / row["ema_off_img_per_s"]["mean"], 4)
        emit(row)
        del trainers
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--sets-mib", type=int, default=800, help="rotate operand sets until their bytes sum to at least this (>> 256 MiB)")
    ap.add_argument("--rows", default="update128,update256,step")
    ap.add_argument("--variants", default="ema_off,ema_on")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    assert torch.cuda.is_available(), "bench_ema.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    from upsparts_amd import configs
    rows = args.rows.split(",")
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": rows})
    dev = torch.device("cuda:0")
    if "update128" in rows:
        update_rows("cub128p10", bucket_sizes(configs.cub_config(10, 8), dev), args.sets_mib, max(args.repeats, 3))
    if "update256" in rows:
        update_rows("cub256p20", bucket_sizes(configs.cub256_config(20, 8), dev), args.sets_mib, max(args.repeats, 3))
    if "step" in rows:
        step_rows(args.steps, max(args.repeats, 3), args.variants.split(","))


if __name__ == "__main__":
    main()
