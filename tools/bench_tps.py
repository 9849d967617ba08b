"""What the device-side TPS parameter and solve kernel (csrc/tps.hip) costs and buys.

(a) params    the parameter route of 2 B samples, K = 9: the torch chain this tree used before (tps_parameters + make_input_tps_param +
              the fp64 torch.linalg.solve, kept below as `torch_route` for this comparison) against one launch of ups_tps_params, at
              n = 16 and n = 128.  Device-event microseconds per call over `--iters` calls, `--repeats` alternated readings (all are
              printed), and the number of device kernels per call as the torch profiler counts them (null where it is unavailable).
              Event time of a chain of small launches is launch-bound: it measures the host's launch rate as much as the device.
(b) training  Trainer.train_step on cub_config(n_parts=25, batch_size=8, use_tps=True), bf16, one fixed device-resident batch, the
              trainer's own noise: images per second of four variants, `--repeats` alternated readings of `--steps` steps each --
                eager            this tree, hip_graph False
                graph            this tree, hip_graph True (captured: the row records that tr.graph.graphs is non-empty)
                graph_no_tps     hip_graph True with use_tps False (the ceiling)
                eager_old_route  this tree's eager step with tps.make_tps replaced by the previous route (torch chain, the target's
                                 system solved a second time): what the step cost before the kernel existed
              and the singular counter of the three TPS variants after the run.
Appends one JSON line per row.

    python tools/bench_tps.py [--repeats 3] [--steps 40] >> profiles/bench_tps.jsonl
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(row):
    print(json.dumps(row), flush=True)


def torch_solve(coord, vector):
    """The fp64 torch solve tps.solve_system was before ups_tps_solve."""
    c = coord.double()
    n, K, _ = c.shape
    p = torch.cat([torch.ones(n, K, 1, dtype=c.dtype, device=c.device), c], dim=2)
    d2 = ((p.unsqueeze(2) - p.unsqueeze(1)) ** 2).sum(dim=3)
    r = d2 * torch.log(d2 + 1e-6)
    W = torch.cat([torch.cat([p, r], dim=2),
                   torch.cat([torch.zeros(n, 3, 3, dtype=c.dtype, device=c.device), p.transpose(1, 2)], dim=2)], dim=1)
    tp = torch.cat([c + vector.double(), torch.zeros(n, 3, 2, dtype=c.dtype, device=c.device)], dim=1)
    return torch.linalg.solve(W, tp).transpose(1, 2).contiguous().float()


def torch_route(PT, u, params):
    coord, vector = PT.make_input_tps_param(PT.tps_parameters(u.shape[0], uniforms=u, **params))
    return coord, vector, torch_solve(coord, vector)


def old_make_tps(PT, L):
    """tps.make_tps as it was: the torch chain, one concatenated warp, and a second solve for the target."""
    def warp(U, coord, vector):
        U, cd = U.contiguous().float(), coord.contiguous().float()
        n, h, w, c = U.shape
        T, out = torch_solve(coord, vector), torch.empty_like(U)
        L.call("ups_tps_warp", L.ptr(U), L.ptr(T), L.ptr(cd), L.ptr(out), n, h, w, c, cd.shape[1], L.stream())
        return out

    def make_tps(views, tps_params, uniforms=None, generator=None, n_singular=None):
        B = views[0].shape[0]
        batch = torch.cat(views[:2], dim=0)
        pd = PT.tps_parameters(2 * B, uniforms=uniforms, generator=generator, device=batch.device, **tps_params)
        coord, vector = PT.make_input_tps_param(pd)
        t = warp(batch, coord, vector)
        out = [t[:B], t[B:]]
        if len(views) > 2:
            out.append(warp(views[2], coord[:B], vector[:B]))
        return out
    return make_tps


def _event_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _kernels_per_call(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:
        return None


def params_rows(iters, repeats):
    from upsparts_amd import configs, tps as PT
    dev = torch.device("cuda:0")
    params = configs.cub_config(use_tps=True)["tps_parameters"]
    for n in (16, 128):
        u = torch.rand(n, PT.N_UNIFORMS, generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        ns = torch.zeros(1, dtype=torch.int32, device=dev)
        routes = {"torch_route": lambda: torch_route(PT, u, params), "ups_tps_params": lambda: PT.tps_system(u, params, n_singular=ns)}
        for fn in routes.values():          # warm up every shape
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in routes}
        for _ in range(repeats):            # alternated
            for k, fn in routes.items():
                us[k].append(_event_us(fn, iters))
        a, b = torch_route(PT, u, params), PT.tps_system(u, params, n_singular=ns)
        row = {"row": "params", "n": n, "K": len(PT.CONTROL_POINTS), "calls_per_reading": iters, "n_singular": int(ns.item()),
               "T_max_abs_diff_between_routes": float((a[2] - b[2]).abs().max())}
        for k, fn in routes.items():
            row[k + "_us"] = round(sum(us[k]) / len(us[k]), 2)
            row[k + "_us_all"] = [round(t, 2) for t in us[k]]
            row[k + "_us_spread"] = round(max(us[k]) - min(us[k]), 2)
            row[k + "_device_kernels"] = _kernels_per_call(fn)
        row["ratio_torch_over_kernel"] = round(row["torch_route_us"] / row["ups_tps_params_us"], 2)
        emit(row)


def training_rows(steps, repeats):
    from upsparts_amd import configs, lib as L, tps as PT
    from upsparts_amd.model import TrainModel, Trainer
    dev = torch.device("cuda:0")
    B, S, P = 8, 128, 25
    g = torch.Generator().manual_seed(1234)
    batch = {k: (torch.rand(B, S, S, 3, generator=g) * 2 - 1).to(dev) for k in ("view0", "view1", "view0_target")}
    new_make, old_make = PT.make_tps, old_make_tps(PT, L)
    variants = {"eager": (dict(hip_graph=False), new_make), "graph": (dict(hip_graph=True), new_make),
                "graph_no_tps": (dict(hip_graph=True, use_tps=False), new_make), "eager_old_route": (dict(hip_graph=False), old_make)}
    trainers = {}
    for name, (over, _) in variants.items():
        cfg = configs.cub_config(n_parts=P, batch_size=B, use_tps=True)
        cfg["precision"] = "bf16"
        cfg.update(over)
        trainers[name] = Trainer(cfg, None, TrainModel(cfg, device=dev, seed=0))

    def run(name, n):
        PT.make_tps = variants[name][1]
        try:
            for _ in range(n):
                trainers[name].train_step(batch)
            torch.cuda.synchronize()
        finally:
            PT.make_tps = new_make
    for name in variants:                   # warm-up: kernel attributes, allocator pools, the capture
        run(name, 8)
    rates = {k: [] for k in variants}
    for _ in range(repeats):
        for name in variants:               # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, steps)
            rates[name].append(steps * B / (time.perf_counter() - t0))
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    spread = {k: max(v) - min(v) for k, v in rates.items()}
    row = {"row": "training", "config": "cub_config(n_parts=25, batch_size=8, use_tps=True)", "B": B, "S": S, "P": P,
           "precision": "bf16", "steps_per_reading": steps, "readings": repeats}
    for k in variants:
        row[k + "_img_per_s"] = round(mean[k], 1)
        row[k + "_all"] = [round(v, 1) for v in rates[k]]
        row[k + "_spread"] = round(spread[k], 1)
        row[k + "_ms_per_step"] = round(1e3 * B / mean[k], 2)
    for k in ("graph", "graph_no_tps"):
        row[k + "_captured"] = bool(trainers[k].graph is not None and trainers[k].graph.graphs)
    row["eager_captured"] = trainers["eager"].graph is not None
    row["n_singular"] = {k: trainers[k].tps_singular_count() for k in ("eager", "graph", "eager_old_route")}
    row["graph_over_eager_old_route"] = round(mean["graph"] / mean["eager_old_route"], 3)
    row["eager_over_eager_old_route"] = round(mean["eager"] / mean["eager_old_route"], 3)
    row["graph_over_graph_no_tps"] = round(mean["graph"] / mean["graph_no_tps"], 3)
    row["graph_not_below_old_route_by_more_than_spread"] = bool(
        mean["graph"] >= mean["eager_old_route"] - max(spread["graph"], spread["eager_old_route"]))
    row["eager_not_below_old_route_by_more_than_spread"] = bool(
        mean["eager"] >= mean["eager_old_route"] - max(spread["eager"], spread["eager_old_route"]))
    emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tps.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "repeats": args.repeats})
    params_rows(args.iters, max(args.repeats, 3))
    if not args.skip_model:
        training_rows(args.steps, max(args.repeats, 3))


if __name__ == "__main__":
    main()
