"""What the landmark regression evaluation costs (csrc/landmarks.hip; ops.part_moments, ops.landmark_gram, ops.landmark_solve).

(a) moments   event time of ups_part_moments (both launches) at soft [128, 128, 128, 10] fp32, with and without the arg-max map, on
              preallocated buffers, against 8 TB/s on the bytes it must read (the soft map once; the int64 arg-max map when given).
              Four operand sets are rotated: 4 x 84 MB is more than the 256 MB last-level cache holds.
(b) fit       event time of ups_landmark_gram + ups_landmark_solve (three launches, through the ops wrappers with their allocations)
              at N = 4096 instances, P = 10 parts (D = 21), K = 15 keypoints, and of the same arithmetic by torch ops in float64:
              einsum for the K masked normal equations + torch.linalg.solve.
A reading is the time of `--iters` calls between two events; the minimum of `--repeats` readings is reported and all are printed.
Synthetic inputs (a seeded soft-max of random logits; uniform centres and keypoints, 70 % visible), not a trained model's.
Prints one JSON line per row.

    python tools/bench_landmarks.py > profiles/bench_landmarks.jsonl
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
NOTE = "synthetic inputs (seeded soft-max of random logits; uniform centres and keypoints, 70 % visible), not a trained model's"


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


def moments_rows(iters, repeats):
    from upsparts_amd import lib as L
    dev = torch.device("cuda:0")
    N, S, P, nsets = 128, 128, 10, 4
    g = torch.Generator(device=dev).manual_seed(1)
    softs = [torch.softmax(4 * torch.randn((N, S, S, P), generator=g, device=dev), dim=-1).contiguous() for _ in range(nsets)]
    preds = [s.argmax(-1).contiguous() for s in softs]
    mass = torch.empty((N, P), dtype=torch.float64, device=dev)
    centre = torch.empty((N, P, 2), dtype=torch.float64, device=dev)
    valid = torch.empty((N, P), dtype=torch.uint8, device=dev)
    hard = torch.zeros((N, P, 3), dtype=torch.int32, device=dev)
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.load().ups_part_moments_scratch_bytes(N, S, S, P) // 8, dtype=torch.float64, device=dev)

    def run(i, with_pred):
        L.call("ups_part_moments", L.ptr(softs[i % nsets]), L.ptr(preds[i % nsets]) if with_pred else None, N, S, S, P, 0.005 * S * S,
               L.ptr(mass), L.ptr(centre), L.ptr(valid), L.ptr(hard) if with_pred else None, L.ptr(invalid) if with_pred else None,
               L.ptr(scratch), L.stream())
    for with_pred in (False, True):
        for i in range(nsets):
            run(i, with_pred)
        torch.cuda.synchronize()
        ts = event_us(lambda i: run(i, with_pred), iters, repeats)
        nbytes = N * S * S * (P * 4 + (8 if with_pred else 0))
        floor_us = nbytes / HBM_BYTES_PER_S * 1e6
        emit({"row": "moments_hard" if with_pred else "moments", "launch": "ups_part_moments (both launches, preallocated buffers)",
              "N": N, "h": S, "w": S, "P": P, "arg_max_map": with_pred, "bytes_read": nbytes, "calls_per_reading": iters,
              "us": round(min(ts), 1), "us_all": [round(t, 1) for t in ts], "hbm_floor_us": round(floor_us, 2),
              "fraction_of_8TBps": round(floor_us / min(ts), 4), "GBps": round(nbytes / min(ts) / 1e3, 1)})


def torch_fit(feat, target, vis, ridge):
    f = torch.cat([feat, torch.ones((feat.shape[0], 1), dtype=torch.float64, device=feat.device)], dim=1)
    m = (vis != 0).to(torch.float64)
    G = torch.einsum("nk,na,nb->kab", m, f, f)
    R = torch.einsum("nk,na,nkc->kac", m, f, target)
    pen = torch.ones(f.shape[1], dtype=torch.float64, device=feat.device)
    pen[-1] = 0.0
    return torch.linalg.solve(G + ridge * torch.diag(pen)[None], R)


def fit_rows(iters, repeats):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    N, P, K, ridge = 4096, 10, 15, 1e-6
    g = torch.Generator(device=dev).manual_seed(2)
    sets = []
    for _ in range(3):
        feat = (torch.rand((N, 2 * P), generator=g, device=dev, dtype=torch.float64) * 2 - 1).contiguous()
        target = (torch.rand((N, K, 2), generator=g, device=dev, dtype=torch.float64) * 2 - 1).contiguous()
        vis = (torch.rand((N, K), generator=g, device=dev) < 0.7).to(torch.uint8).contiguous()
        sets.append((feat, target, vis))

    def fit(i):
        G, R, cnt = ops.landmark_gram(*sets[i % 3])
        return ops.landmark_solve(G, R, cnt, ridge)
    for i in range(3):
        fit(i)
    torch.cuda.synchronize()
    ts = event_us(fit, iters, repeats)
    common = {"N": N, "P": P, "D": 2 * P + 1, "K": K, "ridge": ridge}
    emit(dict(common, row="fit", launch="ups_landmark_gram + ups_landmark_solve (three launches, the wrappers' allocations included)",
              calls_per_reading=iters, us=round(min(ts), 1), us_all=[round(t, 1) for t in ts]))
    W, ns = fit(0)
    Wt = torch_fit(*sets[0], ridge)
    torch.cuda.synchronize()
    tt = event_us(lambda i: torch_fit(*sets[i % 3], ridge), iters, repeats)
    emit(dict(common, row="fit_torch", launch="torch ops in float64: einsum (masked normal equations) + torch.linalg.solve",
              calls_per_reading=iters, us=round(min(tt), 1), us_all=[round(t, 1) for t in tt], kernel_speedup=round(min(tt) / min(ts), 2),
              n_singular=int(ns.item()), max_abs_W_difference=float((W - Wt).abs().max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_landmarks.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "note": NOTE})
    moments_rows(args.iters, args.repeats)
    fit_rows(args.iters, args.repeats)


if __name__ == "__main__":
    main()
