"""What the part-appearance index costs (csrc/partindex.hip; ops.part_knn, ops.part_kmeans_step).

(a) knn      event time of ups_part_knn at N = 4096 codes (self-query), P = 10, A = 64, K = 8, and of the same result by torch ops on the
             device: per part, chunks of queries, float64 broadcast-subtract-square-sum + topk.
(b) kmeans   event time of ups_part_kmeans_step (assignment, counts, feature sums, inertia) at N = 16384, P = 16, A = 64, k = 8, and of
             the torch route: float64 broadcast distances + argmin + bincount + index_add_.
Operand sets are rotated; a reading is the time of `--iters` calls between two events, the minimum of `--repeats` readings is reported
and all are printed.  `fraction_of_fp64_floor`: the arithmetic needs 3 N_q N_g P A (3 N k P A) fp64 vector instructions per lane;
against 39.3e12 per second -- the 78.6 TFLOP/s vector figure counted per INSTRUCTION, which ASSUMES that fp64 add and multiply issue
at the FMA rate (not measured here).  `differing_indices`: neighbour slots where the torch route, whose summation order differs, names
another item (near-ties may flip; recorded, not asserted).  Synthetic codes (seeded blobs), not a trained model's.
Prints one JSON line per row.

    python tools/bench_partindex.py > profiles/bench_partindex.jsonl
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_INSTR_PER_S = 39.3e12
NOTE = "synthetic codes (seeded Gaussian blobs, 20 % invalid), not a trained model's; the fp64 instruction rate is an assumption"


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


def bank(g, dev, N, P, A, blobs=6):
    centres = torch.randn((P, blobs, A), generator=g, device=dev) * 2
    which = torch.randint(0, blobs, (N, P), generator=g, device=dev)
    feat = centres[torch.arange(P, device=dev)[None, :], which] + torch.randn((N, P, A), generator=g, device=dev)
    valid = (torch.rand((N, P), generator=g, device=dev) >= 0.2).to(torch.uint8)
    return feat.contiguous(), valid.contiguous()


def torch_knn(feat, valid, K, chunk=128):
    N, P, A = feat.shape
    idx = torch.full((N, P, K), -1, dtype=torch.int32, device=feat.device)
    dist = torch.full((N, P, K), float("inf"), dtype=torch.float64, device=feat.device)
    f64 = feat.double()
    ar = torch.arange(N, device=feat.device)
    for p in range(P):
        gp = f64[:, p]
        bad = valid[:, p] == 0
        for c0 in range(0, N, chunk):
            d = (f64[c0:c0 + chunk, None, p, :] - gp[None]).pow(2).sum(-1)
            d[:, bad] = float("inf")
            d[ar[c0:c0 + chunk] - c0, ar[c0:c0 + chunk]] = float("inf")
            v, i = torch.topk(d, K, dim=1, largest=False, sorted=True)
            i = torch.where(torch.isinf(v), torch.full_like(i, -1), i)
            q_bad = bad[c0:c0 + chunk]
            v[q_bad], i[q_bad] = float("inf"), -1
            idx[c0:c0 + chunk, p], dist[c0:c0 + chunk, p] = i.to(torch.int32), v
    return idx, dist


def torch_kmeans_step(feat, valid, cent):
    N, P, A = feat.shape
    k = cent.shape[1]
    f64 = feat.double()
    label = torch.empty((N, P), dtype=torch.int64, device=feat.device)
    counts = torch.empty((P, k), dtype=torch.int64, device=feat.device)
    sums = torch.zeros((P, k, A), dtype=torch.float64, device=feat.device)
    inertia = torch.empty(P, dtype=torch.float64, device=feat.device)
    for p in range(P):
        d = (f64[:, None, p, :] - cent[p][None]).pow(2).sum(-1)
        m, j = d.min(dim=1)
        ok = valid[:, p] != 0
        label[:, p] = torch.where(ok, j, torch.full_like(j, -1))
        counts[p] = torch.bincount(j[ok], minlength=k)
        sums[p].index_add_(0, j[ok], f64[ok, p])
        inertia[p] = m[ok].sum()
    return label, counts, sums, inertia


def knn_rows(iters, repeats):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    N, P, A, K = 4096, 10, 64, 8
    g = torch.Generator(device=dev).manual_seed(1)
    sets = [bank(g, dev, N, P, A) for _ in range(3)]
    for f, v in sets:
        ops.part_knn(f, v, K=K)
    torch.cuda.synchronize()
    ts = event_us(lambda i: ops.part_knn(*sets[i % 3], K=K), iters, repeats)
    floor_us = 3.0 * N * N * P * A / FP64_INSTR_PER_S * 1e6
    common = {"N": N, "P": P, "A": A, "K": K, "pairs": N * N * P, "fp64_instructions": 3 * N * N * P * A}
    emit(dict(common, row="knn", launch="ups_part_knn", calls_per_reading=iters, us=round(min(ts), 1), us_all=[round(t, 1) for t in ts],
              fp64_floor_us=round(floor_us, 1), fraction_of_fp64_floor=round(floor_us / min(ts), 4),
              floor_assumption="39.3e12 fp64 VALU instructions/s (78.6 TFLOP/s counted per instruction): assumed, not measured"))
    ki, kd = ops.part_knn(*sets[0], K=K)
    ti, td = torch_knn(*sets[0], K=K)
    torch.cuda.synchronize()
    nt = max(2, iters // 10)
    tt = event_us(lambda i: torch_knn(*sets[i % 3], K=K), nt, min(repeats, 3))
    finite = torch.isfinite(kd) & torch.isfinite(td)
    emit(dict(common, row="knn_torch", launch="torch ops: per part, 128 queries at a time, float64 (q - g)^2 summed + topk",
              calls_per_reading=nt, us=round(min(tt), 1), us_all=[round(t, 1) for t in tt], kernel_speedup=round(min(tt) / min(ts), 2),
              differing_indices=int((ki != ti).sum()), slots=int(ki.numel()),
              max_rel_distance_difference=float(((kd - td).abs()[finite] / td[finite].clamp(min=1e-300)).max())))


def kmeans_rows(iters, repeats):
    from upsparts_amd import ops
    dev = torch.device("cuda:0")
    N, P, A, k = 16384, 16, 64, 8
    g = torch.Generator(device=dev).manual_seed(2)
    sets = []
    for _ in range(3):
        f, v = bank(g, dev, N, P, A)
        cent = f[torch.randint(0, N, (k,), generator=g, device=dev)].permute(1, 0, 2).double().contiguous()
        sets.append((f, v, cent))
    prev = torch.full((N, P), -2, dtype=torch.int32, device=dev)
    for s in sets:
        ops.part_kmeans_step(*s, prev)
    torch.cuda.synchronize()
    ts = event_us(lambda i: ops.part_kmeans_step(*sets[i % 3], prev), iters, repeats)
    floor_us = 3.0 * N * k * P * A / FP64_INSTR_PER_S * 1e6
    common = {"N": N, "P": P, "A": A, "k": k, "fp64_instructions": 3 * N * k * P * A}
    emit(dict(common, row="kmeans_step", launch="ups_part_kmeans_step (+ its reduction launch and the wrapper's allocations)",
              calls_per_reading=iters, us=round(min(ts), 1), us_all=[round(t, 1) for t in ts], fp64_floor_us=round(floor_us, 2),
              fraction_of_fp64_floor=round(floor_us / min(ts), 4),
              floor_assumption="39.3e12 fp64 VALU instructions/s (78.6 TFLOP/s counted per instruction): assumed, not measured"))
    r = ops.part_kmeans_step(*sets[0], prev)
    tl, tc, tsum, tin = torch_kmeans_step(*sets[0])
    torch.cuda.synchronize()
    nt = max(2, iters // 4)
    tt = event_us(lambda i: torch_kmeans_step(*sets[i % 3]), nt, min(repeats, 3))
    emit(dict(common, row="kmeans_step_torch", launch="torch ops: per part, float64 (x - c)^2 summed + min + bincount + index_add_",
              calls_per_reading=nt, us=round(min(tt), 1), us_all=[round(t, 1) for t in tt], kernel_speedup=round(min(tt) / min(ts), 2),
              differing_labels=int((r["label"].long() != tl).sum()), differing_counts=int((r["counts"].long() != tc).sum()),
              max_rel_sum_difference=float(((r["sums"] - tsum).abs() / tsum.abs().clamp(min=1e-300)).max()),
              max_rel_inertia_difference=float(((r["inertia"] - tin).abs() / tin).max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_partindex.py times the GPU: no device"
    import upsparts_amd  # noqa: F401
    emit({"row": "about", "device": torch.cuda.get_device_name(0), "note": NOTE})
    knn_rows(args.iters, args.repeats)
    kmeans_rows(args.iters, args.repeats)


if __name__ == "__main__":
    main()
