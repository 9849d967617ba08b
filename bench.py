"""Headline benchmark: images/sec of full training steps (forward, seven per-key losses, per-key
gradients, TF-Adam, gradient all-reduce) of the part-discovery model on synthetic 128x128 batches.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line.  ``--full`` adds what the headline does not need:
the CPU baseline leg (BASELINE config #1 on the torch-CPU restatement of the reference step, ``cpu_baseline`` in the line;
``--no-cpu-baseline`` drops it again).  ``--dump-outputs DIR`` writes, after the timed steps, what the last timed step computed
(rank 0): its per-key losses (``loss_<key>.npy``, float64 [1]) and a fixed, seeded sample of every optimizer key's updated fp32
master weights (``params_<key>.npy``, float32), so that two builds run with the same arguments can be compared output for output.

N > 1 works both ways the driver may start it:
  * ``python bench.py --gpus N``: this process is only a launcher -- it never touches the GPU, starts N rank
    processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, one per GPU, RCCL over xGMI),
    relays rank 0's JSON line and exits non-zero if any rank failed;
  * ``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N``: WORLD_SIZE is already in the
    environment, the process is one rank.

Workload (BASELINE.json configs[1], the default): CUB yaml, 128x128, n_parts 10, batch 64 per GPU, bf16 activations /
weights (the mask decoder's forward tensors fp16) with fp32 accumulation and fp32 master weights, use_tps False,
synthetic U(-1,1) views resident in HBM before the timed region, noise drawn on device inside the step.
``--config deepfashion256p16 | pennaction128 | cub256p20`` runs BASELINE configs #3 / #4 / #5 the same way (their own
model variant, size, per-GPU batch, algorithmic FLOPs per image and roofline layer).  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0          # MI355X dense bf16 MFMA (guide)
PEAK_F32_TFLOPS = 157.3
PEAK_FP8_TFLOPS = 5000.0           # dense fp8 on the block-scaled K = 128 MFMA (guide); the K = 32 fp8 forms run at the bf16 rate
PMC_FILES = [os.path.join(ROOT, "profiles", f) for f in ("round6_pmc_dv_rb128.json", "round5b_pmc_dv_rb128.json", "round5_pmc_dv_rb128.json", "round4_pmc_dv_rb128.json")]   # tools/profile_round.sh
PMC_FILES_FP8 = [os.path.join(ROOT, "profiles", f) for f in ("round6_pmc_dv_rb128_fp8.json", "round5b_pmc_dv_rb128_fp8.json", "round5_pmc_dv_rb128_fp8.json", "round4_pmc_dv_rb128_fp8.json")]       # the fp8 mode's input-gradient launch
# Which reading of edflow's VGG19Features(original_scale=True) (model.py:610-612; the package is not in the reference tree) the builder
# BELIEVES is the reference's -- stated in every bench line since round 6 (round-5 verdict, measurement hygiene):
PERCEPTUAL_BELIEF = ("UNVERIFIED external: the builder believes `resize256_crop224` (both images resized to 256x256, one random 224x224 "
                     "window of the concatenated pair per step) is what VGG19Features(original_scale=True) does; the headline is timed on "
                     "`native` because BASELINE's 268.9 GFLOP/image is quoted on it, and the same tree's resize256_crop224 line is committed "
                     "beside it every round (profiles/round6_bench_b64_resize256_crop224.json: ~0.82x the native rate)")
CPU_THREAD_CAP = 32                # torch-CPU stops scaling on this graph well before the GPU box's core count (see cpu_baseline)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="cub128p10", help="cub128p10 (BASELINE config #2, the headline) | deepfashion256p16 (#3) | "
                    "pennaction128 (#4) | cub256p20 (#5)")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (0 = the config's)")
    ap.add_argument("--parts", type=int, default=0, help="only for cub128p10 (0 = 10)")
    ap.add_argument("--precision", default="", help="bf16 | fp8 | fp32 (empty = the config's)")
    ap.add_argument("--perceptual-input", default="native", choices=("native", "resize256", "resize256_crop224"),
                    help="what the perceptual trunk sees (the three readings of edflow VGG19Features(original_scale=True), "
                         "model.py:610-612, UNVERIFIED): the images as they are (headline) | bilinear to 256x256 | then one random "
                         "224x224 window per step.  The extra trunk work is counted in train_gflop_per_image.")
    ap.add_argument("--full", action="store_true", help="also run the measurements beyond the headline (the CPU baseline leg)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's losses and a seeded sample of the updated weights to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--cpu-batch", type=int, default=8, help="BASELINE config #1: batch 8")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = min(os.cpu_count(), {})".format(CPU_THREAD_CAP))
    ap.add_argument("--cpu-budget", type=float, default=45.0, help="seconds of timed CPU work (at least 2 steps are timed)")
    ap.add_argument("--rank-entry", default=os.path.abspath(__file__),
                    help="script the launcher starts once per rank (tests point it at a CPU/gloo stand-in)")
    return ap.parse_args()


def launch_ranks(args):
    """Launcher side of ``python bench.py --gpus N``: no HIP call is ever made in this process.  The ranks are fresh child
    processes; they are supervised: the first one to exit non-zero takes the others down (a rank that died on an import
    error or a bad device would otherwise leave its siblings in init_process_group / a collective until the RCCL timeout)."""
    import socket
    import threading
    sock = None
    port = int(os.environ.get("MASTER_PORT", "0"))
    if not port:       # keep the probe socket open (SO_REUSEADDR) until the ranks have been started: nobody else takes the port
        sock = socket.socket()
        sock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ)
        # HSA_ENABLE_IPC_MODE_LEGACY=0: the host driver of this pool only supports dmabuf IPC; with the legacy mode RCCL's
        # intra-node set-up (and any sharing of device tensors between the rank processes) fails with
        # `hipIpcGetMemHandle: invalid argument`.  The image exports it already; it is repeated here so that the ranks get it
        # whatever environment the launcher itself was started from (tests/test_host.py checks the launcher's environment).
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(args.gpus), "LOCAL_WORLD_SIZE": str(args.gpus),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        out = subprocess.PIPE if r == 0 else sys.stderr     # rank 0 prints the JSON line; whatever else the ranks print goes to stderr
        procs.append(subprocess.Popen([sys.executable, args.rank_entry] + sys.argv[1:], env=env, stdout=out))
    if sock is not None:
        sock.close()
    found = {"line": None}

    def drain():
        for raw in procs[0].stdout:
            text = raw.decode(errors="replace")
            if text.lstrip().startswith('{"metric"'):
                found["line"] = text.strip()
            else:
                sys.stderr.write(text)
    th = threading.Thread(target=drain, daemon=True)
    th.start()
    codes = [None] * len(procs)
    while any(c is None for c in codes):
        for i, pr in enumerate(procs):
            if codes[i] is None:
                codes[i] = pr.poll()
        if any(c not in (None, 0) for c in codes):
            for i, pr in enumerate(procs):           # exact children only (never by pattern)
                if codes[i] is None:
                    pr.terminate()
            for i, pr in enumerate(procs):
                if codes[i] is None:
                    try:
                        codes[i] = pr.wait(timeout=20)
                    except subprocess.TimeoutExpired:
                        pr.kill()
                        codes[i] = pr.wait()
            break
        time.sleep(0.2)
    th.join(timeout=5)
    line = found["line"]
    if any(codes) or line is None:
        sys.stderr.write("bench.py: rank exit codes {} (JSON line {})\n".format(codes, "missing" if line is None else "present"))
        # the code of the rank that failed by itself, not the signal of a sibling this launcher terminated
        sys.exit(next((c for c in codes if c and c > 0), next((c for c in codes if c), 1)) & 0xff or 1)
    print(line)
    sys.stdout.flush()


def cpu_baseline(parts, batch, threads, budget_s):
    """The CPU oracle (restatement of the reference's CPU path, kind 'port') on BASELINE config #1: CUB yaml, 128x128,
    P = 10, batch 8, fp32 torch-CPU, whole training steps (7 per-key losses, per-key gradients, TF-Adam).  2 warm-up steps,
    then 5 timed steps -- fewer (never below 2) when the time budget runs out first."""
    import torch
    from oracle import configs as oc, ref_model as R
    cfg = oc.cub_config(n_parts=parts, batch_size=batch)
    torch.set_num_threads(threads)
    params = R.init_params(cfg, 0)
    vp = R.vgg_params(7)
    views = R.synthetic_views(cfg, smooth=False)
    noise = R.synthetic_noise(cfg)
    adam = R.init_adam(params)
    state = R.initial_state(cfg)
    step = 0
    for _ in range(2):
        params, adam, state = R.train_step(params, adam, cfg, views, noise, state, step, vp, dtype=torch.float32, scheme="merged")[:3]
        step += 1
    steps, t0 = 0, time.time()
    while steps < 5 and (steps < 2 or time.time() - t0 < budget_s):
        params, adam, state = R.train_step(params, adam, cfg, views, noise, state, step, vp, dtype=torch.float32, scheme="merged")[:3]
        step += 1
        steps += 1
    dt = time.time() - t0
    return {"value": round(batch * steps / dt, 4), "unit": "images/sec", "cores": threads, "kind": "port",
            "host_cpus": os.cpu_count(),
            "sample": "BASELINE config #1: {} timed training steps after 2 warm-up, batch {}, 128x128, P={}, fp32 torch-CPU restatement "
                      "of the reference step (oracle), {} threads (cap {}: more threads run this graph slower), {:.1f} s, "
                      "{:.2f} s/step".format(steps, batch, parts, threads, CPU_THREAD_CAP, dt, dt / steps)}


DUMP_PARAM_SAMPLE = 1 << 18        # weights per optimizer key in --dump-outputs (7 keys: 7 MiB of float32 at most)


def dump_outputs(out_dir, trainer, losses):
    """--dump-outputs: the per-key losses train_step returned for the last timed step, and the same fixed, seeded positions of every
    optimizer key's flat fp32 master weights after it (all of them where a key has fewer)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    for k, v in sorted(dict(losses).items()):
        np.save(os.path.join(out_dir, "loss_{}.npy".format(k)), np.array([float(v)], dtype=np.float64))
    for k, g in trainer.model.bank.groups.items():
        p = g["flat"]["p"]
        n = int(p.numel())
        if n > DUMP_PARAM_SAMPLE:
            idx = np.sort(np.random.default_rng(0).choice(n, DUMP_PARAM_SAMPLE, replace=False))
            p = p[torch.from_numpy(idx).to(p.device)]
        np.save(os.path.join(out_dir, "params_{}.npy".format(k)), p.detach().float().cpu().numpy())


def run_rank(args):
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        torch.distributed.init_process_group("nccl", init_method="env://", world_size=world, rank=rank)
    dev = torch.device("cuda:{}".format(local))
    torch.cuda.set_device(dev)

    import upsparts_amd  # noqa: F401
    from upsparts_amd import configs, ops
    from upsparts_amd.model import TrainModel, Trainer

    if args.config not in configs.BENCH_CONFIGS:
        raise SystemExit("bench.py: unknown --config {} (one of {})".format(args.config, sorted(configs.BENCH_CONFIGS)))
    build, S, P, B0, prec0, gflop_img, note = configs.BENCH_CONFIGS[args.config]
    args.batch = args.batch or B0
    args.precision = args.precision or prec0
    if args.config == "cub128p10" and args.parts:
        P = args.parts
        cfg = configs.cub_config(n_parts=P, batch_size=args.batch)
    else:
        cfg = build(args.batch)
    args.parts = P
    cfg["precision"] = args.precision
    cfg["perceptual_input"] = args.perceptual_input
    # algorithmic FLOPs of the trunk: 1.5 x F_vgg per image (2 forwards + 1 input gradient over 2 images' worth) scale
    # with its input area: BASELINE.md section 3 counts +109.2 GFLOP / image for 256x256 instead of 128x128 inputs (= 3 x the
    # 36.4 of the native trunk); a 224x224 window is (224 / 256)^2 of that
    if S == 128 and args.perceptual_input != "native":
        area = {"resize256": 4.0, "resize256_crop224": 4.0 * (224.0 / 256.0) ** 2}[args.perceptual_input]
        gflop_img = gflop_img + (area - 1.0) * (109.2 / 3.0)
    elif S == 256 and args.perceptual_input == "resize256_crop224":
        gflop_img = gflop_img - (1.0 - (224.0 / 256.0) ** 2) * 4.0 * (109.2 / 3.0)
    model = TrainModel(cfg, device=dev, seed=0)
    trainer = Trainer(cfg, None, model, world_size=world, rank=rank)
    g = torch.Generator().manual_seed(1234 + rank)
    batch = {k: (torch.rand(args.batch, S, S, 3, generator=g) * 2 - 1).to(dev) for k in model.inputs}

    # roofline layer: the 258 -> 256 3x3 convolution of the mask decoder at full resolution (its last residual block:
    # conv2d_0 nin, conv2d_1, conv2d_2, one block per level, then this one) -- 37 % of the forward FLOPs at 128x128
    ops.KernelTimer.layer = "decoder_visualize/conv2d_{}".format(2 + len(cfg["dv"]["config"]))
    for _ in range(args.warmup):
        trainer.train_step(batch)
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    ops.KernelTimer.enabled = True
    t0 = time.perf_counter()
    losses = None
    for _ in range(args.steps):
        losses = None                  # (a step's lazily read losses are not held across the next step)
        losses = trainer.train_step(batch)
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ops.KernelTimer.enabled = False
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax)
    rccl_world = torch.distributed.get_world_size() if world > 1 else 1
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, trainer, losses)

    if rank == 0:
        images = args.batch * world * args.steps
        value = images / dt
        # fp8: the roofline launches run on the block-scaled K = 128 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4): priced against the
        # dense fp8 peak (MI355X_MICROARCH.md: ~5 PFLOP/s)
        peak = {"bf16": PEAK_BF16_TFLOPS, "fp8": PEAK_FP8_TFLOPS}.get(args.precision, PEAK_F32_TFLOPS)
        dname = {"bf16": "bf16", "fp8": "fp8"}.get(args.precision, "f32")
        traffic = None
        pmc_used = None
        pmc_tree = None
        pmc_alg = None
        # HBM bytes per launch of the roofline kernel from the PMC passes committed for this tree (profiles/), not live; they were
        # taken on the headline shape (2 x 64 images of 128x128, 256 channels, bf16): reported for exactly that launch only
        if args.config == "cub128p10" and args.precision in ("bf16", "fp8") and args.batch == 64:
            for pf in (PMC_FILES_FP8 if args.precision == "fp8" else PMC_FILES):
                try:
                    with open(pf) as f:
                        pj = json.load(f)
                    traffic = pj["traffic_bytes_per_launch"]
                    pmc_used = os.path.relpath(pf, ROOT)
                    pmc_tree = pj.get("tree", "unrecorded (taken before round 5: the 823-launch tree of round 4)")
                    pmc_alg = pj.get("algorithmic_bytes_per_launch_tensor_once")
                    pmc_alg = pmc_alg if isinstance(pmc_alg, (int, float)) else pj.get("algorithmic_total")
                    break
                except Exception:
                    traffic = None
        # fp8 mode: the layer's FORWARD stays fp16 (the mask decoder's logits decide the masks) -- the fp8 roofline is that of its two
        # input-gradient launches, the ones that run on the block-scaled fp8 MFMA
        kms = ops.KernelTimer.mean_ms("dgrad" if args.precision == "fp8" else None)
        ach = ops.KernelTimer.flops / (kms * 1e-3) / 1e12 if kms > 0 else 0.0
        metric = "images/sec training (CUB 128x128, 10 parts)" if args.config == "cub128p10" and P == 10 else \
            "images/sec training ({} {}x{}, {} parts)".format(args.config, S, S, P)
        out = {"metric": metric, "value": round(value, 2), "unit": "images/sec",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": dname, "data": "synthetic",
               "config": {"workload": "{}: {} yaml {}x{} n_parts={} batch {}/GPU, full train step (per-key losses, "
                                      "per-key grads, TF-Adam), use_tps False, VGG19-topology perceptual trunk with "
                                      "stand-in weights, perceptual_input = {} ({}); bf16 storage / fp32 accumulate, the mask decoder's "
                                      "forward tensors fp16 (parity bar of this dtype: part-mask IoU >= 0.99 and losses within 5% "
                                      "of the fp64 oracle; the 1e-3 bar is met by precision=fp32){}".format(
                                          note, args.config, S, S, P, args.batch, args.perceptual_input,
                                          {"native": "the trunk sees the images at their own resolution: the headline reading",
                                           "resize256": "both images bilinearly resized to 256x256 first",
                                           "resize256_crop224": "resized to 256x256, then one random 224x224 window per step"}[args.perceptual_input],
                                          "; precision fp8: e4m3 / e5m2 MFMA "
                                      "operands for the wide 3x3 convolutions whose operand arrives as an fp8 copy (the mask decoder's "
                                      "FORWARD stays fp16: its logits decide the masks), bf16 tensors everywhere"
                                          if args.precision == "fp8" else ""),
                          "name": args.config, "perceptual_input": args.perceptual_input, "perceptual_input_reading": PERCEPTUAL_BELIEF,
                          "global_batch": args.batch * world, "parallelism": "dp{}".format(world),
                          "rccl_world_size": rccl_world, "stream_plan": trainer.stream_plan},
               "model_tflops_per_gpu": round(value * gflop_img / 1e3 / world, 2), "train_gflop_per_image": gflop_img,
               "roofline": {"bound": "mfma", "kernel": "conv3x3_patch_kernel<{}> @ {} ({})".format(
                                "bf16 tensors, block-scaled fp8 MFMA,128,2,16" if args.precision == "fp8" else
                                ("float,128,1,16: v_mfma_f32_32x32x2_f32, exact f32, one block per CU" if dname == "f32" else
                                 "f16 forward / bf16 input gradients,128,2,16"), ops.KernelTimer.layer,
                                "the 2 input-gradient launches per step, e5m2 x e4m3 operands; the layer's forward launch stays fp16 and is "
                                "listed under kernel_ms_forward" if args.precision == "fp8" else
                                "1 forward + 2 input-gradient launches per step, all timed"),
                            "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                            "kernel_ms": round(kms, 4), "kernel_ms_forward": round(ops.KernelTimer.mean_ms("fwd"), 4),
                            "kernel_ms_dgrad": round(ops.KernelTimer.mean_ms("dgrad"), 4),
                            "launches_timed": len(ops.KernelTimer.events), "traffic": traffic,
                            "traffic_note": "HBM bytes of the {} launch from separate --pmc FETCH_SIZE / WRITE_SIZE passes "
                                            "({}); tensor-once algorithmic bytes {}".format(
                                                "input-gradient" if args.precision == "fp8" else "forward",
                                                pmc_used, "{:.3g} of the input-gradient launch (e5m2 copy of the gradient in, the bf16 gradient as residual, the "
                                                "producer's sign bytes for act', bf16 out)".format(pmc_alg or 0.0) if args.precision == "fp8" else
                                                "{:.3g} (input, output, sign bytes, weights)".format(pmc_alg or 0.0)) if traffic else
                                            "no PMC pass committed for this launch shape",
                            "flop_per_launch": ops.KernelTimer.flops}}
        if traffic:      # the PMC passes are not live: say which tree they were taken on, so a traffic regression is not hidden by a stale file
            out["roofline"]["traffic_tree"] = pmc_tree
        dpw = trainer.dp_wait_ms()
        if dpw is not None:      # data parallel: what rank 0's launching stream waited at the end of the backward pass, per step
            out["dp_wait_ms"] = dpw
        if not ops.KernelTimer.events:
            out["roofline"]["note"] = "no launch timed: under HIP-graph replay (hip_graph / UPS_GRAPH=1) the roofline launches are graph nodes"
        if args.full and world == 1 and not args.no_cpu_baseline:
            threads = args.cpu_threads or min(os.cpu_count() or 1, CPU_THREAD_CAP)
            if args.config == "cub128p10":      # the CPU leg is BASELINE config #1 (the CUB yaml at batch 8)
                out["cpu_baseline"] = cpu_baseline(args.parts, args.cpu_batch, threads, args.cpu_budget)
        print(json.dumps(out))
        sys.stdout.flush()
    if world > 1:
        torch.distributed.destroy_process_group()


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args)
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.stderr.write("bench.py: --gpus {} but WORLD_SIZE={} -- using the launcher's world size\n".format(
            args.gpus, os.environ["WORLD_SIZE"]))
    run_rank(args)


if __name__ == "__main__":
    main()
