"""The guarded optimizer step on the device (csrc/stepguard.hip): ups_grad_guard against its NumPy float64 restatement (stepguard_ref.py)
bit for bit -- every count around the block, the chunk and the grid-stride wrap, every alignment, three magnitudes, denormals, planted
NaN / inf -- ups_adam_guarded against ups_adam / ups_adam_dev, ups_state_update_guarded against ups_state_update, and the trainer's
`skip_nonfinite` / `grad_clip_norm` keys: unchanged bits on clean data, clipping under hip_graph, a persistently and a transiently bad
key, two data-parallel ranks."""
import copy
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import stepguard_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGG_W = (8, 8, 16, 16, 16)
C = R.CHUNK
COUNTS = [1, 255, 256, 257, C - 1, C, C + 1, 10 * C + 3]
MAGS = {"1e-20": 1e-20, "1": 1.0, "1e18": 1e18, "denormal": None}


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


@functools.lru_cache(maxsize=None)
def _values(count, mag):
    """N(0,1) * magnitude with a block of denormals in it (mag "denormal": denormals only); the array is shared and never written."""
    rng = np.random.RandomState(count % 9973 + len(mag))
    den = rng.randint(1, 0x7fffff, size=count).astype(np.uint32) | (rng.randint(0, 2, size=count).astype(np.uint32) << 31)
    den = den.view(np.float32)
    if MAGS[mag] is None:
        x = den.copy()
    else:
        x = (rng.standard_normal(count) * MAGS[mag]).astype(np.float32)
        a = count // 3
        x[a:a + 37] = den[a:a + 37]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(count, mag, grad_scale, clip_frac, skip):
    """The restatement's record; the clip norm is clip_frac times the data's own norm (clip_frac < 1: the step is clipped)."""
    x = _values(count, mag)
    clip = float(np.sqrt(R.sumsq(x)) * grad_scale * clip_frac) if clip_frac else 0.0
    return clip, R.grad_guard(x, grad_scale, clip, skip)


def _run_guard(x, dev, grad_scale, clip, skip, offset=0, max_blocks=0, rec=None):
    lib, ops = _mods()
    buf = torch.zeros(x.size + 4, dtype=torch.float32, device=dev)
    g = buf[offset:offset + x.size]
    g.copy_(torch.from_numpy(np.array(x)))
    assert g.data_ptr() == buf.data_ptr() + 4 * offset
    rec = ops.guard_records(1, dev)[0] if rec is None else rec
    ops.grad_guard(g, rec, grad_scale, clip, skip, max_blocks=max_blocks)
    return rec, ops.guard_read(rec)


def _assert_record(got, want, what):
    assert R.same_bits(np.float64(got["sumsq"]), np.float64(want["sumsq"])), (what, "sumsq", got["sumsq"], float(want["sumsq"]))
    assert R.same_bits(np.float64(got["norm"]), np.float64(want["norm"])), (what, "norm", got["norm"], float(want["norm"]))
    assert R.same_bits(np.float32(got["scale"]), np.float32(want["scale"])), (what, "scale", got["scale"], float(want["scale"]))
    for k in ("nonfinite", "skip", "skipped", "clipped", "consecutive"):
        assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.mark.parametrize("mag", list(MAGS))
@pytest.mark.parametrize("count", COUNTS)
def test_grad_guard_bits_equal_the_restatement(count, mag, dev):
    """sumsq, norm, scale, nonfinite: the restatement's bits at every alignment of the base, and under max_blocks = 3 (the grid-stride
    wrap: 11 chunks on 3 blocks); the norm against torch's float64 norm within count 2^-52."""
    x = _values(count, mag)
    clip, want = _ref(count, mag, 0.5, 0.75, True)
    assert want["nonfinite"] == 0 and want["clipped"] == 1 and want["scale"] < 1
    for offset in (0, 1, 2, 3):
        _, got = _run_guard(x, dev, 0.5, clip, True, offset=offset)
        _assert_record(got, want, "offset {}".format(offset))
    if count > 3 * C:
        for offset in (0, 3):
            _, got = _run_guard(x, dev, 0.5, clip, True, offset=offset, max_blocks=3)
            _assert_record(got, want, "max_blocks 3, offset {}".format(offset))
    _, got = _run_guard(x, dev, 1.0, 0.0, False)
    _assert_record(got, _ref(count, mag, 1.0, 0.0, False)[1], "no clip")
    assert got["scale"] == 1.0 and got["clipped"] == 0
    tn = float(torch.linalg.vector_norm(torch.from_numpy(np.array(x)).to(dev).double()))
    assert abs(got["norm"] - tn) <= count * 2.0 ** -52 * tn


def test_grad_guard_empty_bucket(dev):
    lib, ops = _mods()
    rec = ops.guard_records(1, dev)[0]
    ops.grad_guard(torch.zeros(0, dtype=torch.float32, device=dev), rec, 1.0, 2.0, True)
    got = ops.guard_read(rec)
    assert (got["skip"], got["scale"], got["norm"], got["sumsq"], got["nonfinite"]) == (0, 1.0, 0.0, 0.0, 0)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
def test_planted_nonfinite_values_are_counted_wherever_they_sit(value, dev):
    """Element 0, the last element and both sides of a chunk boundary, one at a time and together, at two alignments."""
    count = 2 * C + 5
    base = _values(count, "1")
    spots = [0, count - 1, C - 1, C]
    cases = [[s] for s in spots] + [spots]
    for where in cases:
        x = np.array(base)
        x[where] = value
        want = R.grad_guard(x, 1.0, 1.0, True)
        assert want["nonfinite"] == len(where) and want["skip"] == 1
        for offset in (0, 1):
            _, got = _run_guard(x, dev, 1.0, 1.0, True, offset=offset)
            _assert_record(got, want, (where, offset))
    # skip_nonfinite off: nothing is skipped, the formulas run on the non-finite sum (NaN -> NaN scale, inf -> scale 0)
    x = np.array(base)
    x[C] = value
    want = R.grad_guard(x, 1.0, 1.0, False)
    _, got = _run_guard(x, dev, 1.0, 1.0, False)
    _assert_record(got, want, "skip off")
    assert got["skip"] == 0 and got["nonfinite"] == 1 and (np.isnan(got["scale"]) if np.isnan(value) else got["scale"] == 0.0)


def test_cumulative_fields_over_skip_clean_clipped(dev):
    count = C + 77
    clean = _values(count, "1")
    bad = np.array(clean)
    bad[count // 2] = np.nan
    norm = float(np.sqrt(R.sumsq(clean)))
    rec, want = None, None
    seq = [(bad, 0.0), (clean, 0.0), (clean, 0.5 * norm), (bad, 0.5 * norm), (bad, 0.0), (clean, 2.0 * norm)]
    expect = [(1, 1, 0, 1), (1, 0, 0, 0), (1, 0, 1, 0), (2, 1, 1, 1), (3, 2, 1, 1), (3, 0, 1, 0)]     # skipped, consecutive, clipped, skip
    for (x, clip), e in zip(seq, expect):
        rec, got = _run_guard(x, dev, 1.0, clip, True, rec=rec)
        want = R.grad_guard(x, 1.0, clip, True, want)
        _assert_record(got, want, e)
        assert (got["skipped"], got["consecutive"], got["clipped"], got["skip"]) == e


def _record(dev, scale, skip):
    lib, _ = _mods()
    s = lib.StepGuard()
    s.scale, s.skip = scale, skip
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.int64).clone().to(dev)


def _adam_operands(count, dev):
    gen = torch.Generator(device="cpu").manual_seed(count % 1009)
    p, g, m = (torch.randn(count, generator=gen).to(dev) for _ in range(3))
    v = torch.rand(count, generator=gen).to(dev) * 0.1
    return p, g, m, v


HYPER = (0.5, 0.9, 1e-8)


@pytest.mark.parametrize("count", [1, 257, 2097152 + 257])       # the last: past the 8192-block cap (the grid strides)
def test_adam_guarded_against_adam(count, dev):
    lib, ops = _mods()
    p0, g, m0, v0 = _adam_operands(count, dev)
    lr_t, gs = 3.1e-4, 0.5
    lr_dev = torch.tensor([lr_t], dtype=torch.float32, device=dev)

    def step(lr, guard=None, grad=g, grad_scale=gs):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adam_step(p, grad, m, v, lr, *HYPER, grad_scale, guard=guard)
        return p, m, v

    plain, plain_dev = step(lr_t), step(lr_dev)
    one = _record(dev, 1.0, 0)
    for a, b in ((step(lr_t, one), plain), (step(lr_dev, one), plain_dev)):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert not torch.equal(plain[0], p0)
    for scale in (0.25, 0.37182817):
        pre = (g * gs) * torch.tensor(scale, dtype=torch.float32, device=dev)         # the gradient pre-multiplied in fp32
        want = step(lr_t, grad=pre, grad_scale=1.0)
        got = step(lr_t, _record(dev, scale, 0))
        for x, y in zip(got, want):
            assert torch.equal(x, y), scale
        assert not torch.equal(got[0], plain[0])
    nan_g = torch.full_like(g, float("nan"))
    for lr in (lr_t, lr_dev):
        got = step(lr, _record(dev, 1.0, 1), grad=nan_g)
        for x, y in zip(got, (p0, m0, v0)):
            assert torch.equal(x, y)


def test_state_update_guarded(dev):
    lib, ops = _mods()
    stats = torch.tensor([0.31, -0.12, 0.55, 0.61, 0.69, 0.72], dtype=torch.float32, device=dev)
    old = torch.tensor([0.5, 0.5, 0.01, 1.0, 1.0, 0.02, -0.03, 0.4, 3.3], dtype=torch.float32, device=dev)
    args = (0.99, 1.0 - 0.99, 1, 4.0, 0.27, 1, 0.05, 0.3, 1.0, 7.5)
    want = torch.empty_like(old)
    lib.call("ups_state_update", lib.ptr(stats), lib.ptr(old), lib.ptr(want), *args, lib.stream())
    assert not torch.equal(want, old)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    total = 0
    for i in range(6):
        for consecutive, bad in enumerate((float("nan"), float("inf"), float("-inf")), start=1):
            s = stats.clone()
            s[i] = bad
            out = torch.full_like(old, -7.0)
            ops.state_update_guarded(s, old, out, *args, counters)
            total += 1
            assert torch.equal(out.view(torch.int32), old.view(torch.int32)), (i, bad)
            assert counters.tolist() == [total, consecutive], (i, bad)
        out = torch.empty_like(old)
        ops.state_update_guarded(stats, old, out, *args, counters)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        assert counters.tolist() == [total, 0]


# ---------------------------------------------------------------------------------------------- the trainer
def _cfg(precision, **over):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config(variant="cub"))
    cfg.update(precision=precision, vgg_widths=VGG_W)
    cfg.update(over)
    return cfg


def _snap(model):
    return {k: {n: g["flat"][n].detach().cpu().clone() for n in ("p", "m", "v")} for k, g in model.bank.groups.items()}


def _run(cfg, steps, dev, each=None):
    """`steps` steps on explicit views and noise -> what a run leaves behind.  each(step, trainer, model): called after every step."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as Ro
    model = TrainModel(cfg, device=dev, seed=0)
    tr = Trainer(cfg, None, model)
    first = _snap(model)
    hist = []
    for step in range(steps):
        losses = tr.train_step(Ro.synthetic_views(cfg, seed=100 + step), Ro.synthetic_noise(cfg, seed=200 + step))
        hist.append({k: float(v) for k, v in losses.items()})
        if each is not None:
            each(step, tr, model)
    return {"first": first, "banks": _snap(model), "state": {k: float(v) for k, v in tr.state.items()}, "losses": hist,
            "report": tr.guard_report(), "captured": tr.graph is not None and bool(tr.graph.graphs)}


def _assert_same_run(a, b):
    for k in a["banks"]:
        for n in ("p", "m", "v"):
            assert torch.equal(a["banks"][k][n], b["banks"][k][n]), (k, n)
    assert a["state"] == b["state"]
    assert a["losses"] == b["losses"]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_skip_nonfinite_on_clean_data_changes_no_bit(precision, graph, dev):
    """(i) five steps with `skip_nonfinite: True`: weights, m, v, state and losses are those of the run without the key."""
    plain = _run(_cfg(precision, hip_graph=graph), 5, dev)
    guarded = _run(_cfg(precision, hip_graph=graph, skip_nonfinite=True), 5, dev)
    assert plain["captured"] == guarded["captured"] == graph
    _assert_same_run(plain, guarded)
    rep = guarded["report"]
    assert all(r["skipped"] == 0 and r["consecutive"] == 0 for r in rep.values())
    assert sorted(k for k in rep if k != "state") == sorted(guarded["banks"])         # one record per optimizer key
    assert all(rep[k]["norm"] > 0 and rep[k]["scale"] == 1.0 and rep[k]["nonfinite"] == 0 for k in guarded["banks"])
    assert all(r["norm"] == 0 and r["scale"] == 0 for k, r in plain["report"].items() if k != "state")      # the guard never ran there


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_clipping_under_hip_graph_matches_the_eager_kernel_route(precision, dev):
    """(ii) `grad_clip_norm` at the median decoder_delta norm of an unclipped pass, so that some steps clip and some do not: seven steps
    of hip_graph against eager + skip_nonfinite (both on the kernel route) are bit-equal, with equal clip counts."""
    norms = []
    _run(_cfg(precision, skip_nonfinite=True), 7, dev, each=lambda s, tr, m: norms.append(tr.fetch_logs()["guard/grad_norm_decoder_delta"]))
    clip = float(np.median(norms))
    assert clip > 0 and np.isfinite(clip)
    eager = _run(_cfg(precision, skip_nonfinite=True, grad_clip_norm=clip), 7, dev)
    graph = _run(_cfg(precision, hip_graph=True, grad_clip_norm=clip), 7, dev)
    assert graph["captured"] and not eager["captured"]
    _assert_same_run(eager, graph)
    for k in eager["banks"]:
        assert eager["report"][k]["clipped"] == graph["report"][k]["clipped"], k
        assert eager["report"][k]["norm"] == graph["report"][k]["norm"] and eager["report"][k]["scale"] == graph["report"][k]["scale"]
    assert 0 < graph["report"]["decoder_delta"]["clipped"] < 7, graph["report"]["decoder_delta"]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_persistently_bad_key_never_steps(precision, graph, dev):
    """(iii) `probe: {rec_scale: inf}` makes the mask decoder's logit gradient non-finite and leaves the forward pass finite: over four
    steps decoder_visualize keeps its initial p, m, v and counts four skips in a row; every other key moves and stays finite."""
    run = _run(_cfg(precision, hip_graph=graph, skip_nonfinite=True, probe={"rec_scale": float("inf")}), 4, dev)
    assert run["captured"] == graph
    rep = run["report"]
    for n in ("p", "m", "v"):
        assert torch.equal(run["banks"]["decoder_visualize"][n], run["first"]["decoder_visualize"][n]), n
    assert rep["decoder_visualize"]["consecutive"] == 4 and rep["decoder_visualize"]["skipped"] == 4
    assert rep["decoder_visualize"]["nonfinite"] > 0
    for k in run["banks"]:
        if k == "decoder_visualize":
            continue
        assert rep[k]["skipped"] == 0 and rep[k]["consecutive"] == 0, k
        assert not torch.equal(run["banks"][k]["p"], run["first"][k]["p"]), k
        for n in ("p", "m", "v"):
            assert bool(torch.isfinite(run["banks"][k][n]).all()), (k, n)
    assert rep["state"]["skipped"] == 0


def test_iterate_ends_the_run_after_too_many_skips_in_a_row(dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as Ro
    cfg = _cfg("bf16", skip_nonfinite=True, nonfinite_max_consecutive=2, probe={"rec_scale": float("inf")})
    tr = Trainer(cfg, None, TrainModel(cfg, device=dev, seed=0))
    lines = []
    with pytest.raises(FloatingPointError, match="decoder_visualize"):
        tr.iterate((Ro.synthetic_views(cfg, seed=100 + i) for i in range(6)), num_steps=6, log_fn=lines.append)
    assert tr.global_step == 3          # logged after steps 0 and 2: one skip in a row, then three
    assert any("guard/skipped_decoder_visualize: 3" in ln for ln in lines)


def test_a_transient_bad_step_skips_one_key_once(dev, monkeypatch):
    """(iv) one NaN written into one key's bucket at step 2, right before its guard: that key alone is skipped, its run of skips ends at
    step 3, and every weight is finite afterwards."""
    _, ops = _mods()
    key, real, now = "decoder_delta", ops.grad_guard, {"step": -1, "bucket": None}

    def planted(g, rec, *a, **kw):
        if now["step"] == 2 and g.data_ptr() == now["bucket"]:
            g[5] = float("nan")
        return real(g, rec, *a, **kw)

    monkeypatch.setattr(ops, "grad_guard", planted)
    seen = []

    def each(step, tr, model):
        now["bucket"] = model.bank.groups[key]["flat"]["g"].data_ptr()
        now["step"] = step + 1
        seen.append((tr.guard_report(), model.bank.groups[key]["flat"]["p"].detach().cpu().clone()))

    run = _run(_cfg("bf16", skip_nonfinite=True), 4, dev, each=each)
    reps = [s[0] for s in seen]
    assert [r[key]["consecutive"] for r in reps] == [0, 0, 1, 0]
    assert [r[key]["skipped"] for r in reps] == [0, 0, 1, 1]
    assert reps[2][key]["nonfinite"] == 1 and reps[3][key]["nonfinite"] == 0
    assert torch.equal(seen[2][1], seen[1][1]) and not torch.equal(seen[3][1], seen[2][1]) and not torch.equal(seen[1][1], seen[0][1])
    for k in run["banks"]:
        if k != key:
            assert all(r[k]["skipped"] == 0 for r in reps), k
        for n in ("p", "m", "v"):
            assert bool(torch.isfinite(run["banks"][k][n]).all()), (k, n)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import upsparts_amd  # noqa: F401
    from upsparts_amd import dist as D
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as Ro
    D.init_from_env("gloo")
    dev = torch.device("cuda:0")
    cfg = _cfg("fp32", skip_nonfinite=True, grad_clip_norm=1e-3)
    model = TrainModel(cfg, device=dev, seed=0)
    tr = Trainer(cfg, None, model, world_size=world, rank=rank)
    for step in range(3):
        tr.train_step(Ro.synthetic_views(cfg, seed=1234 + 10 * step + rank), Ro.synthetic_noise(cfg, seed=4321 + 10 * step + rank))
    out[rank] = {"banks": _snap(model), "report": tr.guard_report(), "state": {k: float(v) for k, v in tr.state.items()}}
    torch.distributed.destroy_process_group()


def test_two_ranks_decide_alike(dev):
    """(v) three data-parallel steps (gloo, two ranks on one device) with both keys on: the bucket is guarded after its all-reduce, so
    the replicas stay bit-identical and their guard reports are equal."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    for k in r0["banks"]:
        for n in ("p", "m", "v"):
            assert torch.equal(r0["banks"][k][n], r1["banks"][k][n]), (k, n)
            assert bool(torch.isfinite(r0["banks"][k][n]).all()), (k, n)
    assert r0["report"] == r1["report"] and r0["state"] == r1["state"]
    assert all(r0["report"][k]["norm"] > 0 for k in r0["banks"])
    assert any(r0["report"][k]["clipped"] > 0 for k in r0["banks"])
