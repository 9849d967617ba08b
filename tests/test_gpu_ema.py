"""The weight EMA on the device (csrc/ema.hip): ups_ema_update and ups_ema_swap against their NumPy restatement (ema_ref.py) bit for
bit -- every count around the 16-byte piece, the block and the chunk, shadow and weights misaligned independently, normals, denormals,
+-0, +-inf and NaN, items of very different sizes in one grid, the capped grid, skipped items, the warm-up crossover, refused arguments
-- and the trainer's `ema_decay` / `use_ema` keys: unchanged training bits, the recurrence over a run's weight snapshots, a key that
never steps, the `ema_weights()` scope, native and TensorFlow checkpoints, two data-parallel ranks."""
import copy
import ctypes
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGG_W = (8, 8, 16, 16, 16)
E_ARG = -1
COUNTS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 4099, 65543]
UNEVEN = (7, 300000, 0, 1025)
BAND = 8            # floats of guard band on either side of a placed bucket
SENTINEL = -123.0


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


@functools.lru_cache(maxsize=None)
def _values(count, seed):
    """N(0,1) with denormals, +-0, +-inf, NaNs of both signs and huge values spread through it; shared and never written."""
    rng = np.random.RandomState(1000 * seed + count % 9973)
    x = rng.standard_normal(count).astype(np.float32)
    den = (rng.randint(1, 0x7fffff, size=count).astype(np.uint32) | (rng.randint(0, 2, size=count).astype(np.uint32) << 31)).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1e-38], dtype=np.float32)
    special = np.concatenate([special, np.array([0xffc00001, 0x7f800001], dtype=np.uint32).view(np.float32)])
    kind = rng.randint(0, 12, size=count)
    x = np.where(kind == 0, den, x)
    pick = special[rng.randint(0, special.size, size=count)]
    x = np.where(kind == 1, pick, x).astype(np.float32)
    x.setflags(write=False)
    return x


def _place(x, dev, offset):
    """x on the device at `offset` floats past a 16-byte aligned base, sentinel bands around it -> (whole buffer, the bucket view)."""
    buf = torch.full((x.size + 2 * BAND + 4,), SENTINEL, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[BAND + offset:BAND + offset + x.size]
    v.copy_(torch.from_numpy(np.array(x)))
    assert x.size == 0 or v.data_ptr() == buf.data_ptr() + 4 * (BAND + offset)      # (torch gives an empty view a null pointer)
    return buf, v


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _bands_intact(buf, offset, count):
    b = buf.cpu().numpy()
    return bool(np.all(b[:BAND + offset] == SENTINEL) and np.all(b[BAND + offset + count:] == SENTINEL))


def _skip_record(dev, skip):
    lib, _ = _mods()
    s = lib.StepGuard()
    s.scale, s.skip = 1.0, skip
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.int64).clone().to(dev)


@pytest.mark.parametrize("count", COUNTS)
def test_update_equals_the_restatement_at_every_misalignment(count, dev):
    """One item, shadow and weights each 0 .. 3 floats past a 16-byte boundary (sixteen pairs), four earlier updates behind it (warm-up
    decay 5 / 14), and once without warm-up: the restatement's bits, the count advanced, the weights and the bands around both untouched."""
    _, ops = _mods()
    s0, w0 = _values(count, 1), _values(count, 2)
    for warmup, decay, n0 in ((True, 0.9, 4), (False, 0.999, 0)):
        want, n_want = R.update(s0, w0, decay, warmup, n0)
        for so in range(4):
            for wo in range(4):
                if not warmup and (so, wo) not in ((0, 0), (1, 3), (2, 2)):
                    continue
                sb, s = _place(s0, dev, so)
                wb, w = _place(w0, dev, wo)
                n = torch.full((1,), n0, dtype=torch.int64, device=dev)
                omd = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
                ops.ema_update([(s, w, None)], n, omd, decay, warmup)
                assert np.array_equal(R.canon(s.cpu().numpy()), R.canon(want)), (so, wo, warmup)
                assert np.array_equal(_bits(w), R.bits(w0)), (so, wo)
                assert _bands_intact(sb, so, count) and _bands_intact(wb, wo, count), (so, wo)
                assert n.tolist() == [n_want] and np.float32(omd.item()) == R.one_minus_decay(decay, warmup, n0)


def _uneven(dev, offsets, recs):
    """The four items of UNEVEN at the given (shadow, weights) offsets with the given guard records -> host values, buffers, triples."""
    host = [(_values(c, 10 + i), _values(c, 20 + i)) for i, c in enumerate(UNEVEN)]
    placed = [(_place(s, dev, so), _place(w, dev, wo)) for (s, w), (so, wo) in zip(host, offsets)]
    triples = [(ps[1], pw[1], rec) for (ps, pw), rec in zip(placed, recs)]
    return host, placed, triples


OFFSETS = ((1, 3), (2, 1), (0, 0), (3, 3))


@pytest.mark.parametrize("max_blocks", [0, 1, 3])
@pytest.mark.parametrize("skipped,clear", [(0, 1), (1, 3)], ids=["skip7", "skip300000"])
def test_uneven_items_in_one_call(skipped, clear, max_blocks, dev):
    """Sizes 7, 300000, 0 and 1025 in one grid (75 + 3 chunks; capped at 1 and 3 blocks they stride): one item's record says skip,
    one's says go, two have none.  The skipped item keeps shadow and count, the others equal the restatement."""
    _, ops = _mods()
    recs = [None] * 4
    recs[skipped], recs[clear] = _skip_record(dev, 1), _skip_record(dev, 0)
    host, placed, triples = _uneven(dev, OFFSETS, recs)
    n0 = [2, 9, 5, 0]
    n = torch.tensor(n0, dtype=torch.int64, device=dev)
    omd = torch.full((4,), -1.0, dtype=torch.float32, device=dev)
    ops.ema_update(triples, n, omd, 0.75, True, max_blocks=max_blocks)
    got_n = n.tolist()
    for i, ((s0, w0), ((sb, s), (wb, w)), (so, wo)) in enumerate(zip(host, placed, OFFSETS)):
        want, n_want = R.update(s0, w0, 0.75, True, n0[i], skip=(i == skipped))
        if i == skipped:
            assert np.array_equal(_bits(s), R.bits(s0)) and got_n[i] == n0[i] and omd[i].item() == 0.0
        else:
            assert np.array_equal(R.canon(s.cpu().numpy()), R.canon(want)), i
            assert got_n[i] == n_want == n0[i] + 1 and np.float32(omd[i].item()) == R.one_minus_decay(0.75, True, n0[i])
        assert np.array_equal(_bits(w), R.bits(w0)), i
        assert _bands_intact(sb, so, UNEVEN[i]) and _bands_intact(wb, wo, UNEVEN[i]), i


@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "plain"])
def test_twelve_successive_updates_across_the_warmup_crossover(warmup, dev):
    """decay 0.5: with warm-up the decay is (1 + n) / (10 + n) up to n = 7 and 0.5 from n = 8 on.  Weights change between updates;
    shadows and counts are compared after each one."""
    _, ops = _mods()
    sizes = (1025, 7)
    s_host = [np.array(np.nan_to_num(_values(c, 31 + i), nan=0.5, posinf=2.0, neginf=-2.0)) for i, c in enumerate(sizes)]
    placed = [(_place(s, dev, 1 + i), _place(np.zeros_like(s), dev, 3 - i)) for i, s in enumerate(s_host)]
    triples = [(ps[1], pw[1], None) for ps, pw in placed]
    items = ops.EmaItems(triples)
    n = torch.zeros(2, dtype=torch.int64, device=dev)
    omd = torch.zeros(2, dtype=torch.float32, device=dev)
    counts = [0, 0]
    for step in range(12):
        w_host = [np.array(np.nan_to_num(_values(c, 40 + step), nan=-0.25, posinf=1.0, neginf=-1.0)) for c in sizes]
        for (_, (_, w)), wh in zip(placed, w_host):
            w.copy_(torch.from_numpy(wh))
        ops.ema_update(items, n, omd, 0.5, warmup)
        for i in range(2):
            s_host[i], counts[i] = R.update(s_host[i], w_host[i], 0.5, warmup, counts[i])
            assert np.array_equal(R.canon(placed[i][0][1].cpu().numpy()), R.canon(s_host[i])), (step, i)
        assert n.tolist() == counts == [step + 1] * 2
        want = R.one_minus_decay(0.5, warmup, step)
        assert np.float32(omd[0].item()) == want == (np.float32(0.5) if (step >= 8 or not warmup) else np.float32(1.0 - (1.0 + step) / (10.0 + step)))


@pytest.mark.parametrize("max_blocks", [0, 1, 3])
def test_swap_exchanges_in_place_and_twice_restores(max_blocks, dev):
    """The uneven four-item call at the same misalignments (records are not read by a swap): after one swap either side holds the
    other's bits -- NaN payloads and all -- after two its own; the bands around every bucket stay."""
    _, ops = _mods()
    host, placed, triples = _uneven(dev, OFFSETS, [_skip_record(dev, 1), None, None, _skip_record(dev, 0)])
    items = ops.EmaItems(triples)
    ops.ema_swap(items, max_blocks=max_blocks)
    for i, ((s0, w0), ((sb, s), (wb, w)), (so, wo)) in enumerate(zip(host, placed, OFFSETS)):
        assert np.array_equal(_bits(s), R.bits(w0)) and np.array_equal(_bits(w), R.bits(s0)), i
        assert _bands_intact(sb, so, UNEVEN[i]) and _bands_intact(wb, wo, UNEVEN[i]), i
    ops.ema_swap(items, max_blocks=max_blocks)
    for i, ((s0, w0), ((sb, s), (wb, w)), (so, wo)) in enumerate(zip(host, placed, OFFSETS)):
        assert np.array_equal(_bits(s), R.bits(s0)) and np.array_equal(_bits(w), R.bits(w0)), i
        assert _bands_intact(sb, so, UNEVEN[i]) and _bands_intact(wb, wo, UNEVEN[i]), i


@pytest.mark.parametrize("count", [1, 5, 4099])
def test_swap_at_every_misalignment(count, dev):
    _, ops = _mods()
    s0, w0 = _values(count, 1), _values(count, 2)
    for so in range(4):
        for wo in range(4):
            (sb, s), (wb, w) = _place(s0, dev, so), _place(w0, dev, wo)
            ops.ema_swap([(s, w, None)])
            assert np.array_equal(_bits(s), R.bits(w0)) and np.array_equal(_bits(w), R.bits(s0)), (so, wo)
            assert _bands_intact(sb, so, count) and _bands_intact(wb, wo, count), (so, wo)


def test_refused_arguments_launch_nothing(dev):
    """Every refusal of the header returns UPS_E_ARG and leaves shadow, weights and counts as they were; n_items == 0 is UPS_OK."""
    lib, ops = _mods()
    handle = lib.load()
    count = 1025
    s0, w0 = _values(count, 1), _values(count, 2)
    (sb, s), (wb, w) = _place(s0, dev, 0), _place(w0, dev, 0)
    n = torch.full((2,), 3, dtype=torch.int64, device=dev)
    omd = torch.full((2,), -1.0, dtype=torch.float32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def items(k=2, **edit):
        arr = (lib.EmaItem * max(1, k))()
        for i in range(k):
            arr[i].shadow, arr[i].weights, arr[i].count, arr[i].rec = s.data_ptr(), w.data_ptr(), count, None
        for field, value in edit.items():
            setattr(arr[0], field, value)
        return arr

    def update(arr, k=2, decay=0.5, n_=n, omd_=omd, max_blocks=0):
        return handle.ups_ema_update(arr, k, decay, 1, P(n_) if n_ is not None else None, P(omd_) if omd_ is not None else None,
                                     max_blocks, lib.stream())

    def swap(arr, k=2, max_blocks=0):
        return handle.ups_ema_swap(arr, k, max_blocks, lib.stream())

    def untouched():
        torch.cuda.synchronize(dev)
        return (np.array_equal(_bits(s), R.bits(s0)) and np.array_equal(_bits(w), R.bits(w0)) and n.tolist() == [3, 3]
                and omd.tolist() == [-1.0, -1.0])

    shared = [dict(k=-1), dict(k=17, arr=items(17)), dict(arr=None, k=1), dict(arr=items(shadow=None)), dict(arr=items(weights=None)),
              dict(arr=items(count=-1)), dict(arr=items(shadow=s.data_ptr() + 2)), dict(arr=items(weights=w.data_ptr() + 1)),
              dict(max_blocks=-1)]
    for case in shared:
        case = dict(case)
        arr = case.pop("arr", items())
        assert update(arr, **case) == E_ARG and untouched(), case
        assert swap(arr, **case) == E_ARG and untouched(), case
    for case in (dict(n_=None), dict(omd_=None), dict(decay=float("nan")), dict(decay=1.0), dict(decay=-0.1), dict(decay=1.5)):
        assert update(items(), **case) == E_ARG and untouched(), case
    assert update(items(), k=0) == 0 and swap(items(), k=0) == 0 and update(None, k=0) == 0 and swap(None, k=0) == 0 and untouched()
    # a NULL bucket is fine when the item is empty
    assert update(items(shadow=None, weights=None, count=0)) == 0 and swap(items(shadow=None, weights=None, count=0)) == 0
    torch.cuda.synchronize(dev)
    assert n.tolist() == [4, 4]
    # the python wrappers refuse what the kernels cannot take before calling them
    with pytest.raises(lib.UpsError):
        ops.ema_update([(s.double(), w, None)], n[:1], omd[:1], 0.5, True)
    with pytest.raises(lib.UpsError):
        ops.ema_update([(s, w[:-1], None)], n[:1], omd[:1], 0.5, True)
    with pytest.raises(lib.UpsError):
        ops.ema_update([(s, w, None)], n, omd, 0.5, True)              # two counts for one item
    with pytest.raises(lib.UpsError):
        ops.ema_swap([(s.cpu(), w, None)])
    with pytest.raises(lib.UpsError):
        ops.ema_swap([(s, w, None)] * 17)


# ---------------------------------------------------------------------------------------------- the trainer
def _cfg(precision, **over):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config(variant="cub"))
    cfg.update(precision=precision, vgg_widths=VGG_W)
    cfg.update(over)
    return cfg


def _snap(model):
    return {k: {n: g["flat"][n].detach().cpu().clone() for n in ("p", "m", "v")} for k, g in model.bank.groups.items()}


def _shadows(tr):
    return {k: t.detach().cpu().clone() for k, t in tr._ema["shadow"].items()}


def _make(cfg, dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    model = TrainModel(cfg, device=dev, seed=0)
    return Trainer(cfg, None, model), model


def _steps(tr, cfg, start, stop, each=None):
    from oracle import ref_model as Ro
    hist = []
    for step in range(start, stop):
        losses = tr.train_step(Ro.synthetic_views(cfg, seed=100 + step), Ro.synthetic_noise(cfg, seed=200 + step))
        hist.append({k: float(v) for k, v in losses.items()})
        if each is not None:
            each(step, tr, tr.model)
    return hist


def _result(tr, model, first, hist):
    out = {"first": first, "banks": _snap(model), "state": {k: float(v) for k, v in tr.state.items()}, "losses": hist,
           "captured": tr.graph is not None and bool(tr.graph.graphs)}
    if tr._ema is not None:
        out.update(shadows=_shadows(tr), counts=dict(tr.ema_report()))
    return out


def _run(cfg, steps, dev, each=None):
    """`steps` steps on explicit views and noise -> what a run leaves behind.  each(step, trainer, model): called after every step."""
    tr, model = _make(cfg, dev)
    first = _snap(model)
    return _result(tr, model, first, _steps(tr, cfg, 0, steps, each))


def _assert_same_run(a, b):
    for k in a["banks"]:
        for n in ("p", "m", "v"):
            assert torch.equal(a["banks"][k][n].view(torch.int32), b["banks"][k][n].view(torch.int32)), (k, n)
    assert a["state"] == b["state"]
    assert a["losses"] == b["losses"]


def _assert_same_shadows(a, b):
    assert sorted(a["shadows"]) == sorted(b["shadows"]) and a["counts"] == b["counts"]
    for k in a["shadows"]:
        assert torch.equal(a["shadows"][k].view(torch.int32), b["shadows"][k].view(torch.int32)), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_switching_the_ema_on_changes_no_training_bit(precision, graph, dev):
    plain = _run(_cfg(precision, hip_graph=graph), 5, dev)
    ema = _run(_cfg(precision, hip_graph=graph, ema_decay=0.5), 5, dev)
    assert plain["captured"] == ema["captured"] == graph
    _assert_same_run(plain, ema)
    assert "shadows" not in plain and sorted(ema["shadows"]) == sorted(ema["banks"])
    assert all(c == 5 for c in ema["counts"].values())
    for k in ema["banks"]:          # the shadows trail the weights: neither where they started nor where the weights are
        assert not torch.equal(ema["shadows"][k], ema["first"][k]["p"]) and not torch.equal(ema["shadows"][k], ema["banks"][k]["p"]), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_shadows_follow_the_recurrence_over_the_weight_snapshots(graph, dev):
    """After step k every key's shadow is the restatement applied to the weights after steps 0 .. k, starting from the initial weights,
    with the warm-up decays (1 + n) / (10 + n), and every count is k + 1."""
    want = {}

    def each(step, tr, model):
        for k in tr._ema["keys"]:
            w = model.bank.groups[k]["flat"]["p"].detach().cpu().numpy()
            want[k], n = R.update(want[k], w, 0.75, True, step)
            got = tr._ema["shadow"][k].detach().cpu().numpy()
            assert np.array_equal(R.bits(got), R.bits(want[k])), (step, k)
            assert n == step + 1
        assert list(tr.ema_report().values()) == [step + 1] * len(tr._ema["keys"])

    cfg = _cfg("bf16", hip_graph=graph, ema_decay=0.75)
    tr, model = _make(cfg, dev)
    for k in tr._ema["keys"]:
        want[k] = model.bank.groups[k]["flat"]["p"].detach().cpu().numpy().copy()
        assert torch.equal(tr._ema["shadow"][k], model.bank.groups[k]["flat"]["p"])        # a copy of the weights after construction
    _steps(tr, cfg, 0, 5, each)
    assert (tr.graph is not None and bool(tr.graph.graphs)) == graph


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_persistently_bad_key_keeps_its_shadow(graph, dev):
    """`skip_nonfinite` with `probe: {rec_scale: inf}`: decoder_visualize never steps, so its shadow keeps its initial bits and its count
    stays 0 -- decided on the device at every step, replays included; every other key counts 4."""
    run = _run(_cfg("bf16", hip_graph=graph, skip_nonfinite=True, ema_decay=0.5, probe={"rec_scale": float("inf")}), 4, dev)
    assert run["captured"] == graph
    bad = "decoder_visualize"
    assert torch.equal(run["shadows"][bad].view(torch.int32), run["first"][bad]["p"].view(torch.int32)) and run["counts"][bad] == 0
    for k in run["banks"]:
        if k != bad:
            assert run["counts"][k] == 4, k
            assert not torch.equal(run["shadows"][k], run["first"][k]["p"]), k
            assert bool(torch.isfinite(run["shadows"][k]).all()), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_ema_weights_scope_leaves_training_alone(graph, dev):
    """bf16, four steps, `with tr.ema_weights(): model.segment(views)` after step 2 (counted from 0: under hip_graph the first replayed
    step, so that a replay follows the scope): banks, state and losses are those of the run without the scope; inside it `segment`
    returns what a fresh TrainModel loaded with the shadows returns."""
    from oracle import ref_model as Ro
    cfg = _cfg("bf16", hip_graph=graph, ema_decay=0.5)
    views = Ro.synthetic_views(cfg, seed=77)["view0"]
    seen = {}

    def each(step, tr, model):
        if step == 2:
            before = _snap(model)
            seen["state"] = tr.ema_state()
            with tr.ema_weights():
                for k in tr._ema["keys"]:       # inside: the model's weights are the shadows
                    assert torch.equal(model.bank.groups[k]["flat"]["p"].detach().cpu().view(torch.int32),
                                       _shadow_flat(seen["state"], model, k).view(torch.int32)), k
                seen["segment"] = model.segment(views).cpu()
            after = _snap(model)
            for k in before:
                assert torch.equal(before[k]["p"].view(torch.int32), after[k]["p"].view(torch.int32)), k
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(seen["state"].values(), tr.ema_state().values()))

    plain = _run(cfg, 4, dev)
    scoped = _run(cfg, 4, dev, each=each)
    assert plain["captured"] == scoped["captured"] == graph
    _assert_same_run(plain, scoped)
    _assert_same_shadows(plain, scoped)
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel
    fresh = TrainModel(_cfg("bf16"), device=dev, seed=0)
    fresh.bank.load(seen["state"])
    assert torch.equal(fresh.segment(views).cpu(), seen["segment"])
    live = TrainModel(_cfg("bf16"), device=dev, seed=0)         # (and the shadows are not the weights: the scope mattered)
    assert any(not torch.equal(seen["state"][n], live.bank.params[n].detach().cpu()) for n in seen["state"])


def _shadow_flat(state, model, key):
    return torch.cat([state[n].reshape(-1) for n in model.bank.groups[key]["names"]]) if model.bank.groups[key]["names"] else torch.zeros(0)


def test_ema_weights_refusals(dev):
    tr, _ = _make(_cfg("fp8", ema_decay=0.5), dev)
    with pytest.raises(ValueError, match="fp8"):
        with tr.ema_weights():
            pass
    off, _ = _make(_cfg("bf16"), dev)
    with pytest.raises(ValueError, match="ema_decay"):
        with off.ema_weights():
            pass
    with pytest.raises(ValueError, match="ema_decay"):
        off.ema_report()


@pytest.fixture(scope="module")
def three_steps(dev, tmp_path_factory):
    """A trainer after three steps with the EMA on and its native checkpoint; shared and never stepped again."""
    cfg = _cfg("bf16", ema_decay=0.5)
    tr, model = _make(cfg, dev)
    first = _snap(model)
    hist = _steps(tr, cfg, 0, 3)
    d = tmp_path_factory.mktemp("ema")
    paths = {"native": str(d / "model.ckpt-3"), "tf": str(d / "tf" / "model.ckpt-3"), "tf_ema": str(d / "tf_ema" / "model.ckpt-3")}
    tr.save_checkpoint(paths["native"])
    return {"cfg": cfg, "paths": paths, "trainer": tr, "result": _result(tr, model, first, hist), "hist": hist}


@pytest.fixture(scope="module")
def tf_bundle(three_steps):
    """That trainer's TensorFlow bundle (weights, Adam slots, shadows under `<var>/ExponentialMovingAverage`)."""
    os.makedirs(os.path.dirname(three_steps["paths"]["tf"]))
    three_steps["trainer"].export_tf_checkpoint(three_steps["paths"]["tf"])
    return three_steps["paths"]["tf"]


@pytest.fixture(scope="module")
def tf_ema_bundle(three_steps):
    """That trainer's bundle with the shadows under the plain variable names."""
    os.makedirs(os.path.dirname(three_steps["paths"]["tf_ema"]))
    three_steps["trainer"].export_tf_checkpoint(three_steps["paths"]["tf_ema"], weights="ema")
    return three_steps["paths"]["tf_ema"]


def test_native_checkpoint_resumes_the_shadows(three_steps, dev):
    """Save after three steps, restore into a new trainer, two more steps: five uninterrupted steps, shadows and counts included.  With
    the key off the file's keys are the earlier ones."""
    cfg = three_steps["cfg"]
    whole = _run(cfg, 5, dev)
    ck = torch.load(three_steps["paths"]["native"], map_location="cpu")
    assert sorted(ck["ema"]) == ["n", "params"] and all(v == 3 for v in ck["ema"]["n"].values())
    tr, model = _make(cfg, dev)
    tr.initialize(three_steps["paths"]["native"])
    mid = _result(tr, model, None, [])
    _assert_same_shadows(mid, three_steps["result"])
    hist = three_steps["hist"] + _steps(tr, cfg, 3, 5)
    resumed = _result(tr, model, None, hist)
    _assert_same_run(whole, resumed)
    _assert_same_shadows(whole, resumed)
    assert all(c == 5 for c in resumed["counts"].values())


def test_checkpoint_without_the_key_has_the_earlier_keys(dev, tmp_path):
    cfg = _cfg("bf16")
    tr, model = _make(cfg, dev)
    tr.save_checkpoint(str(tmp_path / "model.ckpt-0"))
    ck = torch.load(str(tmp_path / "model.ckpt-0"), map_location="cpu")
    assert sorted(ck) == sorted(["params", "global_step", "adam", "state", "noise_offset", "gen_state", "rank", "world_size"])
    # feature on, a file without shadows: the shadows are the restored weights, counts 0
    on, m_on = _make(_cfg("bf16", ema_decay=0.5), dev)
    _steps(on, on.config, 0, 1)
    on.initialize(str(tmp_path / "model.ckpt-0"))
    got = _result(on, m_on, None, [])
    assert all(c == 0 for c in got["counts"].values())
    for k in got["shadows"]:
        assert torch.equal(got["shadows"][k].view(torch.int32), got["banks"][k]["p"].view(torch.int32)), k
    # use_ema with such a file: refused
    use, _ = _make(_cfg("bf16", use_ema=True), dev)
    with pytest.raises(ValueError, match="holds no shadow weights"):
        use.initialize(str(tmp_path / "model.ckpt-0"))


def test_tf_bundle_restores_the_shadows(three_steps, tf_bundle, dev):
    src = three_steps["result"]
    tr, model = _make(three_steps["cfg"], dev)
    tr.initialize(tf_bundle)
    got = _result(tr, model, None, [])
    for k in src["shadows"]:
        assert torch.equal(got["shadows"][k].view(torch.int32), src["shadows"][k].view(torch.int32)), k
        assert torch.equal(got["banks"][k]["p"].view(torch.int32), src["banks"][k]["p"].view(torch.int32)), k
    assert not any("ExponentialMovingAverage" in n for n in tr.not_restored_from_tf)
    assert all(c == 3 for c in got["counts"].values())         # (a bundle's counts are its global step)


@pytest.mark.parametrize("route", ["tf_weights_ema", "native_use_ema", "tf_use_ema"])
def test_ema_weights_reach_every_restoring_route(route, three_steps, request, dev):
    """export_tf_checkpoint(weights="ema") read by a plain trainer, and `use_ema: True` on the native file and on the bundle, with the
    feature itself off: the weights are the shadows."""
    src = three_steps["result"]
    cfg = _cfg("bf16") if route == "tf_weights_ema" else _cfg("bf16", use_ema=True)
    path = {"tf_weights_ema": lambda: request.getfixturevalue("tf_ema_bundle"), "tf_use_ema": lambda: request.getfixturevalue("tf_bundle"),
            "native_use_ema": lambda: three_steps["paths"]["native"]}[route]()
    tr, model = _make(cfg, dev)
    tr.initialize(path)
    assert tr._ema is None
    banks = _snap(model)
    for k in src["shadows"]:
        assert torch.equal(banks[k]["p"].view(torch.int32), src["shadows"][k].view(torch.int32)), k
        assert not torch.equal(banks[k]["p"], src["banks"][k]["p"]), k
    if route != "tf_weights_ema":
        return
    # feature off, use_ema off: a file's shadows are ignored
    plain, m_plain = _make(_cfg("bf16"), dev)
    plain.initialize(three_steps["paths"]["native"])
    for k in src["banks"]:
        assert torch.equal(_snap(m_plain)[k]["p"].view(torch.int32), src["banks"][k]["p"].view(torch.int32)), k


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
    cfg = _cfg("fp32", ema_decay=0.5)
    model = TrainModel(cfg, device=dev, seed=0)
    tr = Trainer(cfg, None, model, world_size=world, rank=rank)
    for step in range(3):
        tr.train_step(Ro.synthetic_views(cfg, seed=1234 + 10 * step + rank), Ro.synthetic_noise(cfg, seed=4321 + 10 * step + rank))
    out[rank] = {"banks": _snap(model), "shadows": _shadows(tr), "counts": dict(tr.ema_report())}
    torch.distributed.destroy_process_group()


def test_two_ranks_keep_equal_shadows(dev):
    """Three data-parallel steps (gloo, two ranks on one device) on different data: the replicas' weights are identical after every
    Adam, so their shadows and counts are too, without a collective of their own."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    assert r0["counts"] == r1["counts"] and all(c == 3 for c in r0["counts"].values())
    for k in r0["shadows"]:
        assert torch.equal(r0["shadows"][k].view(torch.int32), r1["shadows"][k].view(torch.int32)), k
        assert torch.equal(r0["banks"][k]["p"].view(torch.int32), r1["banks"][k]["p"].view(torch.int32)), k
        assert not torch.equal(r0["shadows"][k], r0["banks"][k]["p"]), k
