"""The step's host bookkeeping (stepsync.GradSync): which optimizer keys a failed step names, what a failed step that moved nothing
leaves behind, and the order in which a run creates its side streams.  Tiny bf16 steps: the smallest step that has every optimizer
key and every side stream."""
import copy
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGG_W = (8, 8, 16, 16, 16)


def _trainer(dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(precision="bf16", vgg_widths=VGG_W)
    model = TrainModel(cfg, device=dev, seed=0)
    return cfg, model, Trainer(cfg, None, model)


def test_failure_inside_the_final_adam_loop_names_the_keys_that_moved(dev, tmp_path, monkeypatch):
    """With every key's Adam at the end of the step (EARLY_ADAM off) the optimizer fails at its second launch: exactly the first key
    has stepped, the trainer says so and refuses further steps and checkpoints."""
    from upsparts_amd import ops, stepsync as SS
    from oracle import ref_model as R
    cfg, model, tr = _trainer(dev)
    views = R.synthetic_views(cfg)
    tr.train_step(views)
    monkeypatch.setattr(SS, "EARLY_ADAM", False)
    t_before = {k: g["t"] for k, g in model.bank.groups.items()}
    real, calls = ops.adam_step, []

    def second_call_fails(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("injected failure in the optimizer")
        return real(*a, **kw)
    monkeypatch.setattr(ops, "adam_step", second_call_fails)
    with pytest.raises(RuntimeError, match="injected failure"):
        tr.train_step(views)
    monkeypatch.setattr(ops, "adam_step", real)
    moved = sorted(k for k, g in model.bank.groups.items() if g["t"] != t_before[k])
    assert len(moved) == 1 and len(calls) == 2, (moved, calls)
    assert tr._poisoned and "the optimizer keys {} had been updated".format(moved) in tr._poisoned, tr._poisoned
    assert not tr.sync.stepped and not ops.Streams.master_busy
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="inconsistent"):
        tr.train_step(views)
    with pytest.raises(RuntimeError, match="refusing to write a checkpoint"):
        tr.save_checkpoint(str(tmp_path / "bad.ckpt-1"))


def test_failure_with_nothing_stepped_leaves_a_usable_trainer(dev, monkeypatch):
    """EARLY_ADAM off, the mask decoder's forward raises: no key has moved, the trainer is not poisoned, and the step it runs next
    is the second step of a trainer that never failed, bit for bit."""
    from upsparts_amd import stepsync as SS
    from oracle import ref_model as R
    monkeypatch.setattr(SS, "EARLY_ADAM", False)
    losses = {}
    for fail in (False, True):
        cfg, model, tr = _trainer(dev)
        batches = [(R.synthetic_views(cfg, seed=100 + i), R.synthetic_noise(cfg, seed=200 + i)) for i in range(2)]
        tr.train_step(*batches[0])
        if fail:
            def boom(c):
                raise RuntimeError("injected failure in the mask decoder's forward")
            good, tr._fwd_masks = tr._fwd_masks, boom
            with pytest.raises(RuntimeError, match="injected failure"):
                tr.train_step(*batches[1])
            tr._fwd_masks = good
            assert tr._poisoned is None and tr.global_step == 1
            assert all(g["t"] == 1 for g in model.bank.groups.values())
        losses[fail] = {k: float(v) for k, v in tr.train_step(*batches[1]).items()}
        assert tr.global_step == 2
    assert losses[True] == losses[False]


# two tiny eager steps on the `full` plan in a fresh process: the side streams in the order the run created them.  `dp`: the
# data-parallel hand-off (collectives forced over a gloo group of one rank)
_ORDER_CHILD = r"""
import copy, json, os, sys, time
t0 = time.perf_counter()
sys.path.insert(0, sys.argv[1])
if sys.argv[2] == "dp":
    os.environ.update(UPS_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[3], RANK="0", WORLD_SIZE="1")
import torch
import upsparts_amd  # noqa: F401
from upsparts_amd import ops
from upsparts_amd.model import TrainModel, Trainer
from oracle import configs, ref_model as R
cfg = copy.deepcopy(configs.tiny_config())
cfg.update(precision="bf16", vgg_widths=(8, 8, 16, 16, 16), stream_plan="full", hip_graph=False)
if sys.argv[2] == "dp":
    torch.distributed.init_process_group("gloo", world_size=1, rank=0)
tr = Trainer(cfg, None, TrainModel(cfg, device=torch.device("cuda:0"), seed=0))
views = R.synthetic_views(cfg)
t1 = time.perf_counter()
for _ in range(2):
    tr.train_step(views)
torch.cuda.synchronize()
print("STREAMS " + json.dumps({"order": [name for name, _ in ops.Streams._pool], "startup_s": round(t1 - t0, 2),
                               "steps_s": round(time.perf_counter() - t1, 2)}))
"""
# recorded from the parent commit's runs of the same script (docs/design/measurement_ledger.md, "One owner for the gradient hand-off").
# With UPS_COORD_STREAM=0 the CoordConv rows do not create "wgrad2": only the single-rank hand-off does, the data-parallel one never
STREAM_ORDER = {("single", "1"): ["pre", "aux", "aux1", "aux2", "wgrad", "wgrad2"],
                ("single", "0"): ["pre", "aux", "aux1", "aux2", "wgrad", "wgrad2"],
                ("dp", "0"): ["pre", "aux", "aux1", "aux2", "wgrad"]}
# measured at the parent commit on a box whose file cache already held torch (the test process has imported it): 1.9 s of start-up
# (interpreter, torch, the library, the model) + 1.3 s for the two steps with their first-call costs; twenty times that for a loaded box
ORDER_CHILD_TIMEOUT_S = 60


@pytest.mark.parametrize("mode,coord_stream", sorted(STREAM_ORDER))
def test_stream_creation_order(mode, coord_stream, dev):
    """Which HIP streams share a hardware queue depends on the order they are created in (docs/design/negative_results.md): the
    single-rank path creates "wgrad2" on demand, the data-parallel paths never do.  The order of a `full`-plan run must stay what it
    was before the hand-off moved into stepsync.GradSync."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("UPS_") or k == "UPS_LIB"}
    env["UPS_COORD_STREAM"] = coord_stream
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    r = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT, mode, port], env=env, capture_output=True, text=True, timeout=ORDER_CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STREAMS ")][-1]
    assert json.loads(line[8:])["order"] == STREAM_ORDER[(mode, coord_stream)], line
