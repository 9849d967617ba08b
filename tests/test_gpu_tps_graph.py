"""`use_tps: True` under `hip_graph: True`: the step with the in-graph thin-plate-spline augmentation is captured and replayed, and
reproduces the eager trainer bit for bit -- with explicit noise, with the trainer's own draws (one generator stream in both modes),
in the image logs, and across a checkpoint.  Modelled on test_gpu_model.test_hip_graph_replay_matches_eager."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)
TPS_P = {"scal": 0.8, "tps_scal": 0.15, "rot_scal": 0.2, "off_scal": 0.2, "scal_var": 0.1, "augm_scal": 1.0}     # the shipped CUB yaml's
TPS_KEYS = ("tps_view0", "tps_view1", "tps_view0_target")


def _cfg(variant, **over):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config(variant=variant))
    cfg.update(precision="bf16", vgg_widths=VGG_W, use_tps=True, tps_parameters=dict(TPS_P))
    cfg.update(over)
    return cfg


def _trainer(cfg, dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    model = TrainModel(cfg, device=dev, seed=0)
    return model, Trainer(cfg, None, model)


def _banks(model):
    return {k: g["flat"]["p"].detach().cpu().clone() for k, g in model.bank.groups.items()}


@pytest.mark.parametrize("variant", ["cub", "deepfashion"])
def test_tps_step_is_captured_and_matches_eager(variant, dev):
    """Seven steps on explicit noise (tps_u included), with the variance weight's stair moving at step 5 (a re-capture)."""
    from oracle import ref_model as R
    cfg = _cfg(variant)
    cfg["variance_weight"]["options"].update(start=4, step_size=1, stair_factor=2.0, clip_min=1.0, clip_max=64.0)
    runs = {}
    for mode in ("eager", "graph"):
        c = copy.deepcopy(cfg)
        c["hip_graph"] = mode == "graph"
        model, tr = _trainer(c, dev)
        hist = []
        for step in range(7):
            views, noise = R.synthetic_views(c, seed=100 + step), R.synthetic_noise(c, seed=200 + step)
            assert "tps_u" in noise
            losses = tr.train_step(views, noise)
            hist.append({k: float(v) for k, v in losses.items()})
        runs[mode] = (hist, _banks(model), {k: float(v) for k, v in tr.state.items()}, tr.global_step, tr.graph, tr.tps_singular_count())
    assert runs["graph"][4] is not None and runs["graph"][4].graphs, "the step with use_tps was never captured"
    assert runs["eager"][4] is None
    assert runs["eager"][3] == runs["graph"][3] == 7
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        assert a == b, (a, b)
    for k in runs["eager"][1]:
        assert torch.equal(runs["eager"][1][k], runs["graph"][1][k]), k
    assert runs["eager"][2] == runs["graph"][2]
    assert runs["eager"][5] == runs["graph"][5] == 0


@pytest.mark.parametrize("variant", ["cub", "deepfashion"])
def test_trainer_drawn_tps_is_one_stream_in_both_modes(variant, dev):
    """noise=None: the trainer draws the TPS uniforms itself.  Eager and graph mode draw the same ones, step by step, and leave the
    generator in the same state (what a checkpoint carries)."""
    from oracle import ref_model as R
    runs = {}
    for mode in ("eager", "graph"):
        c = _cfg(variant, hip_graph=mode == "graph", noise_seed=97)
        model, tr = _trainer(c, dev)
        seen = []
        for step in range(5):
            tr.train_step(R.synthetic_views(c, seed=100 + step))
            seen.append({k: model._tps[k].detach().cpu().clone() for k in TPS_KEYS})
        runs[mode] = (seen, tr._gen.get_state().cpu(), tr.graph)
    assert runs["graph"][2] is not None and runs["graph"][2].graphs, "the step with use_tps was never captured"
    for step, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        for k in TPS_KEYS:
            assert torch.equal(a[k], b[k]), (step, k)
    assert not torch.equal(runs["eager"][0][0]["tps_view0"], runs["eager"][0][1]["tps_view0"])
    assert torch.equal(runs["eager"][1], runs["graph"][1])


def test_image_logs_of_a_replayed_tps_step(dev):
    """log_images under hip_graph with use_tps: the canvases of the raw views and of the augmented ones are rendered from buffers the
    capture owns, and are byte-equal to the eager run's at every rendered step (0 and 2: eager / warm-up, 4: after a replay)."""
    from oracle import ref_model as R
    runs = {}
    for mode in ("eager", "graph"):
        c = _cfg("cub", hip_graph=mode == "graph", log_images=True)
        model, tr = _trainer(c, dev)
        rendered = []
        for step in range(6):
            views, noise = R.synthetic_views(c, seed=100 + step), R.synthetic_noise(c, seed=200 + step)
            want = step in (0, 2, 4)
            tr.train_step(views, noise, images=want)
            if want:
                rendered.append(tr.fetch_images())
        runs[mode] = (rendered, tr.graph)
    assert runs["graph"][1] is not None and runs["graph"][1].graphs, "the step with use_tps was never captured"
    assert len(runs["eager"][0]) == len(runs["graph"][0]) == 3
    for a, b in zip(runs["eager"][0], runs["graph"][0]):
        for k in ("view0", "view1", "view0_target") + TPS_KEYS:
            assert k in a and k in b, k
            assert np.array_equal(a[k], b[k]), k
    last = runs["graph"][0][-1]
    assert not np.array_equal(last["view0"], last["tps_view0"])
    assert not np.array_equal(runs["graph"][0][0]["tps_view0"], last["tps_view0"])


def test_checkpoint_of_a_graph_run_resumes_onto_the_same_tps(dev, tmp_path):
    """A checkpoint taken after four steps of a graph run, restored into a fresh trainer: the fifth step's augmented view is the one
    the uninterrupted run sees (the generator state in the checkpoint is the one the captured steps advanced)."""
    from oracle import ref_model as R
    c = _cfg("cub", hip_graph=True, noise_seed=97)
    model, tr = _trainer(c, dev)
    for step in range(4):
        tr.train_step(R.synthetic_views(c, seed=100 + step))
    assert tr.graph is not None and tr.graph.graphs
    path = str(tmp_path / "model.ckpt-4")
    tr.save_checkpoint(path)
    views = R.synthetic_views(c, seed=104)
    tr.train_step(views)
    want = model._tps["tps_view0"].detach().cpu().clone()
    model2, tr2 = _trainer(copy.deepcopy(c), dev)
    tr2.initialize(path)
    assert tr2.global_step == 4
    tr2.train_step(views)
    assert torch.equal(model2._tps["tps_view0"].detach().cpu(), want)
