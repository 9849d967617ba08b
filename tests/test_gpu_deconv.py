"""GPU tests of `upsample: conv_transposed` (weight-normalised deconv2d, csrc/deconv3x3_s2.hip): the layer against the fp64
restatement (tests/deconv_ref.py) in fp32, bf16 and the mask decoder's fp16 format, through the one-launch kernel and the per-class
launches; whole training steps with the method in the hourglass and the mask decoder against the oracle (patched in-test);
HIP-graph replay, fp8, the TF checkpoint round trip and a repeat test of the MFMA kernel."""
import copy

import pytest
import torch

import deconv_ref as D
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    from oracle import ref_model as R
    return lib, ops, R


def _pad(t, ld):
    return torch.nn.functional.pad(t, (0, ld - t.shape[-1]))


def _run_layer(dev, mode, coords, h, cin, nf, one_launch, zero_filter=False, n=3, seed=0):
    lib, ops, R = _mods()
    gen = torch.Generator().manual_seed(seed + 7 * h + cin + 13 * nf)
    cv = cin + (2 if coords else 0)
    V = torch.randn((3, 3, nf, cv), generator=gen) * 0.05
    if zero_filter:
        V[:, :, 0, :] = 0
    g = 0.5 + torch.rand((nf,), generator=gen)
    b = torch.randn((nf,), generator=gen) * 0.1
    x = torch.randn((n, h, h, cin), generator=gen)
    gy = torch.randn((n, 2 * h, 2 * h, nf), generator=gen)
    fmt = lib.F16 if mode == "f16" else None
    if mode == "fp32":
        xd, xq, gq = torch.float32, x, gy
    elif mode == "bf16":
        xd, xq, gq = torch.bfloat16, x.bfloat16().float(), gy.bfloat16().float()
    else:           # the mask decoder's scope: fp16 forward tensors in bf16 containers, bf16 gradients
        xd, xq, gq = torch.bfloat16, x.half().float(), gy.bfloat16().float()
    ld_i, ld_o = ops.round8(cin), ops.round8(nf)
    xt = _pad(xq, ld_i)
    xt = (xt.half().view(torch.bfloat16) if mode == "f16" else xt.to(xd)).to(dev).requires_grad_(True)
    gyt = _pad(gq, ld_o).to(xd).to(dev)
    Vt, gt, bt = (t.to(dev).requires_grad_(True) for t in (V, g, b))
    lay = ops.DeconvLayer("t/deconv2d_0", Vt, gt, bt, coords)
    lay.f16 = mode == "f16"
    prev = ops.DECONV_ONE_LAUNCH
    ops.DECONV_ONE_LAUNCH = one_launch
    try:
        y = ops.DeconvFn.apply(xt, Vt, gt, bt, lay, fmt)
        dx, dV, dg, db = torch.autograd.grad([y], [xt, Vt, gt, bt], grad_outputs=[gyt])
    finally:
        ops.DECONV_ONE_LAUNCH = prev
    torch.cuda.synchronize()
    if mode == "f16":
        y = y.view(torch.float16)
    # fp64 reference on the inputs as the kernels see them
    xr = xq.double().requires_grad_(True)
    Vr, grr, br = (t.double().requires_grad_(True) for t in (V, g, b))
    yr = D.layer(xr, Vr, grr, br, coords, R.Scope.add_coordinates)
    ref = torch.autograd.grad([yr], [xr, Vr, grr, br], grad_outputs=[gq.double()])
    out = {"y": (y[..., :nf], yr), "dx": (dx[..., :cin], ref[0]), "dV": (dV, ref[1]), "dg": (dg, ref[2]), "db": (db, ref[3])}
    # pad channels are written as zero
    if ld_o > nf:
        assert float(y.detach()[..., nf:].float().abs().max()) == 0.0
    if ld_i > cin:
        assert float(dx[..., cin:].float().abs().max()) == 0.0
    return out


SHAPES = [(4, 3, 10), (16, 10, 3), (16, 32, 34), (64, 34, 32), (16, 128, 128), (8, 128, 32)]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("coords", [False, True])
@pytest.mark.parametrize("h,cin,nf", SHAPES)
def test_deconv_layer_matches_restatement(dev, mode, coords, h, cin, nf):
    tol = 1e-3 if mode == "fp32" else 2e-2
    for one_launch in ((False,) if mode == "fp32" else (True, False)):
        out = _run_layer(dev, mode, coords, h, cin, nf, one_launch)
        for k, (a, r) in out.items():
            a = a.float().cpu()
            assert torch.isfinite(a).all(), k
            e = rel_err(a, r)
            assert e <= tol, "{} ({}, coords {}, one launch {}): rel err {}".format(k, mode, coords, one_launch, e)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_deconv_zero_filter_gives_the_bias(dev, mode):
    """An all-zero filter: the normalisation's clamp keeps everything finite and that channel's output is its bias."""
    out = _run_layer(dev, mode, False, 16, 32, 16, True, zero_filter=True)
    for k in ("y", "dx", "dV", "dg", "db"):
        assert torch.isfinite(out[k][0].float()).all(), k
    y, yr = out["y"]
    y, yr = y.detach(), yr.detach()
    assert float((yr[..., 0] - yr[0, 0, 0, 0]).abs().max()) == 0.0       # the reference: constant b[0]
    assert float((y[..., 0].float().cpu() - yr[..., 0]).abs().max()) <= (1e-6 if mode == "fp32" else 1e-2) * max(1.0, abs(float(yr[0, 0, 0, 0])))


def test_one_launch_kernel_is_used_and_repeatable(dev):
    """The largest deconvolution of a CUB-128 B=64 step (the hourglass: 64 -> 32 channels, 64x64 -> 128x128) six times: bit-identical
    (the MFMA kernels of this tree carry a repeat test, docs/design/rows_hazard.md); and the one-launch kernel takes that shape."""
    lib, ops, R = _mods()
    gen = torch.Generator().manual_seed(3)
    V = (torch.randn((3, 3, 32, 64), generator=gen) * 0.05).to(dev)
    g, b = torch.ones(32, device=dev), (torch.randn(32, generator=gen) * 0.1).to(dev)
    x = torch.randn((64, 64, 64, 64), generator=gen).bfloat16().to(dev)
    lay = ops.DeconvLayer("t/deconv2d_0", V, g, b, False)
    ent = lay.prepared(lib.BF16, lib.BF16, 64, 64)
    ys = []
    for _ in range(6):
        y = torch.empty((64, 128, 128, 32), dtype=torch.bfloat16, device=dev)
        rc = lib.load().ups_deconv3x3_s2_fwd(lib.ptr(x), lib.BF16, 64, 64, 64, 64, 64, lib.ptr(ent["w_fwd"]), lib.ptr(b), None, 32, 32,
                                             lib.ptr(y), lib.stream())
        assert rc == 0
        ys.append(y)
    torch.cuda.synchronize()
    for y in ys[1:]:
        assert torch.equal(y, ys[0])
    fb = ops.deconv_forward(x, lay, one_launch=False)
    assert rel_err(ys[0][:4].float(), fb[:4].float()) <= 1e-2


# ------------------------------------------------------------------------------------------------------------- whole steps
def _config(size="tiny"):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config() if size == "tiny" else configs.small_config())
    cfg["final_hour"]["upsample_method"] = "conv_transposed"
    n = len(cfg["dv"]["upsample_config"])
    cfg["dv"]["upsample_config"] = ["conv_transposed"] + ["linear"] * (n - 1)
    cfg["vgg_widths"] = VGG_W
    return cfg


def _setup(precision, dev, monkeypatch, size="tiny"):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as R
    D.patch_oracle(monkeypatch)
    cfg = _config(size)
    cfg["precision"] = precision
    params = R.init_params(cfg, 0)
    assert any("/deconv2d_0/g" in n for n in params)
    vp = R.vgg_params(7, widths=VGG_W)
    model = TrainModel(cfg, device=dev, seed=0)
    trainer = Trainer(cfg, None, model)
    for n, p in params.items():
        assert torch.equal(model.variables[n].detach().cpu(), p), n
    return cfg, R, params, vp, model, trainer, R.synthetic_views(cfg), R.synthetic_noise(cfg)


def test_train_step_fp32_with_deconv_matches_oracle(dev, monkeypatch):
    cfg, R, params, vp, model, trainer, views, noise = _setup("fp32", dev, monkeypatch)
    state = R.initial_state(cfg)
    adam = R.init_adam(params)
    p_new, adam, state_new, o, Lo, log, grads = R.train_step(params, adam, cfg, views, noise, state, 0, vp, dtype=torch.float64,
                                                             scheme="per_key")
    losses = trainer.train_step(views, noise)
    dbg = trainer._debug
    B = cfg["batch_size"]
    assert_close(dbg["l_mean"][:B], o["l0_mean"].float(), 1e-3, "l0_mean")
    assert_close(dbg["generated"][..., :3].float(), o["generated"].float(), 1e-3, "generated")
    for k in Lo:
        lo, lh = float(Lo[k]), float(losses[k])
        assert abs(lo - lh) <= 1e-3 * max(1.0, abs(lo)), "loss {}: oracle {} hip {}".format(k, lo, lh)
    logs = trainer.fetch_logs()
    for k in ("prior_gmrf", "mask0_kl", "variance_loss", "perceptual", "patch_loss"):
        lo = float(log[k])
        assert abs(lo - logs[k]) <= 1e-3 * max(1e-6, abs(lo)) + 1e-9, "log {}: oracle {} hip {}".format(k, lo, logs[k])
    assert any("deconv2d" in n for n in grads)
    for n, g in grads.items():
        assert_close(model.bank.grads[n], g.float(), 2e-3, "gradient {}".format(n))


@pytest.mark.parametrize("size", ["tiny", "small"])
def test_train_step_bf16_with_deconv_close_to_oracle(dev, monkeypatch, size):
    cfg, R, params, vp, model, trainer, views, noise = _setup("bf16", dev, monkeypatch, size)
    o, Lo, log, _, grads = R.gradients(params, cfg, views, noise, R.initial_state(cfg), 0, vp, dtype=torch.float64)
    losses = trainer.train_step(views, noise)
    dbg = trainer._debug
    hard_o = torch.cat([R.hard_max(o["m0"]), R.hard_max(o["m1"])], 0).float()
    inter = ((dbg["hard"].cpu() > 0) & (hard_o > 0)).sum(dim=(1, 2)).float()
    union = ((dbg["hard"].cpu() > 0) | (hard_o > 0)).sum(dim=(1, 2)).float().clamp(min=1)
    assert float((inter / union).mean()) >= 0.99, "part-mask IoU vs oracle"
    for k in Lo:
        lo, lh = float(Lo[k]), float(losses[k])
        assert abs(lo - lh) <= 5e-2 * max(1.0, abs(lo)), "loss {}: oracle {} hip(bf16) {}".format(k, lo, lh)


def _run(cfg, dev, steps, seed0=100):
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as R
    model = TrainModel(cfg, device=dev, seed=0)
    tr = Trainer(cfg, None, model)
    hist = []
    for step in range(steps):
        losses = tr.train_step(R.synthetic_views(cfg, seed=seed0 + step), R.synthetic_noise(cfg, seed=seed0 + 100 + step))
        hist.append({k: float(v) for k, v in losses.items()})
    return model, tr, hist


def test_hip_graph_with_deconv_matches_eager(dev):
    cfg = _config()
    cfg["precision"] = "bf16"
    runs = {}
    for mode in ("eager", "graph"):
        c = copy.deepcopy(cfg)
        c["hip_graph"] = mode == "graph"
        model, tr, hist = _run(c, dev, 5)
        runs[mode] = (hist, {k: g["flat"]["p"].detach().cpu().clone() for k, g in model.bank.groups.items()}, tr.graph)
    assert runs["graph"][2] is not None and runs["graph"][2].graphs, "the graph was never captured"
    assert runs["eager"][0] == runs["graph"][0]
    for k in runs["eager"][1]:
        assert torch.equal(runs["eager"][1][k], runs["graph"][1][k]), k


def test_fp8_step_with_deconv_is_finite(dev):
    cfg = _config()
    cfg["precision"] = "fp8"
    model, tr, hist = _run(cfg, dev, 3)
    for h in hist:
        for k, v in h.items():
            assert v == v and abs(v) < float("inf"), (k, v)
    for k, g in model.bank.groups.items():
        assert torch.isfinite(g["flat"]["p"]).all(), k


def test_tf_checkpoint_round_trip_with_deconv(dev, tmp_path):
    """Export a TF bundle (deconv2d's g included), import it into a fresh trainer: the restored run continues identically."""
    cfg = _config()
    cfg["precision"] = "fp32"
    model, tr, _ = _run(cfg, dev, 2)
    prefix = str(tmp_path / "model.ckpt-2")
    tr.export_tf_checkpoint(prefix)
    from upsparts_amd import tfckpt
    bundle = tfckpt.read_bundle(prefix)
    assert "decoder_visualize/deconv2d_0/g" in bundle and "decoder_delta/deconv2d_0/g/Adam" in bundle
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as R
    model2 = TrainModel(cfg, device=dev, seed=5)
    tr2 = Trainer(cfg, None, model2)
    tr2.initialize(prefix)
    assert tr2.global_step == 2
    for n in model.bank.params:
        assert torch.equal(model.bank.params[n].detach().cpu(), model2.bank.params[n].detach().cpu()), n
    views, noise = R.synthetic_views(cfg, seed=300), R.synthetic_noise(cfg, seed=301)
    tr.train_step(views, noise)
    tr2.train_step(views, noise)
    for n in model.bank.params:          # the deconvolutions' g, V and b included
        assert torch.allclose(model.bank.params[n], model2.bank.params[n], atol=1e-7), n
