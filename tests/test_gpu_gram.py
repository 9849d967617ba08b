"""GPU tests of the Gram-matrix perceptual terms (`gram_weight`, csrc/gram.hip): both kernels against the fp64 restatement
(tests/gram_ref.py) at the trunk's real shapes in fp32 and bf16, a repeat test, whole training steps against the oracle (patched
in-test), HIP-graph replay, fp8, DeepFashion's single-sample decoders, the 224 crop, and the untouched default path."""
import copy

import pytest
import torch

import gram_ref as G
from util import assert_close

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)
# (c, h, w, relu): the six maps of the trunk at CUB-128, at the 224 crop of resize256_crop224, and at 256^2
CUB128 = [(3, 128, 128, False), (64, 128, 128, True), (128, 64, 64, True), (256, 32, 32, True), (512, 16, 16, True), (512, 8, 8, True)]
CROP224 = [(3, 224, 224, False), (64, 224, 224, True), (128, 112, 112, True), (256, 56, 56, True), (512, 28, 28, True),
           (512, 14, 14, True)]
S256 = [(3, 256, 256, False), (64, 256, 256, True), (128, 128, 128, True), (256, 64, 64, True), (512, 32, 32, True), (512, 16, 16, True)]
ODD = [(3, 1, 1, False), (40, 1, 1, True), (3, 5, 7, False), (40, 5, 7, True), (33, 6, 6, True)]
CASES = ([(4,) + s for s in CUB128] + [(2,) + s for s in CROP224] + [(1,) + s for s in S256] + [(3,) + s for s in ODD])


def _lib():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _maps(dev, dtype, n, c, h, w, seed):
    """Independent target / generated maps [n,h,w,round8(c)] with garbage in the pad channels."""
    lib, ops = _lib()
    gen = torch.Generator().manual_seed(seed)
    ld = ops.round8(c)
    a = torch.randn((n, h, w, ld), generator=gen)
    b = torch.randn((n, h, w, ld), generator=gen)
    return a.to(dtype).to(dev), b.to(dtype).to(dev)


def _fwd(a, b, c, relu):
    """The kernels' Gram term with weight 1: (loss, sign [n,cp,cp], partial)."""
    lib, ops = _lib()
    n, h, w, ld = b.shape
    hw = h * w
    _, npart, nws, nsign = ops.gram_plan(n, hw, c, lib.dt(b))
    part = torch.empty(npart, dtype=torch.float32, device=b.device)
    sign = torch.empty(nsign, dtype=torch.int8, device=b.device)
    ws = torch.empty(nws, dtype=torch.float32, device=b.device) if nws else None
    out = torch.zeros((), dtype=torch.float32, device=b.device)
    act = lib.ACT_RELU if relu else lib.ACT_NONE
    lib.call("ups_gram_l1_fwd", lib.ptr(a), lib.ptr(b), lib.dt(b), n, hw, c, ld, act, lib.ptr(part), lib.ptr(sign), lib.ptr(ws), lib.stream())
    lib.call("ups_sum_scale", lib.ptr(part), npart, 1.0 / (ops.GRAM_DIV * hw) / (n * c * c), lib.ptr(out), 0, lib.stream())
    cp = (c + 31) // 32 * 32
    return out, sign.view(n, cp, cp), part


def _bwd(b, sign, gb, c, relu, g, coef):
    lib, _ = _lib()
    n, h, w, ld = b.shape
    act = lib.ACT_RELU if relu else lib.ACT_NONE
    lib.call("ups_gram_l1_bwd", lib.ptr(b), lib.ptr(sign), lib.ptr(gb), lib.dt(b), n, h * w, c, ld, act, lib.ptr(g), coef, lib.stream())


def test_gram_constant_is_shared():
    _, ops = _lib()
    assert ops.GRAM_DIV == G.GRAM_DIV


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,c,h,w,relu", CASES)
def test_gram_kernels_match_restatement(dev, dtype, n, c, h, w, relu):
    lib, ops = _lib()
    a, b = _maps(dev, dtype, n, c, h, w, seed=c * 1000 + h + n)
    loss, sign, _ = _fwd(a, b, c, relu)
    Ft, Fg = G.as_F(a.double(), c, relu), G.as_F(b.double(), c, relu)
    ref = G.gram_l1(Ft, Fg, 1.0)
    assert abs(float(loss) - float(ref)) <= 1e-4 * float(ref), "loss {} ref {}".format(float(loss), float(ref))
    # S: symmetric, zero outside [c, c], the sign of D wherever D is not within fp32 rounding of zero
    S = sign.to(torch.float64)
    assert torch.equal(S, S.transpose(1, 2))
    assert float(S[:, c:].abs().sum()) == 0 and float(S[:, :, c:].abs().sum()) == 0
    D = G.gram(Fg) - G.gram(Ft)
    scale = (G.gram(Fg) + G.gram(Ft)).abs().amax() + 1e-30
    clear = D.abs() > 1e-5 * scale
    assert torch.equal(S[:, :c, :c][clear], torch.sign(D)[clear])
    # backward: accumulates into a prefilled gb of the gradient's own scale; channels [c, ld) untouched
    w_g = 0.37
    g = torch.tensor(1.7, device=dev)
    coef = 2.0 * w_g / (n * c * c) / (ops.GRAM_DIV * h * w)
    grad = coef * 1.7 * (Fg @ S[:, :c, :c])
    if relu:
        grad = grad * (Fg > 0).double()
    gen = torch.Generator().manual_seed(c + h)
    gmax = float(grad.abs().max()) + 1e-30
    pre = (torch.randn(b.shape, generator=gen, dtype=torch.float64) * gmax).to(dtype).to(dev)
    gb = pre.clone()
    _bwd(b, sign, gb, c, relu, g, coef)
    torch.cuda.synchronize()
    assert torch.equal(gb[..., c:], pre[..., c:])
    ref_g = pre[..., :c].double().reshape(n, -1, c) + grad
    got = gb[..., :c].double().reshape(n, -1, c)
    err = (got - ref_g).abs()
    if dtype == torch.float32:
        assert float(err.max()) <= 1e-5 * float(ref_g.abs().max()), "bwd max err {}".format(float(err.max()))
    else:
        # one bf16 rounding of the result (the prefill is exact in bf16) plus the fp32 sum over c of exact products
        assert bool((err <= 2.0 ** -8 * ref_g.abs() + 1e-4 * gmax).all()), "bwd err {}".format(float(err.max()))


def test_gram_kernels_repeat_bit_identical(dev):
    """The CUB-128 B=64 bf16 shapes, six launches of both kernels each: bit-identical partials, signs and gradients."""
    lib, ops = _lib()
    g = torch.tensor(1.0, device=dev)
    for c, h, w, relu in CUB128:
        a, b = _maps(dev, torch.bfloat16, 64, c, h, w, seed=c + h)
        pre = torch.randn(b.shape, generator=torch.Generator().manual_seed(1)).bfloat16().to(dev) * 1e-3
        runs = []
        for _ in range(6):
            loss, sign, part = _fwd(a, b, c, relu)
            gb = pre.clone()
            _bwd(b, sign, gb, c, relu, g, 1e-3)
            runs.append((loss, sign, part, gb))
        torch.cuda.synchronize()
        for r in runs[1:]:
            for x, y in zip(r, runs[0]):
                assert torch.equal(x, y), (c, h)


# ------------------------------------------------------------------------------------------------------------- whole steps
def _config(size="tiny", variant="cub", gram_weight=0.1):
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config(variant=variant) if size == "tiny" else configs.small_config(variant=variant))
    cfg["vgg_widths"] = VGG_W
    cfg["gram_weight"] = gram_weight
    return cfg


# the weight used by the whole-step tests: with it the Gram terms are a fair share of `perceptual` in the tiny fixture (asserted)
GW = 0.02


def _setup(precision, dev, monkeypatch, size="tiny", variant="cub"):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as R
    plain = R.perceptual_loss
    G.patch_oracle(monkeypatch, GW)
    cfg = _config(size, variant, GW)
    cfg["precision"] = precision
    params = R.init_params(cfg, 0)
    vp = R.vgg_params(7, widths=VGG_W)
    model = TrainModel(cfg, device=dev, seed=0)
    trainer = Trainer(cfg, None, model)
    return cfg, R, params, vp, model, trainer, R.synthetic_views(cfg), R.synthetic_noise(cfg), plain


@pytest.mark.parametrize("variant", ["cub", "deepfashion"])
def test_train_step_fp32_with_gram_matches_oracle(dev, monkeypatch, variant):
    cfg, R, params, vp, model, trainer, views, noise, plain = _setup("fp32", dev, monkeypatch, variant=variant)
    state = R.initial_state(cfg)
    adam = R.init_adam(params)
    p_new, adam, state_new, o, Lo, log, grads = R.train_step(params, adam, cfg, views, noise, state, 0, vp, dtype=torch.float64,
                                                             scheme="per_key")
    # the Gram terms are a real share of the perceptual loss in this fixture
    l1 = float(plain(vp, o["target"], o["generated"]))
    share = 1.0 - l1 / float(log["perceptual"])
    assert 0.05 <= share <= 0.95, "Gram share of perceptual {}".format(share)
    losses = trainer.train_step(views, noise)
    for k in Lo:
        lo, lh = float(Lo[k]), float(losses[k])
        assert abs(lo - lh) <= 1e-3 * max(1.0, abs(lo)), "loss {}: oracle {} hip {}".format(k, lo, lh)
    if variant == "deepfashion":       # the three single-sample decoders' losses carry the terms
        for k, gen_key, tgt_key in (("d_single", "global_generated", "x0"), ("d_alpha", "alpha_generated", "x1"),
                                    ("d_pi", "pi_generated", "x0")):
            dim = cfg["spatial_size"] ** 2 * 3
            l1k = 1e-3 * 0.5 * dim * float(plain(vp, o[tgt_key], o[gen_key]))
            assert float(losses[k]) > l1k * 1.02, (k, float(losses[k]), l1k)
    logs = trainer.fetch_logs()
    lo = float(log["perceptual"])
    assert abs(lo - logs["perceptual"]) <= 1e-3 * abs(lo), "perceptual: oracle {} hip {}".format(lo, logs["perceptual"])
    for n, g in grads.items():
        assert_close(model.bank.grads[n], g.float(), 2e-3, "gradient {}".format(n))


@pytest.mark.parametrize("size", ["tiny", "small"])
def test_train_step_bf16_with_gram_close_to_oracle(dev, monkeypatch, size):
    cfg, R, params, vp, model, trainer, views, noise, _ = _setup("bf16", dev, monkeypatch, size)
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


def test_hip_graph_with_gram_matches_eager(dev):
    cfg = _config(gram_weight=GW)
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


@pytest.mark.parametrize("vgg_fp8", [False, True])
def test_fp8_step_with_gram_is_finite(dev, vgg_fp8):
    lib, ops = _lib()
    cfg = _config(gram_weight=GW)
    cfg["precision"] = "fp8"
    cfg["vgg_fp8"] = vgg_fp8
    seen = []
    orig = ops.PerceptualTermFn.forward

    def spy(ctx, a, b, *rest):
        seen.append((a.dtype, b.dtype))
        return orig(ctx, a, b, *rest)
    ops.PerceptualTermFn.forward = staticmethod(spy)
    try:
        model, tr, hist = _run(cfg, dev, 3)
    finally:
        ops.PerceptualTermFn.forward = staticmethod(orig)
    assert seen and all(d == (torch.bfloat16, torch.bfloat16) for d in seen), set(seen)
    for h in hist:
        for k, v in h.items():
            assert v == v and abs(v) < float("inf"), (k, v)
    for k, g in model.bank.groups.items():
        assert torch.isfinite(g["flat"]["p"]).all(), k


def test_crop224_step_with_gram(dev):
    """`perceptual_input: resize256_crop224` at 128^2, B = 2, fp32 (the fp64 oracle of a 128^2 step is too slow for the suite; the
    crop's feature-map shapes are covered against the restatement at kernel level): the Gram terms raise `perceptual` and the
    step is finite."""
    from upsparts_amd import configs
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import ref_model as R
    logs = {}
    for w in (0.0, GW):
        cfg = copy.deepcopy(configs.cub_config(n_parts=10, batch_size=2))
        cfg.update({"precision": "fp32", "perceptual_input": "resize256_crop224", "vgg_widths": VGG_W, "gram_weight": w})
        model = TrainModel(cfg, device=dev, seed=0)
        tr = Trainer(cfg, None, model)
        losses = tr.train_step(R.synthetic_views(cfg), R.synthetic_noise(cfg))
        for k, v in losses.items():
            assert torch.isfinite(torch.as_tensor(v)).all(), k
        logs[w] = tr.fetch_logs()["perceptual"]
    assert logs[GW] > logs[0.0] * 1.02, logs


@pytest.mark.parametrize("w", [0, -0.5])
def test_nonpositive_weight_launches_no_gram_kernel(dev, monkeypatch, w):
    lib, ops = _lib()
    names = []
    orig = lib.call

    def spy(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    cfg = _config(gram_weight=w)
    cfg["precision"] = "bf16"
    _run(cfg, dev, 1)
    assert "ups_l1_fwd" in names and not any(n.startswith("ups_gram") for n in names)
    names.clear()
    cfg["gram_weight"] = GW
    _run(cfg, dev, 1)
    assert "ups_gram_l1_fwd" in names and "ups_gram_l1_bwd" in names


def test_dict_gram_weight_raises(dev):
    from upsparts_amd.model import TrainModel, Trainer
    cfg = _config(gram_weight={"var_type": "linear", "options": {"start": 0, "end": 10, "start_value": 0.0, "end_value": 1.0}})
    cfg["precision"] = "bf16"
    model = TrainModel(cfg, device=dev, seed=0)
    with pytest.raises(ValueError, match="gram_weight"):
        Trainer(cfg, None, model)
