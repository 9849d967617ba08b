"""Training image logs on the GPU: the canvas kernels (csrc/canvas.hip) against the fp64 restatement tests/imglog_ref.py, byte for
byte over whole canvases (blank tiles included; every canvas starts from a sentinel, so an unwritten byte fails); the trainer's
``img_ops`` after one step against the restatement applied to the step's own tensors; training with and without image logs, bit
for bit; and the runner's PNG files.

Why byte-exact is the right bar: the kernels take every decision (truncation, thresholds, half-to-even rounding) on fp64 arithmetic
over the fp32 / bf16 source values in the restatement's operation order, so there is no rounding between the two.  The exclusions the
first-item test allows near a decision boundary (|frac(255 m) - 0.5| < 1e-4 for p_heatmap, 1e-5 relative for the edge threshold) are
therefore not needed by this implementation; they are kept as stated, with the cap of 0.5 % excluded pixels per canvas."""
import copy
import os

import numpy as np
import pytest
import torch

import imglog_ref as IR

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 7


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import imglog, lib, ops
    return imglog, lib, ops


def _bin_centred(shape, g, dtype):
    """v = (u + 0.5) / 127.5 - 1 for random bytes u -- the middle of a quantisation bin -- plus exact -1, +1, -1.5, +1.5 (both
    clamps) in the first entries; rounded to `dtype` (the restatement starts from the rounded values)."""
    u = torch.randint(0, 256, shape, generator=g).double()
    v = ((u + 0.5) / 127.5 - 1.0).reshape(-1)
    v[:4] = torch.tensor([-1.0, 1.0, -1.5, 1.5], dtype=torch.float64)
    return v.reshape(shape).float().to(dtype)


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL, dtype=torch.uint8, device=dev)


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, "{}: {} of {} bytes differ (first at {})".format(what, bad, want.size, np.argwhere(got != want)[0].tolist())


def _one_hot(shape, P, g):
    return torch.nn.functional.one_hot(torch.randint(0, P, shape, generator=g), P).float()


def _bits(hot):
    P = hot.shape[-1]
    w = (2 ** torch.arange(P, dtype=torch.int64))
    v = (hot.long() * w).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("ld", [3, 8])
@pytest.mark.parametrize("N,S,cols", [(5, 16, None), (7, 16, 5), (1, 24, None)])
def test_canvas_images(N, S, cols, ld, dtype, dev):
    _, _, ops = _mods()
    g = torch.Generator().manual_seed(10 * N + ld)
    x = torch.full((N, S, S, ld), 99.0).to(dtype)                 # channels 3.. are not read
    x[..., :3] = _bin_centred((N, S, S, 3), g, dtype)
    rows, c = IR.canvas_grid(N, cols)
    out = _sentinel((rows * S, c * S, 3), dev)
    got = ops.canvas_images(x.to(dev), cols=cols, out=out)
    assert got is out
    want = IR.images_canvas(x, cols)
    assert {0, 255} <= set(np.unique(want).tolist())              # both clamps are exercised
    _same(got, want, "images N={} S={} cols={} ld={}".format(N, S, cols, ld))
    if N == 5:
        assert (want[2 * S:, :] == 127).all() and (want[S:2 * S, 2 * S:] == 127).all()      # the four blank tiles


def test_canvas_wrappers_refuse_what_the_kernels_do_not_take(dev):
    IL, lib, ops = _mods()
    x = torch.zeros(2, 8, 8, 3, device=dev)
    col = torch.from_numpy(IL.mask_color_bytes(IL.mask_colors01(3))).to(dev)
    for bad in (x.half(), x.double(), x[..., :2].contiguous(), x[:, :, ::2], x.cpu(), x[0]):
        with pytest.raises(lib.UpsError):
            ops.canvas_images(bad)
    with pytest.raises(lib.UpsError):
        ops.canvas_images(x, out=torch.zeros(16, 16, 3, dtype=torch.uint8, device=dev)[:, :8])
    with pytest.raises(lib.UpsError):
        ops.canvas_images(x, cols=0)
    m = torch.zeros(2, 8, 8, 3, device=dev)
    with pytest.raises(lib.UpsError):
        ops.canvas_mask_rgb(col, mask=m.bfloat16())
    with pytest.raises(lib.UpsError):
        ops.canvas_mask_rgb(col, mask=m, bits=torch.zeros(2, 8, 8, dtype=torch.int32, device=dev), n_parts=3)
    with pytest.raises(lib.UpsError):
        ops.canvas_mask_rgb(col, bits=torch.zeros(2, 8, 8, dtype=torch.int32, device=dev), n_parts=33)
    with pytest.raises(lib.UpsError):
        ops.canvas_mask_rgb(col[:2].contiguous(), mask=m)
    with pytest.raises(lib.UpsError):
        ops.canvas_assigned_parts(x, x.bfloat16(), hard0=m, hard1=m)
    with pytest.raises(lib.UpsError):
        ops.canvas_assigned_parts(x, x, hard0=m, hard1=m[:1])
    with pytest.raises(lib.UpsError):
        ops.canvas_first_item(m[0], col, hard=m[0])                # a [3,3] table where [256,3] is expected
    with pytest.raises(lib.UpsError):           # the library itself refuses a canvas that is not 16-byte aligned
        buf = torch.zeros(16 * 16 * 3 + 16, dtype=torch.uint8, device=dev)
        lib.call("ups_canvas_images", lib.ptr(x), lib.F32, 2, 8, 8, 3, 2, 2, lib.ptr(buf[1:]), lib.stream())


@pytest.mark.parametrize("P", [3, 10, 25])
def test_canvas_mask_rgb(P, dev):
    IL, _, ops = _mods()
    N, S = 5, 16
    g = torch.Generator().manual_seed(P)
    col = torch.from_numpy(IL.mask_color_bytes(IL.mask_colors01(P))).to(dev)
    soft = torch.softmax(torch.randn(N, S, S, P, generator=g), -1)                  # continuous: no ties
    assert int((soft.topk(2, -1).values.diff(dim=-1) == 0).sum()) == 0
    got = ops.canvas_mask_rgb(col, mask=soft.to(dev), out=_sentinel((3 * S, 3 * S, 3), dev))
    _same(got, IR.mask_rgb_canvas(soft), "soft masks P={}".format(P))
    # ties: the lowest index wins (tf.argmax), wherever the tied entries sit
    tied = soft.clone()
    tied[0, 0, 0, :] = 0.5                                    # every part
    tied[0, 0, 1, [P - 2, P - 1]] = 2.0                       # the last two
    tied[1, 3, 5, [0, P - 1]] = 2.0                           # first and last
    tied[4, 15, 15, [1, 2]] = 2.0
    want = IR.mask_rgb_canvas(tied)
    colors = IR.quantise(IR.mask_colors(P))
    assert (want[0, 0] == colors[0]).all() and (want[0, 1] == colors[P - 2]).all() and (want[3, S + 5] == colors[0]).all()
    assert (want[S + 15, S + 15] == colors[1]).all()
    _same(ops.canvas_mask_rgb(col, mask=tied.to(dev), out=_sentinel((3 * S, 3 * S, 3), dev)), want, "ties P={}".format(P))
    # a one-hot input: the path without arg-max and the bit path equal the arg-max path on the same masks
    hot = torch.nn.functional.one_hot(soft.argmax(-1), P).float()
    ref = IR.mask_rgb_canvas(hot)
    _same(ops.canvas_mask_rgb(col, mask=hot.to(dev), out=_sentinel((3 * S, 3 * S, 3), dev)), ref, "one-hot through arg-max")
    _same(ops.canvas_mask_rgb(col, mask=hot.to(dev), one_hot=True, out=_sentinel((3 * S, 3 * S, 3), dev)), ref, "one-hot, no arg-max")
    _same(IR.mask_rgb_canvas(hot, make_hot=False), ref, "restatement: make_hot=False on a one-hot mask")
    _same(ops.canvas_mask_rgb(col, bits=_bits(hot).to(dev), n_parts=P, out=_sentinel((3 * S, 3 * S, 3), dev)), ref, "hard bits")
    # encoding_masks / decoding_masks: one row of N tiles (cols = N), make_hot=False
    row = IR.coding_masks(hot)
    assert row.shape == (S, N * S, 3)
    _same(ops.canvas_mask_rgb(col, mask=hot.to(dev), one_hot=True, cols=N), row, "coding masks, one-hot")
    _same(ops.canvas_mask_rgb(col, bits=_bits(hot).to(dev), n_parts=P, cols=N), row, "coding masks, bits")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,S,P", [(3, 16, 7), (2, 16, 3)])
def test_canvas_assigned_parts(B, S, P, dtype, dev):
    _, _, ops = _mods()
    g = torch.Generator().manual_seed(100 * B + P)
    hard0, hard1 = _one_hot((B, S, S), P, g), _one_hot((B, S, S), P, g)
    v0, v1 = _bin_centred((B, S, S, 3), g, dtype), _bin_centred((B, S, S, 3), g, dtype)
    want = IR.assigned_parts(hard0, hard1, v0, v1)
    gs = IR.canvas_grid(2 * B)[0]
    assert want.shape == (-(-P // 5) * gs * S, 5 * gs * S, 3)
    if (B, P) == (3, 7):            # blank tiles at both nesting levels
        assert (want[gs * S:, 2 * gs * S:] == 127).all() and (want[2 * S:gs * S] == 127).all()
    d = lambda t: t.to(dev)
    _same(ops.canvas_assigned_parts(d(v0), d(v1), hard0=d(hard0), hard1=d(hard1), out=_sentinel(want.shape, dev)), want, "fp32 masks")
    _same(ops.canvas_assigned_parts(d(v0), d(v1), bits0=d(_bits(hard0)), bits1=d(_bits(hard1)), n_parts=P,
                                    out=_sentinel(want.shape, dev)), want, "hard bits")
    # the views may come with 8 physical channels (the activation layout)
    v8 = [torch.full((B, S, S, 8), 99.0).to(dtype) for _ in range(2)]
    v8[0][..., :3], v8[1][..., :3] = v0, v1
    _same(ops.canvas_assigned_parts(d(v8[0]), d(v8[1]), hard0=d(hard0), hard1=d(hard1)), want, "channel stride 8")


def _first_m(S, P, scale, seed):
    """Soft-max of seeded normal logits that were averaged over a 2 x 2 neighbourhood (wrapping) and doubled, times `scale`."""
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(1, S, S, P, generator=g, dtype=torch.float64)
    l = 0.25 * (l + l.roll(-1, 1) + l.roll(-1, 2) + l.roll((-1, -1), (1, 2))) * 2
    return torch.softmax(scale * l, -1).float()


@pytest.mark.parametrize("S,P,scale", [(16, 10, 3), (24, 25, 3), (16, 3, 6)])
def test_canvas_first_item(S, P, scale, dev):
    IL, _, ops = _mods()
    m = _first_m(S, P, scale, 100 + P)
    hard = torch.nn.functional.one_hot(m.argmax(-1), P).float()
    table = torch.from_numpy(IL.viridis_bytes()).to(dev)
    gp = IR.canvas_grid(P)[0]
    shapes = ((P * S, 7 * S, 1), (P * S, 4 * S, 1), (gp * S, gp * S, 3), (gp * S, gp * S, 1))
    want = {"levels": IR.level_sets(m), "edges": IR.edge_sets(m), "p_heatmap": IR.p_heatmap(m), "masks": IR.masks(hard)}
    # neither class of a set is empty: every level column and every edge column has lit and unlit pixels
    for name, n in (("levels", 7), ("edges", 4)):
        for k in range(n):
            lit = float((want[name][:, k * S:(k + 1) * S] == 255).mean())
            print("{} set {}: {:.2%} lit".format(name, k, lit))
            assert 0.0 < lit < 1.0, (name, k, lit)
    excl = {"levels": np.zeros(shapes[0][:2], bool), "masks": np.zeros(shapes[3][:2], bool),
            "p_heatmap": IR.heat_margin(m) < 1e-4, "edges": IR.edge_margin(m) < 1e-5}
    for by_bits in (False, True):
        out = [_sentinel(s, dev) for s in shapes]
        got = ops.canvas_first_item(m[0].to(dev), table, hard=None if by_bits else hard[0].to(dev),
                                    bits=_bits(hard[0]).to(dev) if by_bits else None, out=out)
        for name, t in zip(("levels", "edges", "p_heatmap", "masks"), got):
            a, w, e = t.cpu().numpy(), want[name], excl[name]
            assert a.shape == w.shape, (name, a.shape, w.shape)
            frac = float(e.mean())
            print("{} (bits={}): {:.4%} of the pixels excluded, {} bytes differ".format(name, by_bits, frac, int((a != w).sum())))
            assert frac <= 0.005, "{}: {:.3%} of the pixels lie at a decision boundary".format(name, frac)
            diff = (a != w).any(axis=2) & ~e
            assert not diff.any(), "{}: {} pixels differ (first at {})".format(name, int(diff.sum()), np.argwhere(diff)[0].tolist())
    assert set(np.unique(want["masks"]).tolist()) <= {127, 255} and want["p_heatmap"].min() >= 127       # [0,1] maps: gray to white


def _trainer(dev, variant="cub", **over):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import model as M
    from oracle import ref_model as R, configs
    cfg = copy.deepcopy(configs.tiny_config(variant=variant))
    cfg.update(precision="fp32", vgg_widths=VGG_W)
    cfg.update(over)
    model = M.TrainModel(cfg, device=dev, seed=0)
    return cfg, R, M, model, M.Trainer(cfg, None, model)


CUB_KEYS = ["out_parts_soft_visualization", "m0_sample_visualization", "encoding_masks_visualization", "decoding_masks_visualization",
            "masks", "assigned_parts", "mumford_sha_edges", "p_heatmap", "m0_sample_levels-0_01-0_05-0_1-0_25-0_5-0_75-0_9",
            "view0", "view1", "view0_target", "cross", "generated"]
DF_KEYS = ["out_parts_soft_visualization", "m0_sample_visualization", "encoding_masks_visualization", "decoding_masks_visualization",
           "global_generated", "alpha_generated", "pi_generated", "masks", "assigned_parts", "view0", "view1", "cross", "generated"]


@pytest.mark.parametrize("variant", ["cub", "deepfashion"])
def test_trainer_image_ops_after_one_step(variant, dev):
    cfg, R, M, model, tr = _trainer(dev, variant)
    B, S, P = cfg["batch_size"], cfg["spatial_size"], cfg["n_parts"]
    views, noise = R.synthetic_views(cfg), R.synthetic_noise(cfg)
    assert tr.fetch_images() == {} and len(tr.img_ops) == 0
    tr.train_step(views, noise, images=True)
    imgs = tr.fetch_images()            # (synchronises the side stream the canvases and the outputs below were produced on)
    assert sorted(imgs) == sorted(CUB_KEYS if variant == "cub" else DF_KEYS)
    assert all(v.dtype == np.uint8 and v.ndim == 3 for v in imgs.values())
    o = model.outputs
    hard = tr._debug["hard"].cpu()
    assert torch.equal(hard[:B], o["decoding_mask"].cpu()) and torch.equal(hard[B:], o["encoding_mask"].cpu())
    assert bool((hard.sum(-1) == 1).all())
    g = IR.canvas_grid(B)[0]
    want = {"out_parts_soft_visualization": IR.mask_visualization(o["out_parts_soft"]),
            "m0_sample_visualization": IR.mask_visualization(o["m0_sample"]),
            "encoding_masks_visualization": IR.coding_masks(hard[B:]), "decoding_masks_visualization": IR.coding_masks(hard[:B]),
            "masks": IR.masks(hard[:B]), "assigned_parts": IR.assigned_parts(hard[:B], hard[B:], views["view0"], views["view1"]),
            "view0": IR.images(views["view0"]), "view1": IR.images(views["view1"]), "generated": IR.images(o["generated"])}
    if variant == "cub":
        want.update({"mumford_sha_edges": IR.edge_sets(o["m0_sample"]), "p_heatmap": IR.p_heatmap(o["m0_sample"]),
                     IR.LEVELS_TITLE: IR.level_sets(o["m0_sample"]), "view0_target": IR.images(views["view0_target"])})
        assert want["view0"].shape == (g * S, g * S, 3) and want["masks"].shape[2] == 1
        assert want["encoding_masks_visualization"].shape == (S, B * S, 3)
    else:
        for name, key in (("global_generated", "d_single"), ("alpha_generated", "d_alpha"), ("pi_generated", "d_pi")):
            assert imgs[name].shape == (S, S, 3)
    # cross: the step's own masks and appearance features through decode_mixed (TrainModel.cross_generated's decoding)
    pi, ai = M.reversed_indices(B, P)
    cross = model.decode_mixed(tr._debug["hard"][:B], tr._debug["feat"], pi, ai)
    assert torch.equal(cross, o["cross"])
    want["cross"] = IR.images(cross)
    assert torch.equal(o["generated"], tr._debug["generated"][..., :3].float())
    for k, w in want.items():
        _same(imgs[k], w, "{} {}".format(variant, k))
    # a step that asks for no images launches none: img_ops stays what it was
    before = {k: v.data_ptr() for k, v in tr.img_ops.items()}
    tr.train_step(views, noise)
    assert {k: v.data_ptr() for k, v in tr.img_ops.items()} == before and tr._img_hold is None
    for k, v in tr.fetch_images().items():
        assert np.array_equal(v, imgs[k]), k


def test_trainer_tps_views(dev):
    cfg, R, M, model, tr = _trainer(dev, "cub", use_tps=True)
    views, noise = R.synthetic_views(cfg), R.synthetic_noise(cfg)
    tr.train_step(views, noise, images=True)
    imgs = tr.fetch_images()
    assert sorted(imgs) == sorted(CUB_KEYS + ["tps_view0", "tps_view1", "tps_view0_target"])
    for k in ("view0", "view1", "view0_target"):
        _same(imgs[k], IR.images(views[k]), k)                                  # the inputs as they came
        _same(imgs["tps_" + k], IR.images(model.outputs["tps_" + k]), "tps_" + k)
    hard, B = tr._debug["hard"].cpu(), cfg["batch_size"]
    _same(imgs["assigned_parts"], IR.assigned_parts(hard[:B], hard[B:], model.outputs["tps_view0"], model.outputs["tps_view1"]),
          "assigned_parts of the augmented views")


def _six_steps(dev, log_images, hip_graph):
    cfg, R, M, model, tr = _trainer(dev, "cub", hip_graph=hip_graph, log_images=log_images)
    rendered = []
    for step in range(6):
        views, noise = R.synthetic_views(cfg, seed=100 + step), R.synthetic_noise(cfg, seed=200 + step)
        want = log_images and step in (0, 2, 4)
        tr.train_step(views, noise, images=want)
        if want:        # (fetch_images synchronises the side stream; the step's tensors are copied before a later step refills them)
            rendered.append((tr.fetch_images(), {k: tr._debug[k].cpu().clone() for k in ("hard", "m", "generated")}))
    torch.cuda.synchronize()
    bank = model.bank
    state = {"p:" + k: g["flat"]["p"].detach().clone() for k, g in bank.groups.items()}
    state.update({"m:" + k: g["flat"]["m"].detach().clone() for k, g in bank.groups.items()})
    state.update({"v:" + k: g["flat"]["v"].detach().clone() for k, g in bank.groups.items()})
    state.update({"s:" + k: v.detach().clone().reshape(()) for k, v in tr.state.items()})
    return state, rendered, (tr, model, cfg, R)


@pytest.mark.parametrize("hip_graph", [False, True], ids=["eager", "hip_graph"])
def test_training_is_untouched_by_image_logs(hip_graph, dev):
    """Six steps with images rendered at steps 0, 2 and 4 against six steps without, from the same seed: every weight, Adam slot and
    Lagrangian state bit for bit.  Under hip_graph steps 0 and 1 are the eager warm-up and step 2 and 4 render after a replay, from
    the buffers the capture owns: the canvases of step 4 are held to the restatement there as well."""
    off, _, _ = _six_steps(dev, False, hip_graph)
    on, rendered, (tr, model, cfg, R) = _six_steps(dev, True, hip_graph)
    assert len(rendered) == 3 and set(off) == set(on)
    for k in off:
        assert torch.equal(off[k], on[k]), k
    if hip_graph:
        assert tr.graph is not None and tr.graph.graphs, "the step was not captured"
    B = cfg["batch_size"]
    views = R.synthetic_views(cfg, seed=104)
    last, dbg = rendered[-1]
    hard = dbg["hard"]
    _same(last["view1"], IR.images(views["view1"]), "view1 of step 4")
    _same(last["assigned_parts"], IR.assigned_parts(hard[:B], hard[B:], views["view0"], views["view1"]), "assigned_parts of step 4")
    _same(last["generated"], IR.images(dbg["generated"]), "generated of step 4")
    _same(last[IR.LEVELS_TITLE], IR.level_sets(dbg["m"][:B]), "level sets of step 4")
    assert not np.array_equal(rendered[0][0]["generated"], last["generated"])


def test_runner_writes_the_image_logs(dev, tmp_path):
    import yaml
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"precision": "fp32", "vgg_widths": list(VGG_W), "dataset": "no.such.Dataset"})      # -> synthetic pairs
    ypath = tmp_path / "train.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    B, S, P = cfg["batch_size"], cfg["spatial_size"], cfg["n_parts"]
    root = tmp_path / "run"
    it = runner.main(["-t", str(ypath), "--num_steps", "3", "--set", "log_images=true", "-p", str(root)])
    assert it.global_step == 3 and it.log_images is True
    files = sorted(f for f in os.listdir(str(root / "train")) if f.endswith(".png"))
    assert files == sorted("{}_{:07d}.png".format(k, s) for k in CUB_KEYS for s in (0, 2)), files
    g, gp = IR.canvas_grid(B)[0], IR.canvas_grid(P)[0]
    sizes = {"generated": (g * S, g * S), "view0": (g * S, g * S), "cross": (g * S, g * S), "encoding_masks_visualization": (S, B * S),
             "masks": (gp * S, gp * S), "p_heatmap": (gp * S, gp * S), "mumford_sha_edges": (P * S, 4 * S), IR.LEVELS_TITLE: (P * S, 7 * S),
             "assigned_parts": (-(-P // 5) * IR.canvas_grid(2 * B)[0] * S, 5 * IR.canvas_grid(2 * B)[0] * S)}
    for s in (0, 2):
        for k in CUB_KEYS:
            with Image.open(str(root / "train" / "{}_{:07d}.png".format(k, s))) as im:
                a = np.asarray(im)
            gray = k in ("masks", "mumford_sha_edges", IR.LEVELS_TITLE)
            assert a.dtype == np.uint8 and a.ndim == (2 if gray else 3), (k, a.shape)
            if k in sizes:
                assert a.shape[:2] == sizes[k], (k, a.shape)
    last = it.fetch_images()
    with Image.open(str(root / "train" / "generated_0000002.png")) as im:
        assert np.array_equal(np.asarray(im), last["generated"])
    # a second identical run, stopped after step 0: its view0 canvas is what the first run wrote
    it2 = runner.main(["-t", str(ypath), "--num_steps", "1", "--set", "log_images=true", "-p", str(tmp_path / "run2")])
    with Image.open(str(root / "train" / "view0_0000000.png")) as im:
        assert np.array_equal(np.asarray(im), it2.fetch_images()["view0"])
    # without the key nothing is written
    runner.main(["-t", str(ypath), "--num_steps", "1", "-p", str(tmp_path / "run3")])
    assert [f for f in os.listdir(str(tmp_path / "run3" / "train")) if f.endswith(".png")] == []
