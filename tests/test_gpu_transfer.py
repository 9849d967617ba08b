"""Appearance transfer on the GPU: the mixed-unpool kernel (ups_unpool_mix_fwd) against ups_unpool_fwd on explicitly gathered inputs
(bit for bit: the arithmetic is the same statement for statement) and against the fp64 restatement (tests/transfer_ref.py) at the bars
test_gpu_kernels.py::test_mask_parts_unpool holds unpool_fwd to (1e-5 fp32, 1e-2 bf16); TrainModel's encode / decode / matrix methods
against ``forward`` (bit for bit on the diagonal) and against the CPU oracle (fp32 whole-graph bar, 1e-3, as test_gpu_model.py applies
it to ``generated``); the runner's --transfer; and that a transfer call leaves a training run untouched."""
import copy
import ctypes as C
import logging
import pickle

import pytest
import torch

import transfer_ref as TR
from util import assert_close

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}          # test_gpu_kernels.py::test_mask_parts_unpool, "unpool fwd"
FULL_REF_ELEMS = 1 << 25                                     # larger outputs: the fp64 bar is held on a spread of <= 4 images k


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _hard(n, hw, P, g):
    """One-hot masks [n,hw,P] with ties -- pixels with two active parts, with all P active (weights that are not all 1) and with
    none -- on at most 5 % of the pixels; image 0 holds one of each kind at any size."""
    hard = torch.nn.functional.one_hot(torch.randint(0, P, (n, hw), generator=g), P).float()
    two = torch.zeros(P); two[0] = 1.0; two[P - 1] = 0.75
    every = torch.linspace(0.5, 1.0, P)
    u = torch.rand(n, hw, generator=g)
    if hw >= 1024:
        hard[u < 0.01] = two
        hard[(u >= 0.01) & (u < 0.015)] = every
        hard[(u >= 0.015) & (u < 0.025)] = 0.0
    hard[0, 0], hard[0, 1], hard[0, 2] = two, every, 0.0
    active = (hard != 0).sum(-1)
    assert bool((active == 2).any()) and bool((active == P).any()) and bool((active == 0).any()) and bool((active == 1).any())
    assert float((active >= 2).float().mean()) <= 0.05
    return hard


def _patterns(K, n, m, P, g):
    k = torch.arange(K)
    return {"identity": (k % n, (k % m)[:, None].expand(K, P)),
            "reversed": (k % n, ((K - 1 - k) % m)[:, None].expand(K, P)),
            "full n x m": ((k // m) % n, (k % m)[:, None].expand(K, P)),
            "random per part": (torch.randint(0, n, (K,), generator=g), torch.randint(0, m, (K, P), generator=g))}


def _mix_raw(lib, hard, feat, pi, ai, dtype, ldo=None):
    """The library entry on an output pre-filled with NaN (every byte of `out` must be written, pads included)."""
    n, hw, P = hard.shape
    m, _, F = feat.shape
    K = pi.numel()
    ldo = ldo or (F + P + 7) // 8 * 8
    out = torch.full((K, hw, ldo), float("nan"), dtype=dtype, device=hard.device)
    pd, ad = pi.to(torch.int32).to(hard.device), ai.reshape(-1).to(torch.int32).to(hard.device)
    lib.call("ups_unpool_mix_fwd", lib.ptr(hard), lib.ptr(feat), lib.ptr(pd), lib.ptr(ad), lib.ptr(out), lib.dt(out), K, n, m, hw, P, F,
             ldo, lib.stream())
    return out


# P, F, (H, W), K, n, m: every part count, feature width, image size and K of the issue; 5 x 7 = a ragged single tile
CASES = ([(P, F, (5, 7), K, n, m) for P in (3, 10, 16, 20, 25) for F in (64, 8) for K, n, m in ((1, 3, 2), (7, 5, 3))]
         + [(10, 64, (128, 128), 256, 32, 8), (25, 8, (128, 128), 7, 5, 3), (16, 64, (128, 128), 1, 3, 2), (3, 8, (128, 128), 256, 8, 32),
            (20, 64, (256, 256), 7, 5, 3), (3, 8, (256, 256), 1, 3, 2), (20, 64, (256, 256), 256, 32, 8), (5, 8, (5, 7), 256, 32, 8),
            (10, 8, (256, 256), 7, 5, 3), (16, 64, (256, 256), 7, 3, 5), (25, 64, (256, 256), 1, 2, 3), (20, 8, (128, 128), 7, 5, 3),
            (25, 64, (128, 128), 7, 3, 5), (16, 8, (128, 128), 1, 3, 2)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=["P{}-F{}-{}x{}-K{}".format(c[0], c[1], c[2][0], c[2][1], c[3]) for c in CASES])
def test_mix_kernel_equals_unpool_of_gathered_inputs(case, dtype, dev):
    lib, ops = _mods()
    P, F, (H, W), K, n, m = case
    assert n != m
    g = torch.Generator().manual_seed(1000 * P + F + K)
    hard = _hard(n, H * W, P, g)
    feat = torch.randn(m, P, F, generator=g)
    hd, fd = hard.to(dev), feat.to(dev)
    for name, (pi, ai) in _patterns(K, n, m, P, g).items():
        out = _mix_raw(lib, hd, fd, pi, ai, dtype)
        ld = out.shape[-1]
        hg = hd[pi.to(dev)].view(K, H, W, P).contiguous()                                   # the parent-commit way: gathered operands
        fg = fd[ai.to(dev), torch.arange(P, device=dev)[None, :]].contiguous()
        want = ops.UnpoolFn.apply(hg, fg, dtype).view(K, H * W, ld)
        assert torch.equal(out, want), "{}: differs from ups_unpool_fwd on gathered inputs".format(name)
        assert float(out[..., F + P:].float().abs().max()) == 0.0 if ld > F + P else True, "{}: pad channels".format(name)
        del hg, fg, want
        ks = torch.arange(K) if K * H * W * ld <= FULL_REF_ELEMS else torch.linspace(0, K - 1, 4).round().long().unique()
        ref = TR.unpool_mix_ref(hard, feat, pi[ks], ai[ks])
        assert_close(out[ks.to(dev)][..., :F + P].float(), ref.float(), TOL[dtype], "{}: fp64 restatement".format(name))
        if name == "identity":              # the public call (allocates its own output) is the same launch
            assert torch.equal(ops.unpool_mix(hd.view(n, H, W, P), fd, pi, ai, dtype).view(K, H * W, ld), out)
        del out


def test_mix_kernel_argument_and_index_errors(dev):
    lib, ops = _mods()
    g = torch.Generator().manual_seed(5)
    n, m, hw, P, F = 3, 2, 35, 10, 64
    hd, fd = _hard(n, hw, P, g).to(dev), torch.randn(m, P, F, generator=g).to(dev)
    out = torch.zeros((2, hw, 96), dtype=torch.bfloat16, device=dev)
    pd = torch.zeros(2, dtype=torch.int32, device=dev)
    ad = torch.zeros(2 * P, dtype=torch.int32, device=dev)
    fn = lib.load().ups_unpool_mix_fwd

    def rc(K, ldo):
        return fn(lib.ptr(hd), lib.ptr(fd), lib.ptr(pd), lib.ptr(ad), lib.ptr(out), lib.BF16, K, n, m, hw, P, F, ldo, lib.stream())
    E_ARG = -1                                  # include/upsparts_hip.h: UPS_E_ARG
    assert rc(0, 80) == E_ARG and rc(2, 84) == E_ARG and rc(2, 72) == E_ARG
    off4 = C.c_void_p(fd.data_ptr() + 4)         # feature rows are gathered as 16-byte pieces: an unaligned table is refused, not launched
    assert fn(lib.ptr(hd), off4, lib.ptr(pd), lib.ptr(ad), lib.ptr(out), lib.BF16, 2, n, m, hw, P, F, 80, lib.stream()) == E_ARG
    assert rc(2, 80) == 0 and rc(2, 96) == 0
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) > 0 and float(out[..., F + P:].float().abs().max()) == 0.0
    h4 = hd.view(n, 5, 7, P)
    ok_p, ok_a = torch.tensor([0, 2]), torch.zeros(2, P, dtype=torch.int64)
    for bad_p, bad_a in ((torch.tensor([0, n]), ok_a), (torch.tensor([-1, 0]), ok_a), (ok_p, ok_a + m), (ok_p, ok_a - 1),
                         (torch.zeros(0, dtype=torch.int64), torch.zeros(0, P, dtype=torch.int64)), (ok_p, ok_a[:1])):
        with pytest.raises(lib.UpsError):
            ops.unpool_mix(h4, fd, bad_p, bad_a, torch.bfloat16)
    assert ops.unpool_mix(h4, fd, ok_p, ok_a, torch.bfloat16).shape == (2, 5, 7, 80)


def test_mix_kernel_repeats_bit_identically(dev):
    """The CUB-128 instance (P = 10, A = 64, K = 256, bf16) launched six times on the same operands: identical bits."""
    lib, ops = _mods()
    g = torch.Generator().manual_seed(4242)
    n, m, P, F, hw = 16, 16, 10, 64, 128 * 128
    hd, fd = _hard(n, hw, P, g).to(dev), torch.randn(m, P, F, generator=g).to(dev)
    pi, ai = _patterns(256, n, m, P, g)["full n x m"]
    first = _mix_raw(lib, hd, fd, pi, ai, torch.bfloat16)
    for r in range(1, 6):
        assert torch.equal(_mix_raw(lib, hd, fd, pi, ai, torch.bfloat16), first), "launch {} differs from the first".format(r)


def _model(precision, dev, variant="cub", size="tiny"):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel
    from oracle import ref_model as R, configs
    cfg = copy.deepcopy(configs.tiny_config(variant=variant) if size == "tiny" else configs.small_config(variant=variant))
    cfg.update(precision=precision, vgg_widths=VGG_W)
    return cfg, R, TrainModel(cfg, device=dev, seed=0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", ["tiny", "small"])
@pytest.mark.parametrize("variant", ["cub", "pennaction", "deepfashion"])
def test_matrix_diagonal_equals_forward(variant, size, precision, dev):
    cfg, R, model = _model(precision, dev, variant, size)
    views = R.synthetic_views(cfg)
    fw = {k: v.clone() for k, v in model.forward(views).items()}
    tm = model.transfer_matrix(views["view0"], views["view1"])
    B, S = cfg["batch_size"], cfg["spatial_size"]
    assert tm["generated"].shape == (B, B, S, S, 3) and tm["generated"].dtype == torch.float32
    for i in range(B):
        assert torch.equal(tm["generated"][i, i], fw["generated"][i]), "cell ({0}, {0})".format(i)
    assert torch.equal(tm["row_parts_hard"], fw["out_parts_hard"]) and torch.equal(tm["row_mask_rgb"], fw["view0_mask00_rgb"])
    assert torch.equal(tm["col_parts_hard"], model.forward({"view0": views["view1"], "view1": views["view0"]})["out_parts_hard"])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", ["tiny", "small"])
@pytest.mark.parametrize("variant", ["cub", "pennaction", "deepfashion"])
def test_encode_pose_equals_forward(variant, size, precision, dev):
    """encode_pose(view0) against what ``forward`` returns for view0, bit for bit (the figures are printed before they are held).
    ``forward`` runs the pose path on view0 and view1 as one batch of 2B and the generic convolution picks its split-K factor from
    the number of output tiles, so encode_pose runs a batch of 2B as well; a batch of B gave soft masks 6e-8 off (cub, tiny, fp32)."""
    cfg, R, model = _model(precision, dev, variant, size)
    views = R.synthetic_views(cfg)
    B, S = cfg["batch_size"], cfg["spatial_size"]
    fw = {k: v.clone() for k, v in model.forward(views).items()}
    pose = model.encode_pose(views["view0"])
    assert pose["hard"].shape == (B, S, S, cfg["n_parts"])
    feat = model.encode_appearance(views["view1"])
    assert feat.shape == (B, cfg["n_parts"], cfg["local_app_size"]) and feat.dtype == torch.float32
    for k in ("out_parts_soft", "m0_sample"):
        print("encode_pose vs forward {}: max |diff| {:.3e}, differing elements {} of {}".format(
            k, float((pose[k] - fw[k]).abs().max()), int((pose[k] != fw[k]).sum()), fw[k].numel()))
    for k in ("out_parts_hard", "out_parts_soft", "m0_sample"):
        assert torch.equal(pose[k], fw[k]), k


@pytest.mark.parametrize("variant", ["cub", "deepfashion"])
def test_transfer_matches_the_oracle_fp32(variant, dev):
    """Seed 2 of the synthetic views: the oracle's own hard masks in fp64 and in fp32 agree on every pixel of both views (checked on
    the CPU for the tiny configs of every family; smallest gap between the two largest soft-max values 2.9e-5)."""
    cfg, R, model = _model("fp32", dev, variant)
    B, P = cfg["batch_size"], cfg["n_parts"]
    ocfg = dict(copy.deepcopy(cfg), test_mode=True)
    params = R.init_params(cfg, 0)
    views, noise = R.synthetic_views(cfg, seed=2), R.synthetic_noise(cfg)
    o = R.forward(params, ocfg, views, noise, dtype=torch.float64)
    o32 = R.forward(params, ocfg, views, noise, dtype=torch.float32)
    assert torch.equal(R.hard_max(o["m0"]).float(), R.hard_max(o32["m0"])) and torch.equal(R.hard_max(o["m1"]).float(), R.hard_max(o32["m1"]))
    swapped = R.forward(params, ocfg, {"view0": views["view1"], "view1": views["view0"], "view0_target": views["view1"]}, noise,
                        dtype=torch.float64)
    hard0, feat1, feat0 = o["hard0"], o["local_app_features1"], swapped["local_app_features1"]
    assert torch.equal(model.encode_pose(views["view0"])["hard"].cpu().double(), R.hard_max(o["m0"])), "hard masks of the seed"
    dd = R.Nets(ocfg, params, None).dd

    def check(got, pose_app, table, what):
        want = dd(TR.unpool_mix_ref(hard0, table, *pose_app))
        assert_close(got.reshape(want.shape), want.float(), 1e-3, what)
    check(model.transfer_matrix(views["view0"], views["view1"])["generated"], TR.full_indices(B, B, P), feat1, "full matrix")
    parts = [0, P - 1]
    check(model.transfer_matrix(views["view0"], views["view1"], parts=parts)["generated"], TR.partwise_indices(B, B, P, parts),
          torch.cat([feat0, feat1], 0), "two parts swapped")
    check(model.cross_generated(views), TR.reversed_indices(B, P), feat1, "cross_generated")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", ["tiny", "small"])
def test_decode_mixed_chunking(size, precision, dev):
    cfg, R, model = _model(precision, dev, size=size)
    rows, cols = R.synthetic_views(cfg, seed=3, batch=3)["view0"], R.synthetic_views(cfg, seed=4, batch=2)["view1"]
    hard = model.encode_pose(rows)["hard"]
    feat = model.encode_appearance(cols)
    pi, ai = TR.full_indices(3, 2, cfg["n_parts"])
    outs = [model.decode_mixed(hard, feat, pi, ai, chunk=c) for c in (1, 5, 6)] + [model.decode_mixed(hard, feat, pi, ai)]
    assert outs[0].shape == (6, cfg["spatial_size"], cfg["spatial_size"], 3)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert torch.equal(model.transfer_matrix(rows, cols)["generated"].reshape(outs[0].shape), outs[0])


def test_runner_transfer_on_a_synthetic_block(dev, tmp_path, caplog):
    import yaml
    import upsparts_amd  # noqa: F401
    from upsparts_amd import runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(tmp_path / "nowhere"),
                "data_row_csv": str(tmp_path / "nowhere" / "rows.csv"), "data_col_csv": str(tmp_path / "nowhere" / "cols.csv"),
                "generated_key": "_generated", "vis0_key": "_visualize", "vis1_key": "_app_visualize"})
    ypath = tmp_path / "transfer.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    with pytest.raises(FileNotFoundError):
        runner.main(["--transfer", str(ypath), "-p", str(tmp_path / "strict"), "--strict-dataset"])
    with caplog.at_level(logging.WARNING, logger="upsparts"):
        data = runner.main(["--transfer", str(ypath), "-p", str(tmp_path / "run")])
    assert "SYNTHETIC DATA" in caplog.text
    with open(str(tmp_path / "run" / "comparison_matrix" / "000000" / "data.p"), "rb") as f:
        disk = pickle.load(f)
    n, S = cfg["batch_size"], cfg["spatial_size"]
    assert set(disk) == {"_generated", "_visualize", "_app_visualize", "view0", "view1", "relative_file_path_",
                         "view1_relative_file_path_", "matrix", "matrix_index"}
    assert all(len(v) == n * n for v in disk.values())
    assert [tuple(ix) for ix in disk["matrix_index"]] == [(i, j) for i in range(n) for j in range(n)]
    assert disk["_generated"][0].shape == (S, S, 3) and disk["_visualize"][0].shape == (S, S, 3)
    for a, b in zip(disk["_generated"], data["_generated"]):
        assert (a == b).all()
    listed = runner.main(["--transfer", str(ypath), "-p", str(tmp_path / "run_parts"), "--parts",
                          ",".join(str(p) for p in range(cfg["n_parts"]))])
    for a, b in zip(listed["_generated"], data["_generated"]):
        assert (a == b).all(), "--parts with every part listed differs from --parts absent"


def test_training_is_untouched_by_a_transfer_call(dev):
    """test_gpu_model.py's tiny CUB bf16 whole step: three training steps with a transfer_matrix call on the same model between
    them equal three steps without one bit for bit (losses, every parameter, the state scalars; the Fp8State's counters)."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import model as M
    from oracle import ref_model as R, configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(precision="bf16", vgg_widths=VGG_W)
    runs = {}
    for mode in ("plain", "with_transfer"):
        c = copy.deepcopy(cfg)
        model = M.TrainModel(c, device=dev, seed=0)
        tr = M.Trainer(c, None, model)
        hist = []
        for step in range(3):
            views, noise = R.synthetic_views(c, seed=100 + step), R.synthetic_noise(c, seed=200 + step)
            hist.append({k: float(v) for k, v in tr.train_step(views, noise).items()})
            if mode == "with_transfer":
                before = (model.fp8.count, model.fp8.steps, dict(model.fp8.stats))
                model.transfer_matrix(views["view0"], views["view1"], parts=[0] if step else None)
                assert (model.fp8.count, model.fp8.steps, dict(model.fp8.stats)) == before
        torch.cuda.synchronize()
        runs[mode] = (hist, {k: g["flat"]["p"].detach().cpu().clone() for k, g in model.bank.groups.items()},
                      {k: float(v) for k, v in tr.state.items()})
    assert runs["plain"][0] == runs["with_transfer"][0]
    for k in runs["plain"][1]:
        assert torch.equal(runs["plain"][1][k], runs["with_transfer"][1][k]), k
    assert runs["plain"][2] == runs["with_transfer"][2]
