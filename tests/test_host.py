"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/upsparts_hip.h
declares (no compute calls without a GPU), tap geometry for TF 'SAME', schedules, the variable naming /
optimizer-key grouping, the runner's import-path resolution, and the data-parallel helpers under gloo
(world_size 2)."""
import os
import re
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, nets, schedules, configs
    return lib, ops, nets, schedules, configs


def test_abi_library_loads_and_exports_every_declared_symbol():
    lib, *_ = _pkg()
    handle = lib.load()
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    declared = set(re.findall(r"\b(ups_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 40
    for name in declared:
        assert hasattr(handle, name), "libupsparts_hip.so lacks " + name
    assert declared == set(lib.EXPORTS), declared ^ set(lib.EXPORTS)
    assert handle.ups_abi_version() == lib.ABI_VERSION == int(re.search(r"#define UPS_ABI_VERSION (\d+)", hdr).group(1))
    # the descriptor structs of the ctypes binding are byte-compatible with what the library was compiled against
    import ctypes as C
    sizes = (C.c_int64 * 4)()
    handle.ups_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(lib.ConvDesc), C.sizeof(lib.WgradDesc), C.sizeof(lib.PriorDesc), C.sizeof(lib.PrepItem)]


def test_product_path_fails_loudly_without_gpu_or_library(monkeypatch):
    lib, *_ = _pkg()
    from upsparts_amd.model import TrainModel
    if not torch.cuda.is_available():
        with pytest.raises(lib.UpsError):
            TrainModel(_pkg()[4].cub_config())
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libupsparts_hip.so")
    with pytest.raises(lib.UpsError):
        lib.load()


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "unsupervised-part-segmentation_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("the oracle /", ""), fn + " must not reference oracle/"


def test_tools_do_not_import_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/ (tools/probes/ included since round 6:
    the one probe that used it lives under tests/ now)."""
    for tdir in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tools", "probes")):
        for fn in os.listdir(tdir):
            if fn.endswith(".py"):
                src = open(os.path.join(tdir, fn)).read()
                assert "from oracle" not in src and "import oracle" not in src, os.path.relpath(os.path.join(tdir, fn), ROOT) + " must not use oracle/"
                if tdir.endswith("tools"):
                    assert "oracle" not in src, "tools/" + fn + " must not use oracle/"
    src = open(os.path.join(ROOT, "bench.py")).read()
    head, _, tail = src.partition("def cpu_baseline")
    body, _, rest = tail.partition("\ndef run_rank")
    assert "oracle" not in head.replace("(oracle)", "")
    assert body.count("from oracle") == 1                                       # the cpu_baseline leg is the only importer
    assert "from oracle" not in rest and "import oracle" not in rest


def test_same_geometry_and_taps():
    lib, ops, *_ = _pkg()
    assert ops.same_geometry(128, 3, 1) == (128, 1)
    assert ops.same_geometry(128, 3, 2) == (64, 0)       # Appendix A.1: pad 0 before / 1 after
    assert ops.same_geometry(9, 3, 2) == (5, 1)
    assert ops.same_geometry(4, 1, 1) == (4, 0)
    lay = ops.ConvLayer("x/conv2d_0", torch.zeros(3, 3, 10, 16), torch.zeros(16), 3, 2, True, "leaky_relu")
    assert (lay.ci_log, lay.cin_v, lay.co, lay.act_in) == (8, 10, 16, lib.ACT_LRELU)
    dy, dx, tw = lay.fwd_taps(16, 16)
    assert dy[:9] == [0, 0, 0, 1, 1, 1, 2, 2, 2] and dx[:9] == [0, 1, 2] * 3 and tw[:9] == list(range(9))
    lay1 = ops.ConvLayer("x/conv2d_1", torch.zeros(3, 3, 8, 16), torch.zeros(16), 3, 1, False, None)
    assert lay1.fwd_taps(16, 16)[0][:9] == [-1, -1, -1, 0, 0, 0, 1, 1, 1]
    assert ops.round8(3) == 8 and ops.round8(74) == 80 and ops.round8(256) == 256


def test_schedules_match_yaml_semantics():
    lib, ops, nets, sch, configs = _pkg()
    cfg = configs.cub_config()
    assert sch.make_var(0, cfg["patch_loss_weight"]) == 1e-4
    assert sch.make_var(0, cfg["prior_mumford_sha_weight"]) == 1e-5
    assert sch.make_linear_var(0, **cfg["kl_weight"]) == 1.0
    assert sch.make_staircase_var(25, 0, 1.0, 10, 0.5) == 0.25
    with pytest.raises(ValueError):
        sch.make_var(0, {"var_type": "cosine", "options": {}})


def test_variable_names_shapes_and_optimizer_groups_match_oracle():
    lib, ops, nets, sch, _ = _pkg()
    from oracle import ref_model as R, configs
    cfg = configs.tiny_config()
    n = nets.Nets(cfg, torch.device("cpu"), seed=0)
    ref = R.init_params(cfg, 0)
    assert list(sorted(n.bank.params)) == list(sorted(ref))
    for name, p in ref.items():
        assert tuple(n.bank.params[name].shape) == tuple(p.shape), name
        assert torch.equal(n.bank.params[name].detach(), p), name          # identical per-name initialisation
    assert list(n.bank.groups) == list(R.SUBMODULES)
    tot = 0
    for key, grp in n.bank.groups.items():
        assert grp["names"] == [v for v in n.bank.params if key in v]
        tot += grp["flat"]["p"].numel()
    assert tot == sum(p.numel() for p in ref.values())
    # full CUB config: 33.1 M trainable parameters
    big = nets.Nets(configs.cub_config(), torch.device("cpu"), seed=0)
    sizes = {k: g["flat"]["p"].numel() for k, g in big.bank.groups.items()}
    assert abs(sizes["encoder_0"] - 13.64e6) < 0.05e6 and abs(sizes["decoder_visualize"] - 5.84e6) < 0.05e6
    assert abs(sum(sizes.values()) - 33.1e6) < 0.2e6


def test_runner_resolves_reference_import_paths():
    _pkg()
    from upsparts_amd import runner
    from upsparts_amd.model import TrainModel, Trainer
    assert runner.get_obj_from_str("nips19.SB_model48i.model.TrainModel") is TrainModel
    assert runner.get_obj_from_str("nips19.SB_model48i.model.Trainer") is Trainer
    assert runner.get_obj_from_str("collections.OrderedDict").__name__ == "OrderedDict"
    b = next(iter(runner.SyntheticPairs({"batch_size": 2, "spatial_size": 8})))
    assert set(b) == {"view0", "view1", "view0_target"} and b["view0"].shape == (2, 8, 8, 3)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import upsparts_amd  # noqa: F401
    from upsparts_amd import dist as D
    w, r, _ = D.init_from_env("gloo")
    assert (w, r) == (world, rank)
    buckets = {"encoder_0": torch.full((1000,), float(rank + 1)), "mi_estimator": torch.arange(10.0) * (rank + 1)}
    handles = [D.allreduce_bucket(g, w) for g in buckets.values()]
    D.wait_all(handles)
    stats = D.average_scalars(torch.tensor([float(rank), 1.0]), w)
    out[rank] = (buckets["encoder_0"][0].item(), buckets["mi_estimator"][3].item(), stats.tolist(), D.shard_seed(4321, rank))
    torch.distributed.destroy_process_group()


def test_data_parallel_helpers_gloo_world2():
    mgr = mp.Manager()
    out = mgr.dict()
    port = _free_port()
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    assert out[0][0] == out[1][0] == 3.0                 # sum of (1, 2); the 1/world factor is applied in the Adam kernel
    assert out[0][1] == out[1][1] == 9.0
    assert out[0][2] == out[1][2] == [0.5, 1.0]
    assert out[0][3] != out[1][3]


def test_csv_pair_datasets(tmp_path):
    """upsparts_amd.data: csv -> pairs by character_id (cub/code/data/data.py:31-50,157-175), [-1,1] float32 NHWC, target copy,
    avoid_identity, static batch size."""
    import numpy as np
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import data
    rng = np.random.RandomState(0)
    rows = ["character_id,relative_file_path_,foo,category"]
    for i in range(7):
        Image.fromarray(rng.randint(0, 255, (20 + i, 24, 3), dtype=np.uint8)).save(str(tmp_path / "im{}.png".format(i)))
        rows.append("{},im{}.png,x,bird".format(i // 3, i))          # characters 0,0,0,1,1,1,2
    (tmp_path / "train.csv").write_text("\n".join(rows) + "\n")
    cfg = {"data_root": str(tmp_path), "data_csv": str(tmp_path / "train.csv"), "data_csv_has_header": True,
           "data_csv_columns": ["character_id", "relative_file_path_", "foo", "category"], "spatial_size": 16,
           "data_avoid_identity": True, "batch_size": 3}
    ds = data.AugmentedPair2(cfg)
    assert len(ds) == 7 and [len(c) for c in ds.labels["choices"]] == [3, 3, 3, 3, 3, 3, 1]
    for i in range(7):
        j = ds.pick_partner(i)
        assert ds.labels["character_id"][j] == ds.labels["character_id"][i] and (j != i or i == 6)
    ex = ds.get_example(1)
    assert set(ex) == {"view0", "view1", "view0_target"} and ex["view0"].shape == (16, 16, 3) and ex["view0"].dtype == np.float32
    assert -1.0 <= ex["view0"].min() and ex["view0"].max() <= 1.0 and np.array_equal(ex["view0"], ex["view0_target"])
    it = data.batches(ds, 3, workers=2, epochs=1)
    bs = list(it)
    assert len(bs) == 2 and bs[0]["view1"].shape == (3, 16, 16, 3) and bs[0]["view1"].dtype == torch.float32
    # evaluation: the ragged last batch is padded to the static size and says how many rows are real
    ev = list(data.batches(ds, 3, shuffle=False, workers=2, epochs=1, pad_last=True))
    assert [b["valid"] for b in ev] == [3, 3, 1] and ev[2]["view0"].shape == (3, 16, 16, 3)
    # pairings are reproducible whatever the decoding threads do: a per-index, per-draw generator
    a = [data.AugmentedPair2(cfg).pick_partner(i) for i in range(7)]
    b = [data.AugmentedPair2(cfg).pick_partner(i) for i in reversed(range(7))][::-1]
    assert a == b
    # ground-truth label maps travel with the examples when the csv names them
    for i in range(7):
        Image.fromarray((np.arange(24 * 24).reshape(24, 24) % 5).astype(np.uint8)).save(str(tmp_path / "gt{}.png".format(i)))
    rows_gt = ["character_id,relative_file_path_,foo,category,gt"] + ["{},im{}.png,x,bird,gt{}.png".format(i // 3, i, i) for i in range(7)]
    (tmp_path / "gt.csv").write_text("\n".join(rows_gt) + "\n")
    dsg = data.AugmentedPair2(dict(cfg, data_csv=str(tmp_path / "gt.csv"), data_gt_segmentation_column="gt",
                                   data_csv_columns=["character_id", "relative_file_path_", "foo", "category", "gt"]))
    ex = dsg.get_example(2)
    assert ex["gt_segmentation"].shape == (16, 16) and ex["gt_segmentation"].dtype == np.int64 and ex["gt_segmentation"].max() <= 4
    pair = data.StochasticPairs(dict(cfg, data_flip_h=True))
    assert set(pair.get_example(0)) == {"view0", "view1"}
    # the augmentation switches of the yaml (data.py:56-57, 166-173): reproducible, in range, and with the reference's sync rules
    aug = dict(cfg, data_augment_shape=True, data_augment_appearance=True, spatial_size=32)
    e1, e2 = data.AugmentedPair2(aug).get_example(1), data.AugmentedPair2(aug).get_example(1)
    for k in ("view0", "view1", "view0_target"):
        assert np.array_equal(e1[k], e2[k]) and e1[k].shape == (32, 32, 3) and e1[k].dtype == np.float32
        assert -1.0 <= e1[k].min() and e1[k].max() <= 1.0
    geo = data.AugmentedPair2(dict(aug, data_augment_appearance=False))
    changed = 0
    for i in range(7):
        for _ in range(3):
            ex = geo.get_example(i)
            # shape-only: view0 and its target went through one geometric realisation of the same image -> identical
            assert np.array_equal(ex["view0"], ex["view0_target"])
            changed += int(not np.allclose(ex["view0"], data.AugmentedPair2(dict(cfg, spatial_size=32)).get_example(i)["view0"], atol=1e-2))
    assert changed > 0


def test_augmentation_pipelines():
    """augment.py, the numpy restatement of cub/code/data/data.py:64-117: every transform alone, and the pipelines' sync rule
    (one realisation for all images of a call)."""
    import numpy as np
    import upsparts_amd  # noqa: F401
    from upsparts_amd import augment as A
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (24, 20, 3)).astype(np.uint8)
    # HSV round trip through the cv2 uint8 convention (H halved): within the quantisation of H (2 degrees)
    back = A.hsv_to_rgb_u8(A.rgb_to_hsv_u8(img)).astype(int)
    assert np.abs(back - img.astype(int)).max() <= 12 and np.abs(back - img.astype(int)).mean() < 2.5
    gray = np.repeat(img[..., :1], 3, -1)
    assert np.array_equal(A.hsv_to_rgb_u8(A.rgb_to_hsv_u8(gray)), gray)            # no hue, no saturation: exact
    assert np.array_equal(A._brightness_contrast(img, 1.0, 0.0), img) and A._brightness_contrast(img, 1.2, 0.2).min() >= 51
    assert np.array_equal(A._rgb_shift(img, [0, 0, 0]), img) and np.array_equal(A._hue_sat_val(gray, 0, 0, 0), gray)
    g = A._to_gray(img)
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])
    const = np.full((24, 20, 3), 77, np.uint8)
    assert np.array_equal(A._box3(const), const) and np.array_equal(A._median3(const), const)
    # geometric transforms keep the shape, replicate the border (a constant image stays constant) and move something
    for make in (A._shift_scale_rotate, A._piecewise_affine, A._elastic):
        op = make(np.random.RandomState(3), 24, 20)
        assert np.array_equal(op(const), const) and op(img).shape == img.shape and not np.array_equal(op(img), img)
    # identity shift/scale/rotate parameters give the identity map
    class Zero(object):
        def uniform(self, a, b, *s):
            return np.zeros(s) if s else 0.0
    assert np.array_equal(A._shift_scale_rotate(Zero(), 24, 20)(img), img)
    # one realisation per call: two copies of an image stay equal through either pipeline, over many draws; some draws change it
    f = img.astype(np.float32) / 127.5 - 1.0
    moved = 0
    for seed in range(40):
        r = np.random.RandomState(seed)
        a, b = A.stochastic_appearance_augmentation(r, f, f.copy())
        c, d = A.stochastic_shape_augmentation(r, f, f.copy())
        assert np.array_equal(a, b) and np.array_equal(c, d) and a.dtype == np.float32 and c.shape == f.shape
        assert -1.0 <= min(a.min(), c.min()) and max(a.max(), c.max()) <= 1.0
        moved += int(not np.allclose(a, f, atol=1e-2)) + int(not np.allclose(c, f, atol=1e-2))
    assert 20 < moved < 80                       # p = 0.9 x the inner probabilities: most draws do something, not all


def test_part_iou_evaluation(tmp_path):
    """evalutil: best-IoU remapping of inferred part ids to ground-truth labels + per-label IoU (eval_01.py:229-383 protocol)."""
    import numpy as np
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil as E
    gt = np.zeros((2, 8, 8), dtype=np.int64)
    gt[:, :4, :4] = 1; gt[:, 4:, 4:] = 2                      # background 0, head 1, tail 2
    pred = np.full((2, 8, 8), 7, dtype=np.int64)              # part 7 ~ background
    pred[:, :4, :4] = 3; pred[:, 4:, 4:] = 5; pred[0, 4, 4] = 3  # parts 3 -> head, 5 -> tail (one pixel wrong)
    r = E.evaluate_parts(pred, gt)
    assert r["mapping"] == {3: 1, 5: 2, 7: 0}
    # pooled over the set (one IoU per label over all pixels)
    assert abs(r["pooled"][1] - 32 / 33) < 1e-12 and abs(r["pooled"][2] - 31 / 32) < 1e-12 and r["pooled"][0] == 1.0
    # eval_01.py protocol: IoU per image, then the mean over the images (image 0 has the wrong pixel, image 1 is perfect)
    assert abs(r["per_image"][0][1] - 16 / 17) < 1e-12 and r["per_image"][1][1] == 1.0
    assert abs(r["iou"][1] - 0.5 * (16 / 17 + 1.0)) < 1e-12 and abs(r["iou"][2] - 0.5 * (15 / 16 + 1.0)) < 1e-12
    assert abs(r["overall"] - 0.5 * (r["iou"][1] + r["iou"][2])) < 1e-12
    same = E.evaluate_parts(gt, gt)
    assert same["overall"] == 1.0
    # the files of eval_01.py:355-383
    import pandas as pd
    df, df_mean = E.write_eval_tables(r, str(tmp_path), 71000, {0: "background", 1: "head", 2: "tail"})
    back = pd.read_csv(str(tmp_path / "part_ious.csv"))
    assert list(back.columns) == ["global_step", "batch_idx", "background", "head", "tail"] and len(back) == 2
    assert abs(back["head"][0] - 16 / 17) < 1e-12 and back["global_step"][1] == 71000 and back["batch_idx"][1] == 1
    table = (tmp_path / "mean_part_ios.csv").read_text()
    assert table.startswith("+") and "overall" in table and "{:.6f}".format(r["overall"])[:7] in table
    assert "3: 1" in (tmp_path / "best_remapping.yml").read_text()
    # a label missing from one image's ground truth is written as -1 and left out of the mean (eval_01.py:299, 373)
    gt2 = gt.copy(); gt2[1][gt2[1] == 2] = 0
    r2 = E.evaluate_parts(pred, gt2)
    df2, m2 = E.write_eval_tables(r2, str(tmp_path / "b"), 1, {0: "background", 1: "head", 2: "tail"})
    assert df2["tail"][1] == -1.0 and abs(float(m2["tail"][0]) - df2["tail"][0]) < 1e-12


_RANK_STANDIN = '''
import json, os, sys
import torch
import torch.distributed as dist
world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
assert os.environ["LOCAL_RANK"] == os.environ["RANK"] and os.environ["MASTER_ADDR"] == "127.0.0.1"
assert os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY") == "0", "ranks must run with dmabuf IPC (RCCL on this pool's host driver)"
if os.environ.get("UPS_TEST_DIE_EARLY") == "1" and rank == 1:
    sys.exit(9)           # dies before the rendezvous: rank 0 would sit in init_process_group until its timeout
dist.init_process_group("gloo", init_method="env://", world_size=world, rank=rank)
t = torch.tensor([float(rank + 1)])
dist.all_reduce(t)
dist.barrier()
if "--fail" in sys.argv and rank == 1:
    sys.exit(7)
if rank == 0:
    print("some warm-up chatter")
    print(json.dumps({"metric": "stand-in", "n_gpus": dist.get_world_size(), "sum": float(t), "argv": sys.argv[1:]}))
dist.destroy_process_group()
'''


def test_bench_launcher_spawns_n_ranks(tmp_path):
    """`python bench.py --gpus N` (no WORLD_SIZE in the environment): the parent never touches a GPU, starts N rank processes
    with the torch.distributed.run environment contract, relays rank 0's JSON line, fails when a rank fails."""
    import json
    import subprocess
    import sys
    entry = tmp_path / "rank.py"
    entry.write_text(_RANK_STANDIN)
    # (HSA_ENABLE_IPC_MODE_LEGACY is dropped from the launcher's own environment: it must reach the ranks regardless)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--rank-entry", str(entry)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines                                     # ONE JSON line on stdout, chatter goes to stderr
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["sum"] == 3.0 and "--steps" in out["argv"]
    bad = subprocess.run(cmd + ["--fail"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert bad.returncode != 0 and not bad.stdout.decode().strip()
    # a rank that dies before the rendezvous: the launcher takes its siblings down and reports, instead of hanging with them
    import time
    t0 = time.time()
    dead = subprocess.run(cmd, env=dict(env, UPS_TEST_DIE_EARLY="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert dead.returncode == 9 and not dead.stdout.decode().strip() and time.time() - t0 < 120, dead.stderr.decode()[-500:]


def test_read_vgg_weights_key_spellings(tmp_path):
    import numpy as np
    import upsparts_amd  # noqa: F401
    from upsparts_amd import nets
    k = np.ones((3, 3, 3, 8), np.float32)
    np.savez(str(tmp_path / "a.npz"), **{"block1_conv1/kernel:0": k, "block1_conv1/bias:0": np.zeros(8, np.float32),
                                         "block2_conv1_W": k, "block2_conv1_b": np.zeros(8, np.float32),
                                         "vgg19/block3_conv4/V": k, "vgg19/block3_conv4/b": np.zeros(8, np.float32)})
    st = nets.read_vgg_weights(str(tmp_path / "a.npz"))
    assert sorted(st) == ["vgg19/block1_conv1/V", "vgg19/block1_conv1/b", "vgg19/block2_conv1/V", "vgg19/block2_conv1/b",
                          "vgg19/block3_conv4/V", "vgg19/block3_conv4/b"]
    assert st["vgg19/block1_conv1/V"].shape == (3, 3, 3, 8) and st["vgg19/block1_conv1/V"].dtype == torch.float32


def _integration_stub():
    """The python block of INTEGRATION.md section 2, with the library path made absolute."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text.split("```python\n", 1)[1].split("```", 1)[0]
    return block.replace('"unsupervised-part-segmentation_amd/csrc/libupsparts_hip.so"',
                         repr(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "libupsparts_hip.so")))


def test_integration_stub_matches_the_header():
    """The binder stub a maintainer would copy out of INTEGRATION.md declares the FULL ups_conv_desc: same fields, order
    and size as the header (and as the product's own ctypes mirror)."""
    import ctypes as C
    lib, *_ = _pkg()
    ns = {}
    exec(_integration_stub(), ns)
    stub = ns["ups_conv_desc"]
    assert [f[0] for f in stub._fields_] == [f[0].rstrip("_") for f in lib.ConvDesc._fields_]
    assert C.sizeof(stub) == C.sizeof(lib.ConvDesc)
    for (n0, t0), (n1, t1) in zip(stub._fields_, lib.ConvDesc._fields_):
        assert C.sizeof(t0) == C.sizeof(t1) and getattr(stub, n0).offset == getattr(lib.ConvDesc, n1).offset, n0
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    body = hdr.split("typedef struct {", 1)[1].split("} ups_conv_desc;", 1)[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            for part in decl.split(","):
                names.append(re.sub(r"\[\d+\]", "", part.strip().split()[-1].lstrip("*")))
    assert names == [f[0] for f in stub._fields_], (names, [f[0] for f in stub._fields_])


def test_tf_checkpoint_bundle_reader_and_writer(tmp_path):
    """tfckpt: the tensor-bundle (V2) format of TF-1.x checkpoints -- LevelDB-format index table with prefix-compressed keys
    over several blocks, BundleEntryProto values, raw little-endian data shard -- round trip and byte-level structure."""
    import struct
    import numpy as np
    import upsparts_amd  # noqa: F401
    from upsparts_amd import tfckpt
    rng = np.random.RandomState(0)
    tensors = {"encoder_0/conv2d_{}/V".format(i): rng.randn(3, 3, 5 + i, 8).astype(np.float32) for i in range(40)}
    tensors.update({"encoder_0/conv2d_{}/b".format(i): rng.randn(8).astype(np.float32) for i in range(40)})
    tensors["encoder_0/conv2d_0/V/Adam"] = rng.randn(3, 3, 5, 8).astype(np.float32)
    tensors["global_step"] = np.asarray(60000, dtype=np.int64)
    tensors["some/int32"] = np.arange(6, dtype=np.int32).reshape(2, 3)
    prefix = str(tmp_path / "model.ckpt-60000")
    tfckpt.write_bundle(prefix, tensors, block_bytes=512)                 # many data blocks
    assert tfckpt.is_bundle(prefix) and not tfckpt.is_bundle(str(tmp_path / "nope"))
    raw = open(prefix + ".index", "rb").read()
    assert struct.unpack("<Q", raw[-8:])[0] == 0xDB4775248B80FB57          # table magic (leveldb kTableMagicNumber)
    header, entries = tfckpt.read_index(prefix + ".index")
    assert header["num_shards"] == 1 and set(entries) == set(tensors)
    e = entries["encoder_0/conv2d_3/V"]
    assert e["dtype"] == 1 and e["shape"] == [3, 3, 8, 8] and e["size"] == 3 * 3 * 8 * 8 * 4
    back = tfckpt.read_bundle(prefix)
    for k, v in tensors.items():
        assert back[k].dtype == v.dtype and back[k].shape == v.shape and np.array_equal(back[k], v), k
    some = tfckpt.read_bundle(prefix, names=["global_step", "encoder_0/conv2d_7/b"])
    assert set(some) == {"global_step", "encoder_0/conv2d_7/b"} and int(some["global_step"]) == 60000
    # known-answer checks of the pieces TF verifies: CRC-32C (Castagnoli) and its LevelDB masking
    assert tfckpt.crc32c(b"123456789") == 0xE3069283
    assert tfckpt._mask(tfckpt.crc32c(b"123456789")) == ((0xE3069283 >> 15 | 0xE3069283 << 17) + 0xA282EAD8) & 0xFFFFFFFF
    params, m, v, other = tfckpt.to_trainer_state(back)
    assert "encoder_0/conv2d_0/V" in params and "encoder_0/conv2d_0/V" in m and "global_step" in other
    with pytest.raises(ValueError):
        (tmp_path / "stub.index").write_bytes(b"version https://git-lfs.github.com/spec/v1\n" * 3)
        tfckpt.read_index(str(tmp_path / "stub.index"))


def test_stream_plan_aliases_and_tools_offline(tmp_path):
    """Host logic of round 5 that needs no GPU: the compact stream plan folds the logical streams onto three (ops.Streams.alias);
    `tools/pin_log.py table` renders a dump without a device; `tools/asm_loops.py` splits a listing into loops."""
    import json
    import subprocess
    import sys
    import upsparts_amd  # noqa: F401
    from upsparts_amd import ops
    try:
        ops.Streams.set_plan("compact")
        assert {ops.Streams.alias.get(n, n) for n in ("pre", "aux", "aux1", "aux2", "wgrad", "wgrad2")} == {"aux", "wgrad"}
        ops.Streams.set_plan("full")
        assert not ops.Streams.alias
        with pytest.raises(ValueError):
            ops.Streams.set_plan("seven")
    finally:
        ops.Streams.set_plan("full")
    # a two-case dump in the format tools/pin_log.py global appends to
    steps = (0, 1, 3, 7, 15, 31, 63, 127)
    keys = ("lor", "loa", "avg_loss_dis0", "avg_loss_dis1", "bottleneck_loss", "mask0_kl", "prior_gmrf", "variance_loss", "patch_loss",
            "weakly_superv_loss_p", "loss_mi0_discriminator", "loss_decoder_delta")
    dump = tmp_path / "dump.jsonl"
    with open(dump, "w") as f:
        for case in ("edflow plain", "tf plain"):
            runs = [{str(s): {k: 1.0 + 0.01 * i for i, k in enumerate(keys)} for s in steps} for _ in range(2)]
            f.write(json.dumps({"case": case, "runs": runs}) + "\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pin_log.py"), "table", str(dump)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, r.stderr.decode()[-800:]
    assert "== mask0_kl" in out and "== verdict" in out and "edflow plain" in out and "tf plain" in out
    listing = tmp_path / "k.s"
    listing.write_text("_ZN4testEv: ; @test\n\ts_mov_b32 s0, 0\n.LBB0_1:\n\tv_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]\n"
                       "\tds_read_b128 v[4:7], v12\n\tv_add_u32_e32 v12, 64, v12\n\ts_add_i32 s0, s0, 1\n\ts_cmp_lt_i32 s0, 8\n"
                       "\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_loops.py"), str(listing), "test", "1"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0 and "loop .LBB0_1" in out and "'mfma': 1" in out and "'ds_read': 1" in out, out + r.stderr.decode()


REF = "/root/reference"
REF_YAMLS = [
    # yaml, configs function, trainable parameters (M) of nets.Nets at the yaml's own settings
    ("cub/code/SB_model48i/train_cub_subset_tps.yaml", "cub_config", 33.13),
    ("pennaction/code/SB_model48i/train_pennaction.yaml", "pennaction_config", 33.18),
    ("deepfashion/code/SB_model48c/train_deepfashion.yaml", "deepfashion_config", 50.08),
]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine (the GPU box gets /root/repo only)")
@pytest.mark.parametrize("rel,fn,mparams", REF_YAMLS, ids=[r[1] for r in REF_YAMLS])
def test_reference_yaml_files_drop_in_unchanged(rel, fn, mparams):
    """north_star: "keeping the edflow Iterator/Trainer and config.yaml surface so cub/deepfashion/pennaction configs drop in
    unchanged" (round-5 verdict, missing 5).  The three yaml files the reference ships are loaded through runner.load_config as
    they lie: `model:` / `iterator:` resolve to this package's classes, `dataset:` to a class of data.py, every model / trainer key
    equals what configs.<fn>() builds for the same (n_parts, batch_size, spatial_size) -- the configs the tests and the bench run on --
    and nets.Nets builds the parameter count of the reference's graph."""
    from upsparts_amd import configs, nets, runner
    from upsparts_amd.model import TrainModel, Trainer
    cfg = runner.load_config([os.path.join(REF, rel)])
    assert runner.get_obj_from_str(cfg["model"]) is TrainModel and runner.get_obj_from_str(cfg["iterator"]) is Trainer
    assert cfg["dataset"] in runner.DATA_ALIASES, cfg["dataset"]
    kw = dict(n_parts=cfg["n_parts"], batch_size=cfg["batch_size"], spatial_size=cfg["spatial_size"])
    if fn == "cub_config":
        kw["use_tps"] = bool(cfg.get("use_tps", False))
    ours = getattr(configs, fn)(**kw)
    data_keys = lambda k: k == "dataset" or k.startswith("data_")
    for k in sorted(set(cfg) | set(ours)):
        if data_keys(k):
            continue            # (where the images are: the yaml's business; data.py reads exactly these keys, test_data_* below)
        if k == "d_single" and fn != "deepfashion_config":
            assert k in cfg and k not in ours      # the 48i yamls carry the key, the 48i model never reads it (M:313-521)
            continue
        assert k in cfg and k in ours, "key {} is in {} only".format(k, "the yaml" if k in cfg else "configs." + fn)
        assert cfg[k] == ours[k], "key {}: yaml {!r}, configs.{} {!r}".format(k, cfg[k], fn, ours[k])
    n = nets.Nets(cfg, torch.device("cpu"), seed=0)
    total = sum(int(p.numel()) for p in n.bank.params.values())
    assert abs(total / 1e6 - mparams) < 0.01, "{}: {:.3f} M parameters, expected {:.2f} M".format(rel, total / 1e6, mparams)


def test_runner_does_not_train_on_noise_silently(tmp_path, monkeypatch, caplog):
    """runner.py used to swallow EVERY exception of the dataset constructor and train on U(-1, 1) noise without a word (round-5
    verdict, weak 10).  Now: only a missing file / missing package falls back, the fallback says SYNTHETIC DATA at WARNING level when
    it happens and with every logged step, anything else (a wrong key, a bug in data.py) propagates."""
    from upsparts_amd import runner
    cfg = {"dataset": "src.data.data.AugmentedPair2", "data_root": str(tmp_path / "nowhere"), "data_csv": str(tmp_path / "nowhere" / "x.csv"),
           "batch_size": 2, "spatial_size": 16}
    import logging
    with caplog.at_level(logging.WARNING, logger="upsparts"):
        ds, why = runner.make_dataset(cfg, rank=0, strict=False)
    assert isinstance(ds, runner.SyntheticPairs) and why and "SYNTHETIC DATA" in caplog.text
    with pytest.raises((FileNotFoundError, OSError)):
        runner.make_dataset(cfg, rank=0, strict=True)

    class Boom(object):
        def __init__(self, config):
            raise KeyError("a bug, not a missing file")
    monkeypatch.setitem(runner.DATA_ALIASES, "src.data.data.AugmentedPair2", Boom)
    with pytest.raises(KeyError):
        runner.make_dataset(cfg, rank=0, strict=False)


def test_every_switch_is_documented():
    """switches.py is the one table of the UPS_* environment switches (round-5 verdict, weak 11): every environment read in the package
    and every read through the csrc/env.h helpers names a switch of that table, the package reads its switches through switches.flag /
    value only, the library through env.h only (a raw getenv anywhere else in csrc/ fails), and the table (COMPILE_TIME included) names
    nothing that no longer exists."""
    import re
    from upsparts_amd import switches as SW
    pkg = os.path.join(ROOT, "unsupervised-part-segmentation_amd")
    used = set()
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py") and fn != "switches.py":
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"environ[^\n]*UPS_", src), fn + " reads a UPS_ switch from os.environ directly: use switches.flag / value"
            used |= set(re.findall(r"SW\.(?:flag|value)\(\"(UPS_[A-Z0-9_]+)\"\)", src))
    csrc = os.path.join(pkg, "csrc")
    compiled = set()
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".h")):
            src = open(os.path.join(csrc, fn)).read()
            used |= set(re.findall(r"(?:ups_env_(?:on|off|int|raw)_now|UPS_ENV_(?:ON|OFF|INT|RAW)_CACHED)\(\"(UPS_[A-Z0-9_]+)\"", src))
            assert not re.search(r"getenv\(\"UPS_", src) and (fn == "env.h" or "getenv(" not in src), \
                fn + " reads the environment directly: use the env.h helpers"
            for m in re.findall(r"(?:ifn?def|defined\()\s*(UPS_[A-Z0-9_]+)", src):
                assert m in SW.COMPILE_TIME or m.endswith("_H"), "compile-time form {} of {} is not listed in switches.COMPILE_TIME".format(m, fn)
                compiled.add(m)
    assert not sorted(set(SW.COMPILE_TIME) - compiled), "switches.COMPILE_TIME names forms no source tests: {}".format(sorted(set(SW.COMPILE_TIME) - compiled))
    missing = sorted(used - set(SW.SWITCHES))
    stale = sorted(set(SW.SWITCHES) - used)
    assert not missing, "undocumented switches: {}".format(missing)
    assert not stale, "switches.py documents switches nobody reads: {}".format(stale)
    for name, (default, kind, where, what) in SW.SWITCHES.items():
        assert kind in ("product", "ab", "test", "debug") and what
    assert SW.report().startswith("UPS switches: ")


_ENV_H_PROGRAM = r"""
#include "env.h"
#include <stdio.h>
#include <string.h>
static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static void put(const char* v) { if (v) setenv("UPS_T", v, 1); else unsetenv("UPS_T"); }
// one call site each: what a launcher's cached read is
static bool on_cached() { return UPS_ENV_ON_CACHED("UPS_T"); }
static bool off_cached() { return UPS_ENV_OFF_CACHED("UPS_T"); }
static long long int_cached() { return UPS_ENV_INT_CACHED("UPS_T", 512); }
static const char* raw_cached() { return UPS_ENV_RAW_CACHED("UPS_T"); }
int main() {
    const struct { const char* v; bool on, off; long long i; } rows[] = {
        {nullptr, true, false, 512}, {"", true, false, 0}, {"0", false, false, 0},
        {"1", true, true, 1},        {"force", true, false, 0}, {"64", true, false, 64}};
    for (const auto& r : rows) {
        put(r.v);
        CHECK(ups_env_on_now("UPS_T") == r.on);
        CHECK(ups_env_off_now("UPS_T") == r.off);
        CHECK(ups_env_int_now("UPS_T", 512) == r.i);
        const char* raw = ups_env_raw_now("UPS_T");
        CHECK(r.v ? (raw && !strcmp(raw, r.v)) : raw == nullptr);
    }
    put("0");
    CHECK(!on_cached() && !off_cached() && int_cached() == 0 && !strcmp(raw_cached(), "0"));
    put("1");       // a cached site keeps its first reading, a read-now sees the new value
    CHECK(!on_cached() && !off_cached() && int_cached() == 0);
    CHECK(ups_env_on_now("UPS_T") && ups_env_off_now("UPS_T") && ups_env_int_now("UPS_T", 512) == 1 && !strcmp(ups_env_raw_now("UPS_T"), "1"));
    CHECK(UPS_ENV_ON_CACHED("UPS_T") && UPS_ENV_OFF_CACHED("UPS_T"));       // (another call site: its own first reading)
    put(nullptr);
    CHECK(!on_cached() && raw_cached() != nullptr && ups_env_on_now("UPS_T") && ups_env_raw_now("UPS_T") == nullptr);
    printf(fails ? "FAILED\n" : "env.h ok\n");
    return fails ? 1 : 0;
}
"""


def test_env_h_parse_rules_and_flavours(tmp_path):
    """csrc/env.h alone, in a stand-alone host program built with the address and undefined-behaviour sanitizers: the four parse rules
    (default-on, default-off, integer with a default, raw string) over unset / "" / "0" / "1" / "force" / "64", and the two flavours --
    a cached read does not see a later setenv, a read-now does."""
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc")
    src = tmp_path / "env_h_test.cpp"
    src.write_text(_ENV_H_PROGRAM)
    exe = str(tmp_path / "env_h_test")
    # the sanitizer runtimes linked statically (clang's default), so that the program runs whatever else the loader brings in
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "llvm", "bin", "clang++")
    compilers = [(c, f) for c, f in ((rocm_clang, []), (shutil.which("clang++"), []), (shutil.which("c++"), ["-static-libasan", "-static-libubsan"]))
                 if c and os.path.exists(c)]
    assert compilers, "no host C++ compiler"
    for cxx, static in compilers:       # (the first one whose sanitizer runtimes are installed)
        built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                               + static + ["-I", csrc, str(src), "-o", exe], capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "env.h ok" in run.stdout, run.stdout + run.stderr
