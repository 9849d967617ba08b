"""``edflow -t <yaml>`` work-alike for the hot path (edflow itself is an un-vendored dependency of the
reference: requirements.txt:33).  Keeps the surface the shipped configs rely on:

  * ``model:`` / ``iterator:`` are import paths (train_cub_subset_tps.yaml:1-2); the reference's package names
    ``nips19.*`` / ``src.*`` resolve to this package's TrainModel / Trainer, any other path is imported as is;
  * ``Model(config)`` then ``Iterator(config, root, model)``, ``iterator.initialize(checkpoint)``,
    ``iterator.iterate(batches)`` (cub/train/log.txt:1-9, 201-203);
  * ``[INFO] [LoggingHook]: name: value`` lines at steps 0, 2, 4, 8, ..., then every ``log_freq`` (keys alphabetical, as cub/train/log.txt:204-279); checkpoints every
    ``ckpt_freq`` under ``<root>/train/checkpoints/model.ckpt-<step>``.

Data: ``dataset: src.data.data.AugmentedPair2`` / ``eddata.stochastic_pair.StochasticPairs`` resolve to the csv pair
datasets of ``data.py``; when the csv / images are NOT THERE (FileNotFoundError / ImportError, nothing else) the runner falls back
to ``SyntheticPairs`` (U(-1,1) views), says SYNTHETIC DATA at WARNING level and with every logged step, unless ``--strict-dataset``
is given (then it raises).

``--transfer <yaml> -c <ckpt> [--parts 0,3,..]`` is the work-alike of final_eval/eval_transfer.py: one ``TrainModel.transfer_matrix``
call per block of ``data.TransferData``, the cells pickled to <root>/comparison_matrix/<global_step:06>/data.p with the reference
MatrixHook's key set (its plotting script reads the file) and drawn by ``evalutil.write_transfer_matrix``.

``--segment <yaml> -c <ckpt>`` has no counterpart in the reference: the images listed in ``segment_csv`` are segmented and their part
maps written as PNG files at the resolution of the source photographs, and on request as one COCO annotation file with run-length
masks encoded on the device (``segment``).

``--index <yaml> -c <ckpt>`` is the work-alike of deepfashion/code/eval/eval_02's ``make_clusters`` and more: the part-appearance codes of
the images in ``index_csv``, their per-part nearest neighbours and k-means clusters (``index``; ``partindex.py``).

``--landmarks <yaml> -c <ckpt>`` has no counterpart in the reference either: landmark regression, the score the part-discovery papers
report on CUB and PennAction -- a linear map from the part centres to the keypoints of ``landmark_fit_csv``, its mean error and PCK on
``landmark_test_csv`` (``landmarks``; ``landmarks.py``).
"""
import argparse
import importlib
import logging
import os
import time
from collections import OrderedDict

import torch
import yaml

from .model import TrainModel, Trainer

from . import data as _data
from . import dist as D
from . import switches as SW

LOG = logging.getLogger("upsparts")
ALIASES = {"TrainModel": TrainModel, "Trainer": Trainer}
DATA_ALIASES = {"src.data.data.AugmentedPair2": _data.AugmentedPair2, "nips19.data.data.AugmentedPair2": _data.AugmentedPair2,
                "eddata.stochastic_pair.StochasticPairs": _data.StochasticPairs}


def get_obj_from_str(path):
    mod, name = path.rsplit(".", 1)
    if mod.split(".")[0] in ("nips19", "src") and name in ALIASES:
        return ALIASES[name]
    return getattr(importlib.import_module(mod), name)


def dist_setup():
    """One process per GPU under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*): pick this rank's device
    BEFORE anything touches the GPU, then join the RCCL group.  Returns (world_size, rank, local_rank)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    world, rank, local = D.init_from_env(SW.value("UPS_DIST_BACKEND"))
    return world, rank, local


class SyntheticPairs(object):
    """{"view0","view1","view0_target"} of NHWC float32 in [-1,1] (cub/code/data/data.py:157-175 contract)."""

    def __init__(self, config, seed=1234):
        self.config = config
        self.gen = torch.Generator().manual_seed(seed)

    def __iter__(self):
        B, S = self.config["batch_size"], self.config["spatial_size"]
        while True:
            yield {k: torch.rand(B, S, S, 3, generator=self.gen) * 2 - 1 for k in ("view0", "view1", "view0_target")}


def make_dataset(cfg, rank=0, strict=False, device=None):
    """The yaml's `dataset:` class on this rank's shard seed.  Returns (dataset, None), or (SyntheticPairs, reason) when the data is
    NOT THERE -- the csv / image root does not exist or the dataset's package cannot be imported -- and `strict` is off; that fallback
    is logged at WARNING level here and again with every logged step (main).  Any other exception is a bug and propagates: a run with
    a wrong key must not quietly train on noise (round-5 verdict).
    `data_on_device: True`: the csv pair datasets are fed by `data.device_batches` from a uint8 store on `device` (default: the
    current HIP device) -- same seeds, same batches; every rank holds its own copy of the store.  With `data_augment_on_device: True`
    that path also runs AugmentedPair2's `data_augment_appearance` / `data_augment_shape` (the key alone is a ValueError)."""
    try:
        cls = DATA_ALIASES.get(cfg["dataset"]) or get_obj_from_str(cfg["dataset"])
        ds = cls(dict(cfg, data_seed=D.shard_seed(cfg.get("data_seed", 1), rank)))
        _data.check_augment_on_device(cfg)
        if cfg.get("data_on_device", False):
            if not isinstance(ds, _data.StochasticPairs):
                raise ValueError("data_on_device: {} is not one of the csv pair datasets of data.py".format(cfg["dataset"]))
            dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
            return _data.device_batches(ds, cfg["batch_size"], dev, seed=D.shard_seed(0, rank)), None
        return (_data.batches(ds, cfg["batch_size"], seed=D.shard_seed(0, rank)) if isinstance(ds, _data.StochasticPairs) else ds), None
    except (FileNotFoundError, NotADirectoryError, ImportError) as e:
        if strict:
            raise
        why = "{}: {}".format(type(e).__name__, e)
        LOG.warning("SYNTHETIC DATA: dataset %s is not available (%s); training on U(-1, 1) noise views. "
                    "Pass --strict-dataset to make this an error.", cfg.get("dataset"), why)
        return SyntheticPairs(cfg, seed=D.shard_seed(1234, rank)), why


def load_config(paths):
    cfg = {}
    for p in paths:
        with open(p) as f:
            cfg.update(yaml.safe_load(f))
    return cfg


def main(argv=None):
    ap = argparse.ArgumentParser(prog="upsparts-run")
    ap.add_argument("-t", "--train", nargs="+", default=None,
                    help="training yaml(s); --set log_images=true also writes the image logs, train/<name>_<step:07>.png")
    ap.add_argument("-e", "--eval", nargs="+", default=None,
                    help="evaluation yaml(s): test-mode forward over the dataset, outputs pickled (edflow -e work-alike)")
    ap.add_argument("--transfer", nargs="+", default=None,
                    help="transfer yaml(s): pose i x appearance j comparison matrices (final_eval/eval_transfer.py work-alike)")
    ap.add_argument("--segment", nargs="+", default=None,
                    help="segmentation yaml(s): label maps / overlays / confidence maps of the images in segment_csv, as PNG files "
                         "at source resolution under <root>/segment/<global_step>/")
    ap.add_argument("--index", nargs="+", default=None,
                    help="index yaml(s): the part-appearance codes of the images in index_csv, their per-part nearest neighbours and "
                         "k-means clusters under <root>/index/<global_step>/")
    ap.add_argument("--landmarks", nargs="+", default=None,
                    help="landmark yaml(s): a per-keypoint linear map from the part centres to the keypoints of landmark_fit_csv, its "
                         "mean error and PCK on landmark_test_csv under <root>/landmarks/<global_step>/")
    ap.add_argument("--parts", default=None, help="--transfer: comma-separated part ids taken from the column image (default: all)")
    ap.add_argument("--eval-batches", type=int, default=None, help="number of batches to evaluate (default: one epoch)")
    ap.add_argument("-c", "--checkpoint", default=None,
                    help="checkpoint to restore; with `use_ema: true` in the yaml (or --set use_ema=true) its weight-EMA shadows become "
                         "the weights of -e / --transfer / --segment / --index / --landmarks")
    ap.add_argument("-p", "--project", default=None, help="log root (default logs/<timestamp>)")
    ap.add_argument("--num_steps", type=int, default=None)
    ap.add_argument("--set", nargs="*", default=[], help="key=value overrides (yaml-parsed)")
    ap.add_argument("--strict-dataset", action="store_true")
    args = ap.parse_args(argv)
    if ((args.train is not None) + (args.eval is not None) + (args.transfer is not None) + (args.segment is not None)
            + (args.index is not None) + (args.landmarks is not None) != 1):
        ap.error("exactly one of -t / -e / --transfer / --segment / --index / --landmarks is required")
    if args.landmarks is not None:
        return landmarks(args)
    if args.index is not None:
        return index(args)
    if args.segment is not None:
        return segment(args)
    if args.transfer is not None:
        return transfer(args)
    if args.eval is not None:
        return evaluate(args)
    cfg = load_config(args.train)
    for kv in args.set:
        k, v = kv.split("=", 1)
        cfg[k] = yaml.safe_load(v)
    world, rank, local = dist_setup()
    root = args.project or os.path.join("logs", time.strftime("%Y-%m-%dT%H-%M-%S") + "_" + os.path.basename(args.train[0]).split(".")[0])
    if rank == 0:
        os.makedirs(os.path.join(root, "train"), exist_ok=True)
    Model, Iterator = get_obj_from_str(cfg["model"]), get_obj_from_str(cfg["iterator"])
    # data parallel: `batch_size` is the per-GPU batch (the graph is static in it, model.py:320); every rank draws its own
    # shard order / partners / noise from rank-offset seeds, the weights come from the same seed on every rank
    dataset, synthetic_why = make_dataset(cfg, rank, args.strict_dataset,
                                          device=torch.device("cuda", local) if torch.cuda.is_available() else None)
    model = Model(cfg) if Model is not TrainModel else Model(cfg, device=torch.device("cuda", local))
    kw = {"world_size": world, "rank": rank} if Iterator is Trainer else {}
    it = Iterator(cfg, root, model, **kw)
    it.initialize(args.checkpoint)
    if rank != 0:           # logs and checkpoints are written by rank 0 only
        it.iterate(iter(dataset), num_steps=args.num_steps, log_fn=lambda line: None)
        return it
    log_path = os.path.join(root, "train", "log.txt")
    with open(log_path, "a") as lf:
        def log_fn(line):
            if synthetic_why and "global_step" in line:       # once per logged step: nobody reads a loss curve of noise by mistake
                warn = "[WARNING] [runner]: SYNTHETIC DATA (dataset {} not available: {})".format(cfg.get("dataset"), synthetic_why)
                print(warn)
                lf.write(warn + "\n")
            print(line)
            lf.write(line + "\n")
        it.iterate(iter(dataset), num_steps=args.num_steps, log_fn=log_fn)
    return it


def evaluate(args):
    """``edflow -e eval.yaml -c ckpt`` (cub/code/eval/eval_iclr_01/infer.py:216-224, eval_01.py:152-190): the test-mode graph
    (no sampling noise) is run over the dataset, ``model.outputs[k]`` for k in ``fetch_output_keys`` is collected and
    ``{"inputs", "outputs"}`` is pickled to <root>/eval/<global_step>/model_outputs.p; with ground-truth label maps in the
    batches (key ``gt_segmentation``) the part-IoU protocol of eval_01.py:229-383 is reported too (evalutil.py).
    ``eval_metrics: [reconstruction, parts]`` (default none) also writes metrics.yml: the label-free metrics of the trainer's
    `val_metrics` (evalutil.ReconstructionEvaluator / PartUsageEvaluator) from the same forward passes, without the perceptual term;
    ``equivariance`` adds evalutil.EquivarianceEvaluator's numbers on each batch's view0 (one more pose-path pass per batch);
    ``coherence`` adds evalutil.CoherenceEvaluator's (the connected components of out_parts_hard, from the same forward passes)."""
    import pickle
    import numpy as np
    from . import evalutil
    cfg = load_config(args.eval)
    for kv in args.set:
        k, v = kv.split("=", 1)
        cfg[k] = yaml.safe_load(v)
    cfg["test_mode"] = True
    dist_setup()            # evaluation is single-process; this only selects LOCAL_RANK's device when launched under a launcher
    root = args.project or os.path.join("logs", time.strftime("%Y-%m-%dT%H-%M-%S") + "_eval")
    Model, Iterator = get_obj_from_str(cfg["model"]), get_obj_from_str(cfg["iterator"])
    try:
        cls = DATA_ALIASES.get(cfg["dataset"]) or get_obj_from_str(cfg["dataset"])
        ds = cls(cfg)
        batches_it = (_data.batches(ds, cfg["batch_size"], shuffle=False, epochs=1, pad_last=True)
                      if isinstance(ds, _data.StochasticPairs) else iter(ds))
    except Exception:
        if args.strict_dataset:
            raise
        batches_it = iter(SyntheticPairs(cfg))
        args.eval_batches = args.eval_batches or 1
    model = Model(cfg)
    it = Iterator(cfg, root, model)
    it.initialize(args.checkpoint)
    if cfg.get("eval_on_device", False):
        if cfg.get("eval_metrics"):
            raise ValueError("eval_metrics needs the host route of -e (its forward passes): it cannot be combined with eval_on_device")
        res = evaluate_on_device(model, batches_it, cfg, args.eval_batches)
        odir = os.path.join(root, "eval", str(it.global_step))
        os.makedirs(odir, exist_ok=True)
        write_iou_files(res, odir, cfg, it.global_step)
        print("[INFO] evaluation tables written to", odir)
        return res
    keys = cfg.get("fetch_output_keys", ["out_parts_hard", "out_parts_soft", "generated", "m0_sample"])
    outs, ins, gts = {k: [] for k in keys}, {"view0": [], "view1": []}, []
    # `eval_metrics: [reconstruction, parts]` (default none): the label-free metrics of `val_metrics` from the same forward passes
    from .model import validation_metrics
    metrics = validation_metrics(cfg, "eval_metrics", ())
    if "iou" in metrics:
        raise ValueError("eval_metrics: the part IoU is what -e writes whenever the batches carry label maps; list reconstruction | parts "
                         "| equivariance | coherence")
    if "reconstruction" in metrics and int(cfg["spatial_size"]) < 11:
        raise ValueError("eval_metrics: reconstruction needs spatial_size >= 11, the 11 x 11 SSIM window")
    rec_ev = evalutil.ReconstructionEvaluator(model.device) if "reconstruction" in metrics else None
    use_ev = (evalutil.PartUsageEvaluator(model.device, model.n_parts, float(cfg.get("val_min_part_area", 0.005)))
              if "parts" in metrics else None)
    # equivariance: every batch's view0 against its warped copy (one more pass of the pose path per batch); the uniforms of the running
    # image index come from a CPU generator seeded by `val_seed`, drawn batch by batch in that order
    co_ev = None
    if "coherence" in metrics:                     # the connected components of out_parts_hard, from the same forward passes
        from .model import coherence_config
        co_ev = evalutil.CoherenceEvaluator(model.device, model.n_parts, *coherence_config(cfg))
    eq_ev, eq_gen = None, None
    if "equivariance" in metrics:
        from .model import equivariance_tps_parameters
        from . import tps as _tps
        eq_ev = evalutil.EquivarianceEvaluator(model.device, model.n_parts, equivariance_tps_parameters(cfg))
        eq_gen = torch.Generator(device="cpu")
        eq_gen.manual_seed(int(cfg.get("val_seed", 1)))
    for bi, batch in enumerate(batches_it):
        if args.eval_batches is not None and bi >= args.eval_batches:
            break
        valid = batch.pop("valid", None)           # ragged last batch: padded to the static batch size, only `valid` rows count
        o = model.forward(batch)
        if eq_ev is not None:
            v0 = torch.as_tensor(batch["view0"])
            k = len(v0) if valid is None else int(valid)
            u = torch.rand(k, _tps.N_UNIFORMS, generator=eq_gen, dtype=torch.float32)      # rows [images so far, + k)
            if k < len(v0):                        # the padding is warped like the last valid image and dropped
                u = torch.cat([u, u[-1:].expand(len(v0) - k, -1)], 0)
            eq_ev.update(model, v0, u, valid=valid)
        if rec_ev is not None:
            rec_ev.update(model.generated_act, torch.as_tensor(batch["view0"]).to(model.device, torch.float32), valid=valid)
        if use_ev is not None:
            use_ev.update(o["out_parts_soft"], o["out_parts_hard"], valid=valid)
        if co_ev is not None:
            co_ev.update(o["out_parts_hard"], valid=valid)
        for k in keys:
            outs[k].append((o[k].detach().float().cpu().numpy() if o[k].dtype.is_floating_point else o[k].cpu().numpy())[:valid])
        for k in ins:
            ins[k].append(np.asarray(batch[k])[:valid])
        if "gt_segmentation" in batch:
            gts.append(np.asarray(batch["gt_segmentation"])[:valid])
    data = {"inputs": {k: np.concatenate(v) for k, v in ins.items()}, "outputs": {k: np.concatenate(v) for k, v in outs.items()}}
    odir = os.path.join(root, "eval", str(it.global_step))
    os.makedirs(odir, exist_ok=True)
    with open(os.path.join(odir, "model_outputs.p"), "wb") as f:
        pickle.dump(data, f)
    if metrics:
        vals = evalutil.validation_logs(rec_ev.result() if rec_ev is not None else None, use_ev.result() if use_ev is not None else None,
                                        equiv=eq_ev.result() if eq_ev is not None else None,
                                        **({"coherence": co_ev.result()} if co_ev is not None else {}))
        with open(os.path.join(odir, "metrics.yml"), "w") as f:       # the `val/` names of Trainer.validate without the prefix
            yaml.safe_dump({k[len("val/"):]: (int(v) if isinstance(v, int) else float(v)) for k, v in vals.items()}, f)
    if gts:
        gt = np.concatenate(gts)
        if cfg.get("eval_label_lut"):       # (the same table the device route hands to the kernel)
            gt = evalutil.lut_array(cfg["eval_label_lut"])[evalutil.labels_u8(gt)]
        write_iou_files(evalutil.evaluate_parts(data["outputs"]["out_parts_hard"], gt), odir, cfg, it.global_step)
    print("[INFO] evaluation outputs written to", odir)
    return data


def write_iou_files(res, odir, cfg, global_step):
    """iou.yml, and part_ious.csv / mean_part_ios.csv / best_remapping.yml as eval_01.py:355-383 writes them, from the result dict of
    ``evalutil.evaluate_parts`` or ``evalutil.evaluate_from_counts``."""
    from . import evalutil
    with open(os.path.join(odir, "iou.yml"), "w") as f:
        yaml.safe_dump({"iou": {int(k): float(v) for k, v in res["iou"].items()}, "overall": res["overall"],
                        "pooled_iou": {int(k): float(v) for k, v in res["pooled"].items()},
                        "best_remapping": {int(k): int(v) for k, v in res["mapping"].items()}}, f)
    names = cfg.get("part_names")
    evalutil.write_eval_tables(res, odir, global_step, {int(k): str(v) for k, v in names.items()} if names else None)


def evaluate_on_device(model, batches_it, cfg, eval_batches=None):
    """``eval_on_device: True``: the part-IoU protocol without the generator and without the outputs on the host.  ``view0`` of every
    batch goes through ``model.segment`` (pose path only) and ups_part_confusion (``evalutil.PartEvaluator``); one copy of the
    counts at the end.  ``eval_n_labels`` (default 32, the kernel's table; more counts on the host) and ``eval_label_lut``
    {raw: new} describe the labels.  Batches without ``gt_segmentation`` are a ValueError: this route computes nothing else."""
    import numpy as np
    from . import evalutil
    ev = evalutil.PartEvaluator(model, int(cfg.get("eval_n_labels", 32)), lut=cfg.get("eval_label_lut"))
    views, gts, held = [], [], 0

    def flush():
        ev.update(torch.cat(views, 0), np.concatenate(gts))
        del views[:], gts[:]
    for bi, batch in enumerate(batches_it):
        if eval_batches is not None and bi >= eval_batches:
            break
        if "gt_segmentation" not in batch:
            raise ValueError("eval_on_device: the batches carry no `gt_segmentation` (set data_gt_segmentation_column; without "
                             "ground truth there is nothing this route computes -- run -e without eval_on_device)")
        valid = batch.get("valid")
        views.append(torch.as_tensor(batch["view0"])[:valid])
        gts.append(evalutil.labels_u8(np.asarray(batch["gt_segmentation"]))[:valid])
        held += len(gts[-1])
        if held >= 2 * int(cfg["batch_size"]):       # a whole pass of segment: two batches' view0, nothing padded
            flush()
            held = 0
    if views:
        flush()
    return ev.result()


class SyntheticTransfer(object):
    """One block of U(-1, 1) row / column images in ``data.TransferData``'s block format (the data is not there)."""

    def __init__(self, config, seed=1234):
        self.config, self.seed = config, seed
        self.block_size = int(config.get("data_block_size", config["batch_size"]))

    def __iter__(self):
        gen = torch.Generator().manual_seed(self.seed)
        bs, S = self.block_size, self.config["spatial_size"]
        yield {"matrix": 0, "rows": (torch.rand(bs, S, S, 3, generator=gen) * 2 - 1).numpy(),
               "cols": (torch.rand(bs, S, S, 3, generator=gen) * 2 - 1).numpy(),
               "row_paths": ["synthetic/row_{:03}.png".format(i) for i in range(bs)],
               "col_paths": ["synthetic/col_{:03}.png".format(i) for i in range(bs)]}


def transfer(args):
    """``--transfer``: the comparison matrices of final_eval/eval_transfer.py.  Per block ONE transfer_matrix call (block_size poses
    and block_size appearances encoded once, block_size^2 images decoded) where the reference feeds block_size^2 pairs."""
    import pickle
    from . import evalutil
    cfg = load_config(args.transfer)
    for kv in args.set:
        k, v = kv.split("=", 1)
        cfg[k] = yaml.safe_load(v)
    cfg["test_mode"] = True
    parts = None if args.parts is None else [int(p) for p in args.parts.split(",") if p.strip() != ""]
    dist_setup()
    root = args.project or os.path.join("logs", time.strftime("%Y-%m-%dT%H-%M-%S") + "_transfer")
    try:
        blocks = _data.TransferData(cfg)
        if blocks.n_blocks:                     # the csvs without the image tree (or without PIL) are "data not there" as well
            blocks.preprocess_image(os.path.join(blocks.root, blocks.row_paths[0]))
    except (FileNotFoundError, NotADirectoryError, ImportError) as e:
        if args.strict_dataset:
            raise
        LOG.warning("SYNTHETIC DATA: transfer data is not available (%s: %s); one block of U(-1, 1) noise images. "
                    "Pass --strict-dataset to make this an error.", type(e).__name__, e)
        blocks = SyntheticTransfer(cfg)
    Model, Iterator = get_obj_from_str(cfg["model"]), get_obj_from_str(cfg["iterator"])
    model = Model(cfg)
    it = Iterator(cfg, root, model)
    it.initialize(args.checkpoint)
    gk, k0, k1 = cfg.get("generated_key", "generated"), cfg.get("vis0_key", "vis0"), cfg.get("vis1_key", "vis1")
    data = None
    for block in blocks:
        res = model.transfer_matrix(torch.from_numpy(block["rows"]), torch.from_numpy(block["cols"]), parts=parts)
        data = evalutil.transfer_cells(block, {k: v.cpu().numpy() for k, v in res.items()}, gk, k0, k1, data)
    if data is None:
        raise ValueError("--transfer: no block (fewer than data_block_size = {} rows or columns)".format(blocks.block_size))
    odir = os.path.join(root, "comparison_matrix", "{:06}".format(it.global_step))
    os.makedirs(odir, exist_ok=True)
    with open(os.path.join(odir, "data.p"), "wb") as f:
        pickle.dump(data, f)
    evalutil.write_transfer_matrix(data, os.path.join(odir, "comparison_matrix.png"), gk, k0, k1)
    print("[INFO] comparison matrix data written to", os.path.join(odir, "data.p"))
    return data


SEGMENT_OUTPUTS = ("labels", "overlay", "confidence")


def segment_options(cfg):
    """The `segment_*` keys of a yaml, validated: {"csv", "size", "max_side", "outputs", "alpha"}, with `segment_refine: bilateral`
    also "refine": {"radius", "sigma"}, with `segment_clean_min_area` > 0 also "clean": {"min_area", "rounds", "connectivity"}
    (what ``export_segments`` takes), and with `segment_annotations: coco` also "annotations": {"min_area", "path"} (path None: the
    default, <root>/segment/<global_step>/annotations.json); `segment_outputs` may be empty only then.  ValueError on anything else."""
    csv_path = cfg.get("segment_csv")
    if not csv_path:
        raise ValueError("--segment: `segment_csv` (one image path per line, relative to data_root) is required")
    size = cfg.get("segment_size", "source")
    if isinstance(size, (list, tuple)):
        if len(size) != 2 or any(not isinstance(v, int) or isinstance(v, bool) or v < 1 for v in size):
            raise ValueError("segment_size: source | model | [h, w] with h, w >= 1 (got {!r})".format(size))
        size = (int(size[0]), int(size[1]))
    elif size not in ("source", "model"):
        raise ValueError("segment_size: source | model | [h, w] (got {!r})".format(size))
    max_side = cfg.get("segment_max_side", 1024)
    if not isinstance(max_side, int) or isinstance(max_side, bool) or max_side < 1:
        raise ValueError("segment_max_side: an integer >= 1 (got {!r})".format(max_side))
    outputs = cfg.get("segment_outputs", ["labels", "overlay"])
    if isinstance(outputs, str):
        outputs = [outputs]
    outputs = tuple(outputs)
    annotations = cfg.get("segment_annotations", "none")
    if not isinstance(annotations, str) or annotations not in ("none", "coco"):
        raise ValueError("segment_annotations: none | coco (got {!r})".format(annotations))
    if ((not outputs and annotations != "coco") or len(set(outputs)) != len(outputs)
            or any(k not in SEGMENT_OUTPUTS for k in outputs)):
        raise ValueError("segment_outputs: a non-empty list of distinct names of {} -- empty only with segment_annotations: coco "
                         "(got {!r})".format(SEGMENT_OUTPUTS, list(outputs)))
    alpha = cfg.get("segment_alpha", 0.5)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("segment_alpha: a number in [0, 1] (got {!r})".format(alpha))
    opt = {"csv": csv_path, "size": size, "max_side": int(max_side), "outputs": outputs, "alpha": float(alpha)}
    mode = cfg.get("segment_refine", "none")
    if mode not in ("none", "bilateral"):
        raise ValueError("segment_refine: none | bilateral (got {!r})".format(mode))
    radius = cfg.get("segment_refine_radius", 1)
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= 3:
        raise ValueError("segment_refine_radius: an integer in 0 .. 3 (got {!r})".format(radius))
    sigma = cfg.get("segment_refine_sigma", 16.0)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not 0.0 < float(sigma) < float("inf"):
        raise ValueError("segment_refine_sigma: a number > 0 (got {!r})".format(sigma))
    if mode == "bilateral":
        opt["refine"] = {"radius": int(radius), "sigma": float(sigma)}
    # speck clean-up of the rendered labels: components of fewer than `segment_clean_min_area` output pixels (0 = off, the default)
    min_area = cfg.get("segment_clean_min_area", 0)
    if not isinstance(min_area, int) or isinstance(min_area, bool) or min_area < 0:
        raise ValueError("segment_clean_min_area: an integer count of output pixels >= 0, 0 = off (got {!r})".format(min_area))
    rounds = cfg.get("segment_clean_rounds", 1)
    if not isinstance(rounds, int) or isinstance(rounds, bool) or not 1 <= rounds <= 4:
        raise ValueError("segment_clean_rounds: an integer in 1 .. 4 (got {!r})".format(rounds))
    conn = cfg.get("segment_clean_connectivity", 8)
    if isinstance(conn, bool) or conn not in (4, 8):
        raise ValueError("segment_clean_connectivity: 4 or 8 (got {!r})".format(conn))
    if min_area > 0:
        opt["clean"] = {"min_area": int(min_area), "rounds": int(rounds), "connectivity": int(conn)}
    # COCO annotations of the final labels: one record per image and part of at least `segment_annotation_min_area` pixels
    ann_area = cfg.get("segment_annotation_min_area", 1)
    if not isinstance(ann_area, int) or isinstance(ann_area, bool) or ann_area < 0:
        raise ValueError("segment_annotation_min_area: an integer count of output pixels >= 0 (got {!r})".format(ann_area))
    ann_path = cfg.get("segment_annotation_path")
    if ann_path is not None and (not isinstance(ann_path, str) or not ann_path):
        raise ValueError("segment_annotation_path: a file path (got {!r})".format(ann_path))
    if annotations == "coco":
        opt["annotations"] = {"min_area": int(ann_area), "path": ann_path}
    return opt


def segment_output_size(h, w, opt, S):
    """The rendered size of an h x w source under `segment_size` / `segment_max_side`: (h', w', scaled).  A size whose longer side
    exceeds max_side is scaled down to it, proportions kept (rounded, at least 1)."""
    if opt["size"] == "model":
        h, w = S, S
    elif opt["size"] != "source":
        h, w = opt["size"]
    m = max(h, w)
    if m <= opt["max_side"]:
        return int(h), int(w), False
    return max(1, (h * opt["max_side"] + m // 2) // m), max(1, (w * opt["max_side"] + m // 2) // m), True


def segment_png_path(root, name, step):
    """ImageWriter path rule of the export: name = (kind, relative path) -> <root>/segment/<step>/<kind>/<relative path>.png"""
    kind, rel = name
    return os.path.join(root, "segment", str(step), kind, rel + ".png")


def write_segment_index(path, rows, n_parts):
    """index.csv: one row per image -- file, h, w and area_<p> = count_p / (h w) from the kernel's counts."""
    import csv
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["file", "h", "w"] + ["area_{}".format(p) for p in range(n_parts)])
        for rel, h, w, counts in rows:
            wr.writerow([rel, h, w] + [repr(int(c) / float(h * w)) for c in counts])


def coco_annotations(images, masks, palette, min_area=1):
    """The dict of annotations.json (COCO's layout, uncompressed run-length masks), keys in a fixed order.
    images: [(file_name, h, w)] in csv order; masks: per image the P tuples (counts list, area, (x, y, w, h)) of its parts, as
    ``ops.segment_rle`` gives them; palette [P,3]: the export's colours.  Image ids are 1-based in csv order, category p + 1 is
    part p, annotation ids are 1-based in (image, part) order over the parts of at least `min_area` pixels."""
    P = len(palette)
    doc = OrderedDict()
    doc["images"] = [OrderedDict((("id", i + 1), ("file_name", name), ("height", int(h)), ("width", int(w))))
                     for i, (name, h, w) in enumerate(images)]
    doc["categories"] = [OrderedDict((("id", p + 1), ("name", "part_{}".format(p)), ("color", [int(c) for c in palette[p]])))
                         for p in range(P)]
    anns = []
    for i, ((name, h, w), parts) in enumerate(zip(images, masks)):
        if len(parts) != P:
            raise ValueError("coco_annotations: {} masks for {} parts (image {})".format(len(parts), P, name))
        for p, (counts, area, bbox) in enumerate(parts):
            if int(area) < min_area:
                continue
            anns.append(OrderedDict((
                ("id", len(anns) + 1), ("image_id", i + 1), ("category_id", p + 1),
                ("segmentation", OrderedDict((("size", [int(h), int(w)]), ("counts", [int(c) for c in counts])))),
                ("area", int(area)), ("bbox", [int(v) for v in bbox]), ("iscrowd", 1))))
    doc["annotations"] = anns
    return doc


def write_coco_annotations(path, images, masks, palette, min_area=1):
    """annotations.json with the standard library's json: fixed key order and separators, so two runs write the same bytes."""
    import json
    doc = coco_annotations(images, masks, palette, min_area)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    return doc


def segment_files(model, cfg, root, step, profile=None):
    """The export itself: every image of `segment_csv` is decoded ONCE with PIL, resized to S x S by the dataset's preprocess_image
    rule (bilinear, / 127.5 - 1) for the model and kept at its output size as uint8 for the overlay; passes of 2 * batch_size images
    go through ``TrainModel.export_segments`` (one pose pass and one ups_segment_render launch each) and the planes, copied into
    pinned buffers behind an event, are encoded by the bounded writer thread (it blocks, never drops, and is joined before return).
    With `segment_clean_min_area` > 0 each pass also cleans specks out of its labels before the copies (``export_segments(clean=)``)
    and one line logs how many pixels were relabelled in all; with the key at 0 the call is the one it was.
    With `segment_annotations: coco` each pass also run-length encodes its final labels on the device (``export_segments(rle=True)``)
    and annotations.json is written after the last pass; with `segment_outputs: []` nothing is handed to the writer thread, which
    is then never started, and no PNG directory appears.  index.csv is written either way.
    A missing file raises FileNotFoundError before anything is computed: there is no synthetic fall-back on this route.
    profile: a dict that receives wall-clock seconds per phase (decode, model passes, packing and upload of the sources, kernel,
    copies, encode); the phases are then SYNCHRONISED so that the device time is attributed, which a normal run does not do.
    Returns the index rows."""
    import numpy as np
    from PIL import Image
    from . import imglog as IL
    from . import ops
    opt = segment_options(cfg)
    refine, clean, ann = opt.get("refine"), opt.get("clean"), opt.get("annotations")
    extra = dict(({"clean": clean} if clean is not None else {}), **({"rle": True} if ann is not None else {}))
    relabelled = 0
    if refine is None:
        LOG.info("--segment: segment_refine = none: labels are the arg-max of the bilinearly resampled map")
    else:
        LOG.info("--segment: segment_refine = bilateral (radius %d, sigma %g): labels guided by the source images", refine["radius"],
                 refine["sigma"])
    S, B = int(cfg["spatial_size"]), int(cfg["batch_size"])
    data_root = cfg["data_root"]
    rels = _data.TransferData._read_list(opt["csv"])
    if not rels:
        raise ValueError("--segment: {} lists no image".format(opt["csv"]))
    for rel in rels:
        if not os.path.isfile(os.path.join(data_root, rel)):
            raise FileNotFoundError("--segment: {} (listed in {}) does not exist".format(os.path.join(data_root, rel), opt["csv"]))
    palette = IL.mask_color_bytes(IL.mask_colors01(model.n_parts))
    writer = IL.ImageWriter(root, path_fn=segment_png_path) if opt["outputs"] else None
    rows, pending, warned = [], [], False
    t = dict.fromkeys(("decode", "model", "upload", "kernel", "copies", "encode"), 0.0)
    dev = model.device

    def lap(key, t0):
        if profile is not None:
            torch.cuda.synchronize(dev)
            t[key] += time.perf_counter() - t0
        return time.perf_counter()
    try:
        for c0 in range(0, len(rels), 2 * B):
            chunk = rels[c0:c0 + 2 * B]
            t0 = time.perf_counter()
            views, sizes, sources = [], [], []
            for rel in chunk:
                img = Image.open(os.path.join(data_root, rel)).convert("RGB")
                views.append(np.asarray(img.resize((S, S), Image.BILINEAR), dtype=np.float32) / 127.5 - 1.0)
                h, w, scaled = segment_output_size(img.height, img.width, opt, S)
                if scaled and not warned:
                    warned = True
                    LOG.warning("--segment: sources larger than segment_max_side = %d are rendered scaled down to it (first: %s, "
                                "%d x %d -> %d x %d)", opt["max_side"], rel, img.height, img.width, h, w)
                sizes.append((h, w))
                if "overlay" in opt["outputs"] or refine is not None:
                    sources.append(np.asarray(img if (img.height, img.width) == (h, w) else img.resize((w, h), Image.BILINEAR),
                                              dtype=np.uint8))
            t0 = lap("decode", t0)
            vt = torch.from_numpy(np.stack(views))
            if profile is None:
                res = model.export_segments(vt, sizes, sources=sources or None, outputs=opt["outputs"], alpha=opt["alpha"], colors=palette,
                                            refine=refine, **extra)
            else:                           # the phases apart: the pose pass, the kernel and the copies each behind a synchronisation
                maps = model.segment_soft(vt)
                t0 = lap("model", t0)
                packed = None
                if sources:
                    table, total = ops.segment_table(sizes)
                    packed = ops.segment_pack_sources(sources, table, total).to(dev)
                t0 = lap("upload", t0)
                laps = []
                res = model.export_segments(vt, sizes, sources=packed, outputs=opt["outputs"], alpha=opt["alpha"],
                                            colors=palette, maps=maps, after_launch=lambda: laps.append(lap("kernel", t0)), refine=refine,
                                            **extra)
                res["ready"].synchronize()
                lap("copies", laps[0])
            relabelled += res.get("relabelled", 0)
            images = OrderedDict()
            for i, rel in enumerate(chunk):
                for kind in opt["outputs"]:
                    v = res["views"][kind][i]
                    images[(kind, rel)] = IL.Paletted(v, palette) if kind == "labels" else v
            if writer is not None:
                writer.submit(step, images, res["ready"])
            rle = {k: res["host"][k] for k in ("rle_offsets", "rle_counts", "area", "bbox")} if ann is not None else None
            pending.append((chunk, sizes, res["host"]["counts"], res["ready"], rle))  # (the planes live on in the writer's queue only)
            if profile is not None and writer is not None:      # encoded here and now, not beside the next pass
                t0 = time.perf_counter()
                writer.flush()
                t["encode"] += time.perf_counter() - t0
        if writer is not None:
            writer.flush()
    finally:
        if writer is not None:
            writer.close()
    if clean is not None:
        LOG.info("--segment: clean-up (min_area %d, up to %d round(s), connectivity %d) relabelled %d pixel(s)", clean["min_area"],
                 clean["rounds"], clean["connectivity"], relabelled)
    masks = []
    t0 = time.perf_counter()
    for chunk, sizes, counts, ready, rle in pending:
        ready.synchronize()
        for i, rel in enumerate(chunk):
            rows.append((rel, sizes[i][0], sizes[i][1], [int(c) for c in counts[i].tolist()]))
        if rle is not None:
            lists = ops.rle_lists(rle["rle_offsets"], rle["rle_counts"], len(chunk), model.n_parts)
            area, bbox = rle["area"].tolist(), rle["bbox"].tolist()
            masks.extend([(lists[i][p], area[i][p], bbox[i][p]) for p in range(model.n_parts)] for i in range(len(chunk)))
    odir = os.path.join(root, "segment", str(step))
    os.makedirs(odir, exist_ok=True)
    write_segment_index(os.path.join(odir, "index.csv"), rows, model.n_parts)
    if ann is not None:
        path = ann["path"] or os.path.join(odir, "annotations.json")
        doc = write_coco_annotations(path, [(rel, h, w) for rel, h, w, _ in rows], masks, palette.tolist(), ann["min_area"])
        LOG.info("--segment: %d annotation(s) of %d image(s) written to %s", len(doc["annotations"]), len(rows), path)
        t["annotations"] = time.perf_counter() - t0
    if profile is not None:
        profile.update(t)
    return rows


def segment(args):
    """``--segment``: see ``segment_files``.  Outputs: <root>/segment/<global_step>/{labels,overlay,confidence}/<relative path>.png
    (labels: a palette PNG whose bytes are the part ids) and index.csv; with `segment_annotations: coco` also annotations.json (COCO
    records with uncompressed run-length masks, one per image and part).  Returns {"rows", "root", "dir", "model"}."""
    cfg = load_config(args.segment)
    for kv in args.set:
        k, v = kv.split("=", 1)
        cfg[k] = yaml.safe_load(v)
    cfg["test_mode"] = True
    segment_options(cfg)            # a wrong key fails before a device is touched
    if not cfg.get("data_root"):
        raise ValueError("--segment: `data_root` is required")
    dist_setup()
    root = args.project or os.path.join("logs", time.strftime("%Y-%m-%dT%H-%M-%S") + "_segment")
    Model, Iterator = get_obj_from_str(cfg["model"]), get_obj_from_str(cfg["iterator"])
    model = Model(cfg)
    it = Iterator(cfg, root, model)
    it.initialize(args.checkpoint)
    if args.checkpoint is None:
        LOG.warning("--segment without -c: the part maps of freshly initialised weights")
    rows = segment_files(model, cfg, root, it.global_step)
    odir = os.path.join(root, "segment", str(it.global_step))
    print("[INFO] {} images segmented into {}".format(len(rows), odir))
    return {"rows": rows, "root": root, "dir": odir, "model": model}


def index(args):
    """``--index``: the part-appearance index of the images in ``index_csv`` (``partindex.index_files``; the keys and their defaults:
    ``partindex.INDEX_DEFAULTS``).  Outputs under <root>/index/<global_step>/: features.npz, index.csv, neighbours.npz, clusters.p
    and the contact sheets.  A wrong key raises ValueError before the model is built; a missing image raises FileNotFoundError, as
    on --segment.  Returns {"root", "dir", "model", "index", "neighbours", "clusters"}."""
    from . import partindex
    cfg = load_config(args.index)
    for kv in args.set:
        k, v = kv.split("=", 1)
        cfg[k] = yaml.safe_load(v)
    cfg["test_mode"] = True
    partindex.index_options(cfg)    # a wrong key fails before a device is touched
    if not cfg.get("data_root"):
        raise ValueError("--index: `data_root` is required")
    dist_setup()
    root = args.project or os.path.join("logs", time.strftime("%Y-%m-%dT%H-%M-%S") + "_index")
    Model, Iterator = get_obj_from_str(cfg["model"]), get_obj_from_str(cfg["iterator"])
    model = Model(cfg)
    it = Iterator(cfg, root, model)
    it.initialize(args.checkpoint)
    if args.checkpoint is None:
        LOG.warning("--index without -c: the part codes of freshly initialised weights")
    odir = os.path.join(root, "index", str(it.global_step))
    res = partindex.index_files(model, cfg, odir)
    print("[INFO] {} images indexed into {}".format(res["index"].N, odir))
    return dict(res, root=root, dir=odir, model=model)


def landmarks(args):
    """``--landmarks``: landmark regression from the part centres (``landmarks.landmark_files``; the keys and their defaults:
    ``landmarks.LANDMARK_DEFAULTS``).  Outputs under <root>/landmarks/<global_step>/: regressor.npz, landmarks.csv, summary.yml and
    predictions.npz.  A wrong key raises ValueError before the model is built; a missing csv or image raises FileNotFoundError, as on
    --segment: nothing synthetic stands in.  Returns {"root", "dir", "model", "regressor", "summary", "predictions"}."""
    from . import landmarks as LM
    cfg = load_config(args.landmarks)
    for kv in args.set:
        k, v = kv.split("=", 1)
        cfg[k] = yaml.safe_load(v)
    cfg["test_mode"] = True
    LM.landmark_options(cfg)        # a wrong key fails before a device is touched
    if not cfg.get("data_root"):
        raise ValueError("--landmarks: `data_root` is required")
    dist_setup()
    root = args.project or os.path.join("logs", time.strftime("%Y-%m-%dT%H-%M-%S") + "_landmarks")
    Model, Iterator = get_obj_from_str(cfg["model"]), get_obj_from_str(cfg["iterator"])
    model = Model(cfg)
    it = Iterator(cfg, root, model)
    it.initialize(args.checkpoint)
    if args.checkpoint is None:
        LOG.warning("--landmarks without -c: the part centres of freshly initialised weights")
    odir = os.path.join(root, "landmarks", str(it.global_step))
    res = LM.landmark_files(model, cfg, odir)
    s = res["summary"]
    print("[INFO] landmarks: {} over {} keypoints = {} (over {} visible instances = {}), {} fitted on {} images; written to {}".format(
        s["error"], s["n_keypoints"], s["mean_error"], s["n_visible"], s["mean_error_instances"], s["n_test"], s["n_fit"], odir))
    return dict(res, root=root, dir=odir, model=model)


if __name__ == "__main__":
    main()
