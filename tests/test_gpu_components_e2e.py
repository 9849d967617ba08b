"""GPU tests of the part-coherence feature end to end: the `coherence` metric of Trainer.validate and of the runner's -e against
evalutil.coherence_host on the same part maps, and the speck clean-up of --segment against the restatement of components_ref.py
applied to the files of a run without it.  Everything compared is an integer or a quotient of pooled integers: ==."""
import copy
import csv
import os

import numpy as np
import pytest
import torch

import components_ref as R
from parteval_ref import write_label_dataset

pytestmark = pytest.mark.gpu

VGG_W = (8, 8, 16, 16, 16)


@pytest.fixture(autouse=True)
def _keep_rng_state(dev):
    """Building a model seeds torch's generators; later test files draw unseeded device tensors.  They see the state they saw before
    this file existed."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu, dev)


def _coherence_keys(P):
    return sorted(["fragmentation", "specks"] + ["fragmentation_{}".format(p) for p in range(P)]
                  + ["components_{}".format(p) for p in range(P)])


# ---------------------------------------------------------------------------------------------- Trainer.validate
@pytest.mark.parametrize("metrics", (["parts", "coherence"], ["coherence"]), ids=("with_parts", "alone"))
def test_validate_reports_coherence(dev, tmp_path, metrics):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil
    from upsparts_amd.model import TrainModel, Trainer
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update({"precision": "bf16", "vgg_widths": VGG_W, "ckpt_freq": 0, "log_freq": 250})
    S, P = cfg["spatial_size"], cfg["n_parts"]
    ds = write_label_dataset(tmp_path, n=5, S=S, seed=4, name="val")
    ds.pop("data_gt_segmentation_column")                               # no label column is needed
    cfg.update(ds)
    cfg.update({"val_freq": 2, "val_csv": cfg.pop("data_csv"), "val_metrics": metrics, "val_speck_area": 0.02,
                "val_coherence_connectivity": 4})
    small = int(np.ceil(0.02 * S * S))
    trainer = Trainer(cfg, None, TrainModel(cfg, device=dev, seed=0))
    logs = trainer.validate()
    again = trainer.validate()
    model, pairs = trainer.model, trainer._val["pairs"]
    maps = []
    for ci in range(pairs.chunks()):
        chunk = pairs.chunk_views(ci, trainer.device)
        if "parts" in metrics:                                          # the maps of the forward pass the `parts` metric runs
            maps.append(model.forward(chunk, noise=None)["out_parts_hard"].cpu().numpy())
        else:                                                           # listed alone: a pose pass of its own
            maps.append(model.segment(chunk["view0"]).cpu().numpy())
    maps = np.concatenate(maps)
    stats, invalid = evalutil.coherence_host(maps, P, 4, small)
    want = evalutil.coherence_from_stats(stats, S * S)
    assert invalid == 0 and trainer._val["coherence"].n == len(maps) == len(pairs)
    got = {k[len("val/"):]: v for k, v in logs.items() if k[len("val/"):] in want}
    print("coherence", metrics, got)
    assert sorted(got) == _coherence_keys(P)
    assert got == want
    assert {k: v for k, v in again.items()} == {k: v for k, v in logs.items()}
    assert ("val/part_area_0" in logs) == ("parts" in metrics) and list(logs)[-1] == "val/steps_done"
    # the device table itself, against the two-restatement reference
    dstats, dinv = trainer._val["coherence"].sums()
    for i, m in enumerate(maps):
        comp = R.components_flood(m, P, 4)
        assert np.array_equal(comp, R.components_unionfind(m, P, 4))
        assert np.array_equal(dstats[i], R.stats(m, comp, P, small)[1]), i
    assert dinv == 0


# ---------------------------------------------------------------------------------------------- runner -e
def test_runner_eval_metrics_coherence(dev, tmp_path):
    import pickle
    import yaml
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil, runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(write_label_dataset(tmp_path, n=5, S=cfg["spatial_size"]))
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "val_speck_area": 0.02})
    S, P = cfg["spatial_size"], cfg["n_parts"]
    ypath = tmp_path / "eval.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    runner.main(["-e", str(ypath), "-p", str(tmp_path / "plain"), "--strict-dataset"])
    runner.main(["-e", str(ypath), "-p", str(tmp_path / "metrics"), "--strict-dataset", "--set", "eval_metrics=[coherence]"])
    pdir, mdir = tmp_path / "plain" / "eval" / "0", tmp_path / "metrics" / "eval" / "0"
    assert sorted(os.listdir(str(mdir))) == sorted(os.listdir(str(pdir)) + ["metrics.yml"])
    for f in os.listdir(str(pdir)):
        assert (pdir / f).read_bytes() == (mdir / f).read_bytes(), f
    hard = pickle.loads((mdir / "model_outputs.p").read_bytes())["outputs"]["out_parts_hard"]
    assert hard.shape == (5, S, S)
    stats, invalid = evalutil.coherence_host(hard, P, 8, int(np.ceil(0.02 * S * S)))
    got = yaml.safe_load((mdir / "metrics.yml").read_text())
    assert invalid == 0 and sorted(got) == _coherence_keys(P)
    assert got == evalutil.coherence_from_stats(stats, S * S)


# ---------------------------------------------------------------------------------------------- runner --segment
def _read_run(odir, files, P):
    from PIL import Image
    out = {}
    for rel, _ in files:
        out[rel] = {k: np.asarray(Image.open(os.path.join(odir, k, rel + ".png"))) for k in ("labels", "overlay", "confidence")}
    with open(os.path.join(odir, "index.csv"), newline="") as f:
        out["index"] = list(csv.reader(f))
    return out


def _file_bytes(odir):
    res = {}
    for base, _, names in os.walk(odir):
        for n in names:
            with open(os.path.join(base, n), "rb") as f:
                res[os.path.relpath(os.path.join(base, n), odir)] = f.read()
    return res


def test_runner_segment_clean(dev, tmp_path, caplog):
    """--segment on three small synthetic PNGs.  With `segment_clean_min_area: 0` every byte is the run's without the key; with 6 (the
    default single round, connectivity 8) and with 200 (two rounds, connectivity 4, which is certain to move something) labels,
    overlay, confidence and index.csv equal the restatement applied to the files of the run without it."""
    import logging
    import yaml
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import imglog as IL, runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    P = cfg["n_parts"]
    data_root = tmp_path / "images"
    rng = np.random.RandomState(6)
    files = [("a/one.png", (37, 46)), ("two.png", (21, 13)), ("b/three.png", (40, 33))]
    srcs = {}
    for rel, (h, w) in files:
        os.makedirs(os.path.dirname(str(data_root / rel)), exist_ok=True)
        small = rng.randint(0, 256, size=(4, 5, 3)).astype(np.uint8)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(str(data_root / rel))
        srcs[rel] = np.asarray(Image.open(str(data_root / rel)).convert("RGB"), dtype=np.uint8)
    csv_path = tmp_path / "list.csv"
    csv_path.write_text("\n".join(rel for rel, _ in files) + "\n")
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(data_root), "segment_csv": str(csv_path),
                "segment_outputs": ["labels", "overlay", "confidence"], "segment_alpha": 0.5})
    palette = IL.mask_color_bytes(IL.mask_colors01(P))

    def run(name, **keys):
        ypath = tmp_path / (name + ".yaml")
        ypath.write_text(yaml.safe_dump(dict(cfg, **keys)))
        with caplog.at_level(logging.INFO, logger="upsparts"):
            caplog.clear()
            runner.main(["--segment", str(ypath), "-p", str(tmp_path / name)])
        return str(tmp_path / name / "segment" / "0"), caplog.text

    plain_dir, plain_log = run("plain")
    zero_dir, zero_log = run("zero", segment_clean_min_area=0)
    assert _file_bytes(plain_dir) == _file_bytes(zero_dir) and len(_file_bytes(plain_dir)) == 3 * 3 + 1
    assert "relabelled" not in plain_log and "relabelled" not in zero_log
    plain = _read_run(plain_dir, files, P)
    moved_by_case = []
    for name, keys, conn, rounds, min_area in (("six", {"segment_clean_min_area": 6}, 8, 1, 6),
                                               ("big", {"segment_clean_min_area": 200, "segment_clean_rounds": 2,
                                                        "segment_clean_connectivity": 4}, 4, 2, 200)):
        odir, log = run(name, **keys)
        got = _read_run(odir, files, P)
        total = 0
        for i, (rel, (h, w)) in enumerate(files):
            lab = plain[rel]["labels"].astype(np.int64)
            planes = {"overlay": plain[rel]["overlay"], "confidence": plain[rel]["confidence"],
                      "counts": np.bincount(lab.reshape(-1), minlength=P)}
            for _ in range(rounds):
                new, changed = R.clean_round(lab, P, conn, min_area)
                planes = R.clean_planes(lab, new, P, palette, 0.5, srcs[rel], planes["overlay"], planes["confidence"], planes["counts"])
                lab, total = new, total + changed
                if changed == 0:
                    break
            assert np.array_equal(got[rel]["labels"], lab), (name, rel)
            assert np.array_equal(got[rel]["overlay"], planes["overlay"]), (name, rel)
            assert np.array_equal(got[rel]["confidence"], planes["confidence"]), (name, rel)
            assert got["index"][1 + i][:3] == [rel, str(h), str(w)]
            assert [float(x) for x in got["index"][1 + i][3:]] == [c / float(h * w) for c in planes["counts"]], (name, rel)
            assert np.array_equal(planes["counts"], np.bincount(lab.reshape(-1), minlength=P))
        assert log.count("relabelled") == 1 and "relabelled {} pixel(s)".format(total) in log, log
        moved_by_case.append(total)
    print("relabelled pixels", moved_by_case)
    assert moved_by_case[1] > 0
