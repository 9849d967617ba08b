"""Landmark regression evaluation: how well do the discovered parts' centres predict annotated keypoints?

The score the part-discovery papers report on the data sets that come with keypoints and without dense part labels (CUB's 15 bird
parts, PennAction's 13 joints): take each part's centre, fit a linear map from the P centres to the K keypoints on a fit split -- one
ridge regression per keypoint over the instances where it is visible -- and report the mean error as a fraction of the image edge, and
PCK, on a test split.  The reference has no such evaluation; the definitions are this project's own (DESIGN.md section 8,
include/upsparts_hip.h "landmark regression evaluation").  The arithmetic is four HIP kernels (csrc/landmarks.hip through
``ops.part_moments`` / ``landmark_gram`` / ``landmark_solve`` / ``landmark_predict``): fp64, fixed orders of summation, results equal
from run to run and to the NumPy restatement of tests/landmarks_ref.py.  The host keeps what is not hot: the csv files, the square
root, the means and the PCK counts on the N x K array of squared distances, and the output files.

Keypoint csv: one line per image, ``relative_path, x_1, y_1, v_1, .., x_K, y_K, v_K`` -- pixel coordinates of the source file (pixel
centres at integers), v != 0: visible.  Targets are normalised with the source size, (2x + 1) / w - 1, onto the [-1, 1] square of the
part centres; an error is sqrt(dx^2 + dy^2) / 2, a fraction of the edge of the model's square view.
"""
import csv
import json
import os

import numpy as np
import torch

from . import lib as L
from . import ops
from .partindex import save_npz

SOURCES = ("soft", "hard")
LANDMARK_DEFAULTS = {"landmark_test_csv": None, "landmark_source": "soft", "landmark_min_part_area": 0.005, "landmark_ridge": 1e-6,
                     "landmark_pck": [0.05, 0.1], "landmark_names": None}


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v)


def landmark_options(cfg):
    """The `landmark_*` keys of a yaml, validated and with their defaults: {"fit_csv", "test_csv" (None: the fit csv), "source",
    "min_part_area", "ridge", "pck", "names"}.  ValueError on anything else."""
    unknown = sorted(k for k in cfg if k.startswith("landmark_") and k != "landmark_fit_csv" and k not in LANDMARK_DEFAULTS)
    if unknown:
        raise ValueError("--landmarks: unknown key(s) {} (known: landmark_fit_csv, {})".format(unknown, ", ".join(sorted(LANDMARK_DEFAULTS))))
    o = {k[len("landmark_"):]: cfg.get(k, d) for k, d in LANDMARK_DEFAULTS.items()}
    o["fit_csv"] = cfg.get("landmark_fit_csv")
    if not o["fit_csv"] or not isinstance(o["fit_csv"], str):
        raise ValueError("--landmarks: `landmark_fit_csv` (path, x_1, y_1, v_1, .. per line; paths relative to data_root) is required")
    if o["test_csv"] is not None and (not isinstance(o["test_csv"], str) or not o["test_csv"]):
        raise ValueError("landmark_test_csv: a path (got {!r})".format(o["test_csv"]))
    if o["source"] not in SOURCES:
        raise ValueError("landmark_source: soft | hard (got {!r})".format(o["source"]))
    if not _number(o["min_part_area"]) or not 0.0 <= float(o["min_part_area"]) <= 1.0:
        raise ValueError("landmark_min_part_area: a fraction of the image in [0, 1] (got {!r})".format(o["min_part_area"]))
    o["min_part_area"] = float(o["min_part_area"])
    if not _number(o["ridge"]) or float(o["ridge"]) < 0.0:
        raise ValueError("landmark_ridge: a number >= 0 (got {!r})".format(o["ridge"]))
    o["ridge"] = float(o["ridge"])
    pck = o["pck"]
    if not isinstance(pck, (list, tuple)) or not pck or any(not _number(t) or not 0.0 < float(t) <= 1.0 for t in pck):
        raise ValueError("landmark_pck: a non-empty list of thresholds in (0, 1] (got {!r})".format(pck))
    o["pck"] = [float(t) for t in pck]
    if len(set(o["pck"])) != len(o["pck"]):
        raise ValueError("landmark_pck: thresholds listed once each (got {!r})".format(pck))
    if o["names"] is not None and (not isinstance(o["names"], (list, tuple)) or not o["names"]
                                   or any(not isinstance(s, str) or not s for s in o["names"])):
        raise ValueError("landmark_names: a list of K names (got {!r})".format(o["names"]))
    o["names"] = None if o["names"] is None else [str(s) for s in o["names"]]
    return o


def read_landmark_csv(path):
    """-> (files [N], xy [N,K,2] float64 source pixels, vis [N,K] uint8).  K = (columns - 1) / 3, the same on every line; a missing
    file raises FileNotFoundError, a malformed line ValueError with its number.  Blank lines are skipped."""
    if not os.path.isfile(path):
        raise FileNotFoundError("--landmarks: keypoint csv {} does not exist".format(path))
    files, rows = [], []
    with open(path, newline="") as f:
        for ln, row in enumerate(csv.reader(f), 1):
            row = [c.strip() for c in row]
            if not row or all(c == "" for c in row):
                continue
            if len(row) < 4 or (len(row) - 1) % 3 or (rows and len(row) - 1 != len(rows[0])):
                raise ValueError("{}:{}: path, x_1, y_1, v_1, .., x_K, y_K, v_K with one K per file (got {} columns)".format(path, ln, len(row)))
            try:
                rows.append([float(c) for c in row[1:]])
            except ValueError:
                raise ValueError("{}:{}: a coordinate or visibility flag is not a number".format(path, ln))
            files.append(row[0])
    if not files:
        raise ValueError("--landmarks: {} lists no image".format(path))
    a = np.asarray(rows, dtype=np.float64).reshape(len(files), -1, 3)
    vis = (a[..., 2] != 0).astype(np.uint8)
    if not np.isfinite(a[..., :2][vis != 0]).all():
        raise ValueError("{}: a visible keypoint has a coordinate that is not finite".format(path))
    return files, np.ascontiguousarray(a[..., :2]), vis


def normalise_targets(xy, sizes):
    """Source pixels -> [-1, 1]: ((2x + 1) / w - 1, (2y + 1) / h - 1) with sizes [N,2] = (h, w) of each source file."""
    sizes = np.asarray(sizes, dtype=np.float64).reshape(-1, 1, 2)
    return np.stack([(2.0 * xy[..., 0] + 1.0) / sizes[..., 1] - 1.0, (2.0 * xy[..., 1] + 1.0) / sizes[..., 0] - 1.0], axis=-1)


def to_source_pixels(u, sizes):
    """The inverse of ``normalise_targets``: x = ((u_x + 1) w - 1) / 2."""
    sizes = np.asarray(sizes, dtype=np.float64).reshape(-1, 1, 2)
    return np.stack([((u[..., 0] + 1.0) * sizes[..., 1] - 1.0) / 2.0, ((u[..., 1] + 1.0) * sizes[..., 0] - 1.0) / 2.0], axis=-1)


def metrics_from_d2(d2, pck, n_singular=0):
    """The host half of the evaluation, NumPy float64 on d2 [N,K] (squared distances on [-1, 1]; < 0: not visible):
    error = sqrt(d2) / 2.  -> {"keypoints": [{"n_visible", "mean_error", "pck@<t>"..}] (None where nothing is visible), "mean_error":
    the mean of the keypoints' mean errors (keypoints with a visible instance), "pck@<t>": likewise, "mean_error_instances": the mean
    over all visible instances, "n_visible": their number, "n_singular"}."""
    d2 = np.asarray(d2, dtype=np.float64)
    see = d2 >= 0
    err = np.sqrt(np.where(see, d2, 0.0)) / 2.0
    keys = ["pck@{:g}".format(t) for t in pck]
    per = []
    for k in range(d2.shape[1]):
        e = err[see[:, k], k]
        row = {"n_visible": int(e.size), "mean_error": float(e.mean()) if e.size else None}
        for key, t in zip(keys, pck):
            row[key] = float((e <= t).mean()) if e.size else None
        per.append(row)
    seen = [r for r in per if r["n_visible"]]
    out = {"keypoints": per, "n_visible": int(see.sum()), "n_singular": int(n_singular),
           "mean_error": float(np.mean([r["mean_error"] for r in seen])) if seen else None,
           "mean_error_instances": float(err[see].mean()) if see.any() else None}
    for key in keys:
        out[key] = float(np.mean([r[key] for r in seen])) if seen else None
    return out


class LandmarkRegressor(object):
    """One ridge regression per keypoint from the part centres to the keypoint: W [K, 2P + 1, 2] float64 (the last row is the bias,
    which the ridge does not penalise).  The features of an instance are its centres (x_0, y_0, x_1, ..), a part that is not valid as
    (0, 0).  ``fit`` and ``predict`` run on the device (there is no host route)."""

    def __init__(self, W=None, cnt=None, n_singular=0, options=None, device=None):
        self.W = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
        self.cnt = None if cnt is None else np.ascontiguousarray(cnt, dtype=np.int32)
        self.n_singular = int(n_singular)
        self.options = dict(options or {})
        self.device = device

    def _dev(self):
        if not torch.cuda.is_available():
            raise L.UpsError("LandmarkRegressor: the regression kernels need a HIP device (there is no host route)")
        return torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def _features(self, centre, valid):
        dev = self._dev()
        centre = torch.as_tensor(centre).to(dev, torch.float64)
        valid = torch.as_tensor(valid).to(dev)
        if centre.dim() != 3 or centre.shape[0] == 0 or centre.shape[2] != 2 or tuple(valid.shape) != tuple(centre.shape[:2]):
            raise ValueError("LandmarkRegressor: centre [N >= 1,P,2] and valid [N,P] (got {} and {})".format(tuple(centre.shape), tuple(valid.shape)))
        if 2 * centre.shape[1] + 1 > ops.LANDMARK_MAX_D:
            raise ValueError("LandmarkRegressor: at most {} parts (got {})".format((ops.LANDMARK_MAX_D - 1) // 2, centre.shape[1]))
        return torch.where((valid != 0)[..., None], centre, torch.zeros_like(centre)).reshape(centre.shape[0], -1).contiguous()

    def _targets(self, target, vis, N):
        dev = self._dev()
        target = torch.as_tensor(np.ascontiguousarray(target, dtype=np.float64) if not torch.is_tensor(target) else target).to(dev, torch.float64)
        vis = torch.as_tensor(vis).to(dev)
        if target.dim() != 3 or target.shape[0] != N or target.shape[2] != 2 or tuple(vis.shape) != tuple(target.shape[:2]):
            raise ValueError("LandmarkRegressor: target [{},K,2] and vis [N,K] (got {} and {})".format(N, tuple(target.shape), tuple(vis.shape)))
        if not 1 <= target.shape[1] <= ops.LANDMARK_MAX_K:
            raise ValueError("LandmarkRegressor: 1 <= K <= {} keypoints (got {})".format(ops.LANDMARK_MAX_K, target.shape[1]))
        return target.contiguous(), (vis != 0).to(torch.uint8).contiguous()

    def fit(self, centre, valid, target, vis, ridge=1e-6):
        """centre [N,P,2], valid [N,P], target [N,K,2] on [-1, 1], vis [N,K]: ups_landmark_gram + ups_landmark_solve.  A keypoint that
        is never visible, or whose system has a pivot that is not positive, gets W_k = 0 and counts in ``n_singular``.  Returns self."""
        feat = self._features(centre, valid)
        target, vis = self._targets(target, vis, feat.shape[0])
        G, R, cnt = ops.landmark_gram(feat, target, vis)
        W, ns = ops.landmark_solve(G, R, cnt, float(ridge))
        self.W, self.cnt, self.n_singular = W.cpu().numpy(), cnt.cpu().numpy(), int(ns.item())
        self.options = dict(self.options, ridge=float(ridge))
        return self

    def _W(self, P):
        if self.W is None:
            raise ValueError("LandmarkRegressor: fit or load first")
        if self.W.shape[1] != 2 * P + 1:
            raise ValueError("LandmarkRegressor: fitted on {} parts, asked about {}".format((self.W.shape[1] - 1) // 2, P))
        return torch.from_numpy(self.W).to(self._dev())

    def predict(self, centre, valid):
        """-> NumPy [N,K,2] float64 on [-1, 1]."""
        feat = self._features(centre, valid)
        return ops.landmark_predict(feat, self._W(feat.shape[1] // 2))[0].cpu().numpy()

    def squared_distances(self, centre, valid, target, vis):
        """-> (pred [N,K,2], d2 [N,K]) as NumPy arrays: ups_landmark_predict's outputs (d2 = -1 where not visible)."""
        feat = self._features(centre, valid)
        target, vis = self._targets(target, vis, feat.shape[0])
        pred, d2 = ops.landmark_predict(feat, self._W(feat.shape[1] // 2), target, vis)
        return pred.cpu().numpy(), d2.cpu().numpy()

    def evaluate(self, centre, valid, target, vis, pck=(0.05, 0.1)):
        """``metrics_from_d2`` of this regressor's predictions: per keypoint n_visible, mean_error and pck@t, their means over the
        keypoints, mean_error_instances over the visible instances, n_singular (of the fit)."""
        return metrics_from_d2(self.squared_distances(centre, valid, target, vis)[1], list(pck), self.n_singular)

    def save(self, path):
        """regressor.npz: W, cnt, singular (the fit's n_singular), options (a JSON string).  The same regressor gives the same bytes."""
        if self.W is None:
            raise ValueError("LandmarkRegressor: fit or load first")
        save_npz(path, W=self.W, cnt=self.cnt, singular=np.array(self.n_singular, dtype=np.int32),
                 options=np.array(json.dumps(self.options, sort_keys=True)))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path) as z:
            return cls(z["W"], z["cnt"], int(z["singular"]), json.loads(str(z["options"])), device=device)


# ---------------------------------------------------------------------------------------------- the runner's route (--landmarks)
def _centres_of(model, cfg, rels, opt):
    """Every image of `rels` (decoded as --segment decodes: PIL, bilinear to S x S, / 127.5 - 1) through ``part_centres`` in passes of
    2 * batch_size.  -> (centre [N,P,2] float64, valid [N,P] uint8, sizes [N,2] int64 = (h, w) of the source files)."""
    from PIL import Image
    S, B = int(cfg["spatial_size"]), int(cfg["batch_size"])
    centre, valid, sizes = [], [], []
    for c0 in range(0, len(rels), 2 * B):
        u8 = []
        for rel in rels[c0:c0 + 2 * B]:
            im = Image.open(os.path.join(cfg["data_root"], rel)).convert("RGB")
            sizes.append((im.size[1], im.size[0]))
            u8.append(np.asarray(im.resize((S, S), Image.BILINEAR), dtype=np.uint8))
        r = model.part_centres(torch.from_numpy(np.stack(u8).astype(np.float32) / 127.5 - 1.0), source=opt["source"],
                               min_part_area=opt["min_part_area"])
        centre.append(r["centre"].cpu().numpy())
        valid.append(r["valid"].cpu().numpy())
    return np.concatenate(centre), np.concatenate(valid), np.asarray(sizes, dtype=np.int64)


def _split(cfg, path):
    rels, xy, vis = read_landmark_csv(path)
    for rel in rels:
        if not os.path.isfile(os.path.join(cfg["data_root"], rel)):
            raise FileNotFoundError("--landmarks: {} (listed in {}) does not exist".format(os.path.join(cfg["data_root"], rel), path))
    return {"files": rels, "xy": xy, "vis": vis}


def landmark_files(model, cfg, odir):
    """The --landmarks route: the part centres of the images of `landmark_fit_csv` and `landmark_test_csv`, the regressor fitted on
    the first and evaluated on the second (on the first when there is no second: the summary then says "fit error"), written into
    `odir`: regressor.npz, landmarks.csv (one row per keypoint), summary.yml and predictions.npz (the test predictions in source
    pixels, the test centres, valid and files).  Two runs write the same bytes.  Returns {"regressor", "summary", "predictions"}."""
    import yaml
    opt = landmark_options(cfg)
    if 2 * model.n_parts + 1 > ops.LANDMARK_MAX_D:
        raise ValueError("--landmarks: at most {} parts (n_parts = {})".format((ops.LANDMARK_MAX_D - 1) // 2, model.n_parts))
    fit = _split(cfg, opt["fit_csv"])
    test = fit if opt["test_csv"] is None else _split(cfg, opt["test_csv"])      # (every file is checked before any pass)
    K = fit["xy"].shape[1]
    if test["xy"].shape[1] != K:
        raise ValueError("--landmarks: {} has {} keypoints, {} has {}".format(opt["fit_csv"], K, opt["test_csv"], test["xy"].shape[1]))
    if K > ops.LANDMARK_MAX_K:
        raise ValueError("--landmarks: at most {} keypoints (got {})".format(ops.LANDMARK_MAX_K, K))
    if opt["names"] is not None and len(opt["names"]) != K:
        raise ValueError("landmark_names: {} names for {} keypoints".format(len(opt["names"]), K))
    for part in ((fit,) if test is fit else (fit, test)):
        part["centre"], part["valid"], part["sizes"] = _centres_of(model, cfg, part["files"], opt)
        part["target"] = normalise_targets(part["xy"], part["sizes"])
    reg = LandmarkRegressor(device=model.device, options={k: opt[k] for k in ("source", "min_part_area", "pck")})
    reg.fit(fit["centre"], fit["valid"], fit["target"], fit["vis"], ridge=opt["ridge"])
    pred, d2 = reg.squared_distances(test["centre"], test["valid"], test["target"], test["vis"])
    res = metrics_from_d2(d2, opt["pck"], reg.n_singular)
    names = opt["names"] or ["keypoint_{}".format(k) for k in range(K)]
    keys = ["pck@{:g}".format(t) for t in opt["pck"]]
    os.makedirs(odir, exist_ok=True)
    reg.save(os.path.join(odir, "regressor.npz"))
    with open(os.path.join(odir, "landmarks.csv"), "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["keypoint", "name", "n_fit", "n_visible", "mean_error"] + keys)
        for k, row in enumerate(res["keypoints"]):
            wr.writerow([k, names[k], int(reg.cnt[k]), row["n_visible"]] + ["" if row[c] is None else repr(row[c]) for c in ["mean_error"] + keys])
    summary = {"split": "fit" if test is fit else "test", "error": "fit error" if test is fit else "test error",
               "n_fit": len(fit["files"]), "n_test": len(test["files"]), "n_keypoints": K, "n_parts": int(model.n_parts),
               "source": opt["source"], "min_part_area": opt["min_part_area"], "ridge": opt["ridge"],
               "mean_error": res["mean_error"], "mean_error_instances": res["mean_error_instances"], "n_visible": res["n_visible"],
               "n_singular": res["n_singular"], "keypoints": [dict(row, name=names[k]) for k, row in enumerate(res["keypoints"])]}
    summary.update({key: res[key] for key in keys})
    with open(os.path.join(odir, "summary.yml"), "w") as f:
        yaml.safe_dump(summary, f, default_flow_style=False, sort_keys=True)
    predictions = {"pred": to_source_pixels(pred, test["sizes"]), "centre": test["centre"], "valid": test["valid"],
                   "files": np.array(test["files"])}
    save_npz(os.path.join(odir, "predictions.npz"), **predictions)
    return {"regressor": reg, "summary": summary, "predictions": predictions}
