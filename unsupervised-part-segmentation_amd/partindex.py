"""Part-appearance index: per-part nearest neighbours and k-means on the bank of appearance codes ``TrainModel.encode_parts`` returns.

The two questions the appearance code exists for -- "which images have a part that looks like this one?" and "what kinds of
appearance does part p take across the data set?" -- the reference answers off-line (deepfashion/code/eval/eval_02: ``make_clusters``,
scikit-learn on a pickle of model outputs).  Here the arithmetic on the bank is two HIP kernels (csrc/partindex.hip through
``ops.part_knn`` / ``ops.part_kmeans_step``): fp64 direct squared distances, no distance matrix, results equal from run to run and to
the NumPy restatement of tests/partindex_ref.py.  The host keeps what is not hot: the seeding, the Lloyd loop's control (one int32
read per iteration), the files and the contact sheets.  Definitions: include/upsparts_hip.h, "part-appearance index".
"""
import csv
import math
import os
import pickle

import numpy as np
import torch

from . import lib as L
from . import ops

INITS = ("kmeans++", "random")


def channel_sum_of_squares(f64):
    """sum_a f64[.., a]^2 accumulated in ascending a from 0.0 (the order of the kernels' distance)."""
    acc = np.zeros(f64.shape[:-1], dtype=np.float64)
    for a in range(f64.shape[-1]):
        acc = acc + f64[..., a] * f64[..., a]
    return acc


def save_npz(path, **arrays):
    """np.savez with a fixed time stamp in the archive: the same arrays give the same bytes (np.load reads it as any .npz)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


class PartIndex(object):
    """A bank of part codes: feat [N,P,A] float32, valid [N,P] (an entry that is not valid -- an absent part -- is never a query, a
    neighbour or a cluster member), files: N names or None, area [N,P] int32 or None (kept for the files only).
    normalize=True divides every code by its float64 L2 norm, rounded to float32, before anything else (cosine ranking by the same
    kernels); a code of norm 0 becomes invalid.  The bank lives on the host; the kernels get a device copy on first use."""

    def __init__(self, feat, valid, files=None, area=None, normalize=False, device=None, normalized=False):
        feat = feat.detach().cpu().numpy() if torch.is_tensor(feat) else np.asarray(feat)
        valid = valid.detach().cpu().numpy() if torch.is_tensor(valid) else np.asarray(valid)
        if feat.ndim != 3 or feat.shape[0] < 1 or valid.shape != feat.shape[:2]:
            raise ValueError("PartIndex: feat [N >= 1,P,A] and valid [N,P] (got {} and {})".format(feat.shape, valid.shape))
        feat = np.ascontiguousarray(feat, dtype=np.float32)
        if not np.isfinite(feat).all():
            raise ValueError("PartIndex: the codes must be finite")
        valid = valid != 0
        if normalize:
            f64 = feat.astype(np.float64)
            norm = np.sqrt(channel_sum_of_squares(f64))
            ok = norm > 0
            feat = (f64 / np.where(ok, norm, 1.0)[..., None]).astype(np.float32)
            valid = valid & ok
        if files is not None and len(files) != feat.shape[0]:
            raise ValueError("PartIndex: {} file names for {} items".format(len(files), feat.shape[0]))
        self.feat, self.valid = feat, np.ascontiguousarray(valid.astype(np.uint8))
        self.files = None if files is None else [str(f) for f in files]
        self.area = None if area is None else np.ascontiguousarray(
            area.detach().cpu().numpy() if torch.is_tensor(area) else area, dtype=np.int32)
        self.normalized = bool(normalize or normalized)
        self.device = device
        self._dev = None

    N = property(lambda self: self.feat.shape[0])
    P = property(lambda self: self.feat.shape[1])
    A = property(lambda self: self.feat.shape[2])

    def bank(self):
        """(feat, valid) on the device."""
        if self._dev is None:
            if not torch.cuda.is_available():
                raise L.UpsError("PartIndex: the index kernels need a HIP device (there is no host route)")
            dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            self._dev = (torch.from_numpy(self.feat).to(dev), torch.from_numpy(self.valid).to(dev))
        return self._dev

    # ------------------------------------------------------------------ neighbours
    def neighbours(self, K, queries=None):
        """(idx [Nq,P,K] int32, dist [Nq,P,K] float64) as NumPy arrays: per part the K nearest valid items of this bank for every valid
        query, ascending in (distance, index), padded with -1 / +inf.  queries: another PartIndex (with the same [P,A]) or None -- the
        bank itself, each item's own entry excluded."""
        g, gv = self.bank()
        if queries is None:
            idx, dist = ops.part_knn(g, gv, K=K)
        else:
            if (queries.P, queries.A) != (self.P, self.A):
                raise ValueError("PartIndex.neighbours: queries [P,A] = {} differ from the bank's {}".format(
                    (queries.P, queries.A), (self.P, self.A)))
            q, qv = queries.bank()
            idx, dist = ops.part_knn(q, qv, g, gv, K=K)
        return idx.cpu().numpy(), dist.cpu().numpy()

    # ------------------------------------------------------------------ k-means
    def assign(self, clusters):
        """(label [N,P] int32, mind [N,P] float64) of the items on centroids [P,k,A] float64: the first nearest centroid and its
        squared distance; -1 / +inf where invalid.  One assignment-only launch."""
        f, v = self.bank()
        r = ops.part_kmeans_step(f, v, torch.as_tensor(np.ascontiguousarray(clusters, dtype=np.float64)).to(f.device), accumulate=False)
        return r["label"].cpu().numpy(), r["mind"].cpu().numpy()

    def seed_centres(self, k, seed=1, init="kmeans++"):
        """Initial centroids [P,k,A] float64, a pure function of (bank, k, seed, init).  Part p draws from
        np.random.RandomState(seed * 1000 + p).  kmeans++: the first centre is a uniform draw among the valid items; centre j is the
        valid item at searchsorted(cumsum(mind over the valid items in index order), u * total, side="right"), clamped, with
        u = random_sample() and mind from an assignment-only launch on the j centres so far.  random: the first k of a permutation of
        the valid items.  A part with fewer than k valid items raises ValueError and names the part."""
        if init not in INITS:
            raise ValueError("init: one of {} (got {!r})".format(INITS, init))
        k = int(k)
        if not 1 <= k <= ops.PART_KMEANS_MAX_K:
            raise ValueError("k-means: 1 <= k <= {} (got {})".format(ops.PART_KMEANS_MAX_K, k))
        items = [np.flatnonzero(self.valid[:, p]) for p in range(self.P)]
        for p in range(self.P):
            if len(items[p]) < k:
                raise ValueError("k-means: part {} has {} valid items, fewer than k = {}".format(p, len(items[p]), k))
        rngs = [np.random.RandomState(int(seed) * 1000 + p) for p in range(self.P)]
        f64 = self.feat.astype(np.float64)
        cent = np.zeros((self.P, k, self.A), dtype=np.float64)
        if init == "random":
            for p in range(self.P):
                cent[p] = f64[items[p][rngs[p].permutation(len(items[p]))[:k]], p]
            return cent
        for p in range(self.P):
            cent[p, 0] = f64[items[p][rngs[p].randint(len(items[p]))], p]
        for j in range(1, k):
            mind = self.assign(cent[:, :j])[1]
            for p in range(self.P):
                cum = np.cumsum(mind[items[p], p])
                u = rngs[p].random_sample()
                at = min(int(np.searchsorted(cum, u * cum[-1], side="right")), len(items[p]) - 1)
                cent[p, j] = f64[items[p][at], p]
        return cent

    def kmeans(self, k, seed=1, init="kmeans++", max_iter=100):
        """Lloyd's algorithm for every part at once -> {"clusters" [P,k,A] float64, "labels" [P,N] int32 (-1: not valid), "counts"
        [P,k] int32, "inertia" [P] float64, "iterations"}.  Each iteration is one ups_part_kmeans_step (assignment, counts, feature
        sums, inertia, number of changed labels) and the new centroids sums / counts in fp64 on the device, an empty cluster keeping
        its centroid; it stops when no label changed or after max_iter steps.  One int32 read per iteration is the only
        synchronisation.  labels, counts and inertia are those of the last step; clusters are the centroids that step used (when it
        converged) or produced (at max_iter)."""
        max_iter = int(max_iter)
        if max_iter < 1:
            raise ValueError("k-means: max_iter >= 1 (got {})".format(max_iter))
        f, v = self.bank()
        cent = torch.from_numpy(self.seed_centres(k, seed, init)).to(f.device)
        prev = torch.full((self.N, self.P), -2, dtype=torch.int32, device=f.device)
        it = 0
        while it < max_iter:
            r = ops.part_kmeans_step(f, v, cent, prev)
            it += 1
            if int(r["changed"].item()) == 0:
                break
            has = (r["counts"] > 0)[..., None]
            cent = torch.where(has, r["sums"] / r["counts"].clamp(min=1).to(torch.float64)[..., None], cent)
            prev = r["label"]
        return {"clusters": cent.cpu().numpy(), "labels": np.ascontiguousarray(r["label"].cpu().numpy().T),
                "counts": r["counts"].cpu().numpy(), "inertia": r["inertia"].cpu().numpy(), "iterations": it}

    # ------------------------------------------------------------------ files
    def save(self, directory):
        """<directory>/features.npz (feat, valid, normalized and, when known, area) and, with file names, index.csv (file, area_<p>)."""
        os.makedirs(directory, exist_ok=True)
        arrays = {"feat": self.feat, "valid": self.valid, "normalized": np.array(self.normalized)}
        if self.area is not None:
            arrays["area"] = self.area
        save_npz(os.path.join(directory, "features.npz"), **arrays)
        if self.files is not None:
            with open(os.path.join(directory, "index.csv"), "w", newline="") as f:
                wr = csv.writer(f)
                wr.writerow(["file"] + (["area_{}".format(p) for p in range(self.P)] if self.area is not None else []))
                for i, name in enumerate(self.files):
                    wr.writerow([name] + ([int(a) for a in self.area[i]] if self.area is not None else []))

    @classmethod
    def load(cls, directory, device=None):
        with np.load(os.path.join(directory, "features.npz")) as z:
            feat, valid, normalized = z["feat"], z["valid"], bool(z["normalized"])
            area = z["area"] if "area" in z.files else None
        files, path = None, os.path.join(directory, "index.csv")
        if os.path.isfile(path):
            with open(path, newline="") as f:
                files = [row[0] for row in list(csv.reader(f))[1:]]
        return cls(feat, valid, files=files, area=area, device=device, normalized=normalized)


# ---------------------------------------------------------------------------------------------- the runner's route (--index)
INDEX_DEFAULTS = {"index_query_csv": None, "index_neighbours": 8, "index_clusters": 0, "index_min_part_area": 0.005,
                  "index_normalize": False, "index_init": "kmeans++", "index_seed": 1, "index_max_iter": 100, "index_sheets": True,
                  "index_n_vis": 20}
SHEET_HOST_BYTES = 8 << 30


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def index_options(cfg):
    """The `index_*` keys of a yaml, validated and with their defaults: {"csv", "query_csv", "neighbours", "clusters",
    "min_part_area", "normalize", "init", "seed", "max_iter", "sheets", "n_vis"}.  ValueError on anything else."""
    unknown = sorted(k for k in cfg if k.startswith("index_") and k != "index_csv" and k not in INDEX_DEFAULTS)
    if unknown:
        raise ValueError("--index: unknown key(s) {} (known: index_csv, {})".format(unknown, ", ".join(sorted(INDEX_DEFAULTS))))
    o = {k[len("index_"):]: cfg.get(k, d) for k, d in INDEX_DEFAULTS.items()}
    o["csv"] = cfg.get("index_csv")
    if not o["csv"] or not isinstance(o["csv"], str):
        raise ValueError("--index: `index_csv` (one image path per line, relative to data_root) is required")
    if o["query_csv"] is not None and (not isinstance(o["query_csv"], str) or not o["query_csv"]):
        raise ValueError("index_query_csv: a path (got {!r})".format(o["query_csv"]))
    if not _is_int(o["neighbours"]) or not 0 <= o["neighbours"] <= ops.PART_KNN_MAX_K:
        raise ValueError("index_neighbours: an integer in [0, {}], 0 = off (got {!r})".format(ops.PART_KNN_MAX_K, o["neighbours"]))
    if not _is_int(o["clusters"]) or not 0 <= o["clusters"] <= ops.PART_KMEANS_MAX_K:
        raise ValueError("index_clusters: an integer in [0, {}], 0 = off (got {!r})".format(ops.PART_KMEANS_MAX_K, o["clusters"]))
    a = o["min_part_area"]
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 <= float(a) <= 1.0:
        raise ValueError("index_min_part_area: a fraction of the image in [0, 1] (got {!r})".format(a))
    o["min_part_area"] = float(a)
    for key in ("normalize", "sheets"):
        if not isinstance(o[key], bool):
            raise ValueError("index_{}: true | false (got {!r})".format(key, o[key]))
    if o["init"] not in INITS:
        raise ValueError("index_init: kmeans++ | random (got {!r})".format(o["init"]))
    if not _is_int(o["seed"]) or o["seed"] < 0:
        raise ValueError("index_seed: an integer >= 0 (got {!r})".format(o["seed"]))
    for key in ("max_iter", "n_vis"):
        if not _is_int(o[key]) or o[key] < 1:
            raise ValueError("index_{}: an integer >= 1 (got {!r})".format(key, o[key]))
    if not o["neighbours"] and not o["clusters"] and not o["sheets"]:
        raise ValueError("--index: index_neighbours = 0, index_clusters = 0 and index_sheets = false leave nothing to compute")
    return o


def min_area_pixels(min_part_area, S):
    """valid[n, p] = area[n, p] >= ceil(min_part_area * S^2)."""
    return int(math.ceil(min_part_area * S * S))


def part_crop(view_u8, label_u8, p):
    """view x (argmax == p): uint8 [S,S,3]."""
    return view_u8 * (label_u8 == p)[..., None].astype(np.uint8)


def tile_sheet(rows, S, cols):
    """rows: lists of uint8 [S,S,3] crops (None: a black tile) -> one uint8 [len(rows) S, cols S, 3] sheet."""
    sheet = np.zeros((max(1, len(rows)) * S, cols * S, 3), dtype=np.uint8)
    for r, row in enumerate(rows):
        for c, tile in enumerate(row[:cols]):
            if tile is not None:
                sheet[r * S:(r + 1) * S, c * S:(c + 1) * S] = tile
    return sheet


def neighbour_sheet(q_views, q_labels, q_valid, g_views, g_labels, idx, p, n_vis):
    """One row per query for the first n_vis valid queries of part p: the query's part crop, then its K neighbours' crops."""
    K = idx.shape[2]
    rows = []
    for n in np.flatnonzero(q_valid[:, p])[:n_vis]:
        rows.append([part_crop(q_views[n], q_labels[n], p)] +
                    [part_crop(g_views[g], g_labels[g], p) if g >= 0 else None for g in idx[n, p]])
    return tile_sheet(rows, q_views.shape[1], K + 1)


def cluster_sheet(views, labels, members, p, n_vis):
    """One row of n_vis tiles: `members` (item indices, nearest the centroid first) as part crops."""
    return tile_sheet([[part_crop(views[n], labels[n], p) for n in members[:n_vis]]], views.shape[1], n_vis)


def _load_bank(model, cfg, csv_path, opt, keep):
    """Every image of `csv_path` (decoded as --segment decodes: PIL, bilinear to S x S, / 127.5 - 1) through encode_parts in passes of
    2 * batch_size.  Returns (PartIndex, views uint8 [N,S,S,3] | None, labels uint8 [N,S,S] | None)."""
    from PIL import Image
    from . import data as _data
    S, B = int(cfg["spatial_size"]), int(cfg["batch_size"])
    rels = _data.TransferData._read_list(csv_path)
    if not rels:
        raise ValueError("--index: {} lists no image".format(csv_path))
    for rel in rels:
        if not os.path.isfile(os.path.join(cfg["data_root"], rel)):
            raise FileNotFoundError("--index: {} (listed in {}) does not exist".format(os.path.join(cfg["data_root"], rel), csv_path))
    if keep and len(rels) * S * S * 4 > SHEET_HOST_BYTES:
        raise ValueError("--index: the contact sheets keep uint8 views and part maps of {} images at {} x {} on the host, more than "
                         "8 GB; set `index_sheets: False`".format(len(rels), S, S))
    feat, area = [], []
    views_u8 = np.empty((len(rels), S, S, 3), dtype=np.uint8) if keep else None
    labels_u8 = np.empty((len(rels), S, S), dtype=np.uint8) if keep else None
    for c0 in range(0, len(rels), 2 * B):
        u8 = np.stack([np.asarray(Image.open(os.path.join(cfg["data_root"], rel)).convert("RGB").resize((S, S), Image.BILINEAR),
                                  dtype=np.uint8) for rel in rels[c0:c0 + 2 * B]])
        r = model.encode_parts(torch.from_numpy(u8.astype(np.float32) / 127.5 - 1.0))
        feat.append(r["feat"].cpu().numpy())
        area.append(r["area"].cpu().numpy())
        if keep:
            views_u8[c0:c0 + len(u8)] = u8
            labels_u8[c0:c0 + len(u8)] = r["out_parts_hard"].to(torch.uint8).cpu().numpy()
    area = np.concatenate(area)
    index = PartIndex(np.concatenate(feat), area >= min_area_pixels(opt["min_part_area"], S), files=rels, area=area,
                      normalize=opt["normalize"], device=model.device)
    return index, views_u8, labels_u8


def index_files(model, cfg, odir):
    """The --index route: the bank of `index_csv` (and of `index_query_csv`), its neighbours and clusters, written into `odir`:
    features.npz, index.csv, neighbours.npz (idx, dist), clusters.p (the ``PartIndex.kmeans`` dict: `clusters` and `labels` are the
    two keys of eval_02's clusters.p, stacked over the parts) and, with index_sheets, neighbours/part<pp>.png and
    clusters/part<pp>_cluster<jj>.png.  Returns {"index", "neighbours", "clusters"}."""
    from PIL import Image
    opt = index_options(cfg)
    if opt["sheets"] and model.n_parts > 255:
        raise ValueError("--index: the contact sheets keep uint8 part maps (n_parts <= 255); set `index_sheets: False`")
    index, views, labels = _load_bank(model, cfg, opt["csv"], opt, opt["sheets"])
    queries, q_views, q_labels = (index, views, labels)
    if opt["query_csv"] is not None:
        queries, q_views, q_labels = _load_bank(model, cfg, opt["query_csv"], opt, opt["sheets"])
    os.makedirs(odir, exist_ok=True)            # (a missing image has raised by now: nothing is left behind)
    index.save(odir)
    out = {"index": index, "neighbours": None, "clusters": None}
    if opt["neighbours"]:
        idx, dist = index.neighbours(opt["neighbours"], None if queries is index else queries)
        save_npz(os.path.join(odir, "neighbours.npz"), idx=idx, dist=dist)
        out["neighbours"] = (idx, dist)
        if opt["sheets"]:
            os.makedirs(os.path.join(odir, "neighbours"), exist_ok=True)
            for p in range(index.P):
                sheet = neighbour_sheet(q_views, q_labels, queries.valid, views, labels, idx, p, opt["n_vis"])
                Image.fromarray(sheet).save(os.path.join(odir, "neighbours", "part{:02}.png".format(p)))
    if opt["clusters"]:
        res = index.kmeans(opt["clusters"], seed=opt["seed"], init=opt["init"], max_iter=opt["max_iter"])
        with open(os.path.join(odir, "clusters.p"), "wb") as f:
            pickle.dump(res, f, protocol=2)
        out["clusters"] = res
        if opt["sheets"]:
            os.makedirs(os.path.join(odir, "clusters"), exist_ok=True)
            label, mind = index.assign(res["clusters"])
            for p in range(index.P):
                for j in range(opt["clusters"]):
                    members = np.flatnonzero(label[:, p] == j)
                    members = members[np.lexsort((members, mind[members, p]))]
                    Image.fromarray(cluster_sheet(views, labels, members, p, opt["n_vis"])).save(
                        os.path.join(odir, "clusters", "part{:02}_cluster{:02}.png".format(p, j)))
    return out
