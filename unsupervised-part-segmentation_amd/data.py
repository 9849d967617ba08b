"""Data feeding for the runner: work-alikes of the reference's dataset classes (outside the hot path).

  * ``StochasticPairs``  -- eddata.stochastic_pair.StochasticPairs (external; used by the PennAction / DeepFashion yamls):
    a csv with at least ``character_id`` and ``relative_file_path_`` columns; example i = (image i, a random image j of
    the same character_id), both resized to ``spatial_size`` and scaled to [-1, 1]; ``data_avoid_identity`` excludes
    j = i when the character has more than one image; ``data_flip_h`` / ``data_flip_v`` flip BOTH views together.
  * ``AugmentedPair2``   -- cub/code/data/data.py:52-175 on top of it: adds ``view0_target`` (a copy of view0).  The
    appearance / shape augmentations (data_augment_appearance / data_augment_shape, both False in the shipped yaml) are the
    numpy restatement of the albumentations pipelines in ``augment.py`` (same transforms, defaults and sync rules; the
    sample stream is not albumentations').

  * ``TransferData``     -- final_eval/eval_transfer.py's dataset of the comparison matrix (row csv x column csv, one relative
    path per line), yielding whole BLOCKS (block_size row images, block_size column images) instead of block_size^2 pairs:
    ``TrainModel.transfer_matrix`` encodes each image once.

The exact resize filter / cropping of eddata's ``preprocess_image`` is not visible in the reference tree: bilinear resize
of the whole image is used (UNVERIFIED).  ``batches`` turns a dataset into the ``{"view0", "view1"[, "view0_target"]}``
float32 NHWC batches ``Trainer.iterate`` consumes, with a small thread pool for decoding.

Device-resident data (yaml ``data_on_device: True``; docs/design/surroundings.md 8c).  ``batches`` decodes and resizes 2 B files per
step.  ``preprocess_image`` is ``uint8 -> / 127.5 - 1``, so nothing is lost by decoding every file ONCE into a uint8 array
``[N,S,S,3]`` (``build_u8_store``, optionally cached on disk under ``data_cache``) and keeping it in device memory.
``device_batches`` then draws the SAME pairs, flips and order as ``batches`` -- ``StochasticPairs.plan_example`` is the decision half
of ``get_example`` -- sends B x 3 int32 per step and lets ``ups_gather_views`` (csrc/dataset.hip) write the float32 views: the same
bits as the host path.  The label maps stay host-only; so do the albumentations-style augmentations unless
``data_augment_on_device: True``: then ``fill_aug_plan`` draws the host iterator's realisations (``augment.draw_appearance`` /
``draw_shape``) into one fixed-size record per output image and ``ups_augment_views`` (csrc/augment.hip) executes them -- the same
draws, pixels within two uint8 levels of the host path's (two of the host's transforms run in double precision inside scipy).
"""
import concurrent.futures as cf
import hashlib
import json
import os

import numpy as np
import torch

from .configs import DATA_AUGMENT_ON_DEVICE, DATA_ON_DEVICE


def add_choices(character_ids):
    """cub/code/data/data.py:31-50: for every row the indices of all rows with the same character_id."""
    cid = np.asarray(character_ids)
    by_cid = {c: np.nonzero(cid == c)[0] for c in np.unique(cid)}
    return [by_cid[c] for c in cid]


class StochasticPairs(object):
    n_images = 2

    def __init__(self, config):
        import pandas as pd
        self.config = config
        self.size = config.get("spatial_size", 256)
        self.root = config["data_root"]
        cols = config.get("data_csv_columns", ["character_id", "relative_file_path_"])
        header = 0 if config.get("data_csv_has_header", False) else None
        df = pd.read_csv(config["data_csv"], header=header, names=cols if header is None else None)
        if header == 0:
            df.columns = list(cols)[:len(df.columns)]
        self.labels = {c: df[c].tolist() for c in df.columns}
        self.labels["file_path_"] = [os.path.join(self.root, p) for p in self.labels["relative_file_path_"]]
        self.labels["choices"] = add_choices(self.labels["character_id"])
        self.avoid_identity = config.get("data_avoid_identity", True)
        self.flip_h, self.flip_v = config.get("data_flip_h", False), config.get("data_flip_v", False)
        self.seed = int(config.get("data_seed", 1))
        self.prng = np.random.RandomState(self.seed)          # (kept for callers that draw from the dataset-wide stream)
        self.draws = {}                                        # index -> number of examples drawn so far
        # optional ground-truth label maps for evaluation (eval_01.py:229-383 reads them as batch["gt_segmentation"]):
        # a csv column with the relative path of a label image (nearest-neighbour resized like denseposelib.resize_labels)
        self.gt_column = config.get("data_gt_segmentation_column")

    def __len__(self):
        return len(self.labels["character_id"])

    def preprocess_u8(self, path):
        """The decoded, resized image as uint8 [S,S,3]: what ``preprocess_image`` normalises and what the device store keeps."""
        from PIL import Image
        img = Image.open(path).convert("RGB").resize((self.size, self.size), Image.BILINEAR)
        return np.asarray(img, dtype=np.uint8)

    def preprocess_image(self, path):
        return self.preprocess_u8(path).astype(np.float32) / 127.5 - 1.0

    def _rng(self, i):
        """Per-index, per-draw generator: examples are decoded by a thread pool, so partner and flip decisions must not
        depend on which thread reaches a shared stream first (reproducible pairings)."""
        k = self.draws.get(int(i), 0)
        self.draws[int(i)] = k + 1
        return np.random.RandomState([self.seed & 0x7fffffff, int(i), k])

    def pick_partner(self, i, rng=None):
        rng = rng if rng is not None else self._rng(i)
        choices = self.labels["choices"][i]
        if self.avoid_identity and len(choices) > 1:
            choices = [c for c in choices if c != i]
        return int(rng.choice(choices))

    def preprocess_labels(self, path):
        from PIL import Image
        return np.asarray(Image.open(path).resize((self.size, self.size), Image.NEAREST), dtype=np.int64)

    def plan_example(self, i):
        """The decisions of example i without its pixels: (i, partner j, flip_h, flip_v).  Draws from ``_rng(i)`` in a fixed order --
        the partner, the horizontal draw (only with ``data_flip_h``), the vertical draw (only with ``data_flip_v``) -- so the host
        path (``get_example``) and the device path (``device_batches``) see the same examples."""
        rng = self._rng(i)
        j = self.pick_partner(i, rng)
        flip_h = bool(self.flip_h and rng.rand() < 0.5)
        flip_v = bool(self.flip_v and rng.rand() < 0.5)
        return int(i), j, flip_h, flip_v

    def get_example(self, i):
        i, j, flip_h, flip_v = self.plan_example(i)
        view0 = self.preprocess_image(self.labels["file_path_"][i])
        view1 = self.preprocess_image(self.labels["file_path_"][j])
        if flip_h:
            view0, view1 = view0[:, ::-1].copy(), view1[:, ::-1].copy()
        if flip_v:
            view0, view1 = view0[::-1].copy(), view1[::-1].copy()
        ex = {"view0": view0, "view1": view1}
        if self.gt_column and self.gt_column in self.labels:
            gt = self.preprocess_labels(os.path.join(self.root, self.labels[self.gt_column][i]))
            if flip_h:
                gt = gt[:, ::-1].copy()
            if flip_v:
                gt = gt[::-1].copy()
            ex["gt_segmentation"] = gt
        return ex


class AugmentedPair2(StochasticPairs):
    n_images = 3

    def __init__(self, config):
        super(AugmentedPair2, self).__init__(config)
        self.use_appearance_augmentation = config.get("data_augment_appearance", False)       # data.py:56-57
        self.use_shape_augmentation = config.get("data_augment_shape", False)

    def get_example(self, i):
        from . import augment
        ex = super(AugmentedPair2, self).get_example(i)
        view0, view1 = ex["view0"], ex["view1"]
        target = view0.copy()                           # data.py:164
        if self.use_appearance_augmentation or self.use_shape_augmentation:
            rng = np.random.RandomState([self.seed & 0x7fffffff, int(i), self.draws[int(i)], 7])
            if self.use_appearance_augmentation:        # data.py:167-169: view1 and the target share one realisation
                view0, = augment.stochastic_appearance_augmentation(rng, view0)
                view1, target = augment.stochastic_appearance_augmentation(rng, view1, target)
            if self.use_shape_augmentation:             # data.py:171-173: view0 and the target share one realisation
                view0, target = augment.stochastic_shape_augmentation(rng, view0, target)
                view1, = augment.stochastic_shape_augmentation(rng, view1)
        ex.update(view0=view0, view1=view1, view0_target=target)
        return ex


class TransferData(object):
    """Blocks of the comparison matrix.  ``data_row_csv`` / ``data_col_csv`` list one path per line, relative to ``data_root``;
    block b pairs rows [b * bs, (b + 1) * bs) with columns of the same range, bs = ``data_block_size`` (default ``batch_size``), and
    there are min(n_rows, n_cols) // bs blocks (the reference's length rule: its dataset has that many times bs * bs pairs).
    ``get_block(b)`` -> {"matrix": b, "rows" / "cols": float32 [bs,S,S,3] in [-1, 1], "row_paths" / "col_paths": the csv lines}."""

    def __init__(self, config):
        self.size = config["spatial_size"]
        self.root = config["data_root"]
        self.block_size = int(config.get("data_block_size", config["batch_size"]))
        self.row_paths = self._read_list(config["data_row_csv"])
        self.col_paths = self._read_list(config["data_col_csv"])
        self.n_rows, self.n_cols = len(self.row_paths), len(self.col_paths)
        self.n_blocks = min(self.n_rows, self.n_cols) // self.block_size

    @staticmethod
    def _read_list(path):
        with open(path) as f:                   # (a missing csv raises FileNotFoundError: the runner's "data is not there")
            return [line for line in f.read().splitlines() if line.strip()]

    def __len__(self):
        """Number of (row, column) cells, as the reference's pair dataset counts them."""
        return self.n_blocks * self.block_size * self.block_size

    def cell(self, k):
        """Cell k of the reference's flat ordering -> (matrix, block row, block column, row image index, column image index)."""
        bs = self.block_size
        b, r = divmod(int(k), bs * bs)
        bi, bj = divmod(r, bs)
        return b, bi, bj, b * bs + bi, b * bs + bj

    def preprocess_image(self, path):
        from PIL import Image
        img = Image.open(path).convert("RGB").resize((self.size, self.size), Image.BILINEAR)
        return np.asarray(img, dtype=np.float32) / 127.5 - 1.0

    def get_block(self, b):
        if not 0 <= b < self.n_blocks:
            raise IndexError("block {} of {}".format(b, self.n_blocks))
        sl = slice(b * self.block_size, (b + 1) * self.block_size)
        rp, cp = self.row_paths[sl], self.col_paths[sl]
        return {"matrix": b, "row_paths": rp, "col_paths": cp,
                "rows": np.stack([self.preprocess_image(os.path.join(self.root, p)) for p in rp]),
                "cols": np.stack([self.preprocess_image(os.path.join(self.root, p)) for p in cp])}

    def __iter__(self):
        return (self.get_block(b) for b in range(self.n_blocks))


def batches(dataset, batch_size, shuffle=True, workers=8, seed=0, epochs=None, pad_last=False):
    """Endless (or ``epochs``-bounded) iterator of float32 NHWC torch batches.  The model's batch size is static
    (model.py:320): in training the ragged last batch of an epoch is dropped; with ``pad_last`` (evaluation) it is filled up
    by repeating its last example and carries ``"valid": n`` so that the caller keeps only the first n rows."""
    rng = np.random.RandomState(seed)
    pool = cf.ThreadPoolExecutor(max_workers=workers)
    ep = 0
    while epochs is None or ep < epochs:
        order = rng.permutation(len(dataset)) if shuffle else np.arange(len(dataset))
        nb = -(-len(order) // batch_size) if pad_last else len(order) // batch_size
        for b in range(nb):
            idx = list(order[b * batch_size:(b + 1) * batch_size])
            valid = len(idx)
            idx += [idx[-1]] * (batch_size - valid)
            exs = [dataset.get_example(i) for i in idx] if workers <= 1 else list(pool.map(dataset.get_example, idx))
            out = {k: torch.from_numpy(np.stack([e[k] for e in exs])) for k in exs[0]}
            if pad_last:
                out["valid"] = valid
            yield out
        ep += 1


# ------------------------------------------------------------------ device-resident data
MAX_STORE_WORKERS = 16          # decoding threads of build_u8_store: a fixed cap, never the machine's CPU count


def _store_key(dataset):
    """What a cached store must have been built from: row count, size and the csv's path column."""
    paths = "\n".join(str(p) for p in dataset.labels["relative_file_path_"])
    return {"N": len(dataset), "spatial_size": int(dataset.size), "sha1": hashlib.sha1(paths.encode("utf-8")).hexdigest()}


def _cache_paths(cache):
    npy = cache if cache.endswith(".npy") else cache + ".npy"
    return npy, npy[:-len(".npy")] + ".json"


AUG_KEYS = ("data_augment_appearance", "data_augment_shape")


def augment_on_device(cfg):
    return bool(cfg.get("data_augment_on_device", DATA_AUGMENT_ON_DEVICE["data_augment_on_device"]))


def check_augment_on_device(cfg):
    """``data_augment_on_device`` without ``data_on_device`` is a ValueError naming both keys (``runner.make_dataset`` asks before it
    chooses the iterator; on the device path ``check_on_device`` refuses a dataset that is not an ``AugmentedPair2``)."""
    if augment_on_device(cfg) and not cfg.get("data_on_device", DATA_ON_DEVICE["data_on_device"]):
        raise ValueError("data_augment_on_device needs data_on_device: True (it is a route of the device-resident data path)")


def check_on_device(dataset):
    """The refusals of ``data_on_device`` (ValueError, before a file or the device is touched): host-only transforms, and a store
    that would not fit ``data_on_device_max_gb``.  There is no silent fall-back to the host path.  ``data_augment_on_device: True``
    lifts the refusal of the two augmentation switches on an ``AugmentedPair2`` (the label maps stay refused)."""
    cfg = dataset.config
    on_device = augment_on_device(cfg)
    if on_device and not isinstance(dataset, AugmentedPair2):
        raise ValueError("data_augment_on_device with data_on_device: {} is not an AugmentedPair2, the only dataset with "
                         "data_augment_appearance / data_augment_shape".format(type(dataset).__name__))
    host_only = [] if on_device else [k for k in AUG_KEYS if cfg.get(k, False)]
    if dataset.gt_column:
        host_only.append("data_gt_segmentation_column")
    if host_only:
        raise ValueError("data_on_device cannot be combined with {}: those transforms / label maps exist on the host path only "
                         "(set data_on_device: False, or drop them)".format(", ".join(host_only)))
    nbytes = len(dataset) * int(dataset.size) ** 2 * 3
    max_gb = float(cfg.get("data_on_device_max_gb", DATA_ON_DEVICE["data_on_device_max_gb"]))
    if nbytes > max_gb * 1e9:
        raise ValueError("data_on_device: the uint8 store of {} images at {}x{} is {:.6g} GB, more than data_on_device_max_gb = {:g} GB"
                         .format(len(dataset), dataset.size, dataset.size, nbytes / 1e9, max_gb))


def build_u8_store(dataset, cache=None, workers=8):
    """Every row of the dataset's csv decoded ONCE: uint8 [N,S,S,3] (``dataset.preprocess_u8``, a pool of at most 16 threads).
    ``cache`` (yaml ``data_cache``): the array is kept as ``<cache>.npy`` beside ``<cache>.json`` = {N, spatial_size, sha1 of the joined
    ``relative_file_path_`` column}; a cache whose sidecar matches is loaded without opening an image, any other is rebuilt, never used."""
    key = _store_key(dataset)
    shape = (key["N"], key["spatial_size"], key["spatial_size"], 3)
    if cache:
        npy, side = _cache_paths(cache)
        try:
            with open(side) as f:
                found = json.load(f)
            if found == key:
                store = np.load(npy)
                if store.dtype == np.uint8 and store.shape == shape:
                    return store
        except (OSError, ValueError):
            pass                    # no cache, or an unreadable one: build it
    paths = dataset.labels["file_path_"]
    workers = max(1, min(int(workers), MAX_STORE_WORKERS))
    store = np.empty(shape, dtype=np.uint8)
    with cf.ThreadPoolExecutor(max_workers=workers) as pool:
        for i, img in enumerate(pool.map(dataset.preprocess_u8, paths)):
            store[i] = img
    if cache:
        # the sidecar goes first and comes back last: whatever interrupts the two writes leaves no sidecar that vouches for the
        # wrong array.  Both are written under a temporary name and renamed (several ranks may build the same cache at once).
        if os.path.dirname(npy):
            os.makedirs(os.path.dirname(npy), exist_ok=True)
        if os.path.exists(side):
            os.remove(side)
        tmp = "{}.tmp-{}".format(npy, os.getpid())
        with open(tmp, "wb") as f:
            np.save(f, store)
        os.replace(tmp, npy)
        with open(tmp, "w") as f:
            json.dump(key, f)
        os.replace(tmp, side)
    return store


def fill_plan(dataset, idx, plan):
    """plan [B,3] int32 (a NumPy view) <- (view0 source, view1 source, flip bits: 1 horizontal | 2 vertical) of the examples `idx`,
    drawn in order by ``plan_example``.  Every index is checked against the store's row count here, on the host."""
    n = len(dataset)
    for r, i in enumerate(idx):
        i, j, fh, fv = dataset.plan_example(i)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("data_on_device: example ({}, {}) is outside the store of {} images".format(i, j, n))
        plan[r, 0], plan[r, 1], plan[r, 2] = i, j, int(fh) | (int(fv) << 1)


PLAN_RING = 4                   # pinned plan buffers in flight (a copy is waited for only when its buffer comes round again)

# ---- the record of one output image of the augmented route: int32 words, floats by bit pattern (csrc/augment.hip R_*)
REC_WORDS = 272
REC_SRC, REC_FLIP, REC_MID, REC_FILTER, REC_COLOR, REC_CPAR, REC_GRAY, REC_PERM, REC_PIDX = 0, 1, 2, 3, 4, 7, 16, 17, 18
REC_HFLIP, REC_AFFINE, REC_WARP, REC_FIELD, REC_AMAT, REC_EMAT, REC_JY, REC_JX, REC_BC = 21, 22, 23, 24, 32, 38, 44, 60, 76
FILTER_CODE = {"median": 1, "box": 2}
COLOR_CODE = {"bc": 1, "rgb": 2, "hsv": 3}
GAUSS_SIGMA, GAUSS_RADIUS = 50.0, 200          # ElasticTransform's field: scipy's truncate = 4 sigma


def aug_luts():
    """uint8 [2,256]: T_in[u] = _to_u8(float32(u) / 127.5 - 1), what ``preprocess_image`` followed by a pipeline's first cast gives, and
    T_mid[v] = _to_u8(_from_u8(v)), the round trip between the two pipelines -- augment.py's own expressions."""
    from . import augment
    u = np.arange(256, dtype=np.uint8)
    return np.stack([augment._to_u8(u.astype(np.float32) / 127.5 - 1.0), augment._to_u8(augment._from_u8(u))])


def gauss_weights(sigma=GAUSS_SIGMA, radius=GAUSS_RADIUS):
    """The 2 * radius + 1 weights of scipy's gaussian_filter1d: float64, normalised, rounded to float32."""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return (w / w.sum()).astype(np.float32)


def write_appearance(rec, recs):
    """The records of ``augment.draw_appearance`` into one image's int32 record (a NumPy view of REC_WORDS words)."""
    slot = 0
    for r in recs:
        kind = r[0]
        if kind in FILTER_CODE:
            rec[REC_FILTER] = FILTER_CODE[kind]
        elif kind in COLOR_CODE:
            rec[REC_COLOR + slot] = COLOR_CODE[kind]
            if kind == "bc":
                rec[REC_BC + 64 * slot:REC_BC + 64 * (slot + 1)] = np.asarray(r[1], dtype=np.uint8).view(np.int32)
            else:
                rec[REC_CPAR + 3 * slot:REC_CPAR + 3 * slot + 3] = r[1] if kind == "rgb" else r[1:]
            slot += 1
        elif kind == "gray":
            rec[REC_GRAY] = 1
        elif kind == "perm":
            rec[REC_PERM] = 1
            rec[REC_PIDX:REC_PIDX + 3] = r[1]
        else:
            raise ValueError("unknown appearance record {!r}".format(kind))


def write_shape(rec, recs, field):
    """The records of ``augment.draw_shape`` into one image's record; `field` is the index of the realisation's elastic noise."""
    f32 = rec.view(np.float32)
    for r in recs:
        kind = r[0]
        if kind == "hflip":
            rec[REC_HFLIP] = 1
        elif kind == "affine":
            rec[REC_AFFINE] = 1
            f32[REC_AMAT:REC_AMAT + 6] = r[1].reshape(6)
        elif kind == "grid":
            rec[REC_WARP] = 1
            f32[REC_JY:REC_JY + 16], f32[REC_JX:REC_JX + 16] = r[1].reshape(16), r[2].reshape(16)
        elif kind == "elastic":
            rec[REC_WARP], rec[REC_FIELD] = 2, field
            f32[REC_EMAT:REC_EMAT + 6] = r[1].reshape(6)
        else:
            raise ValueError("unknown shape record {!r}".format(kind))


def fill_aug_plan(dataset, idx, recs, noise):
    """recs [3,B,REC_WORDS] int32 and noise [>= 2 B,2,S,S] float32 (NumPy views of pinned buffers) <- the examples `idx` of an
    ``AugmentedPair2``: ``plan_example`` as in ``fill_plan``, then the generator of ``get_example`` --
    RandomState([seed, i, draws[i], 7]), draws[i] read AFTER plan_example incremented it -- drawn in the host's order: A1 appearance of
    view0, A2 appearance shared by view1 and the target, S3 shape shared by view0 and the target, S4 shape of view1, each kind only when
    its switch is on.  Role r of item b is recs[r, b] (0 view0, 1 view1, 2 target).  Returns the number of elastic noise pairs written
    (noise[e] = (dx, dy) of one elastic realisation, S3's shared by its two images).  Nothing per pixel happens here but those draws."""
    from . import augment
    n, S = len(dataset), int(dataset.size)
    app, shp = bool(dataset.use_appearance_augmentation), bool(dataset.use_shape_augmentation)
    recs[...] = 0
    n_el = 0
    for b, i in enumerate(idx):
        i, j, fh, fv = dataset.plan_example(i)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("data_on_device: example ({}, {}) is outside the store of {} images".format(i, j, n))
        recs[:, b, REC_SRC] = (i, j, i)
        recs[:, b, REC_FLIP] = int(fh) | (int(fv) << 1)
        recs[:, b, REC_MID] = int(app and shp)
        rng = np.random.RandomState([dataset.seed & 0x7fffffff, int(i), dataset.draws[int(i)], 7])
        if app:
            write_appearance(recs[0, b], augment.draw_appearance(rng))
            a2 = augment.draw_appearance(rng)
            write_appearance(recs[1, b], a2)
            write_appearance(recs[2, b], a2)
        if shp:
            for roles in ((0, 2), (1,)):
                drawn = augment.draw_shape(rng, S, S)
                for r in drawn:
                    if r[0] == "elastic":
                        noise[n_el, 0], noise[n_el, 1] = r[2], r[3]
                for role in roles:
                    write_shape(recs[role, b], drawn, n_el)
                n_el += any(r[0] == "elastic" for r in drawn)
    return n_el


def device_batches(dataset, batch_size, device, shuffle=True, seed=0, epochs=None):
    """``batches`` fed from device memory: the same ``RandomState(seed).permutation`` per epoch, the ragged last batch dropped, the
    same per-index draw counters -- and so the same tensors, bit for bit -- but float32 NHWC DEVICE tensors, freshly allocated per
    batch.  Per step the host draws the plan (``fill_plan``), copies its B x 3 int32 from a pinned buffer (non-blocking) and launches
    ``ups_gather_views`` on the current stream of `device`; nothing is decoded and the host never waits for the device.
    The store is built (or loaded from ``data_cache``) and uploaded HERE, not at the first ``next()``: the refusals of
    ``check_on_device`` and a missing image tree raise at construction.
    With ``data_augment_on_device`` and one of ``data_augment_appearance`` / ``data_augment_shape`` the batches take the augmented
    route (``fill_aug_plan`` + ``ups_augment_views``): the same order, partners, flips and draw counters, the host iterator's
    realisations, pixels within two uint8 levels of the host iterator's."""
    from . import lib as L
    check_on_device(dataset)
    if batch_size < 1 or len(dataset) < batch_size:
        raise ValueError("data_on_device: batch_size {} with {} images gives no batch".format(batch_size, len(dataset)))
    device = torch.device(device)
    store = build_u8_store(dataset, cache=dataset.config.get("data_cache", DATA_ON_DEVICE["data_cache"]))
    images = torch.from_numpy(store).to(device)
    with_target = dataset.n_images == 3          # AugmentedPair2: view0_target = a copy of view0 (cub/code/data/data.py:164)
    if augment_on_device(dataset.config) and (dataset.use_appearance_augmentation or dataset.use_shape_augmentation):
        return _device_aug_batches(L, dataset, images, batch_size, device, shuffle, seed, epochs)
    return _device_batches(L, dataset, images, batch_size, device, shuffle, seed, epochs, with_target)


def _device_batches(L, dataset, images, batch_size, device, shuffle, seed, epochs, with_target):
    N, S = images.shape[0], images.shape[1]
    rng = np.random.RandomState(seed)
    ring = [torch.empty((batch_size, 3), dtype=torch.int32).pin_memory() for _ in range(PLAN_RING)]
    copied = [None] * PLAN_RING
    k, ep = 0, 0
    while epochs is None or ep < epochs:
        order = rng.permutation(N) if shuffle else np.arange(N)
        for b in range(len(order) // batch_size):
            slot = k % PLAN_RING
            k += 1
            if copied[slot] is not None:
                copied[slot].synchronize()       # (four batches old: long done)
            fill_plan(dataset, order[b * batch_size:(b + 1) * batch_size], ring[slot].numpy())
            with torch.cuda.device(device):
                plan = torch.empty((batch_size, 3), dtype=torch.int32, device=device)
                plan.copy_(ring[slot], non_blocking=True)
                copied[slot] = torch.cuda.Event()
                copied[slot].record()
                out = {key: torch.empty((batch_size, S, S, 3), dtype=torch.float32, device=device)
                       for key in (("view0", "view1", "view0_target") if with_target else ("view0", "view1"))}
                L.call("ups_gather_views", L.ptr(images), N, L.ptr(plan), batch_size, S, L.ptr(out["view0"]), L.ptr(out["view1"]),
                       L.ptr(out.get("view0_target")), L.stream())
            yield out
        ep += 1


def _device_aug_batches(L, dataset, images, batch_size, device, shuffle, seed, epochs):
    """The augmented route of ``device_batches``.  Pinned ring buffers hold the records [3,B,REC_WORDS] and the elastic noise
    [2 B,2,S,S] (at most two elastic realisations per example); both are copied non-blocking and the host never waits for the device.
    The uint8 scratch of the three passes, the device copy of the noise and the field buffers are allocated once and reused on the
    iterator's stream; records and views are fresh per batch."""
    N, S, B = images.shape[0], images.shape[1], batch_size
    if L.load().ups_augment_record_words() != REC_WORDS:
        raise L.UpsError("ups_augment_record_words() = {} but data.REC_WORDS = {}: rebuild the library".format(
            L.load().ups_augment_record_words(), REC_WORDS))
    rng = np.random.RandomState(seed)
    shape = bool(dataset.use_shape_augmentation)
    ring = [torch.zeros((3, B, REC_WORDS), dtype=torch.int32).pin_memory() for _ in range(PLAN_RING)]
    nring = [torch.zeros((2 * B if shape else 1, 2, S, S), dtype=torch.float32).pin_memory() for _ in range(PLAN_RING)]
    copied = [None] * PLAN_RING
    with torch.cuda.device(device):
        luts = torch.from_numpy(aug_luts()).to(device)
        weights = torch.from_numpy(gauss_weights()).to(device)
        scratch = torch.empty((2, 3 * B, S, S, 3), dtype=torch.uint8, device=device)
        fields = torch.empty((3, 2 * B if shape else 1, 2, S, S), dtype=torch.float32, device=device)     # noise, tmp, field
    k, ep = 0, 0
    while epochs is None or ep < epochs:
        order = rng.permutation(N) if shuffle else np.arange(N)
        for b in range(len(order) // B):
            slot = k % PLAN_RING
            k += 1
            if copied[slot] is not None:
                copied[slot].synchronize()       # (four batches old: long done)
            n_el = fill_aug_plan(dataset, order[b * B:(b + 1) * B], ring[slot].numpy(), nring[slot].numpy())
            with torch.cuda.device(device):
                recs = torch.empty((3, B, REC_WORDS), dtype=torch.int32, device=device)
                recs.copy_(ring[slot], non_blocking=True)
                if n_el:
                    fields[0, :n_el].copy_(nring[slot][:n_el], non_blocking=True)
                copied[slot] = torch.cuda.Event()
                copied[slot].record()
                if n_el:
                    L.call("ups_augment_field", L.ptr(fields[0]), L.ptr(weights), n_el, S, L.ptr(fields[1]), L.ptr(fields[2]), L.stream())
                out = {key: torch.empty((B, S, S, 3), dtype=torch.float32, device=device) for key in ("view0", "view1", "view0_target")}
                L.call("ups_augment_views", L.ptr(images), N, L.ptr(recs), L.ptr(luts), L.ptr(fields[2]), n_el, B, S, L.ptr(scratch[0]),
                       L.ptr(scratch[1]), L.ptr(out["view0"]), L.ptr(out["view1"]), L.ptr(out["view0_target"]), 7, L.stream())
            yield out
        ep += 1


# ------------------------------------------------------------------ validation set of `val_freq` (Trainer.validate)
class ValidationSet(object):
    """``val_csv`` decoded ONCE: uint8 views [n,S,S,3] and uint8 label maps [n,S,S] (pinned when a device is there), the first
    ``val_max_images`` rows (default 512) in csv order, no flips, no partners.  Every other key -- data_root, the csv columns,
    spatial_size, ``data_gt_segmentation_column`` (required) -- is the training dataset's."""

    def __init__(self, config, workers=8):
        from .evalutil import labels_u8
        col = config.get("data_gt_segmentation_column")
        if not config.get("val_csv") or not col:
            raise ValueError("val_freq needs `val_csv` and `data_gt_segmentation_column` (the csv column with the label images)")
        ds = StochasticPairs(dict(config, data_csv=config["val_csv"]))
        if col not in ds.labels:
            raise ValueError("val_csv {} has no column {}".format(config["val_csv"], col))
        n = min(len(ds), int(config.get("val_max_images", 512)))
        if n < 1:
            raise ValueError("val_csv {} lists no image".format(config["val_csv"]))
        S = int(ds.size)
        views, labels = np.empty((n, S, S, 3), dtype=np.uint8), np.empty((n, S, S), dtype=np.uint8)
        with cf.ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_STORE_WORKERS))) as pool:
            for i, img in enumerate(pool.map(ds.preprocess_u8, ds.labels["file_path_"][:n])):
                views[i] = img
            for i, lab in enumerate(pool.map(ds.preprocess_labels, [os.path.join(ds.root, q) for q in ds.labels[col][:n]])):
                labels[i] = labels_u8(lab)
        self.views, self.labels = torch.from_numpy(views), torch.from_numpy(labels)
        if torch.cuda.is_available():
            self.views, self.labels = self.views.pin_memory(), self.labels.pin_memory()

    def __len__(self):
        return self.views.shape[0]

    def float_views(self, c0, c1, device):
        """Views [c0, c1) as float32 [k,S,S,3] on `device`, current stream: the bytes are copied (non-blocking) and ``ups_gather_views``
        applies the host path's `u / 127.5 - 1` bit for bit (plan: image b -> view b, no flip)."""
        from . import lib as L
        u8 = self.views[c0:c1].to(device, non_blocking=True)
        k, S = u8.shape[0], u8.shape[1]
        plan = torch.arange(k, dtype=torch.int32, device=device)[:, None].repeat(1, 3)
        plan[:, 2] = 0
        out = torch.empty((2, k, S, S, 3), dtype=torch.float32, device=device)
        L.call("ups_gather_views", L.ptr(u8), k, L.ptr(plan), k, S, L.ptr(out[0]), L.ptr(out[1]), None, L.stream())
        return out[0]


def plan_validation_pairs(dataset, batch_size, max_images):
    """The fixed (pose row, appearance row) plan of a validation csv: rows 0 .. n-1 with n = floor(min(len, max_images) / B) * B, each
    with the partner ``plan_example`` draws for it on a fresh dataset (draw 0 of its per-index generator: it depends on the csv and
    the dataset's seed alone).  -> int32 [n,2].  n < B is a ValueError: only whole chunks of batch_size pairs run."""
    B = int(batch_size)
    n = min(len(dataset), int(max_images)) // B * B
    if n < B:
        raise ValueError("validation pairs: {} row(s) (val_max_images {}) give no whole chunk of batch_size {}".format(
            len(dataset), int(max_images), B))
    pairs = np.empty((n, 2), dtype=np.int32)
    for i in range(n):
        pairs[i] = dataset.plan_example(i)[:2]
    return pairs


class ValidationPairs(object):
    """``val_csv`` as (pose image, appearance image) pairs for the label-free metrics of `val_metrics` (Trainer.validate): the
    sibling of ``ValidationSet`` that needs no label column.  Partners are drawn ONCE, here, by ``plan_validation_pairs`` with
    ``data_seed = val_seed`` (default 1) and both flips off, so the plan is a function of the csv and ``val_seed``.  Every image a pair
    names is decoded once into a uint8 store [m,S,S,3] (pinned when a device is there); ``pairs`` [n,2] int32 indexes that store.
    ``chunk_views`` gives one chunk of batch_size pairs as float32 device views through ups_gather_views."""

    def __init__(self, config, workers=8):
        if not config.get("val_csv"):
            raise ValueError("val_metrics: reconstruction / parts need `val_csv`")
        self.batch_size = int(config["batch_size"])
        ds = StochasticPairs(dict(config, data_csv=config["val_csv"], data_seed=int(config.get("val_seed", 1)),
                                  data_flip_h=False, data_flip_v=False))
        self.rows = plan_validation_pairs(ds, self.batch_size, config.get("val_max_images", 512))     # indices into the csv
        used, inverse = np.unique(self.rows.reshape(-1), return_inverse=True)
        self.pairs = inverse.reshape(-1, 2).astype(np.int32)                                         # indices into the store
        S = int(ds.size)
        store = np.empty((len(used), S, S, 3), dtype=np.uint8)
        with cf.ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_STORE_WORKERS))) as pool:
            for k, img in enumerate(pool.map(ds.preprocess_u8, [ds.labels["file_path_"][int(r)] for r in used])):
                store[k] = img
        self.store = torch.from_numpy(store)
        if torch.cuda.is_available():
            self.store = self.store.pin_memory()
        self._dev = None

    def __len__(self):
        return self.pairs.shape[0]

    def chunks(self):
        return len(self) // self.batch_size

    def chunk_views(self, c, device):
        """Chunk c (pairs [c B, (c + 1) B)) -> {"view0", "view1"} float32 [B,S,S,3] on `device`, current stream: the host path's
        `u / 127.5 - 1` bit for bit (ups_gather_views, no flips).  The store and the plan are uploaded on first use and kept."""
        from . import lib as L
        device = torch.device(device)
        if self._dev is None or self._dev[0] != device:
            plan = np.zeros((len(self), 3), dtype=np.int32)
            plan[:, :2] = self.pairs
            self._dev = (device, self.store.to(device, non_blocking=True), torch.from_numpy(plan).to(device))
        _, images, plan = self._dev
        B, S = self.batch_size, images.shape[1]
        out = torch.empty((2, B, S, S, 3), dtype=torch.float32, device=device)
        L.call("ups_gather_views", L.ptr(images), images.shape[0], L.ptr(plan[c * B:(c + 1) * B]), B, S, L.ptr(out[0]), L.ptr(out[1]),
               None, L.stream())
        return {"view0": out[0], "view1": out[1]}
