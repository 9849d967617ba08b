"""Part-segmentation evaluation helpers: the IoU protocol of cub/code/eval/eval_iclr_01/eval_01.py:229-383.

The reference takes these from the un-vendored ``denseposelib`` (``compute_best_iou_remapping``, ``remap_parts``,
``compute_iou``); semantics re-derived from their call sites: every inferred part id is mapped to the ground-truth label it
overlaps best (IoU over the whole evaluation set), the remapped prediction is scored per label, and the reported "overall"
number averages the labels except ``background`` (cub_semantic_ours.ipynb:615).  ``evaluate_parts`` is NumPy on the pixel maps;
``evaluate_from_counts`` computes the same dict from the per-image part x label histogram (``confusion_counts`` on the host,
ups_part_confusion on the device through ``PartEvaluator``), which is all the protocol needs.

Label-free metrics (`val_metrics` / `eval_metrics`: reconstruction, parts; no counterpart in the reference):
``ReconstructionEvaluator`` / ``PartUsageEvaluator`` collect the per-image sums of ups_image_metrics / ups_part_usage on the device and
``reconstruction_from_sums`` / ``usage_from_counts`` are the pure steps from those sums to the reported numbers.
`equivariance`: ``EquivarianceEvaluator`` warps each view with its own thin-plate spline, runs the pose path once over originals and
warped copies and collects ups_part_equivariance's counts; ``equivariance_from_counts`` is the pure step, ``equivariance_host`` the
NumPy route for more than 32 parts.
`coherence`: ``CoherenceEvaluator`` labels the connected components of the part maps (ups_label_components) and collects
ups_label_component_stats' per-part table; ``coherence_from_stats`` is the pure step, ``coherence_host`` the NumPy route.
"""
import logging
import os

import numpy as np

LOG = logging.getLogger("upsparts")
TRANSFER_META_KEYS = ("view0", "view1", "relative_file_path_", "view1_relative_file_path_", "matrix", "matrix_index")


def compute_best_iou_remapping(inferred, gt):
    """inferred, gt: integer label maps of equal shape [N,H,W] -> {inferred id: gt label with the highest IoU}."""
    inferred, gt = np.asarray(inferred), np.asarray(gt)
    mapping = {}
    gl = np.unique(gt)
    for p in np.unique(inferred):
        m = inferred == p
        best, best_iou = int(gl[0]), -1.0
        for g in gl:
            t = gt == g
            union = np.logical_or(m, t).sum()
            iou = np.logical_and(m, t).sum() / union if union else 0.0
            if iou > best_iou:
                best, best_iou = int(g), float(iou)
        mapping[int(p)] = best
    return mapping


def remap_parts(labels, mapping):
    labels = np.asarray(labels)
    out = np.zeros_like(labels)
    for k, v in mapping.items():
        out[labels == k] = v
    return out


def compute_iou(pred, gt):
    """-> (iou per label, labels) over the labels present in gt."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    labels = np.unique(gt)
    ious = []
    for g in labels:
        a, b = pred == g, gt == g
        union = np.logical_or(a, b).sum()
        ious.append(np.logical_and(a, b).sum() / union if union else 0.0)
    return np.asarray(ious, dtype=np.float64), labels


def evaluate_parts(out_parts_hard, gt_segmentation, background_label=0):
    """out_parts_hard [N,H,W] (TrainModel.outputs["out_parts_hard"]), gt [N,H,W] -> per-label IoU and the overall number.

    Protocol of eval_01.py:229-383: ONE remapping for the whole set (best IoU over all images), then the IoU of every label
    PER IMAGE (a row of part_ious.csv; labels absent from an image's ground truth are left out of that row), the per-label
    means over the images (mean_part_ios.csv) and their mean without the background = "overall".  ``pooled`` additionally
    reports the IoU over all pixels of the set at once."""
    out_parts_hard, gt_segmentation = np.asarray(out_parts_hard), np.asarray(gt_segmentation)
    mapping = compute_best_iou_remapping(out_parts_hard, gt_segmentation)
    pred = remap_parts(out_parts_hard, mapping)
    labels_all = np.unique(gt_segmentation)
    rows = []
    for i in range(len(pred)):
        ious, labels = compute_iou(pred[i], gt_segmentation[i])
        rows.append(dict(zip(labels.tolist(), ious.tolist())))
    per_label = {int(g): float(np.mean([r[g] for r in rows if g in r])) for g in labels_all.tolist()}
    fg = [v for g, v in per_label.items() if g != background_label]
    pooled, pl = compute_iou(pred, gt_segmentation)
    return {"mapping": mapping, "iou": per_label, "per_image": rows,
            "overall": float(np.mean(fg)) if fg else float("nan"),
            "pooled": dict(zip(pl.tolist(), pooled.tolist()))}


def lut_array(lut):
    """The raw label -> evaluated label table as uint8 [256]: None, a {raw: new} dict (the reference's dp_remap_dict; raw labels it
    does not list keep their value) or 256 values.  ValueError on an entry outside 0..255."""
    if lut is None:
        return None
    if isinstance(lut, dict):
        t = np.arange(256, dtype=np.int64)
        for k, v in lut.items():
            if not 0 <= int(k) <= 255:
                raise ValueError("label lut: raw label {} is outside 0..255".format(k))
            t[int(k)] = int(v)
    else:
        t = np.asarray(lut).astype(np.int64).reshape(-1)
    if t.size != 256 or t.min() < 0 or t.max() > 255:
        raise ValueError("label lut: 256 entries in 0..255 expected (got {} in [{}, {}])".format(t.size, t.min(), t.max()))
    return t.astype(np.uint8)


def labels_u8(gt):
    """Ground-truth label maps as uint8; a label outside 0..255 is a ValueError (the device stores labels as bytes)."""
    gt = np.asarray(gt)
    if gt.dtype == np.uint8:
        return gt
    if gt.size and (gt.min() < 0 or gt.max() > 255 or np.any(gt != np.floor(gt))):
        raise ValueError("ground-truth labels must be integers in 0..255 (got values in [{}, {}])".format(gt.min(), gt.max()))
    return gt.astype(np.uint8)


def confusion_counts(pred, gt, P, G, lut=None, return_invalid=False):
    """counts [N,P,G] int32 with counts[i,p,g] = #{pixels of image i with pred == p and lut[gt] == g} (lut None: identity): the joint
    histogram ups_part_confusion (csrc/evalparts.hip) computes, in NumPy -- its test reference and the host fallback for P or G
    above 32.  pred, gt: integer maps [N,..] of one shape; lut: see ``lut_array``.  A pixel with pred outside [0,P) or a mapped
    label >= G is counted nowhere; return_invalid=True returns (counts, number of such pixels)."""
    pred = np.asarray(pred)
    N = pred.shape[0]
    pred = pred.reshape(N, -1).astype(np.int64)
    lab = np.asarray(gt).reshape(N, -1).astype(np.int64)
    if pred.shape != lab.shape:
        raise ValueError("confusion_counts: pred and gt differ in shape")
    t = lut_array(lut)
    if t is not None:
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("confusion_counts: a lut needs labels in 0..255")
        lab = t.astype(np.int64)[lab]
    ok = (pred >= 0) & (pred < P) & (lab >= 0) & (lab < G)
    counts = np.zeros((N, P, G), dtype=np.int32)
    for i in range(N):
        key = pred[i][ok[i]] * G + lab[i][ok[i]]
        counts[i] = np.bincount(key, minlength=P * G).reshape(P, G)
    return (counts, int(ok.size - ok.sum())) if return_invalid else counts


def _quot(inter, union):
    # the division evaluate_parts performs: np.int64 / np.int64 -> float64 (0.0 on an empty union)
    return np.int64(inter) / np.int64(union) if union else 0.0


def _iou_rows(R, labels):
    """compute_iou on remapped counts R [L,G] (R[a,b] = pixels predicted as labels[a] with ground truth labels[b]) -> (ious, present)."""
    pred_n, gt_n = R.sum(axis=1), R.sum(axis=0)
    present = [b for b in range(len(labels)) if gt_n[b] > 0]
    ious = [_quot(R[b, b], pred_n[b] + gt_n[b] - R[b, b]) for b in present]
    return np.asarray(ious, dtype=np.float64), [labels[b] for b in present]


def evaluate_from_counts(counts, part_ids=None, labels=None, background_label=0):
    """``evaluate_parts`` from the joint histogram counts [N,P,G] (``confusion_counts`` / ups_part_confusion): the same dict --
    mapping, iou, per_image, pooled, overall -- with the same integers divided, hence the same float64 values and the same ties.
    part_ids [P] / labels [G]: the part id of row p and the (ascending) label of column g; default 0..P-1 / 0..G-1.
    "Present" = a non-zero row / column sum: over the set for `mapping` and `iou`, per image for `per_image`.  Tie rules as
    ``compute_best_iou_remapping``: labels are tried in ascending order and only a strictly larger IoU replaces the best; a part that
    occurs nowhere has no mapping entry; a label absent from an image's ground truth is absent from that image's row."""
    C = np.asarray(counts).astype(np.int64)
    N, P, G = C.shape
    part_ids = list(range(P)) if part_ids is None else [int(p) for p in part_ids]
    labels = list(range(G)) if labels is None else [int(g) for g in labels]
    if len(part_ids) != P or len(labels) != G or sorted(labels) != labels or sorted(part_ids) != part_ids:
        raise ValueError("evaluate_from_counts: {} ascending part ids and {} ascending labels expected".format(P, G))
    T = C.sum(axis=0)
    part_n, label_n = T.sum(axis=1), T.sum(axis=0)
    gl = [g for g in range(G) if label_n[g] > 0]
    mapping, col = {}, {}
    for p in range(P):
        if part_n[p] == 0:
            continue
        best, best_iou = gl[0], -1.0
        for g in gl:
            iou = _quot(T[p, g], part_n[p] + label_n[g] - T[p, g])
            if iou > best_iou:
                best, best_iou = g, float(iou)
        mapping[part_ids[p]], col[p] = labels[best], best
    # remap_parts: the rows of the parts mapped to one label are added up (every present part has a mapping)
    R = np.zeros((N, G, G), dtype=np.int64)
    for p, g in col.items():
        R[:, g, :] += C[:, p, :]
    rows = []
    for i in range(N):
        ious, present = _iou_rows(R[i], labels)
        rows.append(dict(zip(present, ious.tolist())))
    per_label = {labels[g]: float(np.mean([r[labels[g]] for r in rows if labels[g] in r])) for g in gl}
    fg = [v for g, v in per_label.items() if g != background_label]
    pooled, pl = _iou_rows(R.sum(axis=0), labels)
    return {"mapping": mapping, "iou": per_label, "per_image": rows,
            "overall": float(np.mean(fg)) if fg else float("nan"),
            "pooled": dict(zip(pl, pooled.tolist()))}


class _Accumulator(object):
    """What the evaluators share: named per-image columns gathered on the device and copied to the host once.
    columns: (name, width or row shape, torch.int32 / torch.float64, zero) each.  zero: fresh rows are zero -- a count column, which the
    kernels ADD to; a float64 column is written completely and may start empty.  `invalid` is the [1] int32 counter of the pixels that
    were counted nowhere.  on_device False is the host route: ``add_host`` keeps the NumPy arrays of the restatements in lists."""

    def __init__(self, who, device, columns, on_device=True):
        self.who, self.device, self.on_device = who, device, on_device
        self.columns = [(name, (shape,) if isinstance(shape, int) else tuple(shape), dtype, zero) for name, shape, dtype, zero in columns]
        self.reset()

    def _new(self, rows, shape, dtype, zero):
        import torch
        return (torch.zeros if zero else torch.empty)((rows,) + shape, dtype=dtype, device=self.device)

    def reset(self):
        """Fresh buffers of 64 rows, a zero `invalid`, no image, no pixel count."""
        import torch
        self.n, self.HW, self.capacity, self._host, self._host_invalid = 0, None, 64, [], 0
        self._buf = self.invalid = None
        if self.on_device:
            self._buf = [self._new(self.capacity, *c[1:]) for c in self.columns]
            self.invalid = self._new(1, (), torch.int32, True)

    def take(self, n):
        """The next n rows of every column (contiguous row-offset views, in column order).  The buffers grow stream-ordered to
        max(2 * rows, needed): the filled rows are kept and fresh count rows are zero."""
        if self.n + n > self.capacity:
            self.capacity = max(2 * self.capacity, self.n + n)
            for k, c in enumerate(self.columns):
                grown = self._new(self.capacity, *c[1:])
                grown[:self.n] = self._buf[k][:self.n]
                self._buf[k] = grown
        views = tuple(b[self.n:self.n + n] for b in self._buf)
        self.n += n
        return views

    def add_host(self, n, arrays, invalid):
        """The host route: `arrays` (one per column) and the invalid count of n more images."""
        self._host.append(arrays)
        self._host_invalid += invalid
        self.n += n

    def same_pixels(self, what, HW):
        if self.HW is not None and HW != self.HW:
            raise ValueError("{}.update: {} of {} pixels after {} of {}".format(self.who, what, HW, what, self.HW))
        self.HW = HW

    def fetch(self):
        """((one NumPy array [n, ..] per column, in its own dtype), invalid as int).  On the device route this is the ONE copy to the
        host: a single .cpu() of every filled row and `invalid` concatenated.  Beside float64 columns the int32 values ride as
        float64: every |int32| < 2^31 is exact there (a count is at most HW < 2^31)."""
        import torch
        np_of = {torch.int32: np.int32, torch.float64: np.float64}
        if not self.on_device:
            if not self._host:
                return tuple(np.zeros((0,) + shape, np_of[dtype]) for _, shape, dtype, _ in self.columns), 0
            return tuple(np.concatenate([a[k] for a in self._host]) for k in range(len(self.columns))), self._host_invalid
        wide = torch.float64 if any(c[2] == torch.float64 for c in self.columns) else torch.int32
        both = torch.cat([b[:self.n].reshape(-1).to(wide) for b in self._buf] + [self.invalid.to(wide)]).cpu().numpy()
        out, at = [], 0
        for _, shape, dtype, _ in self.columns:
            size = self.n * int(np.prod(shape, dtype=np.int64))
            out.append(both[at:at + size].astype(np_of[dtype], copy=False).reshape((self.n,) + shape))
            at += size
        return tuple(out), int(both[-1])

    def finish(self, sentence):
        """``fetch`` and the evaluators' common ending: UpsError "<who>: <invalid> <sentence>" when pixels were left out, ValueError
        when no image was evaluated.  Returns the columns."""
        from .lib import UpsError
        columns, invalid = self.fetch()
        if invalid != 0:
            raise UpsError("{}: {} {}".format(self.who, invalid, sentence))
        if self.n == 0:
            raise ValueError("{}.result: no image was evaluated".format(self.who))
        return columns


class PartEvaluator(object):
    """The part-IoU protocol with the pixels left on the device: ``update`` runs ``model.segment`` (pose path only) and
    ups_part_confusion into a device buffer of counts that grows by one [P,G] row per image, without synchronising with the host;
    ``result`` copies the counts once and returns ``evaluate_from_counts``.
    n_labels = G: evaluated labels are 0..G-1 (columns no pixel hits are "absent", so a G larger than needed changes nothing).
    lut: raw label -> evaluated label (``lut_array``).  P or G above 32 (the kernel's table) falls back to ``confusion_counts`` on
    the host, with one logged line."""

    def __init__(self, model, n_labels, lut=None, background_label=0):
        import torch
        self.model, self.P, self.G, self.background_label = model, int(model.n_parts), int(n_labels), background_label
        self.lut = lut_array(lut)
        self.on_device = self.P <= 32 and self.G <= 32
        if self.P < 1 or self.G < 1:
            raise ValueError("PartEvaluator: n_parts and n_labels must be positive (got {}, {})".format(self.P, self.G))
        if not self.on_device:
            LOG.info("PartEvaluator: P = %d, G = %d exceed the device table (32 x 32): counting on the host", self.P, self.G)
        self._lut_dev = None if self.lut is None or not self.on_device else torch.from_numpy(self.lut).to(model.device)
        self._acc = _Accumulator("PartEvaluator", model.device, [("counts", (self.P, self.G), torch.int32, True)], self.on_device)

    n = property(lambda self: self._acc.n)

    def reset(self):
        self._acc.reset()

    def _labels(self, gt):
        import torch
        if torch.is_tensor(gt) and gt.dtype == torch.uint8:
            return gt
        return torch.from_numpy(np.ascontiguousarray(labels_u8(gt.cpu().numpy() if torch.is_tensor(gt) else gt)))

    def update(self, views, gt, valid=None):
        """views [n,S,S,3] in [-1,1], gt [n,S,S] integer labels (cast to uint8 on the host: a label outside 0..255 raises ValueError
        before anything is launched); valid: only the first `valid` images count (a padded last batch)."""
        import torch
        from . import ops
        gt = self._labels(gt)
        n = len(gt) if valid is None else int(valid)
        if n == 0:
            return
        views, gt = views[:n], gt[:n]
        pred = self.model.segment(torch.as_tensor(views))
        if tuple(pred.shape) != tuple(gt.shape):
            raise ValueError("PartEvaluator.update: label maps {} do not match the part maps {}".format(tuple(gt.shape), tuple(pred.shape)))
        if not self.on_device:
            c, bad = confusion_counts(pred.cpu().numpy(), gt.cpu().numpy(), self.P, self.G, self.lut, return_invalid=True)
            return self._acc.add_host(n, (c,), bad)
        ops.part_confusion(pred, gt.to(pred.device, non_blocking=True), self.P, self.G, lut=self._lut_dev,
                           counts=self._acc.take(n)[0], invalid=self._acc.invalid)

    def counts(self):
        """(counts [n,P,G] int32 NumPy, invalid): the one copy to the host."""
        (counts,), invalid = self._acc.fetch()
        return counts, invalid

    def result(self):
        counts, = self._acc.finish("pixel(s) with a part id outside [0, {}) or a label outside [0, {}) were not counted "
                                   "(n_labels too small, or a label lut is missing)".format(self.P, self.G))
        return evaluate_from_counts(counts, background_label=self.background_label)


# ------------------------------------------------------------------ label-free validation metrics (`val_metrics`, `eval_metrics`)
def reconstruction_from_sums(rows, H, W):
    """rows [n,3] = (sse, sae, ssim_sum) per image (ups_image_metrics) of H x W images -> {"mse", "l1", "psnr", "ssim"}: the means over
    the images of mse_i = sse_i / (3 H W), l1_i = sae_i / (3 H W), psnr_i = 10 log10(1 / max(mse_i, 1e-10)) (images in [0, 1]: the
    floor caps a perfect reconstruction at 100 dB) and ssim_i = ssim_sum_i / (3 (H - 10) (W - 10))."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    if rows.shape[0] == 0:
        raise ValueError("reconstruction_from_sums: no image was evaluated")
    if H < 11 or W < 11:
        raise ValueError("reconstruction_from_sums: the 11 x 11 SSIM window needs H, W >= 11 (got {} x {})".format(H, W))
    mse = rows[:, 0] / (3.0 * H * W)
    l1 = rows[:, 1] / (3.0 * H * W)
    psnr = 10.0 * np.log10(1.0 / np.maximum(mse, 1e-10))
    ssim = rows[:, 2] / (3.0 * (H - 10) * (W - 10))
    return {"mse": float(mse.mean()), "l1": float(l1.mean()), "psnr": float(psnr.mean()), "ssim": float(ssim.mean())}


def usage_from_counts(counts, sharp, HW, min_area):
    """counts [n,P] integers (pixels of image i whose arg-max part is p), sharp [n,2] = (sum of max_p soft, sum of the per-pixel
    entropies) per image (ups_part_usage), HW pixels per image -> {"part_area": [P] with part_area[p] = sum_i counts[i,p] / (n HW),
    "parts_active": #{p : part_area[p] >= min_area}, "confidence", "entropy": the per-pixel means over the set}."""
    counts = np.asarray(counts).astype(np.int64)
    sharp = np.asarray(sharp, dtype=np.float64).reshape(-1, 2)
    n = counts.shape[0]
    if n == 0 or sharp.shape[0] != n:
        raise ValueError("usage_from_counts: counts [n >= 1,P] and sharp [n,2] expected (got {} and {})".format(counts.shape, sharp.shape))
    px = np.int64(n) * np.int64(HW)
    area = counts.sum(axis=0) / px
    return {"part_area": [float(v) for v in area], "parts_active": int((area >= min_area).sum()),
            "confidence": float(sharp[:, 0].sum() / px), "entropy": float(sharp[:, 1].sum() / px)}


def part_usage_host(soft, pred, P):
    """ups_part_usage in NumPy float64 (the host route for P > 32): (counts [N,P] int32, invalid, sharp [N,2])."""
    soft = np.asarray(soft, dtype=np.float64)
    N = soft.shape[0]
    soft = soft.reshape(N, -1, P)
    pred = np.asarray(pred).reshape(N, -1).astype(np.int64)
    ok = (pred >= 0) & (pred < P)
    counts = np.stack([np.bincount(pred[i][ok[i]], minlength=P) for i in range(N)]).astype(np.int32)
    pos = soft > 0
    ent = -(np.where(pos, soft, 0.0) * np.log(np.where(pos, soft, 1.0))).sum(axis=2)
    sharp = np.stack([soft.max(axis=2).sum(axis=1), ent.sum(axis=1)], axis=1)
    return counts, int(ok.size - ok.sum()), sharp


class ReconstructionEvaluator(object):
    """mse / l1 / psnr / ssim of generated images against their targets with the pixels left on the device: ``update`` runs
    ups_image_metrics into a device buffer of (sse, sae, ssim_sum) rows, without synchronising with the host; ``result`` copies the
    rows once and returns ``reconstruction_from_sums``."""

    def __init__(self, device):
        import torch
        self.device = device
        self._acc = _Accumulator("ReconstructionEvaluator", device, [("rows", 3, torch.float64, False)])

    n = property(lambda self: self._acc.n)
    H = property(lambda self: None if self._acc.HW is None else self._acc.HW[0])
    W = property(lambda self: None if self._acc.HW is None else self._acc.HW[1])

    def reset(self):
        self._acc.reset()

    def update(self, generated, target, valid=None):
        """generated, target [n,H,W,>=3] float32 / bfloat16 on the device, values in [-1, 1]; only the first `valid` images count."""
        from . import ops
        n = generated.shape[0] if valid is None else int(valid)
        if n == 0:
            return
        self._acc.same_pixels("images", (int(generated.shape[1]), int(generated.shape[2])))
        ops.image_metrics(generated[:n], target[:n], out=self._acc.take(n)[0])

    def rows(self):
        """[n,3] float64 NumPy: the one copy to the host."""
        return self._acc.fetch()[0][0]

    def result(self):
        rows, = self._acc.finish("pixel(s) were not counted")  # (ups_image_metrics has no `invalid`: the refusal of n == 0 alone)
        return reconstruction_from_sums(rows, self.H, self.W)


class PartUsageEvaluator(object):
    """Part areas, active parts, mask confidence and entropy with the pixels left on the device: ``update`` runs ups_part_usage into
    device buffers that grow by one row per image; ``result`` makes one copy and returns ``usage_from_counts``.  n_parts above 32 (the
    kernel's table) is computed by ``part_usage_host``, with one logged line."""

    def __init__(self, device, n_parts, min_area=0.005):
        import torch
        self.device, self.P, self.min_area = device, int(n_parts), float(min_area)
        if self.P < 1:
            raise ValueError("PartUsageEvaluator: n_parts must be positive (got {})".format(self.P))
        self.on_device = self.P <= 32
        if not self.on_device:
            LOG.info("PartUsageEvaluator: P = %d exceeds the device table (32): counting on the host", self.P)
        self._acc = _Accumulator("PartUsageEvaluator", device, [("counts", self.P, torch.int32, True), ("sharp", 2, torch.float64, False)],
                                 self.on_device)

    n = property(lambda self: self._acc.n)
    HW = property(lambda self: self._acc.HW)

    def reset(self):
        self._acc.reset()

    def update(self, soft, pred, valid=None):
        """soft [n,..,P] float32 (out_parts_soft), pred [n,..] int64 (out_parts_hard); only the first `valid` images count."""
        from . import ops
        n = pred.shape[0] if valid is None else int(valid)
        if n == 0:
            return
        soft, pred = soft[:n], pred[:n]
        if soft.shape[-1] != self.P or tuple(soft.shape[:-1]) != tuple(pred.shape):
            raise ValueError("PartUsageEvaluator.update: soft {} and pred {} do not describe the same pixels of {} parts".format(
                tuple(soft.shape), tuple(pred.shape), self.P))
        self._acc.same_pixels("maps", int(pred[0].numel()))
        if not self.on_device:
            c, bad, s = part_usage_host(soft.cpu().numpy(), pred.cpu().numpy(), self.P)
            return self._acc.add_host(n, (c, s), bad)
        counts, sharp = self._acc.take(n)
        ops.part_usage(soft, pred, counts=counts, invalid=self._acc.invalid, sharp=sharp)

    def sums(self):
        """(counts [n,P] int32, sharp [n,2] float64, invalid) as NumPy: the one copy to the host."""
        (counts, sharp), invalid = self._acc.fetch()
        return counts, sharp, invalid

    def result(self):
        counts, sharp = self._acc.finish("pixel(s) with a part id outside [0, {}) were not counted".format(self.P))
        return usage_from_counts(counts, sharp, self.HW, self.min_area)


# ------------------------------------------------------------------ part equivariance under thin-plate-spline warps (`equivariance`)
def equivariance_from_counts(counts, tv, HW):
    """counts [n,P,P] integers (counts[i,la,lb]: inside pixels of image i whose original's part, sampled where the warp took the pixel
    from, is la and whose warped image's part is lb) and tv [n] (the per-pixel total variation summed over those pixels), both from
    ups_part_equivariance, HW pixels per image ->
      "valid"      sum counts / (n HW): the share of pixels whose source lies inside the image
      "agreement"  sum_i trace(counts[i]) / sum counts
      "iou"        [P], on the pooled table C = sum_i counts[i]: C[p,p] / (row_p + col_p - C[p,p]); -1.0 where that denominator is 0
                   (the marker the reference's part_ious.csv uses for an absent label)
      "miou"       the mean of iou over the parts whose denominator is positive
      "tv"         sum tv / sum counts
    ValueError: no image, shapes that do not match, or no counted pixel at all."""
    counts = np.asarray(counts).astype(np.int64)
    tv = np.asarray(tv, dtype=np.float64).reshape(-1)
    if counts.ndim != 3 or counts.shape[0] == 0 or counts.shape[1] != counts.shape[2] or tv.shape[0] != counts.shape[0]:
        raise ValueError("equivariance_from_counts: counts [n >= 1,P,P] and tv [n] expected (got {} and {})".format(counts.shape, tv.shape))
    if int(HW) < 1:
        raise ValueError("equivariance_from_counts: HW must be positive (got {})".format(HW))
    n, total = counts.shape[0], int(counts.sum())
    if total == 0:
        raise ValueError("equivariance_from_counts: no pixel was counted (every source position outside the image, or invalid)")
    C = counts.sum(axis=0)
    diag = np.diagonal(C)
    den = C.sum(axis=1) + C.sum(axis=0) - diag
    iou = np.where(den > 0, diag / np.maximum(den, 1), -1.0)
    return {"valid": float(total / (np.int64(n) * np.int64(HW))), "agreement": float(diag.sum() / total),
            "iou": [float(v) for v in iou], "miou": float(iou[den > 0].mean()), "tv": float(tv.sum() / total)}


def equivariance_host(soft_a, soft_b, pred_b, grid):
    """ups_part_equivariance in NumPy float64 (the host route for P > 32; the definitions: include/upsparts_hip.h):
    soft_a, soft_b [N,h,w,P] float32, pred_b [N,h,w] integers, grid [N,h,w,2] float32 -> (counts [N,P,P] int32, invalid, tv [N])."""
    a, b = np.asarray(soft_a, dtype=np.float64), np.asarray(soft_b, dtype=np.float64)
    N, h, w, P = a.shape
    lb = np.asarray(pred_b).reshape(N, h, w).astype(np.int64)
    g = np.asarray(grid).reshape(N, h, w, 2).astype(np.float64)
    X, Y = g[..., 0], g[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (X >= 0.0) & (X <= w - 1) & (Y >= 0.0) & (Y <= h - 1)           # NaN and +-inf compare false
    X, Y = np.where(inside, X, 0.0), np.where(inside, Y, 0.0)
    x0, y0 = np.floor(X), np.floor(Y)
    fx, fy = (X - x0)[..., None], (Y - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    i = np.arange(N).reshape(N, 1, 1)
    with np.errstate(invalid="ignore"):
        top = (1.0 - fx) * a[i, y0, x0] + fx * a[i, y0, x1]
        bot = (1.0 - fx) * a[i, y1, x0] + fx * a[i, y1, x1]
        v = (1.0 - fy) * top + fy * bot
        acc = np.zeros((N, h, w))
        for p in range(P):
            acc = acc + np.abs(v[..., p] - b[..., p])
    nan = np.isnan(v).any(axis=-1) | np.isnan(b).any(axis=-1)
    counted = inside & ~nan & (lb >= 0) & (lb < P)
    la = np.argmax(np.where(np.isnan(v), -np.inf, v), axis=-1)                    # the first maximal part
    t = 0.5 * acc
    counts, tv = np.zeros((N, P, P), dtype=np.int32), np.zeros(N)
    for k in range(N):
        m = counted[k]
        counts[k] = np.bincount(la[k][m] * P + lb[k][m], minlength=P * P).reshape(P, P)
        tv[k] = t[k][m].sum()
    return counts, int((inside & ~counted).sum()), tv


class EquivarianceEvaluator(object):
    """Part equivariance under thin-plate-spline warps with the pixels left on the device.  ``update(model, views, uniforms)`` solves
    one warp per view from its row of uniforms (``tps.tps_system``: a singular system keeps the identity transform and counts in
    `n_singular`), warps the views (ups_tps_warp), runs ONE ``model.segment_soft`` over the originals and their warped copies together
    -- for batch_size views one pass of the pose path -- takes the warp's own sampling positions (``ops.tps_grid``) and adds
    ups_part_equivariance's counts and distance sums to device buffers that grow by one row per image; ``result`` makes one copy and
    returns ``equivariance_from_counts``.  n_parts above 32 (the kernel's table) is computed by ``equivariance_host``, with one
    logged line."""

    def __init__(self, device, n_parts, tps_params, n_singular=None):
        import torch
        self.device, self.P, self.tps_params, self.n_singular = device, int(n_parts), dict(tps_params), n_singular
        if self.P < 1:
            raise ValueError("EquivarianceEvaluator: n_parts must be positive (got {})".format(self.P))
        self.on_device = self.P <= 32
        if not self.on_device:
            LOG.info("EquivarianceEvaluator: P = %d exceeds the device table (32 x 32): counting on the host", self.P)
        self._acc = _Accumulator("EquivarianceEvaluator", device, [("counts", (self.P, self.P), torch.int32, True), ("tv", (), torch.float64, False)],
                                 self.on_device)

    n = property(lambda self: self._acc.n)
    HW = property(lambda self: self._acc.HW)

    def reset(self):
        self._acc.reset()

    def maps(self, model, views, uniforms):
        """(soft_a, soft_b, pred_b, grid) of `views` [n,S,S,3] under the warps of `uniforms` [n, tps.N_UNIFORMS]: what ``update``
        hands to the kernel."""
        import torch
        from . import ops, tps
        views = torch.as_tensor(views).to(self.device, torch.float32).contiguous()
        n, h, w = views.shape[:3]
        u = torch.as_tensor(uniforms).to(self.device, torch.float32)
        if tuple(u.shape) != (n, tps.N_UNIFORMS):
            raise ValueError("EquivarianceEvaluator: uniforms [{}, {}] expected, one row per view (got {})".format(
                n, tps.N_UNIFORMS, tuple(u.shape)))
        coord, _, T = tps.tps_system(u, self.tps_params, n_singular=self.n_singular)
        warped = tps._warp(views, T, coord)
        hard, soft = model.segment_soft(torch.cat([views, warped], 0))
        return soft[:n], soft[n:], hard[n:], ops.tps_grid(T, coord, h, w)

    def update(self, model, views, uniforms, valid=None):
        """views [n,S,S,3] in [-1,1], uniforms [n, tps.N_UNIFORMS] in [0,1) (row i draws view i's warp); only the first `valid`
        images count (a padded last batch)."""
        from . import ops
        n = len(views) if valid is None else int(valid)
        if n == 0:
            return
        soft_a, soft_b, pred_b, grid = (t[:n] for t in self.maps(model, views, uniforms))
        if soft_a.shape[-1] != self.P:
            raise ValueError("EquivarianceEvaluator.update: maps of {} parts, {} expected".format(soft_a.shape[-1], self.P))
        self._acc.same_pixels("maps", int(pred_b[0].numel()))
        if not self.on_device:
            c, bad, tv = equivariance_host(soft_a.cpu().numpy(), soft_b.cpu().numpy(), pred_b.cpu().numpy(), grid.cpu().numpy())
            return self._acc.add_host(n, (c, tv), bad)
        counts, tv = self._acc.take(n)
        ops.part_equivariance(soft_a, soft_b, pred_b, grid, counts=counts, invalid=self._acc.invalid, tv=tv)

    def sums(self):
        """(counts [n,P,P] int32, tv [n] float64, invalid) as NumPy: the one copy to the host."""
        (counts, tv), invalid = self._acc.fetch()
        return counts, tv, invalid

    def result(self):
        counts, tv = self._acc.finish("pixel(s) with a NaN in a part map or a part id outside [0, {}) were not counted".format(self.P))
        return equivariance_from_counts(counts, tv, self.HW)


def equivariance_uniforms(n, seed):
    """The [n, tps.N_UNIFORMS] float32 uniforms of `val_metrics` / `eval_metrics`: equivariance, drawn once from a CPU generator
    seeded by `val_seed`; row i belongs to image i."""
    import torch
    from . import tps
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return torch.rand(int(n), tps.N_UNIFORMS, generator=gen, dtype=torch.float32)


# ------------------------------------------------------------------ part coherence: connected components of the part maps (`coherence`)
def coherence_from_stats(stats, HW):
    """stats [n,P,4] integers per image and part (ups_label_component_stats: pixels, components, largest component, components smaller
    than the speck area), HW pixels per image -> a flat dict:
      "components_<p>"     the mean component count of part p over the images where it is present; -1.0 if it is present nowhere
      "fragmentation_<p>"  1 - sum_i largest[i,p] / sum_i pixels[i,p] on the pooled integers (0: every image's part p is one region);
                           -1.0 if it is present nowhere
      "fragmentation"      the same pooled over the parts too (-1.0 without a single valid pixel)
      "specks"             the small components per image."""
    stats = np.asarray(stats).astype(np.int64)
    if stats.ndim != 3 or stats.shape[0] == 0 or stats.shape[2] != 4:
        raise ValueError("coherence_from_stats: stats [n >= 1,P,4] expected (got {})".format(stats.shape))
    px, comps, largest, small = (stats[:, :, k] for k in range(4))
    if (px.sum(axis=1) > int(HW)).any() or (stats < 0).any():
        raise ValueError("coherence_from_stats: more pixels in an image's parts than the image's {} (or a negative count)".format(HW))
    res = {}
    present = px > 0
    for p in range(stats.shape[1]):
        k = int(present[:, p].sum())
        res["components_{}".format(p)] = float(comps[present[:, p], p].sum() / k) if k else -1.0
        tot = int(px[:, p].sum())
        res["fragmentation_{}".format(p)] = float(1.0 - largest[:, p].sum() / tot) if tot else -1.0
    tot = int(px.sum())
    res["fragmentation"] = float(1.0 - largest.sum() / tot) if tot else -1.0
    res["specks"] = float(small.sum() / stats.shape[0])
    return res


def _components_host(lab, P, conn):
    """comp int64 [h,w] of one map in NumPy: every valid pixel starts as its own index and takes the minimum over its equally
    labelled neighbours, then jumps to its representative's representative, until nothing changes (at most h * w sweeps)."""
    h, w = lab.shape
    ok = (lab >= 0) & (lab < P)
    big = h * w
    comp = np.where(ok, np.arange(big, dtype=np.int64).reshape(h, w), big)
    shifts = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if conn == 8 else [])
    for _ in range(big + 1):
        new = comp.copy()
        for dy, dx in shifts:                                # the pair (y, x) / (y + dy, x + dx), both ways
            a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
            b = (slice(dy, h), slice(max(0, dx), w - max(0, -dx)))
            same = ok[a] & ok[b] & (lab[a] == lab[b])
            lo = np.minimum(new[a], new[b])
            new[a] = np.where(same, lo, new[a])
            new[b] = np.where(same, np.minimum(lo, new[b]), new[b])       # (a and b overlap: keep what the line above lowered)
        flat = new.reshape(-1)
        idx = np.nonzero(flat < big)[0]
        flat[idx] = flat[flat[idx]]                          # the representative's representative: the same component, no larger
        if np.array_equal(new, comp):
            break
        comp = new
    else:
        raise RuntimeError("coherence_host: the propagation did not settle in h * w sweeps")
    return np.where(ok, comp, -1)


def coherence_host(pred, P, conn=8, small=0):
    """ups_label_components + ups_label_component_stats in NumPy (the host route, where the device cannot be used):
    pred [N,h,w] integers -> (stats [N,P,4] int32, invalid)."""
    pred = np.asarray(pred)
    if pred.ndim != 3 or conn not in (4, 8) or P < 1:
        raise ValueError("coherence_host: pred [N,h,w], conn 4 or 8, P >= 1 (got {}, {}, {})".format(pred.shape, conn, P))
    pred = pred.astype(np.int64)
    N, h, w = pred.shape
    stats = np.zeros((N, P, 4), dtype=np.int32)
    invalid = 0
    for i in range(N):
        comp = _components_host(pred[i], P, conn).reshape(-1)
        lab = pred[i].reshape(-1)
        invalid += int((comp < 0).sum())
        area = np.bincount(comp[comp >= 0], minlength=h * w)
        roots = np.nonzero(comp == np.arange(h * w))[0]
        for p in range(P):
            a = area[roots[lab[roots] == p]]
            stats[i, p] = (int(a.sum()), a.size, int(a.max()) if a.size else 0, int((a < small).sum()))
    return stats, invalid


class CoherenceEvaluator(object):
    """Whether each part is one region or many, with the pixels left on the device: ``update`` runs ups_label_components and
    ups_label_component_stats on the part maps into a device buffer that grows by one [P,4] row per image; ``result`` makes one copy
    and returns ``coherence_from_stats``.  speck_area: components of fewer pixels count as specks.  n_parts above 255 (a label is a
    byte in the kernels' tables) is computed by ``coherence_host``, with one logged line."""

    def __init__(self, device, n_parts, conn=8, speck_area=0):
        import torch
        self.device, self.P, self.conn, self.speck_area = device, int(n_parts), int(conn), int(speck_area)
        if self.P < 1 or self.conn not in (4, 8) or self.speck_area < 0:
            raise ValueError("CoherenceEvaluator: n_parts >= 1, conn 4 or 8, speck_area >= 0 (got {}, {}, {})".format(
                n_parts, conn, speck_area))
        self.on_device = self.P <= 255
        if not self.on_device:
            LOG.info("CoherenceEvaluator: P = %d exceeds the kernels' 255: labelling on the host", self.P)
        self._acc = _Accumulator("CoherenceEvaluator", device, [("stats", (self.P, 4), torch.int32, True)], self.on_device)
        self._err = None

    n = property(lambda self: self._acc.n)
    HW = property(lambda self: self._acc.HW)

    def reset(self):
        self._acc.reset()
        self._err = None

    def update(self, pred, valid=None):
        """pred [n,h,w] int64 (out_parts_hard); only the first `valid` images count."""
        import torch
        from . import ops
        n = pred.shape[0] if valid is None else int(valid)
        if n == 0:
            return
        pred = pred[:n]
        if pred.dim() != 3:
            raise ValueError("CoherenceEvaluator.update: pred [n,h,w] expected (got {})".format(tuple(pred.shape)))
        self._acc.same_pixels("maps", int(pred[0].numel()))
        if not self.on_device:
            s, bad = coherence_host(pred.cpu().numpy(), self.P, self.conn, self.speck_area)
            return self._acc.add_host(n, (s,), bad)
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=pred.device)
        pred = pred.contiguous()
        comp, _ = ops.label_components(pred, self.P, conn=self.conn, err=self._err)
        ops.label_component_stats(pred, comp, self.P, small=self.speck_area, stats=self._acc.take(n)[0], invalid=self._acc.invalid)

    def sums(self):
        """(stats [n,P,4] int32, invalid) as NumPy: the one copy to the host."""
        (stats,), invalid = self._acc.fetch()
        return stats, invalid

    def result(self):
        from . import ops
        stats, = self._acc.finish("pixel(s) with a part id outside [0, {}) belong to no component".format(self.P))
        if self._err is not None:
            ops.components_check(self._err)
        return coherence_from_stats(stats, self.HW)


def validation_logs(rec=None, usage=None, rec_loss=None, equiv=None, coherence=None):
    """The `val/` keys of the label-free metrics: rec = ``reconstruction_from_sums`` (val/mse, val/l1, val/psnr, val/ssim), rec_loss the
    perceptual reconstruction term (val/rec), usage = ``usage_from_counts`` (val/part_area_<p>, val/parts_active, val/confidence,
    val/entropy), equiv = ``equivariance_from_counts`` (val/equiv_agreement, val/equiv_miou, val/equiv_iou_<p>, val/equiv_tv,
    val/equiv_valid), coherence = ``coherence_from_stats`` (val/fragmentation, val/fragmentation_<p>, val/components_<p>, val/specks).
    All of them sort before val/steps_done."""
    logs = {}
    if coherence is not None:
        logs.update({"val/" + k: v for k, v in coherence.items()})
    if equiv is not None:
        logs.update({"val/equiv_iou_{}".format(p): v for p, v in enumerate(equiv["iou"])})
        logs.update({"val/equiv_" + k: equiv[k] for k in ("agreement", "miou", "tv", "valid")})
    if rec is not None:
        logs.update({"val/" + k: rec[k] for k in ("mse", "l1", "psnr", "ssim")})
    if rec_loss is not None:
        logs["val/rec"] = rec_loss
    if usage is not None:
        logs.update({"val/part_area_{}".format(p): v for p, v in enumerate(usage["part_area"])})
        logs.update({"val/parts_active": usage["parts_active"], "val/confidence": usage["confidence"], "val/entropy": usage["entropy"]})
    return logs


def write_eval_tables(res, root, global_step, part_names=None, background_label=0):
    """The files eval_01.py:229-383 leaves in the evaluation directory, from ``evaluate_parts``' result:
    ``part_ious.csv``     one row per image: global_step, batch_idx, then one IoU column per ground-truth part (-1.0 where the
                          image's ground truth lacks the part, eval_01.py:299-309, 371)
    ``mean_part_ios.csv`` (the reference's spelling) the column means over the rows with the -1 entries left out plus
                          ``overall`` = the mean of the part columns without ``background``, as a psql table (eval_01.py:373-383)
    ``best_remapping.yml`` inferred part id -> ground-truth label (eval_01.py:254-258).
    part_names: {ground-truth label: column name} (the sorted keys of the yaml's dp_semantic_remap_dict in the reference);
    default "background" for `background_label`, "part_<label>" otherwise."""
    import pandas as pd
    import yaml
    from tabulate import tabulate
    labels = sorted(res["iou"])
    names = {g: ("background" if g == background_label else "part_{}".format(g)) for g in labels}
    names.update(part_names or {})
    cols = [names[g] for g in labels]
    rows = []
    for i, r in enumerate(res["per_image"]):
        row = {"global_step": global_step, "batch_idx": i}
        row.update({names[g]: float(r.get(g, -1.0)) for g in labels})
        rows.append(row)
    df = pd.DataFrame(rows, columns=["global_step", "batch_idx"] + cols)
    os.makedirs(root, exist_ok=True)
    df.to_csv(os.path.join(root, "part_ious.csv"), index=False, header=True)
    df_mean = df[df != -1].mean().to_frame().transpose()
    df_mean["overall"] = df_mean[[c for c in cols if c != "background"]].mean(axis=1)
    with open(os.path.join(root, "mean_part_ios.csv"), "w") as f:
        print(tabulate(df_mean, headers="keys", tablefmt="psql", showindex="never"), file=f)
    with open(os.path.join(root, "best_remapping.yml"), "w") as f:
        yaml.dump({"best_remapping": {int(k): int(v) for k, v in res["mapping"].items()}}, f, default_flow_style=False)
    return df, df_mean


def transfer_cells(block, result, generated_key, vis0_key, vis1_key, data=None):
    """Append one block's cells to the comparison-matrix record: the key set final_eval/eval_transfer.py's MatrixHook leaves in
    ``data.p`` (the three yaml-named keys plus TRANSFER_META_KEYS), one list entry per cell, row-major within the block.
    block: ``data.TransferData.get_block``; result: ``TrainModel.transfer_matrix`` as NumPy arrays."""
    if data is None:
        data = {k: [] for k in (generated_key, vis0_key, vis1_key) + TRANSFER_META_KEYS}
    n, m = result["generated"].shape[:2]
    for i in range(n):
        for j in range(m):
            data[generated_key].append(result["generated"][i, j])
            data[vis0_key].append(result["row_mask_rgb"][i])
            data[vis1_key].append(result["col_mask_rgb"][j])
            data["view0"].append(block["rows"][i])
            data["view1"].append(block["cols"][j])
            data["relative_file_path_"].append(block["row_paths"][i])
            data["view1_relative_file_path_"].append(block["col_paths"][j])
            data["matrix"].append(block["matrix"])
            data["matrix_index"].append((i, j))
    return data


def write_transfer_matrix(data, out_path, generated_key="generated", vis0_key="vis0", vis1_key="vis1"):
    """PNG grids of a comparison-matrix record (``transfer_cells``), one per matrix: <dir>/<matrix:06>_<name of out_path>.  Two header
    columns (row image, its mask visualisation), two header rows (column image, its mask visualisation), the synthesis of
    (pose i, appearance j) in the body.  Returns the written paths; without matplotlib nothing is written and that is logged."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except ImportError as e:
        LOG.warning("comparison matrix image %s not written: matplotlib is not available (%s)", out_path, e)
        return []
    written = []
    for matrix in sorted(set(data["matrix"])):
        cells = [c for c in range(len(data["matrix"])) if data["matrix"][c] == matrix]
        at = {tuple(data["matrix_index"][c]): c for c in cells}
        n = 1 + max(i for i, _ in at)
        m = 1 + max(j for _, j in at)
        S = np.asarray(data[generated_key][cells[0]]).shape[0]
        canvas = np.ones(((n + 2) * S, (m + 2) * S, 3), dtype=np.float32)

        def put(img, r, c):
            canvas[r * S:(r + 1) * S, c * S:(c + 1) * S] = np.clip((np.asarray(img, dtype=np.float32)[..., :3] + 1.0) / 2.0, 0.0, 1.0)
        for i in range(n):
            put(data["view0"][at[(i, 0)]], i + 2, 0)
            put(data[vis0_key][at[(i, 0)]], i + 2, 1)
        for j in range(m):
            put(data["view1"][at[(0, j)]], 0, j + 2)
            put(data[vis1_key][at[(0, j)]], 1, j + 2)
        for (i, j), c in at.items():
            put(data[generated_key][c], i + 2, j + 2)
        d, name = os.path.split(out_path)
        path = os.path.join(d, "{:06}_{}".format(int(matrix), name))
        plt.imsave(path, canvas)
        written.append(path)
    return written
