"""Part-segmentation evaluation helpers: the IoU protocol of cub/code/eval/eval_iclr_01/eval_01.py:229-383.

The reference takes these from the un-vendored ``denseposelib`` (``compute_best_iou_remapping``, ``remap_parts``,
``compute_iou``); semantics re-derived from their call sites: every inferred part id is mapped to the ground-truth label it
overlaps best (IoU over the whole evaluation set), the remapped prediction is scored per label, and the reported "overall"
number averages the labels except ``background`` (cub_semantic_ours.ipynb:615).  NumPy only -- outside the hot path.
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
