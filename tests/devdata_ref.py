"""Shared by test_host_devdata.py and test_gpu_devdata.py: the NumPy restatement of ups_gather_views (csrc/dataset.hip) and the small
csv pair dataset both files train on."""
import numpy as np


def gather_ref(store, plan, with_target=True):
    """store uint8 [N,S,S,3], plan int [B,3] = (view0 source, view1 source, flip bits: 1 horizontal | 2 vertical) ->
    {"view0", "view1"[, "view0_target"]} float32 [B,S,S,3].  The pixels are flipped as whole RGB triples (the channel axis is never
    reversed) and normalised as the host path does: np.float32(u) / 127.5 - 1.0."""
    plan = np.asarray(plan)
    B, S = plan.shape[0], store.shape[1]
    out = {k: np.empty((B, S, S, 3), dtype=np.float32) for k in ("view0", "view1")}
    for b, (i0, i1, bits) in enumerate(plan):
        for key, src in (("view0", i0), ("view1", i1)):
            img = store[src]
            if bits & 1:
                img = img[:, ::-1]
            if bits & 2:
                img = img[::-1]
            out[key][b] = img.astype(np.float32) / 127.5 - 1.0
    if with_target:
        out["view0_target"] = out["view0"].copy()
    return out


def write_dataset(root, n=8, seed=0):
    """n PNGs of mixed source sizes under `root`, 3 character_ids, and the csv; returns the dataset config (spatial_size 16, both
    flips on)."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    rows = ["character_id,relative_file_path_,foo,category"]
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (20 + 3 * i, 31 - 2 * i, 3), dtype=np.uint8)).save(str(root / "im{}.png".format(i)))
        rows.append("{},im{}.png,x,bird".format(i * 3 // n, i))
    (root / "train.csv").write_text("\n".join(rows) + "\n")
    return {"data_root": str(root), "data_csv": str(root / "train.csv"), "data_csv_has_header": True,
            "data_csv_columns": ["character_id", "relative_file_path_", "foo", "category"], "spatial_size": 16,
            "data_avoid_identity": True, "data_flip_h": True, "data_flip_v": True, "batch_size": 4}
