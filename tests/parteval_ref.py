"""Shared by test_host_parteval.py and test_gpu_parteval.py: the label-map cases of the counts route (evalutil.confusion_counts /
evaluate_from_counts against evaluate_parts), a model stand-in for the host tests and the small csv dataset with label images."""
import numpy as np


def iou_case():
    """The arrays of test_host.py::test_part_iou_evaluation."""
    gt = np.zeros((2, 8, 8), dtype=np.int64)
    gt[:, :4, :4] = 1
    gt[:, 4:, 4:] = 2
    pred = np.full((2, 8, 8), 7, dtype=np.int64)
    pred[:, :4, :4] = 3
    pred[:, 4:, 4:] = 5
    pred[0, 4, 4] = 3
    return pred, gt


def random_case(seed):
    """N <= 4 maps of 8 x 8, P <= 6 part ids, G <= 4 labels (at least two, one of them not the background, so `overall` is a number)."""
    rng = np.random.RandomState(1000 + seed)
    N, P, G = rng.randint(1, 5), rng.randint(1, 7), rng.randint(2, 5)
    pred = rng.randint(0, P, (N, 8, 8)).astype(np.int64)
    gt = rng.randint(0, G, (N, 8, 8)).astype(np.int64)
    if seed % 3 == 0:           # blocky maps: equal quotients and empty intersections are likelier than in noise
        pred = np.repeat(np.repeat(rng.randint(0, P, (N, 2, 2)), 4, axis=1), 4, axis=2).astype(np.int64)
        gt = np.repeat(np.repeat(rng.randint(0, G, (N, 4, 4)), 2, axis=1), 2, axis=2).astype(np.int64)
    gt[0, 0, 0] = 1
    return pred, gt


def crafted_cases():
    """name -> (pred, gt): one case per tie rule of evaluate_parts."""
    cases = {}
    # part 0 = pixels {1, 2}: IoU with label 0 (pixels 0-1) is 1 / 3, with label 1 (pixels 2-3) is 1 / 3: the lower label wins
    gt = np.array([[[0, 0, 1, 1], [2, 2, 2, 2]]], dtype=np.int64)
    pred = np.array([[[1, 0, 0, 1], [1, 1, 1, 1]]], dtype=np.int64)
    cases["equal_quotients_lower_label_wins"] = (pred, gt)
    # the same quotient from different integers: part 0 = pixels {0, 1, 2} has 1 / 3 with label 0 (pixel 0) and 2 / 6 with label 1
    # (pixels 1-5): equal as float64 quotients, so label 0 stays (a cross-multiplied comparison would agree; a rounded one must too)
    gt = np.array([[[0, 1, 1, 1, 1, 1, 2, 2]]], dtype=np.int64)
    pred = np.array([[[0, 0, 0, 1, 1, 1, 2, 2]]], dtype=np.int64)
    cases["equal_quotients_other_integers"] = (pred, gt)
    pred, gt = iou_case()
    cases["part_ids_that_never_occur"] = (pred, gt)                 # ids 0, 1, 2, 4, 6 of P = 8 occur nowhere
    gt2 = gt.copy()
    gt2[1][gt2[1] == 2] = 0
    cases["label_missing_from_one_image"] = (pred, gt2)
    gt3 = gt.copy()
    gt3[gt3 == 1] = 3
    cases["label_missing_from_the_set"] = (pred, gt3)               # labels 0, 2, 3: column 1 of G = 4 is empty
    cases["one_image"] = (pred[:1], gt[:1])
    cases["pred_equals_gt"] = (gt.copy(), gt.copy())
    return cases


def all_cases():
    cases = {"test_part_iou_evaluation": iou_case()}
    cases.update(crafted_cases())
    cases.update({"random{:02}".format(s): random_case(s) for s in range(20)})
    return cases


def sizes(pred, gt):
    return int(pred.max()) + 1, int(gt.max()) + 1


class StubModel(object):
    """What PartEvaluator needs of a TrainModel, on the host; `segment` must not be reached by the tests that use it."""
    n_parts = 3

    def __init__(self):
        import torch
        self.device = torch.device("cpu")
        self.config = {"batch_size": 2, "spatial_size": 8}

    def segment(self, views):
        raise AssertionError("segment was reached")


def block_labels(rng, n, S, n_labels=3):
    """[n,S,S] uint8 label maps made of 4 x 4 blocks (S % 4 == 0), every label present in the first map."""
    small = rng.randint(0, n_labels, (n, S // 4, S // 4))
    small[0].reshape(-1)[:n_labels] = np.arange(n_labels)
    return np.repeat(np.repeat(small, 4, axis=1), 4, axis=2).astype(np.uint8)


def write_label_dataset(root, n=5, S=16, seed=0, name="eval"):
    """n PNG views and n 8-bit label PNGs (3 labels, already S x S) under `root` with <name>.csv; returns the dataset keys."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    labels = block_labels(rng, n, S)
    rows = ["character_id,relative_file_path_,seg"]
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (S + 4, S + 2, 3), dtype=np.uint8)).save(str(root / "{}_im{}.png".format(name, i)))
        Image.fromarray(labels[i], mode="L").save(str(root / "{}_seg{}.png".format(name, i)))
        rows.append("{},{}_im{}.png,{}_seg{}.png".format(i // 2, name, i, name, i))
    (root / (name + ".csv")).write_text("\n".join(rows) + "\n")
    return {"dataset": "eddata.stochastic_pair.StochasticPairs", "data_root": str(root), "data_csv": str(root / (name + ".csv")),
            "data_csv_has_header": True, "data_csv_columns": ["character_id", "relative_file_path_", "seg"],
            "data_gt_segmentation_column": "seg", "data_avoid_identity": False}
