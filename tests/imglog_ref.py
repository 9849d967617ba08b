"""fp64 NumPy restatement of the training image logs: the img_ops of cub/code/SB_model48i/model.py:968-1053 (M) with the helpers of
cub/code/nn.py (N) they call, one function per img_op, each returning the uint8 canvas that is written as a PNG.  Plain loops over
tiles and NumPy expressions in float64 -- nothing shared with the code under test.

Two pieces of edflow are absent from the reference tree and are re-derived here (UNVERIFIED):
  quantise          edflow's save_image: byte = uint8(clip((v + 1) * 127.5, 0, 255)), truncating.  Maps the reference leaves in
                    [0,1] (level sets, edge sets, masks, p_heatmap) go through the same rule: gray (127) to white (255).
  batch_to_canvas   tf_batches.tf_batch_to_canvas(X, cols): cols=None -> rows = cols = ceil(sqrt(N)), else rows = ceil(N / cols);
                    row-major; missing tiles are value 0.  plot_batch tiles a 4-D img_op with N > 1 once more with cols=None.
"""
import math

import numpy as np

P_LEVELS = (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9)                  # M:1009
RATIOS = (1.0e-3, 5 * 1.0e-3, 1.0e-2, 5 * 1.0e-2)                   # M:1021
LEVELS_TITLE = ("m0_sample_levels" + "-{}" * len(P_LEVELS)).format(*P_LEVELS).replace(".", "_")     # M:1018-1019


def f64(x):
    """A tensor / array as float64 (bf16 and fp32 values are exact in it)."""
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def quantise(v):
    return np.clip((f64(v) + 1.0) * 127.5, 0.0, 255.0).astype(np.uint8)       # astype truncates


def canvas_grid(n, cols=None):
    """(rows, cols) of tf_batch_to_canvas for n tiles."""
    if cols is None:
        cols = int(math.ceil(math.sqrt(n)))
        return cols, cols
    return int(math.ceil(n / float(cols))), int(cols)


def batch_to_canvas(x, cols=None):
    """x [N,H,W,C] float -> [rows*H, cols*W, C] float; tile n at (n // cols, n % cols), missing tiles 0."""
    x = f64(x)
    n, h, w, c = x.shape
    rows, cols = canvas_grid(n, cols)
    out = np.zeros((rows * h, cols * w, c), dtype=np.float64)
    for i in range(n):
        r, q = divmod(i, cols)
        out[r * h:(r + 1) * h, q * w:(q + 1) * w] = x[i]
    return out


def plot_batch(x):
    """What is written for a 4-D img_op: N > 1 is tiled with cols=None, then quantised."""
    x = f64(x)
    return quantise(batch_to_canvas(x) if x.shape[0] > 1 else x[0])


def mask_colors(n_parts):
    """N:2118-2120, 2075-2077: inferno at n_parts evenly spaced points, (c - 0.5) * 2, cast to float32."""
    from matplotlib import pyplot as plt
    colors = plt.cm.inferno(np.linspace(0, 1, n_parts), alpha=False, bytes=False)[:, :3]
    return ((colors - 0.5) * 2).astype(np.float32)


def mask2rgb(mask, make_hot=True):
    """N:2067-2089: (one-hot of the arg-max over parts | the mask itself) x colours, summed over parts.  np.argmax returns the
    first maximal index, as tf.argmax does."""
    mask = f64(mask)
    P = mask.shape[3]
    hot = np.eye(P)[np.argmax(mask, axis=3)] if make_hot else mask            # N:2086-2089
    return (hot[..., None] * f64(mask_colors(P))[None, None, None]).sum(axis=3)   # N:2073-2082


def images(x):
    """view0, view1, view0_target, generated, cross, tps_* (M:1039-1053): [N,H,W,>=3] in [-1,1], the first three channels."""
    return plot_batch(f64(x)[..., :3])


def images_canvas(x, cols=None):
    """The same with an explicit column count (kernel tests)."""
    return quantise(batch_to_canvas(f64(x)[..., :3], cols))


def mask_visualization(mask):
    """out_parts_soft_visualization, m0_sample_visualization (M:968-971): visualize_mask(.., make_hot=True), M:559-562."""
    return plot_batch(mask2rgb(mask, True))


def mask_rgb_canvas(mask, cols=None, make_hot=True):
    return quantise(batch_to_canvas(mask2rgb(mask, make_hot), cols))


def coding_masks(hard):
    """encoding_masks_visualization / decoding_masks_visualization (M:973-984): the B one-hot masks side by side (cols = B), then
    mask2rgb WITHOUT arg-max; the result has batch size 1 and is written as it is."""
    hard = f64(hard)
    canvas = batch_to_canvas(hard, hard.shape[0])[None]                        # M:975 / 981
    return plot_batch(mask2rgb(canvas, False))


def masks(decoding_mask):
    """masks (M:986-988): image 0 of the decoding mask with the parts moved to the batch axis, [P,H,W,1]."""
    first = f64(decoding_mask)[:1]                                             # N:2197 take_only_first_item_in_the_batch
    return plot_batch(np.transpose(first, (3, 1, 2, 0)))


def assigned_parts(decoding_mask, encoding_mask, view0, view1):
    """assigned_parts (M:990-1007): mask_p * view for the B images of view 0 then the B of view 1, one cols=None grid per part,
    the P grids in 5 columns."""
    c0 = f64(decoding_mask)[..., None] * f64(view0)[..., :3][:, :, :, None, :]     # M:990-992  [B,H,W,P,3]
    c1 = f64(encoding_mask)[..., None] * f64(view1)[..., :3][:, :, :, None, :]     # M:994-996
    corr = np.concatenate([np.transpose(c0, (3, 0, 1, 2, 4)), np.transpose(c1, (3, 0, 1, 2, 4))], axis=1)    # M:993-998  [P,2B,H,W,3]
    grids = np.stack([batch_to_canvas(corr[p]) for p in range(corr.shape[0])])     # M:1001-1005
    return plot_batch(batch_to_canvas(grids, 5)[None])                             # M:1006


def level_sets(m0_sample):
    """m0_sample_levels-... (M:1009-1019): for part i the seven maps m[..., i] > p, parts outermost; 7 columns."""
    m = np.asarray(f64(m0_sample)[:1], dtype=np.float32)                       # M:1010; the comparison is between float32 values
    sets = [(m[0, :, :, i] > np.float32(p)).astype(np.float64) for i in range(m.shape[3]) for p in P_LEVELS]    # M:1012-1015
    return plot_batch(batch_to_canvas(np.stack(sets)[..., None], len(P_LEVELS))[None])          # M:1016-1017


def squared_grad(m):
    """N:1366-1390 on [H,W,P]: a 3x3 'SAME' correlation whose x filter is 0.5 * [0, 0.5, -0.5] in its centre row (the y filter the
    same in its centre column): gx = (m[y][x] - m[y][x+1]) / 4, zero beyond the border; gx^2 + gy^2."""
    m = f64(m)
    right = np.zeros_like(m)
    right[:, :-1] = m[:, 1:]
    down = np.zeros_like(m)
    down[:-1] = m[1:]
    gx, gy = 0.25 * (m - right), 0.25 * (m - down)
    return gx * gx + gy * gy


def edge_sets(m0_sample):
    """mumford_sha_edges (M:1021-1029): edge_set(m, 1, r) = squared gradient > r / 1 (N:1401-1404) for the four ratios; the
    transpose / reshape of M:1025-1027 puts the parts outermost; 4 columns."""
    g = squared_grad(f64(m0_sample)[0])
    sets = [(g[:, :, i] > np.float64(np.float32(r))).astype(np.float64) for i in range(g.shape[2]) for r in RATIOS]
    return plot_batch(batch_to_canvas(np.stack(sets)[..., None], len(RATIOS))[None])


def viridis():
    import matplotlib as mpl
    return np.asarray(mpl.colormaps["viridis"].colors, dtype=np.float32)       # N:2060-2061


def color_index(m):
    """N:2054-2057 with vmin 0, vmax 1: rint(m * 255), half to even as tf.round; clamped to the table."""
    return np.clip(np.rint(f64(m) * 255.0), 0, 255).astype(np.int64)


def p_heatmap(m0_sample):
    """p_heatmap (M:1031-1032): colorize(m) of image 0, parts to the batch axis."""
    idx = color_index(f64(m0_sample)[0])                                       # [H,W,P]
    return plot_batch(np.transpose(f64(viridis())[idx], (2, 0, 1, 3)))


def edge_margin(m0_sample):
    """Per pixel of the edge canvas: |g - r| / r of the fp64 squared gradient against the threshold float32(r) (same layout)."""
    g = squared_grad(f64(m0_sample)[0])
    sets = [np.abs(g[:, :, i] - np.float64(np.float32(r))) / np.float64(np.float32(r)) for i in range(g.shape[2]) for r in RATIOS]
    return batch_to_canvas(np.stack(sets)[..., None], len(RATIOS))[..., 0]


def heat_margin(m0_sample):
    """Per pixel of the p_heatmap canvas: | frac(255 m) - 0.5 | (blank tiles: 0.5, never excluded)."""
    v = f64(m0_sample)[0] * 255.0
    d = np.abs((v - np.floor(v)) - 0.5)
    canvas = batch_to_canvas(np.transpose(d, (2, 0, 1))[..., None] - 0.5)[..., 0] + 0.5
    return canvas
