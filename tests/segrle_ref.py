"""The run-length annotations of the segmentation export (include/upsparts_hip.h "run-length annotations"),
restated twice: once with NumPy (labels.T.ravel(), np.diff, np.flatnonzero) and once as a plain loop over the pixels.  The device
results of ups_segment_rle_count / ups_segment_rle_write are compared with these by ==.

For an h x w label map and part p the mask in COCO's column-major order is m[k] = (labels[y, x] == p), k = x h + y; T = the
ascending positions with m[k] != m[k-1] (m[-1] = 0); the counts are [T0, T1 - T0, .., h w - T_last], [h w] when T is empty.  A label
>= P belongs to no part."""
import numpy as np

ALIGN = 16          # ops.SEGMENT_ALIGN
CHUNK = 1024        # ops.SEGMENT_CHUNK


def encode_numpy(labels, p):
    """The counts of part p of an [h, w] label map: NumPy restatement."""
    labels = np.asarray(labels)
    m = (labels.T.ravel() == p).astype(np.int8)
    T = np.flatnonzero(np.diff(np.concatenate([[0], m])))
    return np.diff(np.concatenate([[0], T, [m.size]])).astype(np.int64).tolist()


def encode_loop(labels, p):
    """The same, pixel by pixel in column-major order."""
    labels = np.asarray(labels)
    h, w = labels.shape
    counts, prev, start = [], 0, 0
    for x in range(w):
        for y in range(h):
            cur = 1 if int(labels[y, x]) == p else 0
            if cur != prev:
                k = x * h + y
                counts.append(k - start)
                start, prev = k, cur
    counts.append(h * w - start)
    return counts


def decode(counts, h, w):
    """counts -> the [h, w] bool mask: alternating runs beginning with zeros, in column-major order."""
    flat = np.zeros(h * w, dtype=bool)
    at, v = 0, False
    for c in counts:
        flat[at:at + c] = v
        at, v = at + c, not v
    assert at == h * w, (at, h, w)
    return flat.reshape(w, h).T.copy()


def area_bbox(labels, p):
    """(the pixels of part p, (x_min, y_min, x_max - x_min + 1, y_max - y_min + 1)); (0, 0, 0, 0) for a part without a pixel."""
    ys, xs = np.nonzero(np.asarray(labels) == p)
    if ys.size == 0:
        return 0, (0, 0, 0, 0)
    return int(ys.size), (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def encode_all(maps, P, encode=encode_numpy):
    """A list of [h, w] maps -> {"offsets" int64 [n P + 1], "counts" int32, "area" int32 [n, P], "bbox" int32 [n, P, 4]}: what the
    device returns for the same maps."""
    offsets, counts, area, bbox = [0], [], [], []
    for m in maps:
        for p in range(P):
            c = encode(m, p)
            counts.extend(c)
            offsets.append(len(counts))
            a, b = area_bbox(m, p)
            area.append(a)
            bbox.append(b)
    n = len(maps)
    return {"offsets": np.asarray(offsets, dtype=np.int64), "counts": np.asarray(counts, dtype=np.int32),
            "area": np.asarray(area, dtype=np.int32).reshape(n, P), "bbox": np.asarray(bbox, dtype=np.int32).reshape(n, P, 4)}


def table_of(sizes):
    """ops.segment_table restated: rows (pixel_offset, h, w, first_block), total."""
    rows, off, blk = [], 0, 0
    for h, w in sizes:
        rows.append((off, h, w, blk))
        blk += -(-(h * w) // CHUNK)
        off = -(-(off + h * w) // ALIGN) * ALIGN
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), off


def pack(maps, fill=0):
    """[h_i, w_i] uint8 maps -> (plane uint8 [total] with the alignment gaps set to `fill`, table, total)."""
    table, total = table_of([m.shape for m in maps])
    plane = np.full(total, fill, dtype=np.uint8)
    for (off, h, w, _), m in zip(table.tolist(), maps):
        plane[off:off + h * w] = np.asarray(m, dtype=np.uint8).reshape(-1)
    return plane, table, total


# ------------------------------------------------------------------------------------------------------------- the cases
def blocks_map(h, w, P, seed, cell=5):
    """Block-constant labels: cells of `cell` x `cell` pixels of one seeded label each."""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, P, size=(-(-h // cell), -(-w // cell)))
    return np.kron(g, np.ones((cell, cell), dtype=np.int64))[:h, :w].astype(np.uint8)


def noise_map(h, w, P, seed):
    return np.random.RandomState(seed).randint(0, P, size=(h, w)).astype(np.uint8)


def checkerboard(h, w):
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2).astype(np.uint8)


def with_invalid(m, P, seed):
    """`m` with the bytes P and 255 sprinkled in (about one pixel in five)."""
    rng = np.random.RandomState(seed)
    out = m.copy()
    r = rng.rand(*m.shape)
    out[r < 0.1] = min(P, 255)
    out[r > 0.9] = 255
    return out


def change_at(h, w, k):
    """Label 0 before column-major position k, label 1 from k on."""
    flat = np.zeros(h * w, dtype=np.uint8)
    flat[k:] = 1
    return flat.reshape(w, h).T.copy()


def host_cases(C=CHUNK):
    """(name, map, P) for the CPU tests and the single-image GPU cases; C is the kernel's chunk."""
    cases = []
    for h, w in ((1, 1), (1, 7), (7, 1), (1, C - 1), (C, 1), (C + 1, 1), (C // 2, 2), (3, (C + 1) // 3 + 1), (37, 29), (70, 50)):
        cases.append(("noise_{}x{}".format(h, w), noise_map(h, w, 3, h * 31 + w), 3))
        cases.append(("blocks_{}x{}".format(h, w), blocks_map(h, w, 4, h * 17 + w), 4))
    cases.append(("constant", np.full((37, 29), 1, dtype=np.uint8), 2))
    cases.append(("leading_zero", np.pad(np.zeros((5, 4), dtype=np.uint8), ((0, 3), (0, 3)), constant_values=1), 2))
    cases.append(("checkerboard", checkerboard(37, 29), 2))
    cases.append(("checkerboard_first_one", 1 - checkerboard(70, 50), 2))        # (even height: no change at a column's end)
    cases.append(("checkerboard_odd", checkerboard(71, 49), 2))
    cases.append(("change_at_C", change_at(70, 50, C), 2))
    cases.append(("change_at_C-1", change_at(70, 50, C - 1), 2))
    cases.append(("change_at_4C", change_at(97, 61, 4 * C), 2))
    cases.append(("invalid_P3", with_invalid(noise_map(37, 29, 3, 5), 3, 6), 3))
    cases.append(("invalid_blocks", with_invalid(blocks_map(70, 50, 10, 7), 10, 8), 10))
    cases.append(("P1", noise_map(37, 29, 2, 9), 1))
    cases.append(("P10", noise_map(70, 50, 10, 10), 10))
    cases.append(("P255", np.random.RandomState(11).randint(0, 256, size=(70, 50)).astype(np.uint8), 255))
    cases.append(("tall_3_columns", blocks_map(5000, 3, 4, 12, cell=3), 4))             # (the position-by-position read of the kernel)
    cases.append(("tall_noise", noise_map(3001, 2, 3, 13), 3))
    cases.append(("wide_2_rows", noise_map(2, 3001, 3, 14), 3))
    return cases


def pass_of_nine():
    """Nine images of different sizes, P = 4; packed by the caller with the gaps filled with a valid label."""
    sizes = ((37, 29), (1, 1), (70, 50), (7, 1), (1, 7), (33, 31), (64, 16), (5, 205), (41, 25))
    return [(noise_map(h, w, 4, 100 + i) if i % 2 else blocks_map(h, w, 4, 100 + i)) for i, (h, w) in enumerate(sizes)], 4
