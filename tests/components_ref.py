"""NumPy restatements of the part-coherence definitions (include/upsparts_hip.h "part coherence"): connected
components twice, independently (a flood fill and a two-pass union-find), component sizes and per-part statistics, one clean-up
round with its effect on the export's planes, and the label patterns the tests run.  Integer arithmetic only: the device results are
compared with ==.  A map is a 2-D integer array; a pixel is valid if 0 <= label < P."""
import numpy as np

ALIGN = 16


def _valid(lab, P):
    lab = np.asarray(lab)
    if lab.dtype == np.uint8:
        return lab < P
    return (lab >= 0) & (lab < P)


def _neighbours(conn):
    assert conn in (4, 8)
    if conn == 4:
        return ((0, -1), (0, 1), (-1, 0), (1, 0))
    return ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))


def components_flood(lab, P, conn):
    """comp int32 [h,w] by flood fill: pixels are visited in raster order, so a component's seed is its smallest index."""
    lab = np.asarray(lab)
    h, w = lab.shape
    ok = _valid(lab, P)
    comp = np.full((h, w), -1, dtype=np.int32)
    nb = _neighbours(conn)
    for y in range(h):
        for x in range(w):
            if not ok[y, x] or comp[y, x] >= 0:
                continue
            seed, l = y * w + x, lab[y, x]
            comp[y, x] = seed
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and ok[ny, nx] and comp[ny, nx] < 0 and lab[ny, nx] == l:
                        comp[ny, nx] = seed
                        stack.append((ny, nx))
    return comp


def components_unionfind(lab, P, conn):
    """comp int32 [h,w] by the classical two passes: provisional labels with recorded equivalences, then their resolution; every
    class is finally named by the smallest pixel index it holds."""
    lab = np.asarray(lab)
    h, w = lab.shape
    ok = _valid(lab, P)
    parent = []

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    prov = np.full((h, w), -1, dtype=np.int64)
    back = ((0, -1), (-1, 0)) if conn == 4 else ((0, -1), (-1, -1), (-1, 0), (-1, 1))
    assert conn in (4, 8)
    for y in range(h):
        for x in range(w):
            if not ok[y, x]:
                continue
            mine = -1
            for dy, dx in back:
                ny, nx = y + dy, x + dx
                if 0 <= ny and 0 <= nx < w and ok[ny, nx] and lab[ny, nx] == lab[y, x]:
                    r = find(prov[ny, nx])
                    if mine < 0:
                        mine = r
                    elif r != mine:
                        parent[max(r, mine)] = min(r, mine)
                        mine = min(r, mine)
            if mine < 0:
                mine = len(parent)
                parent.append(mine)
            prov[y, x] = mine
    comp = np.full((h, w), -1, dtype=np.int32)
    if parent:
        roots = np.array([find(i) for i in range(len(parent))], dtype=np.int64)
        flat = prov.reshape(-1)
        idx = np.nonzero(flat >= 0)[0]
        cls = roots[flat[idx]]
        first = np.full(len(parent), h * w, dtype=np.int64)
        np.minimum.at(first, cls, idx)
        comp.reshape(-1)[idx] = first[cls].astype(np.int32)
    return comp


def areas(comp):
    """area int32 [h,w]: the pixel count of each pixel's component, 0 at invalid pixels."""
    flat = comp.reshape(-1)
    cnt = np.bincount(flat[flat >= 0], minlength=flat.size)
    return np.where(flat >= 0, cnt[np.maximum(flat, 0)], 0).astype(np.int32).reshape(comp.shape)


def stats(lab, comp, P, small):
    """(area, stats int64 [P,4], invalid) of one map: pixels, components, largest component, components with area < small."""
    lab = np.asarray(lab)
    area = areas(comp)
    ok = _valid(lab, P)
    st = np.zeros((P, 4), dtype=np.int64)
    flat_l, flat_c, flat_a = lab.reshape(-1), comp.reshape(-1), area.reshape(-1)
    roots = np.nonzero(flat_c == np.arange(flat_c.size))[0]
    for p in range(P):
        st[p, 0] = int(np.count_nonzero(ok & (lab == p)))
        a = flat_a[roots[flat_l[roots] == p]]
        st[p, 1] = a.size
        st[p, 2] = int(a.max()) if a.size else 0
        st[p, 3] = int(np.count_nonzero(a < small))
    return area, st, int(np.count_nonzero(~ok))


def accumulate_stats(prev, st):
    """What a stats table `prev` holds after a launch that found `st`: sums, and a maximum in column 2."""
    out = prev.astype(np.int64) + st
    out[..., 2] = np.maximum(prev[..., 2], st[..., 2])
    return out


def clean_round(lab, P, conn, min_area, comp=None):
    """(out, changed): one clean-up round.  Every decision is read from `lab`."""
    lab = np.asarray(lab)
    h, w = lab.shape
    comp = components_flood(lab, P, conn) if comp is None else comp
    area = areas(comp)
    ok = _valid(lab, P)
    out = lab.copy()
    changed = 0
    flat_c = comp.reshape(-1)
    for root in np.nonzero((flat_c == np.arange(h * w)) & (area.reshape(-1) < min_area))[0]:
        ys, xs = np.nonzero(comp == root)
        votes = np.zeros(P, dtype=np.int64)
        for y, x in zip(ys, xs):
            for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                ny, nx = y + dy, x + dx
                if 0 <= ny < h and 0 <= nx < w and ok[ny, nx] and area[ny, nx] >= min_area:
                    votes[lab[ny, nx]] += 1
        if votes.max() > 0:
            out[ys, xs] = int(np.argmax(votes))          # the first index of the maximum
            changed += len(ys)
    return out, changed


def to_byte(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def clean_planes(lab, out, P, colors=None, alpha=0.5, src=None, overlay=None, confidence=None, counts=None):
    """The export's planes of one image after a clean-up round lab -> out: copies of overlay [h,w,3], confidence [h,w], counts [P]
    (each may be None) changed at the relabelled pixels only -- the overlay blended anew as the render does, confidence 0, one
    count moved from the old part to the new."""
    moved = np.asarray(lab) != np.asarray(out)
    res = {}
    if overlay is not None:
        o = overlay.copy()
        col = np.asarray(colors, dtype=np.uint8)[out[moved].astype(np.int64)]
        if src is None:
            o[moved] = col
        else:
            alpha = float(alpha)
            o[moved] = to_byte(alpha * col.astype(np.float64) + (1.0 - alpha) * src[moved].astype(np.float64))
        res["overlay"] = o
    if confidence is not None:
        c = confidence.copy()
        c[moved] = 0
        res["confidence"] = c
    if counts is not None:
        n = counts.astype(np.int64).copy()
        n -= np.bincount(np.asarray(lab)[moved].astype(np.int64), minlength=P)[:P]
        n += np.bincount(np.asarray(out)[moved].astype(np.int64), minlength=P)[:P]
        res["counts"] = n
    return res


# ---------------------------------------------------------------------------------------------- packed planes
def table(sizes, chunk=1024):
    """The packing table of the export's planes (ops.segment_table): rows (pixel_offset, h, w, first_block) int32, and total."""
    rows, off, blk = [], 0, 0
    for h, w in sizes:
        rows.append((off, h, w, blk))
        blk += -(-(h * w) // chunk)
        off = -(-(off + h * w) // ALIGN) * ALIGN
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), off


def pack(maps, tab, total, dtype, fill):
    """The maps [h_i,w_i] (or [h_i,w_i,c]) in one plane [total] (or [total,c]); the alignment gaps hold `fill`."""
    tail = tuple(np.asarray(maps[0]).shape[2:])
    plane = np.full((total,) + tail, fill, dtype=dtype)
    for (off, h, w, _), m in zip(tab.tolist(), maps):
        plane[off:off + h * w] = np.asarray(m, dtype=dtype).reshape((h * w,) + tail)
    return plane


def unpack(plane, tab):
    tail = tuple(plane.shape[1:])
    return [plane[off:off + h * w].reshape((h, w) + tail) for off, h, w, _ in tab.tolist()]


# ---------------------------------------------------------------------------------------------- patterns
def spiral(h, w):
    """A one-pixel-wide spiral of part 1 in part 0 with one-pixel gaps, wound inwards from (0, 0): the longest chain of a map.  A walk
    that turns right whenever the next cell is taken, outside, or would touch an earlier turn of the spiral."""
    m = np.zeros((h, w), dtype=np.int64)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y, x, d = 0, 0, 0
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx = y + dy, x + dx
        ay, ax = y + 2 * dy, x + 2 * dx
        free = 0 <= ny < h and 0 <= nx < w and m[ny, nx] == 0
        ahead_clear = not (0 <= ay < h and 0 <= ax < w) or m[ay, ax] == 0
        if free and ahead_clear and _sides_clear(m, ny, nx, dy, dx, h, w):
            y, x = ny, nx
            m[y, x] = 1
            turns = 0
        else:
            d = (d + 1) % 4
            turns += 1
    return m


def _sides_clear(m, y, x, dy, dx, h, w):
    """The new cell (y, x) touches, by an edge, no spiral cell but the one it was entered from."""
    for sy, sx in ((dx, dy), (-dx, -dy)):                # the two cells beside the direction of travel
        ty, tx = y + sy, x + sx
        if 0 <= ty < h and 0 <= tx < w and m[ty, tx] == 1:
            return False
    return True


def serpentine(h, w):
    """Rows of part 1 on every other line, joined alternately at the right and the left end: one long component."""
    m = np.zeros((h, w), dtype=np.int64)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def combs(h, w):
    """Vertical teeth of part 1 on every other column, joined only by the last row: equivalences that appear last."""
    m = np.zeros((h, w), dtype=np.int64)
    m[:, 0::2] = 1
    m[h - 1, :] = 1
    return m


def checkerboard(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((y + x) % 2).astype(np.int64)


def diagonals(h, w, P=3):
    """Diagonal stripes one pixel wide: every pixel its own component at conn 4, whole diagonals at conn 8."""
    y, x = np.mgrid[0:h, 0:w]
    return ((y + x) % P).astype(np.int64)


def filled(h, w, p=0):
    return np.full((h, w), p, dtype=np.int64)


def noise(h, w, P, seed):
    return np.random.RandomState(seed).randint(0, P, size=(h, w)).astype(np.int64)


def with_invalid(m, P, values, seed):
    """`m` with a fifth of its pixels replaced by the invalid `values` in turn."""
    m = np.array(m, copy=True)
    rng = np.random.RandomState(seed)
    idx = np.nonzero(rng.rand(*m.shape) < 0.2)
    for k, (y, x) in enumerate(zip(*idx)):
        m[y, x] = values[k % len(values)]
    return m


def patterns(h, w):
    """[(name, map int64, P)]: every pattern of the issue at one size (valid labels only)."""
    return [("spiral", spiral(h, w), 2), ("serpentine", serpentine(h, w), 2), ("combs", combs(h, w), 2),
            ("checkerboard", checkerboard(h, w), 2), ("diagonals", diagonals(h, w), 3), ("filled", filled(h, w), 1),
            ("noise2", noise(h, w, 2, 11), 2), ("noise25", noise(h, w, 25, 12), 25)]
