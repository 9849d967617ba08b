"""GPU tests of the part-coherence kernels (csrc/components.hip): ups_label_components, ups_label_component_stats and
ups_label_components_clean through the C ABI and through ops, against the NumPy restatements of components_ref.py.  Everything is an
integer and is compared with ==.  Every output and scratch buffer sits between sentinel guard bands and is pre-filled, so that an
alignment gap that was written is visible; every launch sequence runs twice and gives the same bytes.  The shapes are the smallest at
which each failure can occur: 1 x 1, single rows and columns, sizes that are no multiple of the 32 x 32 tile, one tile exactly, and
one spiral each at 128 x 128 and 256 x 256 so that unions across many tile borders run."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
ISENT, IFILL = -0x5A5A5A5B, 0x01234567
BSENT, BFILL = 0xA5, 7
E_ARG, E_UNSUPPORTED = -1, -2
SIZES = ((1, 1), (1, 7), (7, 1), (19, 33), (33, 19), (64, 64))
NP_OF = {torch.uint8: np.uint8, torch.int64: np.int64, torch.int32: np.int32}


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


class _Guarded(object):
    """`shape` elements inside a sentinel-filled buffer with GUARD rows on each side, pre-filled with `inside` (a value or an array)."""

    def __init__(self, dev, shape, dtype, inside):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.sent = BSENT if dtype == torch.uint8 else ISENT
        self.buf = torch.full((GUARD + shape[0] + GUARD,) + shape[1:], self.sent, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + shape[0]]
        if isinstance(inside, np.ndarray):
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(inside.astype(NP_OF[dtype]))).to(dev))
        else:
            self.view.fill_(inside)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def numpy(self):
        return self.view.cpu().numpy()


def _null():
    return C.c_void_p(None)


def _launch(L, dev, maps, P, conn, dtype, small=3, min_area=4, stats0=None, gap=0, planes=None, colors=None, alpha=0.5, in_place=False):
    """components -> stats -> clean on the packed `maps` through the C ABI, everything guarded.  planes: None, or a dict of NumPy
    packed planes src / overlay / confidence / counts (each may be missing: a NULL pointer).  Returns the outputs as NumPy arrays,
    the table, and whether every guard band is intact."""
    lib = L.load()
    sizes = [m.shape for m in maps]
    tab, total = R.table(sizes)
    n = len(maps)
    th = tab.ctypes.data_as(C.POINTER(C.c_int32))
    td = torch.from_numpy(tab).to(dev)
    lab = _Guarded(dev, total, dtype, R.pack(maps, tab, total, np.int64, gap))
    assert lib.ups_label_components_scratch_bytes(total) == 0
    assert lib.ups_label_component_stats_scratch_bytes(total) == 4 * total
    assert lib.ups_label_components_clean_scratch_bytes(total) == 12 * total <= 16 * total
    o = {"comp": _Guarded(dev, total, torch.int32, IFILL), "err": _Guarded(dev, 1, torch.int32, 0),
         "area": _Guarded(dev, total, torch.int32, IFILL),
         "stats": _Guarded(dev, n * P * 4, torch.int32, 0 if stats0 is None else stats0.reshape(-1)),
         "invalid": _Guarded(dev, 1, torch.int32, 5), "changed": _Guarded(dev, 1, torch.int32, 9),
         "out": lab if in_place else _Guarded(dev, total, dtype, BFILL),
         "scratch_s": _Guarded(dev, total, torch.int32, IFILL), "scratch_c": _Guarded(dev, 3 * total, torch.int32, IFILL)}
    pl = {}
    for k in ("src", "overlay", "confidence", "counts"):
        if planes is not None and planes.get(k) is not None:
            a = planes[k]
            pl[k] = _Guarded(dev, a.shape, torch.int32 if k == "counts" else torch.uint8, a)
    col = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
    lb = 1 if dtype == torch.uint8 else 8
    s = L.stream()
    L.call("ups_label_components", lab.ptr(), lb, n, th, L.ptr(td), total, P, conn, o["comp"].ptr(), o["err"].ptr(), _null(), s)
    L.call("ups_label_component_stats", lab.ptr(), lb, o["comp"].ptr(), n, th, L.ptr(td), total, P, small, o["area"].ptr(),
           o["stats"].ptr(), o["invalid"].ptr(), o["scratch_s"].ptr(), s)
    L.call("ups_label_components_clean", lab.ptr(), lb, o["comp"].ptr(), o["area"].ptr(), n, th, L.ptr(td), total, P, min_area,
           o["out"].ptr(), o["changed"].ptr(), pl["src"].ptr() if "src" in pl else _null(), L.ptr(col), float(alpha),
           pl["overlay"].ptr() if "overlay" in pl else _null(), pl["confidence"].ptr() if "confidence" in pl else _null(),
           pl["counts"].ptr() if "counts" in pl else _null(), o["scratch_c"].ptr(), s)
    torch.cuda.synchronize(dev)
    intact = all(g.intact() for g in list(o.values()) + list(pl.values()) + [lab])
    res = {k: g.numpy() for k, g in o.items() if not k.startswith("scratch")}
    res.update({k: g.numpy() for k, g in pl.items()})
    res["stats"] = res["stats"].reshape(n, P, 4)
    return res, tab, intact


def _expected(maps, P, conn, small, min_area, np_dtype):
    """The restatement's comp / area / stats / invalid / out / changed of every map (both restatements of comp must agree)."""
    exp = []
    for m in maps:
        m = m.astype(np_dtype)
        comp = R.components_flood(m, P, conn)
        assert np.array_equal(comp, R.components_unionfind(m, P, conn))
        area, st, inv = R.stats(m, comp, P, small)
        out, changed = R.clean_round(m, P, conn, min_area, comp)
        exp.append({"comp": comp, "area": area, "stats": st, "invalid": inv, "out": out, "changed": changed})
    return exp


def _check(res, tab, intact, exp, maps, stats0=None, gap_out=BFILL, in_place_gap=None):
    assert intact, "a guard band was written"
    assert int(res["err"][0]) == 0
    n = len(maps)
    total = res["comp"].shape[0]
    inside = np.zeros(total, dtype=bool)
    for i, (off, h, w, _) in enumerate(tab.tolist()):
        inside[off:off + h * w] = True
        for k in ("comp", "area", "out"):
            got = res[k][off:off + h * w].reshape(h, w)
            assert np.array_equal(got.astype(np.int64), exp[i][k].astype(np.int64)), "{} of image {} ({} x {})".format(k, i, h, w)
        prev = np.zeros_like(exp[i]["stats"]) if stats0 is None else stats0[i]
        assert np.array_equal(res["stats"][i].astype(np.int64), R.accumulate_stats(prev, exp[i]["stats"])), "stats of image {}".format(i)
    assert (res["comp"][~inside] == IFILL).all() and (res["area"][~inside] == IFILL).all(), "an alignment gap was written"
    assert (res["out"][~inside] == (gap_out if in_place_gap is None else in_place_gap)).all(), "an alignment gap of out was written"
    assert int(res["invalid"][0]) == 5 + sum(e["invalid"] for e in exp)
    assert int(res["changed"][0]) == 9 + sum(e["changed"] for e in exp)


def _twice(L, dev, maps, P, conn, dtype, **kw):
    a, tab, ia = _launch(L, dev, maps, P, conn, dtype, **kw)
    b, _, ib = _launch(L, dev, maps, P, conn, dtype, **kw)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "two launches differ in {}".format(k)
    return a, tab, ia and ib


def _groups(h, w):
    """The patterns of one size grouped by P: each group is one packed batch (the P = 2 group has N = 5, the others N = 1)."""
    by_p = {}
    for name, m, P in R.patterns(h, w):
        by_p.setdefault(P, []).append(m)
    return sorted(by_p.items())


# ---------------------------------------------------------------------------------------------- patterns
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "{}x{}".format(*s))
def test_patterns(dev, size, conn):
    L, _ = _mods()
    assert L.load().ups_components_tile() == 32
    for P, maps in _groups(*size):
        exp = _expected(maps, P, conn, 3, 4, np.int64)
        for dtype in (torch.uint8, torch.int64):
            res, tab, intact = _twice(L, dev, maps, P, conn, dtype)
            _check(res, tab, intact, exp, maps)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("size", ((19, 33), (64, 64)), ids=lambda s: "{}x{}".format(*s))
def test_invalid_values(dev, size, conn):
    L, _ = _mods()
    P = 5
    base = R.noise(size[0], size[1], P, 21)
    m64 = R.with_invalid(base, P, (-1, P, 1 << 40), 22)
    m8 = R.with_invalid(base, P, (P, 255), 23)
    for m, dtype, npd in ((m64, torch.int64, np.int64), (m8, torch.uint8, np.uint8)):
        exp = _expected([m], P, conn, 2, 3, npd)
        assert exp[0]["invalid"] > 0 and (exp[0]["comp"] == -1).any()
        res, tab, intact = _twice(L, dev, [m], P, conn, dtype, small=2, min_area=3)
        _check(res, tab, intact, exp, [m])
        assert np.array_equal(res["out"][:m.size].reshape(m.shape)[exp[0]["comp"] < 0], m.astype(npd)[exp[0]["comp"] < 0])


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("side", (128, 256))
def test_large_spiral(dev, side, conn):
    """Every level of the kernel: 16 and 64 tiles, a chain that crosses every tile border many times."""
    L, _ = _mods()
    m = R.spiral(side, side)
    exp = _expected([m], 2, conn, 3, 4, np.int64)
    assert len(np.unique(exp[0]["comp"])) == 2
    res, tab, intact = _twice(L, dev, [m], 2, conn, torch.uint8)
    _check(res, tab, intact, exp, [m])


# ---------------------------------------------------------------------------------------------- isolation
def _row_wrap(h, w):
    """Part 1 at x = w - 1 of the even rows and x = 0 of the odd rows: neighbours in memory, never in the image."""
    m = np.zeros((h, w), dtype=np.int64)
    if w >= 3:
        m[0::2, w - 1] = 1
        m[1::2, 0] = 1
    return m


@pytest.mark.parametrize("conn", (4, 8))
def test_isolation(dev, conn):
    """Unequal sizes in one packed batch, equal labels at the facing borders of consecutive images (and in the gaps between them), and
    equal labels at x = w - 1 / x = 0 of consecutive rows: no merge across images, no row wrap."""
    L, _ = _mods()
    sizes = ((5, 9), (32, 32), (1, 1), (19, 33))
    for maps, gap in (([R.filled(h, w, 1) for h, w in sizes], 1), ([_row_wrap(h, w) for h, w in sizes], 1),
                      ([R.noise(h, w, 2, 31 + i) for i, (h, w) in enumerate(sizes)], 0)):
        exp = _expected(maps, 2, conn, 3, 4, np.int64)
        for dtype in (torch.uint8, torch.int64):
            res, tab, intact = _twice(L, dev, maps, 2, conn, dtype, gap=gap)
            _check(res, tab, intact, exp, maps)
    wrap = _expected([_row_wrap(19, 33)], 2, conn, 3, 4, np.int64)[0]
    assert wrap["stats"][1, 1] == 19                                       # every marked pixel is its own component


# ---------------------------------------------------------------------------------------------- stats
@pytest.mark.parametrize("small", (0, 7, 64 * 64 + 1))
def test_stats_accumulate(dev, small):
    L, _ = _mods()
    P = 4
    maps = [R.noise(19, 33, P, 41), R.noise(19, 33, P, 42), R.filled(19, 33, 2)]
    rng = np.random.RandomState(43)
    stats0 = rng.randint(0, 700, size=(3, P, 4)).astype(np.int64)
    exp = _expected(maps, P, 8, small, 4, np.int64)
    if small == 0:
        assert all((e["stats"][:, 3] == 0).all() for e in exp)
    if small > 64 * 64:
        assert all((e["stats"][:, 3] == e["stats"][:, 1]).all() for e in exp)
    res, tab, intact = _twice(L, dev, maps, P, 8, torch.int64, small=small, stats0=stats0)
    _check(res, tab, intact, exp, maps, stats0=stats0)


# ---------------------------------------------------------------------------------------------- clean-up
def _island_maps():
    inside = np.zeros((9, 11), dtype=np.int64)
    inside[3:5, 4:6] = 2                                  # an island of part 2 inside part 0
    tie = np.zeros((8, 10), dtype=np.int64)
    tie[:, 5:] = 1
    tie[3, 4:6] = 2                                       # on the boundary of parts 0 and 1: 3 votes each, the first (0) wins
    among = R.checkerboard(6, 7)                          # islands that touch only islands (conn 4): nothing moves
    whole = np.full((2, 3), 1, dtype=np.int64)            # one small component: stays
    return [inside, tie, among, whole]


def test_clean_cases(dev):
    L, _ = _mods()
    maps = _island_maps()
    exp = _expected(maps, 3, 4, 3, 7, np.int64)
    assert (exp[0]["out"] == 0).all() and exp[0]["changed"] == 4
    assert (exp[1]["out"][3, 4:6] == 0).all() and exp[1]["changed"] == 2
    assert np.array_equal(exp[2]["out"], maps[2]) and np.array_equal(exp[3]["out"], maps[3])
    for dtype in (torch.uint8, torch.int64):
        res, tab, intact = _twice(L, dev, maps, 3, 4, dtype, min_area=7)
        _check(res, tab, intact, exp, maps)


def test_clean_two_rounds(dev):
    """A pixel of part 2 in the middle of a small block of part 0: in round one all its neighbours are small, so it stays while the
    block around it goes to part 1; the second round then sees large neighbours and moves it too."""
    L, ops = _mods()
    m = np.ones((9, 9), dtype=np.int64)
    m[2:7, 2:7] = 0                                       # a 5 x 5 block of part 0 (24 pixels of it: small at min_area 30)
    m[4, 4] = 2                                           # a pixel of part 2 in its middle: its neighbours are all small
    r1, c1 = R.clean_round(m, 3, 8, 30)
    r2, c2 = R.clean_round(r1, 3, 8, 30)
    assert c1 == 24 and r1[4, 4] == 2 and c2 == 1 and (r2 == 1).all()
    t = torch.from_numpy(m[None]).to(dev)
    total = 0
    for rounds, want in ((1, r1), (2, r2)):
        cur = t
        for _ in range(rounds):
            comp, err = ops.label_components(cur, 3, conn=8)
            area, _, _ = ops.label_component_stats(cur, comp, 3, small=0)
            cur, changed = ops.label_components_clean(cur, comp, area, 3, 30)
            ops.components_check(err)
            total = int(changed.item())
        assert np.array_equal(cur[0].cpu().numpy(), want)
    assert total == c2


@pytest.mark.parametrize("with_src", (True, False))
def test_clean_planes(dev, with_src):
    """overlay / confidence / counts follow the relabelled pixels exactly as the restatement says, and NULL planes are skipped."""
    L, _ = _mods()
    P = 4
    maps = [R.noise(19, 33, P, 51), R.noise(5, 9, P, 52)]
    tab, total = R.table([m.shape for m in maps])
    rng = np.random.RandomState(53)
    colors = rng.randint(0, 256, size=(P, 3)).astype(np.uint8)
    src = [rng.randint(0, 256, size=m.shape + (3,)).astype(np.uint8) for m in maps]
    over = [rng.randint(0, 256, size=m.shape + (3,)).astype(np.uint8) for m in maps]
    conf = [rng.randint(1, 256, size=m.shape).astype(np.uint8) for m in maps]
    counts = np.stack([np.bincount(m.reshape(-1), minlength=P) for m in maps]).astype(np.int32)
    planes = {"src": R.pack(src, tab, total, np.uint8, 9) if with_src else None, "overlay": R.pack(over, tab, total, np.uint8, 9),
              "confidence": R.pack(conf, tab, total, np.uint8, 9), "counts": counts}
    exp = _expected(maps, P, 8, 3, 5, np.int64)
    assert sum(e["changed"] for e in exp) > 0
    res, tab, intact = _twice(L, dev, maps, P, 8, torch.uint8, min_area=5, planes=planes, colors=colors, alpha=0.375)
    _check(res, tab, intact, exp, maps)
    want_over, want_conf = planes["overlay"].copy(), planes["confidence"].copy()
    for i, (off, h, w, _) in enumerate(tab.tolist()):
        r = R.clean_planes(maps[i], exp[i]["out"], P, colors, 0.375, src[i] if with_src else None, over[i], conf[i], counts[i])
        want_over[off:off + h * w] = r["overlay"].reshape(-1, 3)
        want_conf[off:off + h * w] = r["confidence"].reshape(-1)
        assert np.array_equal(res["counts"][i].astype(np.int64), r["counts"])
        assert np.array_equal(r["counts"], np.bincount(exp[i]["out"].reshape(-1), minlength=P))
    assert np.array_equal(res["overlay"], want_over) and np.array_equal(res["confidence"], want_conf)
    # all optional planes NULL, and the round written over its own input
    res, tab, intact = _twice(L, dev, maps, P, 8, torch.uint8, min_area=5)
    _check(res, tab, intact, exp, maps)
    res, tab, intact = _launch(L, dev, maps, P, 8, torch.uint8, min_area=5, in_place=True, gap=2)
    _check(res, tab, intact, exp, maps, in_place_gap=2)


# ---------------------------------------------------------------------------------------------- the C entries' refusals
def test_refusals(dev):
    L, _ = _mods()
    lib = L.load()
    tab, total = R.table([(4, 4)])
    th, td = tab.ctypes.data_as(C.POINTER(C.c_int32)), torch.from_numpy(tab).to(dev)
    lab = torch.zeros(total, dtype=torch.uint8, device=dev)
    comp = torch.zeros(total, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    s = L.stream()

    def cc(P=2, conn=8, lb=1, table_host=th, n=1, tot=total):
        return lib.ups_label_components(L.ptr(lab), lb, n, table_host, L.ptr(td), tot, P, conn, L.ptr(comp), L.ptr(err), None, s)

    assert cc() == 0
    assert cc(P=0) == E_ARG and cc(P=256) == E_UNSUPPORTED and cc(conn=6) == E_ARG and cc(lb=4) == E_ARG and cc(n=0) == E_ARG
    big, _ = R.table([(1025, 1024)])
    assert cc(table_host=big.ctypes.data_as(C.POINTER(C.c_int32)), tot=1025 * 1024) == E_ARG            # h * w > 2^20
    bad = tab.copy()
    bad[0, 0] = 8
    assert cc(table_host=bad.ctypes.data_as(C.POINTER(C.c_int32))) == E_ARG                              # offset no multiple of 16
    area = torch.zeros(total, dtype=torch.int32, device=dev)
    st = torch.zeros(2 * 4, dtype=torch.int32, device=dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    scr = torch.zeros(3 * total, dtype=torch.int32, device=dev)
    assert lib.ups_label_component_stats(L.ptr(lab), 1, L.ptr(comp), 1, th, L.ptr(td), total, 2, -1, L.ptr(area), L.ptr(st), L.ptr(one),
                                         L.ptr(scr), s) == E_ARG
    assert lib.ups_label_components_clean(L.ptr(lab), 1, L.ptr(comp), L.ptr(area), 1, th, L.ptr(td), total, 2, 0, L.ptr(lab), L.ptr(one),
                                          None, None, 0.5, None, None, None, L.ptr(scr), s) == E_ARG
    assert lib.ups_label_components_clean(L.ptr(lab), 1, L.ptr(comp), L.ptr(area), 1, th, L.ptr(td), total, 2, 1, L.ptr(lab), L.ptr(one),
                                          None, None, 0.5, L.ptr(scr), None, None, L.ptr(scr), s) == E_ARG   # overlay without colors
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------------------------------------- through ops
@pytest.mark.parametrize("shape", ((5, 19, 33), (1, 64, 64), (2, 32, 48)), ids=lambda s: "x".join(map(str, s)))
def test_ops_regular_batch(dev, shape):
    """A regular [N,h,w] batch, also one whose h * w is no multiple of 16 (packed by the wrapper), int64 and uint8."""
    _, ops = _mods()
    N, h, w = shape
    P = 6
    maps = [R.noise(h, w, P, 60 + i) for i in range(N)]
    exp = _expected(maps, P, 8, 5, 6, np.int64)
    for dtype in (torch.int64, torch.uint8):
        t = torch.from_numpy(np.stack(maps)).to(dev).to(dtype)
        outs = []
        for _ in range(2):
            comp, err = ops.label_components(t, P, conn=8)
            area, stats, invalid = ops.label_component_stats(t, comp, P, small=5)
            out, changed = ops.label_components_clean(t, comp, area, P, 6)
            ops.components_check(err)
            outs.append([x.cpu().numpy() for x in (comp, area, stats, invalid, out, changed)])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
        comp, area, stats, invalid, out, changed = outs[0]
        assert comp.shape == (N, h, w) and out.shape == (N, h, w) and out.dtype == NP_OF[dtype]
        for i in range(N):
            assert np.array_equal(comp[i], exp[i]["comp"]) and np.array_equal(area[i], exp[i]["area"])
            assert np.array_equal(stats[i], exp[i]["stats"]) and np.array_equal(out[i], exp[i]["out"])
        assert int(invalid[0]) == 0 and int(changed[0]) == sum(e["changed"] for e in exp)


def test_ops_packed_and_errors(dev):
    L, ops = _mods()
    sizes = [(5, 9), (32, 32), (1, 1), (19, 33)]
    P = 3
    maps = [R.noise(h, w, P, 70 + i) for i, (h, w) in enumerate(sizes)]
    tab, total = ops.segment_table(sizes)
    assert np.array_equal(tab, R.table(sizes)[0])
    plane = torch.from_numpy(R.pack(maps, tab, total, np.uint8, 0)).to(dev)
    comp, err = ops.label_components(plane, P, conn=4, sizes=sizes)
    area, stats, _ = ops.label_component_stats(plane, comp, P, small=2, sizes=sizes)
    out, changed = ops.label_components_clean(plane, comp, area, P, 3, sizes=sizes, out=plane)
    ops.components_check(err)
    assert out.data_ptr() == plane.data_ptr()
    exp = _expected(maps, P, 4, 2, 3, np.int64)
    for i, got in enumerate(R.unpack(out.cpu().numpy(), tab)):
        assert np.array_equal(got, exp[i]["out"]) and np.array_equal(stats[i].cpu().numpy(), exp[i]["stats"])
    t = torch.zeros((2, 8, 8), dtype=torch.int64, device=dev)
    for bad in (lambda: ops.label_components(t.float(), 3), lambda: ops.label_components(t, 0), lambda: ops.label_components(t, 256),
                lambda: ops.label_components(t, 3, conn=6), lambda: ops.label_components(t.view(-1), 3),
                lambda: ops.label_components(t.cpu(), 3), lambda: ops.label_component_stats(t, t, 3),
                lambda: ops.label_component_stats(t, t.int(), 3, small=-1),
                lambda: ops.label_components_clean(t, t.int(), t.int(), 3, 0),
                lambda: ops.label_components(t, 3, comp=torch.zeros(5, dtype=torch.int32, device=dev)),
                lambda: ops.components_check(torch.ones(1, dtype=torch.int32, device=dev))):
        with pytest.raises(L.UpsError):
            bad()
