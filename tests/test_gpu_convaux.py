"""Edge parity of the convolution helper kernels of csrc/conv_aux.hip -- ups_weight_prep, ups_weight_prep_batch (with
ups_prep_item_blocks), ups_weight_prep_d2s, ups_weight_prep_f8, ups_coord_table, ups_batch_sum, ups_coord_wgrad, ups_col_sum --
through the C ABI, against the restatements of convaux_ref.py: bit for bit wherever the arithmetic is exact (index permutations,
one rounding, integer or dyadic sums), within the forward error bound of the kernel's own summation elsewhere (the fraction of the
bound used is printed before it is asserted).  parity_ledger.md, section 11, has the branch -> case table.

Every destination is a view into a larger allocation: the payload pre-filled with 0x55 bytes (NaN for fp32 results), 64 elements of
0xa5 bytes behind it and, where the destination is handed in as a view, in front of it; the bands are asserted untouched."""
import ctypes as C

import pytest
import torch

import convaux_ref as A

pytestmark = pytest.mark.gpu

F32, BF16, F16 = A.F32, A.BF16, A.F16
DTYPES = [BF16, F16, F32]
BAND = 64
SENT = -777.0           # pre-fill of gradV: only the coordinate rows may change


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _refused(lib, name, *args):
    """The call is refused by the entry point's argument check (which is before any launch), not by the runtime."""
    with pytest.raises(lib.UpsError) as e:
        lib.call(name, *args)
    assert "argument check failed" in str(e.value), str(e.value)


def _ids(c):
    return c[0] if isinstance(c[0], str) else "x".join(map(str, c))


class Dest(object):
    """`n` elements of `tdtype` inside an allocation of lead + n + BAND: payload 0x55 bytes (or NaN), the rest 0xa5 bytes."""

    def __init__(self, n, tdtype, dev, view=False, nan=False):
        es = torch.empty((), dtype=tdtype).element_size()
        lead = BAND if view else 0
        self.buf = torch.full(((lead + n + BAND) * es,), 0xa5, dtype=torch.uint8, device=dev)
        self.lo, self.hi = lead * es, (lead + n) * es
        self.t = self.buf[self.lo:self.hi].view(tdtype)
        self.nan = nan
        if nan:
            self.t.fill_(float("nan"))
        else:
            self.buf[self.lo:self.hi] = 0x55
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def bands_ok(self):
        return bool((self.buf[:self.lo] == 0xa5).all()) and bool((self.buf[self.hi:] == 0xa5).all())

    def untouched(self):
        return self.bands_ok() and bool((torch.isnan(self.t) if self.nan else self.buf[self.lo:self.hi] == 0x55).all())


def _same_bits(got, want, what):
    got, want = A.bits(got.cpu()), A.bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("{}: {} of {} elements differ, first at {}: got bits {:#x}, want {:#x}".format(
            what, len(bad), got.numel(), i, int(got[i]) & 0xffffffff, int(want[i]) & 0xffffffff))


def _axy(hi, wi):
    """(ax, ay) of a launch, formed as ops.py forms them at each of its call sites -- not by convaux_ref.axy, which the references use:
    a reference that pairs ax with the width must not move the launch with it."""
    return 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)


def _i9(v):
    return (C.c_int32 * 9)(*(list(v) + [0] * (9 - len(v))))


# ----------------------------------------------------------------------------- ups_weight_prep
def _prep_layer(lib, dev, Vd, ntaps, cin_v, ci_log, co, dtype, fwd=True, dgrad=True):
    """One ups_weight_prep launch into guarded destinations -> (w_fwd, w_dgrad) on the device, None where not asked for."""
    bk, td = A.bk_of(dtype), A.TORCH_DT[dtype]
    ci_pad, dk = A.round8(ci_log), A.round8(co)
    wf = Dest(ntaps * A.cdiv(ci_pad, bk) * co * bk, td, dev, view=True) if fwd else None
    wd = Dest(ntaps * A.cdiv(dk, bk) * ci_log * bk, td, dev) if dgrad else None
    lib.call("ups_weight_prep", lib.ptr(Vd), ntaps, cin_v, ci_log, co, dtype, wf.ptr() if fwd else None, ci_pad,
             wd.ptr() if dgrad else None, ci_log, dk, lib.stream())
    torch.cuda.synchronize()
    for d in (wf, wd):
        assert d is None or d.bands_ok(), "written outside the image"
    return (wf.t if fwd else None), (wd.t if dgrad else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=A.DT_NAME.get)
@pytest.mark.parametrize("case", A.PREP_CASES, ids=_ids)
def test_weight_prep_layouts(case, dtype, dev):
    """Both images bit for bit: ragged co, ci_pad > ci_log, a second k-chunk that is mostly padding, CoordConv rows left out;
    +-0, fp32 denormals and (fp16) values past +-65504 among the weights; then each image alone, the other pointer NULL."""
    lib, ops = _mods()
    name, k, ci_log, coords, co = case
    ntaps, cin_v = k * k, ci_log + (2 if coords else 0)
    V = A.edge_weights((ntaps, cin_v, co), 11, dtype)
    Vd = V.to(dev)
    want_f, want_d = A.blocked_k(V, ntaps, ci_log, co, A.round8(ci_log), ci_log, A.round8(co), dtype)
    for fwd, dgrad in ((True, True), (True, False), (False, True)):
        wf, wd = _prep_layer(lib, dev, Vd, ntaps, cin_v, ci_log, co, dtype, fwd, dgrad)
        if fwd:
            _same_bits(wf.view(want_f.shape), want_f, "{} w_fwd ({}, {})".format(name, fwd, dgrad))
        if dgrad:
            _same_bits(wd.view(want_d.shape), want_d, "{} w_dgrad ({}, {})".format(name, fwd, dgrad))


def test_weight_prep_grid_stride_trips(dev):
    """3x3, 512 -> 512 in bf16: 4.7 M elements on 8192 x 256 threads, the loop's second and third trip (w_dgrad begins inside the
    second)."""
    lib, ops = _mods()
    name, k, ci_log, coords, co = A.PREP_BIG
    V = A.edge_weights((9, ci_log, co), 12, BF16)
    want_f, want_d = A.blocked_k(V, 9, ci_log, co, ci_log, ci_log, co, BF16)
    assert want_f.numel() + want_d.numel() > 2 * 8192 * 256
    wf, wd = _prep_layer(lib, dev, V.to(dev), 9, ci_log, ci_log, co, BF16)
    _same_bits(wf.view(want_f.shape), want_f, "w_fwd")
    _same_bits(wd.view(want_d.shape), want_d, "w_dgrad")


# ----------------------------------------------------------------------------- ups_weight_prep_batch
def _table_layer(lib, dev, Vd, it):
    hi, wi = it.hw
    ax, ay = _axy(hi, wi)
    tab = Dest(64 * 3 * it.co, torch.float32, dev, nan=True)
    lib.call("ups_coord_table", lib.ptr(Vd), it.k, it.k, it.ci_log, it.co, _i9([r for r in A.taps(hi, it.k, it.stride) for _ in range(it.k)]),
             _i9(A.taps(wi, it.k, it.stride)), it.stride, it.stride, ax, ay, tab.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert tab.bands_ok()
    return tab.t


def _batch(lib, dev, items, dtype, seed_of):
    """One ups_weight_prep_batch launch over `items` -> (prefix, [per item: dict name -> device tensor or None, V, Vd])."""
    td, bk = A.TORCH_DT[dtype], A.bk_of(dtype)
    arr = (lib.PrepItem * len(items))()
    keep, prefix = [], [0]
    h = lib.load()
    for i, it in enumerate(items):
        ntaps, cin_v, ci_pad, drows, dk, nf, nd, nc = A.item_geometry(it, dtype)
        V = A.item_weights(it, seed_of(it), dtype)
        flat = torch.full((it.lead + V.numel() + 4,), float("nan"), dtype=torch.float32, device=dev)
        flat[it.lead:it.lead + V.numel()] = V.view(-1).to(dev)
        Vd = flat[it.lead:it.lead + V.numel()]
        assert Vd.data_ptr() % 16 == 4 * (it.lead % 4)
        d = {"w_fwd": Dest(nf, td, dev, view=True) if it.fwd else None, "w_dgrad": Dest(nd, td, dev) if it.dgrad else None,
             "ctab": Dest(3 * nc, torch.float32, dev, nan=True) if it.tab else None}
        p = arr[i]
        p.src = Vd.data_ptr()
        for n in d:
            setattr(p, n, d[n].t.data_ptr() if d[n] is not None else None)
        p.ntaps, p.cin_v, p.ci_log, p.co, p.ci_pad, p.dgrad_rows, p.dgrad_k = ntaps, cin_v, it.ci_log, it.co, ci_pad, drows, dk
        p.kh = p.kw = it.k
        p.in_sy = p.in_sx = it.stride
        dy, dx = A.taps(it.hw[0], it.k, it.stride), A.taps(it.hw[1], it.k, it.stride)
        for r in range(3):
            p.dy[r], p.dx[r] = (dy[r], dx[r]) if r < it.k else (0, 0)
        p.ax, p.ay = _axy(*it.hw)
        prefix.append(prefix[-1] + h.ups_prep_item_blocks(C.byref(p), dtype))
        keep.append((d, V, Vd, flat))
    items_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    prefix_dev = torch.tensor(prefix, dtype=torch.int64, device=dev)
    lib.call("ups_weight_prep_batch", lib.ptr(items_dev), lib.ptr(prefix_dev), len(items), prefix[-1], dtype, lib.stream())
    torch.cuda.synchronize()
    return prefix, keep


def _seed_by_shape(it):
    return 100 + 7 * it.k + 3 * it.ci_log + it.co + (1000 if it.coords else 0)


def _check_items(lib, dev, items, keep, dtype, what):
    """Every item of a batched launch: bit for bit against blocked_k and against the per-layer launches; the table within its bound
    against coord_table and bit for bit against ups_coord_table.  Returns the largest fraction of the table bound used."""
    worst = 0.0
    for it, (d, V, Vd, _) in zip(items, keep):
        ref = A.item_reference(it, V, dtype)
        ntaps, cin_v = A.item_geometry(it, dtype)[:2]
        for dd in d.values():
            assert dd is None or dd.bands_ok(), (what, it.name)
        lf, ld = _prep_layer(lib, dev, Vd, ntaps, cin_v, it.ci_log, it.co, dtype, it.fwd, it.dgrad)
        for n, layer in (("w_fwd", lf), ("w_dgrad", ld)):
            if ref[n] is not None:
                _same_bits(d[n].t.view(ref[n].shape), ref[n], "{} {} {}".format(what, it.name, n))
                _same_bits(d[n].t, layer.cpu(), "{} {} {} against the per-layer launch".format(what, it.name, n))
        if it.tab:
            got = d["ctab"].t.view(64, 3, it.co).cpu()
            frac = A.fraction_used(got, ref["ctab"], A.sum_bound(A.TABLE_D, ref["ctab_abs"]))
            worst = max(worst, frac)
            assert frac <= 1.0, (what, it.name, frac)
            _same_bits(d["ctab"].t, _table_layer(lib, dev, Vd, it).cpu(), "{} {} table against ups_coord_table".format(what, it.name))
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=A.DT_NAME.get)
def test_weight_prep_batch_list(dtype, dev):
    """The eight items of convaux_ref.BATCH_ITEMS in one launch: the 4-chunk unit, its j + 4 > chunks-per-block fallback (item
    co64_coord starts at chunk 14 of a block; asserted here from the prefix this launch used, and path by path in
    test_host_convaux), the 8-channel path, the scalar path, the table tail, an unaligned src (same bits as its aligned twin), items
    without w_fwd / without w_dgrad, item boundaries inside blocks, a last block that is not full."""
    lib, ops = _mods()
    items = A.BATCH_ITEMS
    prefix, keep = _batch(lib, dev, items, dtype, _seed_by_shape)
    cpb = lib.load().ups_prep_chunks_per_block()
    names = [it.name for it in items]
    if dtype != F32:
        assert prefix == A.BATCH_PREFIX_16BIT and prefix[names.index("co64_coord")] % cpb == 14
        routes = A.batch_routes(items, prefix, dtype, cpb)
        assert [r[1:] for r in routes if r[0] == names.index("co64_coord")][:5] == \
            [(0, 14, "turn8"), (1, 15, "turn8"), (2, 0, "turn8"), (3, 1, "turn8"), (4, 2, "unit4")]
    worst = _check_items(lib, dev, items, keep, dtype, A.DT_NAME[dtype])
    print("batched list {}: prefix {}, table bound used {:.3f}".format(A.DT_NAME[dtype], prefix, worst))
    a, b = keep[names.index("co64_aligned")], keep[names.index("co64_view")]
    assert torch.equal(a[1], b[1]) and a[2].data_ptr() % 16 == 0 and b[2].data_ptr() % 16 == 4
    for n in ("w_fwd", "w_dgrad"):
        _same_bits(b[0][n].t, a[0][n].t.cpu(), "unaligned src against its aligned twin, " + n)


def test_weight_prep_batch_single_chunk(dev):
    """total_blocks = 1: one item of one chunk."""
    lib, ops = _mods()
    items = [A.item("one_chunk", 1, 8, False, 8, dgrad=False)]
    prefix, keep = _batch(lib, dev, items, BF16, _seed_by_shape)
    assert prefix == [0, 1]
    _check_items(lib, dev, items, keep, BF16, "single chunk")


def test_weight_prep_batch_tables_against_coord_table(dev):
    """Every map and (k, stride) of the ups_coord_table cases as one item each of ONE bf16 launch (the table arithmetic does not
    depend on the dtype): the table tail of the batched launch has the bits of ups_coord_table."""
    lib, ops = _mods()
    items = [A.item("tab_{}x{}_k{}s{}".format(hi, wi, k, s), k, 8, True, 16, hw=(hi, wi), stride=s)
             for hi, wi in A.TABLE_DYADIC + A.TABLE_GAUSS for k, s in A.TABLE_KS]
    prefix, keep = _batch(lib, dev, items, BF16, lambda it: 300 + it.hw[0] + it.k)
    worst = _check_items(lib, dev, items, keep, BF16, "tables")
    print("{} table items in one launch: bound used {:.3f}".format(len(items), worst))


def test_weight_prep_batch_prefix_in_global_memory(dev):
    """1030 items of 1x1 8 -> 8 (one forward chunk on the 8-channel path, one input-gradient chunk on the scalar path): more than the
    1024 prefix entries held in LDS, so every block searches the prefix in global memory.  All images are slices of one allocation
    with 64-element sentinel gaps between them."""
    lib, ops = _mods()
    h = lib.load()
    n = 1030
    assert n > h.ups_prep_lds_items()
    V = torch.randn(n, 1, 8, 8, generator=A.gen(77)) * 0.25
    Vd = V.to(dev)
    slot = BAND + 256
    store = torch.full((n * 2 * slot + BAND,), 0x5555, dtype=torch.int16, device=dev)
    grid = store[:n * 2 * slot].view(n, 2, slot)
    grid[:, :, :BAND] = -0x5a5b            # 0xa5a5
    store[n * 2 * slot:] = -0x5a5b
    arr = (lib.PrepItem * n)()
    prefix = [0]
    for i in range(n):
        p = arr[i]
        p.src = Vd.data_ptr() + i * 256
        p.w_fwd = store.data_ptr() + 2 * ((i * 2 + 0) * slot + BAND)
        p.w_dgrad = store.data_ptr() + 2 * ((i * 2 + 1) * slot + BAND)
        p.ctab = None
        p.ntaps, p.cin_v, p.ci_log, p.co, p.ci_pad, p.dgrad_rows, p.dgrad_k = 1, 8, 8, 8, 8, 8, 8
        p.kh = p.kw = p.in_sy = p.in_sx = 1
        prefix.append(prefix[-1] + h.ups_prep_item_blocks(C.byref(p), BF16))
    assert prefix[-1] == 2 * n
    items_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    prefix_dev = torch.tensor(prefix, dtype=torch.int64, device=dev)
    lib.call("ups_weight_prep_batch", lib.ptr(items_dev), lib.ptr(prefix_dev), n, prefix[-1], BF16, lib.stream())
    torch.cuda.synchronize()
    got = grid.cpu()
    assert bool((got[:, :, :BAND] == -0x5a5b).all()) and bool((store[n * 2 * slot:] == -0x5a5b).all()), "a sentinel gap was written"
    want = torch.empty(n, 2, 256, dtype=torch.bfloat16)
    for i in range(n):
        wf, wd = A.blocked_k(V[i], 1, 8, 8, 8, 8, 8, BF16)
        want[i, 0], want[i, 1] = wf.view(-1), wd.view(-1)
    _same_bits(got[:, :, BAND:].contiguous().view(torch.bfloat16), want, "1030 items")


# ----------------------------------------------------------------------------- ups_weight_prep_d2s
@pytest.mark.parametrize("pad_y,pad_x", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("case", A.D2S_CASES, ids=_ids)
def test_weight_prep_d2s(case, pad_y, pad_x, dev):
    """co = 32 / 40 / 3 / 64 (whole, ragged, below one piece, two chunks), C = ci_log and C > ci_log (rows of zero channels), the
    CoordConv rows of V left out, all four pad pairs: bit for bit."""
    lib, ops = _mods()
    ci_log, Cc, co = case
    V = A.edge_weights((9, ci_log + 2, co), 13 + co, BF16)
    want = A.d2s_image(V, ci_log, co, pad_y, pad_x, Cc)
    w = Dest(want.numel(), torch.bfloat16, dev, view=True)
    lib.call("ups_weight_prep_d2s", lib.ptr(V.to(dev)), ci_log + 2, ci_log, co, pad_y, pad_x, Cc, w.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert w.bands_ok()
    _same_bits(w.t.view(want.shape), want, "d2s {} pads ({}, {})".format(case, pad_y, pad_x))


# ----------------------------------------------------------------------------- ups_weight_prep_f8
@pytest.mark.parametrize("transpose", [0, 1], ids=["fwd", "transposed"])
@pytest.mark.parametrize("case", A.F8_CASES, ids=_ids)
def test_weight_prep_f8(case, transpose, dev):
    """Bytes and deq bit for bit on Gaussian weights: k-chunk padding, kdim not a multiple of 64 / of 4, CoordConv rows that must
    not enter the row maximum, an all-zero row, a row with maximum 2^-100, a row that holds +-max."""
    lib, ops = _mods()
    name, k, ci_log, coords, co = case
    V = A.f8_weights(case, 21)
    want_b, want_q = A.f8_rows(V, k * k, ci_log, co, transpose)
    wq = Dest(want_b.numel(), torch.uint8, dev, view=True)
    deq = Dest(want_q.numel(), torch.float32, dev, nan=True)
    lib.call("ups_weight_prep_f8", lib.ptr(V.to(dev)), k * k, V.shape[1], ci_log, co, transpose, wq.ptr(), deq.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert wq.bands_ok() and deq.bands_ok()
    _same_bits(deq.t, want_q, "{} deq".format(name))
    _same_bits(wq.t.view(want_b.shape), want_b, "{} bytes".format(name))


# ----------------------------------------------------------------------------- ups_coord_table
def _table_case(lib, dev, hi, wi, k, stride, co, integer, seed):
    ci_log = 8
    V = A.int_weights((k * k, ci_log + 2, co), seed) if integer else torch.randn(k * k, ci_log + 2, co, generator=A.gen(seed))
    it = A.item("t", k, ci_log, True, co, hw=(hi, wi), stride=stride)
    got = _table_layer(lib, dev, V.to(dev), it).view(64, 3, co).cpu()
    dy, dx = A.taps(hi, k, stride), A.taps(wi, k, stride)
    ax, ay = A.axy(hi, wi)
    want = A.coord_table(V, k, ci_log, co, dy, dx, stride, ax, ay)
    absr = A.coord_table(V, k, ci_log, co, dy, dx, stride, ax, ay, absolute=True)
    assert bool(torch.isfinite(got).all())
    return got, want, absr


@pytest.mark.parametrize("k,stride", A.TABLE_KS)
@pytest.mark.parametrize("hi,wi", A.TABLE_DYADIC)
def test_coord_table_dyadic(hi, wi, k, stride, dev):
    """hi - 1 and wi - 1 powers of two, integer coordinate rows: every product and sum is exact, bit for bit (h != w: ax belongs
    to H and multiplies the COLUMN offset)."""
    lib, ops = _mods()
    got, want, absr = _table_case(lib, dev, hi, wi, k, stride, 16, True, 40 + hi)
    assert float(want.abs().max()) > 0
    _same_bits(got, (want + 0.0).float(), "table {}x{} k{} s{}".format(hi, wi, k, stride))


@pytest.mark.parametrize("k,stride", A.TABLE_KS)
@pytest.mark.parametrize("hi,wi", A.TABLE_GAUSS)
def test_coord_table_gauss(hi, wi, k, stride, dev):
    """Gaussian rows, co = 130 (a second block of 128 channels, ragged): every entry within (18 + 2) 2^-24 sum |terms|."""
    lib, ops = _mods()
    got, want, absr = _table_case(lib, dev, hi, wi, k, stride, 130, False, 50 + hi)
    frac = A.fraction_used(got, want, A.sum_bound(A.TABLE_D, absr))
    print("table {}x{} k{} s{}: bound used {:.3f}".format(hi, wi, k, stride, frac))
    assert frac <= 1.0


def test_ops_layer_copies_at_a_dyadic_map(dev):
    """What ops.ConvLayer.prepared itself launches (its own ax, ay, taps, ci_pad and dgrad_k) on a 17 x 33 map with integer
    coordinate rows: both images and the table bit for bit."""
    lib, ops = _mods()
    k, ci_log, co, hi, wi = 3, 20, 10, 17, 33
    V = A.edge_weights((9, ci_log + 2, co), 14, BF16)
    V[:, ci_log:] = A.int_weights((9, 2, co), 15)
    lay = ops.ConvLayer("t/conv2d_0", V.view(3, 3, ci_log + 2, co).to(dev), torch.zeros(co, device=dev), k, 1, True, "leaky_relu")
    ops.WeightVersion.value += 1
    ent = lay.prepared(lib.BF16, hi, wi)
    torch.cuda.synchronize()
    it = A.item("layer", k, ci_log, True, co, hw=(hi, wi))
    ref = A.item_reference(it, V, BF16)
    _same_bits(ent["w_fwd"], ref["w_fwd"], "w_fwd")
    _same_bits(ent["w_dgrad"], ref["w_dgrad"], "w_dgrad")
    _same_bits(ent["ctab"], (ref["ctab"] + 0.0).float(), "ctab")


# ----------------------------------------------------------------------------- ups_batch_sum
def _sum_input(shape, co, tdtype, seed):
    """Integers in [-4, 4]; the padding channels [co, ldo) hold +-3e4."""
    x = torch.randint(-4, 5, shape, generator=A.gen(seed)).float()
    if shape[-1] > co:
        sign = torch.randint(0, 2, shape[:-1] + (shape[-1] - co,), generator=A.gen(seed + 1)).float() * 2 - 1
        x[..., co:] = 3e4 * sign
    return x.to(tdtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=A.DT_NAME.get)
@pytest.mark.parametrize("case", A.BATCH_SUM_CASES, ids=_ids)
def test_batch_sum(case, dtype, dev):
    """Exact on integers: one image, n past the unroll of 4, co below one 16-byte piece, co not a multiple of it with ldo > co (the
    output stride is co, the padding channels do not reach it)."""
    lib, ops = _mods()
    n, pix, co, ldo = case
    x = _sum_input((n, pix, ldo), co, A.TORCH_DT[dtype], 60 + n)
    want = A.batch_sum(x, co)
    g = Dest(pix * co, torch.float32, dev, view=True, nan=True)
    lib.call("ups_batch_sum", lib.ptr(x.to(dev)), dtype, n, pix, co, ldo, g.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert g.bands_ok()
    got = g.t.view(pix, co).cpu().double()
    assert torch.equal(got, want), int((got != want).sum())


def test_batch_sum_grid_stride_trip(dev):
    """bf16 (2, 65536, 520, 520): 65536 x 65 pieces on 16384 x 256 threads, a second trip for the first 65 536 threads.  Inputs and
    the exact integer sum are made on the device."""
    lib, ops = _mods()
    n, pix, co, ldo = A.BATCH_SUM_BIG
    x = torch.randint(-4, 5, (n, pix, ldo), device=dev, dtype=torch.int8).to(torch.bfloat16)
    want = x[0].float() + x[1].float()
    g = Dest(pix * co, torch.float32, dev, nan=True)
    lib.call("ups_batch_sum", lib.ptr(x), BF16, n, pix, co, ldo, g.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert g.bands_ok()
    same = torch.equal(g.t.view(pix, co), want)
    nonzero = float(want.abs().max())
    del x, want, g
    torch.cuda.empty_cache()
    assert same and nonzero == 8.0


# ----------------------------------------------------------------------------- ups_coord_wgrad
def _wgrad(lib, dev, g, hi, wi, k, stride, with_bias):
    ho, wo, co = g.shape
    ci_log = 3
    gV = torch.full((k * k, ci_log + 2, co), SENT, dtype=torch.float32, device=dev)
    gb = Dest(co, torch.float32, dev, nan=True)
    scratch = Dest((2 * k + 1) * wo * co, torch.float32, dev, nan=True)
    ax, ay = _axy(hi, wi)
    dy, dx = A.taps(hi, k, stride), A.taps(wi, k, stride)
    lib.call("ups_coord_wgrad", lib.ptr(g.to(dev)), hi, wi, ho, wo, co, k, k, _i9([r for r in dy for _ in range(k)]), _i9(dx), stride, stride,
             ax, ay, ci_log, lib.ptr(gV), gb.ptr() if with_bias else None, scratch.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert scratch.bands_ok(), "scratch of (2k + 1) wo co floats overrun"
    assert gb.bands_ok() if with_bias else gb.untouched()
    gV = gV.cpu()
    assert bool((gV[:, :ci_log] == SENT).all()), "a main-channel row of gradV was written"
    return gV[:, ci_log], gV[:, ci_log + 1], (gb.t.cpu() if with_bias else None)


def _wgrad_case(lib, dev, case, integer):
    hi, wi, k, stride, co = case
    ho, wo = A.same_pad(hi, k, stride)[0], A.same_pad(wi, k, stride)[0]
    gen = A.gen(70 + hi + wi)
    g = torch.randint(-4, 5, (ho, wo, co), generator=gen).float() if integer else torch.randn(ho, wo, co, generator=gen)
    ax, ay = A.axy(hi, wi)
    ref = A.coord_wgrad(g, hi, wi, k, stride, A.taps(hi, k, stride), A.taps(wi, k, stride), ax, ay)
    vx, vy, b = _wgrad(lib, dev, g, hi, wi, k, stride, True)
    vx0, vy0, _ = _wgrad(lib, dev, g, hi, wi, k, stride, False)
    _same_bits(vx0, vx, "dVx without grad_bias")
    _same_bits(vy0, vy, "dVy without grad_bias")
    return ref, {"vx": vx, "vy": vy, "b": b}, (ho, wo)


@pytest.mark.parametrize("case", A.WGRAD_DYADIC, ids=_ids)
def test_coord_wgrad_dyadic(case, dev):
    """Integer gsum on dyadic maps (stride 1 at h == w and h != w, stride 2 with odd sizes): every sum is exact, equal by value; with
    grad_bias (the bias block row of coord_cols_kernel) and without."""
    lib, ops = _mods()
    ref, got, _ = _wgrad_case(lib, dev, case, True)
    for n in ("vx", "vy", "b"):
        assert float(ref[n].abs().max()) > 0
        assert torch.equal(got[n].double(), ref[n]), (n, int((got[n].double() != ref[n]).sum()))


@pytest.mark.parametrize("case", A.WGRAD_GAUSS, ids=_ids)
def test_coord_wgrad_gauss(case, dev):
    """A single pixel; ho < 8 (row groups with nothing to sum); wo < 4 and wo co = 9 (one ragged block of 32); odd sizes at stride
    2; two channel blocks of 64, the second ragged; 128 x 48.  Every output within (d + 2) 2^-24 sum |terms|, d = wgrad_d."""
    lib, ops = _mods()
    ref, got, (ho, wo) = _wgrad_case(lib, dev, case, False)
    fr = {}
    for n in ("vx", "vy", "b"):
        assert bool(torch.isfinite(got[n]).all())
        fr[n] = A.fraction_used(got[n], ref[n], A.sum_bound(A.wgrad_d(ho, wo, n != "b"), ref["abs_" + n]))
    print("coord_wgrad {}: bound used dVx {:.3f} dVy {:.3f} db {:.3f}".format(case, fr["vx"], fr["vy"], fr["b"]))
    assert max(fr.values()) <= 1.0


# ----------------------------------------------------------------------------- ups_col_sum
@pytest.mark.parametrize("dtype", [BF16, F32], ids=A.DT_NAME.get)
@pytest.mark.parametrize("case", A.COL_SUM_CASES, ids=_ids)
def test_col_sum(case, dtype, dev):
    """One element; co past 128 (tx = 256, one row lane) with ldo > co; 20000 rows of 32 channels = 157 row blocks.  Exact on
    integers; the workspace holds exactly nb x co partials, nb from the formula."""
    lib, ops = _mods()
    rows, co, ldo = case
    x = _sum_input((rows, ldo), co, A.TORCH_DT[dtype], 80 + co)
    want = A.col_sum(x, co)
    tx, nb = A.col_sum_blocks(rows, co)
    out = Dest(co, torch.float32, dev, view=True, nan=True)
    ws = Dest(1024 * co, torch.float32, dev, nan=True)
    lib.call("ups_col_sum", lib.ptr(x.to(dev)), dtype, rows, co, ldo, out.ptr(), ws.ptr(), lib.stream())
    torch.cuda.synchronize()
    assert out.bands_ok() and ws.bands_ok()
    written = ~torch.isnan(ws.t.cpu())
    assert bool(written[:nb * co].all()) and not bool(written[nb * co:].any()), (nb, int(written.sum()))
    got = out.t.cpu().double()
    assert torch.equal(got, want), (got - want).abs().max()


# ----------------------------------------------------------------------------- refusals
def test_refusals(dev):
    """One case for every clause of the argument checks of these entry points; nothing is launched, nothing written."""
    lib, ops = _mods()
    s = lib.stream()
    V = torch.zeros(9 * 18 * 16, dtype=torch.float32, device=dev)
    w, w2 = Dest(9 * 32 * 16 * 4, torch.bfloat16, dev), Dest(9 * 32 * 16 * 4, torch.bfloat16, dev)
    f = Dest(64 * 3 * 16, torch.float32, dev)
    pV, pw, pw2, pf = lib.ptr(V), w.ptr(), w2.ptr(), f.ptr()
    # ups_weight_prep(src, ntaps, cin_v, ci_log, co, dtype, w_fwd, ci_pad, w_dgrad, dgrad_rows, dgrad_k)
    _refused(lib, "ups_weight_prep", None, 9, 18, 16, 16, BF16, pw, 16, pw2, 16, 16, s)
    _refused(lib, "ups_weight_prep", pV, 9, 18, 16, 16, BF16, None, 16, None, 16, 16, s)
    _refused(lib, "ups_weight_prep", pV, 9, 18, 19, 16, BF16, pw, 24, pw2, 19, 16, s)          # ci_log > cin_v
    _refused(lib, "ups_weight_prep", pV, 9, 18, 16, 16, BF16, pw, 8, pw2, 16, 16, s)           # ci_pad < ci_log
    _refused(lib, "ups_weight_prep", pV, 9, 18, 16, 16, BF16, pw, 16, pw2, 16, 8, s)           # dgrad_k < co
    # ups_weight_prep_f8(src, ntaps, cin_v, ci_log, co, transpose, w_f8, deq)
    ok = [pV, 9, 18, 16, 16, 0, pw, pf]
    for i, bad in ((0, None), (6, None), (7, None), (1, 0), (3, 0), (2, 15), (4, 0)):
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_weight_prep_f8", *a, s)
    # ups_weight_prep_d2s(src, cin_v, ci_log, co, pad_y, pad_x, C, w)
    ok = [pV, 18, 16, 16, 0, 0, 16, pw]
    for i, bad in ((0, None), (7, None), (2, 0), (1, 15), (3, 0), (6, 24), (6, 8)):            # C = 24: no power of two; C = 8 < ci_log
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_weight_prep_d2s", *a, s)
    _refused(lib, "ups_weight_prep_d2s", pV, 6, 4, 16, 0, 0, 4, pw, s)                         # C = 4 < 8
    # ups_weight_prep_batch(items, prefix, n_items, total_blocks, dtype)
    items = torch.zeros(C.sizeof(lib.PrepItem), dtype=torch.uint8, device=dev)
    prefix = torch.zeros(2, dtype=torch.int64, device=dev)
    ok = [lib.ptr(items), lib.ptr(prefix), 1, 1, BF16]
    for i, bad in ((0, None), (1, None), (2, 0), (3, 0), (3, 0x7fffffff)):
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_weight_prep_batch", *a, s)
    assert lib.load().ups_prep_item_blocks(None, BF16) == -1
    # ups_coord_table(V, kh, kw, ci_log, co, dy, dx, in_sy, in_sx, ax, ay, tab)
    t9 = _i9([0])
    ok = [pV, 3, 3, 16, 16, t9, t9, 1, 1, 0.125, 0.125, pf]
    for i, bad in ((0, None), (11, None), (5, None), (6, None), (1, 0), (1, 4), (2, 0), (2, 4)):
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_coord_table", *a, s)
    # ups_batch_sum(dout, dtype, n, pix, co, ldo, gsum)
    ok = [pw, BF16, 1, 4, 16, 16, pf]
    for i, bad in ((0, None), (6, None), (2, 0), (3, 0), (1, F16), (1, 7), (5, 12), (0, C.c_void_p(w.t.data_ptr() + 8))):
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_batch_sum", *a, s)
    # ups_coord_wgrad(gsum, hi, wi, ho, wo, co, kh, kw, dy, dx, in_sy, in_sx, ax, ay, ci_log, gradV, grad_bias, scratch)
    f2, f3 = Dest(9 * 18 * 16, torch.float32, dev), Dest(7 * 4 * 16, torch.float32, dev)
    ok = [pf, 4, 4, 4, 4, 16, 3, 3, t9, t9, 1, 1, 0.5, 0.5, 16, f2.ptr(), None, f3.ptr()]
    for i, bad in ((0, None), (15, None), (17, None), (6, 0), (6, 4), (7, 0), (7, 4)):
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_coord_wgrad", *a, s)
    # ups_col_sum(dout, dtype, rows, co, ldo, out, workspace)
    ok = [pw, BF16, 4, 16, 16, pf, f2.ptr()]
    for i, bad in ((0, None), (5, None), (6, None), (2, 0), (3, 0), (1, F16), (1, 7)):
        a = list(ok)
        a[i] = bad
        _refused(lib, "ups_col_sum", *a, s)
    torch.cuda.synchronize()
    for d in (w, w2, f, f2, f3):
        assert d.untouched()
