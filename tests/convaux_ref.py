"""Plain restatements of the convolution helper kernels of csrc/conv_aux.hip -- the blocked-K weight images (ups_weight_prep,
ups_weight_prep_batch), the depth-to-space input-gradient image (ups_weight_prep_d2s), the per-row e4m3 image (ups_weight_prep_f8),
the CoordConv table (ups_coord_table) and its gradient (ups_batch_sum, ups_coord_wgrad), ups_col_sum -- and the cases the host
and GPU tests share.  Every function states the layout or the sum by index, in torch / NumPy on the CPU; the one rounding of a
weight image is ``.to(dtype)``, every sum is fp64.  test_host_convaux.py holds each against the oracle (conv2d_same and its
autograd); test_gpu_convaux.py holds the kernels against these (parity_ledger.md, section 11)."""
import collections
import math

import numpy as np
import torch

F32, BF16, F16 = 0, 1, 2                                  # include/upsparts_hip.h
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DT_NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
U = 2.0 ** -24                                            # unit roundoff of fp32


def cdiv(a, b):
    return -(-a // b)


def round8(c):
    return (c + 7) // 8 * 8


def bk_of(dtype):
    """Elements of one 64-byte K piece."""
    return 16 if dtype == F32 else 32


def same_pad(size, k, stride):
    """TF 'SAME': (out, pad_before)."""
    out = cdiv(size, stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def taps(size, k, stride):
    """Input offset of tap r relative to stride * (output index): r - pad_before."""
    pad = same_pad(size, k, stride)[1]
    return [r - pad for r in range(k)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rounded(v, dtype):
    """The one rounding of a weight image.  fp16 saturates at +-65504 (st_from_float<f16>): it does not overflow to inf."""
    if dtype == F16:
        v = v.clamp(-65504.0, 65504.0)
    return v.to(TORCH_DT[dtype])


def bits(t):
    """Integer view of a tensor's storage, for bit-for-bit comparisons (-0 != +0, NaN == the same NaN)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ----------------------------------------------------------------------------- blocked-K weight images
def blocked_k(V, ntaps, ci_log, co, ci_pad, drows, dk, dtype):
    """V [ntaps][cin_v][co] fp32 -> (w_fwd [tap][kc][co][BK], w_dgrad [tap][kc][drows][BK]) in `dtype`.
    w_fwd[tap][kc][c][kk] = V[tap][kc BK + kk][c] for k < ci_log, else 0;
    w_dgrad[tap][kc][r][kk] = V[tap][r][kc BK + kk] for k < co and r < ci_log, else 0."""
    V = V.reshape(ntaps, -1, co)
    bk = bk_of(dtype)
    kcf, kcd = cdiv(ci_pad, bk), cdiv(dk, bk)
    assert ci_pad >= ci_log and dk >= co
    R = rounded(V[:, :ci_log, :], dtype)                                  # [tap][k][c]
    wf = torch.zeros(ntaps, kcf * bk, co, dtype=TORCH_DT[dtype])          # [tap][k][c]
    wf[:, :ci_log, :] = R
    wf = wf.view(ntaps, kcf, bk, co).permute(0, 1, 3, 2).contiguous()
    wd = torch.zeros(ntaps, kcd * bk, drows, dtype=TORCH_DT[dtype])       # [tap][k = output channel][r = input channel]
    nr = min(ci_log, drows)
    wd[:, :co, :nr] = R[:, :nr, :].transpose(1, 2)
    wd = wd.view(ntaps, kcd, bk, drows).permute(0, 1, 3, 2).contiguous()
    return wf, wd


def unblock(w):
    """[tap][kc][row][BK] -> [tap][kc BK][row]."""
    t, kc, rows, bk = w.shape
    return w.permute(0, 1, 3, 2).reshape(t, kc * bk, rows)


# ----------------------------------------------------------------------------- depth-to-space input-gradient image
def d2s_image(V, ci_log, co, pad_y, pad_x, C):
    """V [9][cin_v][co] fp32 -> [9][ceil(co/32)][4C][32] bf16: row (py*2+px)*C + c of lattice offset t9 = (dy, dx) holds forward tap
    (py + pad_y - 2 dy, px + pad_x - 2 dx) of input channel c, over the gradient channel kk; zero where that tap is outside 3x3,
    c >= ci_log or kk >= co."""
    V = V.reshape(9, -1, co)
    kc = cdiv(co, 32)
    assert C >= ci_log
    img = torch.zeros(9, kc * 32, 4 * C, dtype=torch.float32)            # [t9][kk][row]
    for t9 in range(9):
        dy, dx = t9 // 3 - 1, t9 % 3 - 1
        for py in range(2):
            for px in range(2):
                rr, ss = py + pad_y - 2 * dy, px + pad_x - 2 * dx
                if 0 <= rr < 3 and 0 <= ss < 3:
                    r0 = (py * 2 + px) * C
                    img[t9, :co, r0:r0 + ci_log] = V[rr * 3 + ss, :ci_log, :].t()
    return img.view(9, kc, 32, 4 * C).permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def d2s_input_gradient(w, g, C, hi, wi):
    """dx[2i+py][2j+px][c] = sum_t9 sum_kk g[i+dy][j+dx][kk] w[t9][kk/32][(py*2+px) C + c][kk%32], cropped to hi x wi; fp64.
    g [ho][wo][co]."""
    ho, wo, co = g.shape
    W = unblock(w).double()[:, :co, :]                                  # [t9][kk][row]
    gp = torch.zeros(ho + 2, wo + 2, co, dtype=torch.float64)
    gp[1:ho + 1, 1:wo + 1] = g.double()
    out = torch.zeros(2 * ho, 2 * wo, C, dtype=torch.float64)
    for t9 in range(9):
        dy, dx = t9 // 3 - 1, t9 % 3 - 1
        sh = gp[1 + dy:1 + dy + ho, 1 + dx:1 + dx + wo]                 # g[i+dy][j+dx]
        rows = sh @ W[t9]                                               # [ho][wo][4C]
        for py in range(2):
            for px in range(2):
                r0 = (py * 2 + px) * C
                out[py::2, px::2] += rows[..., r0:r0 + C]
    return out[:hi, :wi]


# ----------------------------------------------------------------------------- e4m3 rows
def f8_rows(V, ntaps, ci_log, co, transpose):
    """V [ntaps][cin_v][co] fp32 -> (bytes [tap][ceil(k/64)][rows][64] uint8, deq [rows] fp32).  Element (t, row, k) is V[t][k][row]
    (forward: rows = co, k < ci_log) or V[t][row][k] (transposed: rows = ci_log, k < co); the row maximum is taken over the first
    ci_log input channels only (the coordinate rows of a CoordConv V are not part of this GEMM); sc = 448 / m and deq = m / 448
    in fp32; an all-zero row has sc = deq = 1; value = (v * sc).clamp(+-448).to(float8_e4m3fn); padding is zero."""
    V = V.reshape(ntaps, -1, co)
    E = V[:, :ci_log, :]
    E = E if transpose else E.transpose(1, 2)                            # [t][row][k]
    rows, kdim = E.shape[1], E.shape[2]
    m = E.abs().amax(dim=(0, 2))
    f448 = torch.tensor(448.0, dtype=torch.float32)
    one = torch.ones_like(m)
    safe = torch.where(m > 0, m, one)
    sc = torch.where(m > 0, f448 / safe, one)
    deq = torch.where(m > 0, safe / f448, one)
    q = (E * sc.view(1, rows, 1)).clamp(-448.0, 448.0)
    kc = cdiv(kdim, 64)
    full = torch.zeros(ntaps, rows, kc * 64, dtype=torch.float32)
    full[:, :, :kdim] = q
    by = full.to(torch.float8_e4m3fn).view(torch.uint8)
    return by.view(ntaps, rows, kc, 64).permute(0, 2, 1, 3).contiguous(), deq


# ----------------------------------------------------------------------------- CoordConv table
# d of a table entry (coord_table_entry): k0 is a chain of 2 fused multiply-adds per tap, 18 for 3x3 -- 18 roundings of partial sums
# that never exceed sum |terms|; the coefficient fma(ax, dx, -1) of each term is one more rounding of that term, and the second of
# the "+ 2" stays unused.  kj and ki are 9 roundings of a chain + the rounding of ax * stride: inside the same bound.
TABLE_D = 18


def coord_table(V, k, ci_log, co, dy, dx, stride, ax, ay, absolute=False):
    """[64][3][co] fp64: entry (ym << 3 | xm, 0..2, c) = (k0, kj, ki) with bit r of ym / bit s of xm = tap row r / column s is inside
    the image; the coordinate planes' contribution to output pixel (i, j) of that class is k0 + kj j + ki i.
    xx(column x) = ax x - 1 and yy(row y) = ay y - 1 with ax, ay as the fp32 numbers the kernel is given; x = j stride + dx[s].
    absolute: the sums of the terms' magnitudes instead (for the error bound)."""
    V = V.reshape(k * k, -1, co).double()
    ax, ay = float(np.float32(ax)), float(np.float32(ay))
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    tab = torch.zeros(64, 3, co, dtype=torch.float64)
    for cls in range(64):
        ym, xm = cls >> 3, cls & 7
        for r in range(k):
            for s in range(k):
                if (ym >> r) & 1 and (xm >> s) & 1:
                    vx, vy = V[r * k + s, ci_log], V[r * k + s, ci_log + 1]
                    tab[cls, 0] += f((ax * dx[s] - 1.0) * vx) + f((ay * dy[r] - 1.0) * vy)
                    tab[cls, 1] += f(ax * stride * vx)
                    tab[cls, 2] += f(ay * stride * vy)
    return tab


def tap_class(i, size, k, stride, d):
    """Bit r set: tap r of output index i reads inside [0, size)."""
    return sum(1 << r for r in range(k) if 0 <= i * stride + d[r] < size)


def table_map(tab, hi, wi, k, stride, dy, dx):
    """[ho][wo][co]: k0 + kj j + ki i with each pixel's own class."""
    ho, wo = same_pad(hi, k, stride)[0], same_pad(wi, k, stride)[0]
    out = torch.zeros(ho, wo, tab.shape[2], dtype=torch.float64)
    for i in range(ho):
        ym = tap_class(i, hi, k, stride, dy)
        for j in range(wo):
            cls = ym << 3 | tap_class(j, wi, k, stride, dx)
            out[i, j] = tab[cls, 0] + tab[cls, 1] * j + tab[cls, 2] * i
    return out


def axy(hi, wi):
    """(ax, ay) as every caller in ops.py forms them: the oracle's add_coordinates divides the COLUMN index by H - 1 and the ROW
    index by W - 1 (nn.py:2145-2148)."""
    return 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)


# ----------------------------------------------------------------------------- CoordConv weight gradient
def wgrad_d(ho, wo, weighted):
    """Roundings on the longest path to one output of ups_coord_wgrad: coord_rows_kernel adds ceil(ho / 8) terms per row group and
    folds the 8 groups with 7 additions, coord_cols_kernel adds ceil(wo / 4) terms per column group and folds the 4 groups with 3; a
    row- or column-weighted output has the two operations of its coordinate (ay y - 1, or its fused form) on top."""
    return cdiv(ho, 8) + 7 + cdiv(wo, 4) + 3 + (2 if weighted else 0)


def coord_wgrad(gsum, hi, wi, k, stride, dy, dx, ax, ay):
    """gsum [ho][wo][co] -> dict: "vx", "vy" [k*k][co] (the two coordinate rows of dV per tap), "b" [co], and "abs_*", the sums
    of the terms' magnitudes.  dVx[r, s] = sum_ij valid (ax x - 1) g[i][j], dVy[r, s] = sum_ij valid (ay y - 1) g[i][j], x = j stride +
    dx[s], y = i stride + dy[r], valid = both inside the image; fp64."""
    g = gsum.double()
    ho, wo, co = g.shape
    ax, ay = float(np.float32(ax)), float(np.float32(ay))
    out = {n: torch.zeros(k * k, co, dtype=torch.float64) for n in ("vx", "vy", "abs_vx", "abs_vy")}
    ii, jj = torch.arange(ho, dtype=torch.float64), torch.arange(wo, dtype=torch.float64)
    for r in range(k):
        y = ii * stride + dy[r]
        vy_ok = ((y >= 0) & (y < hi)).double()
        for s in range(k):
            x = jj * stride + dx[s]
            vx_ok = ((x >= 0) & (x < wi)).double()
            valid = vy_ok.view(ho, 1, 1) * vx_ok.view(1, wo, 1)
            cx = (ax * x - 1.0).view(1, wo, 1) * valid
            cy = (ay * y - 1.0).view(ho, 1, 1) * valid
            out["vx"][r * k + s] = (cx * g).sum((0, 1))
            out["vy"][r * k + s] = (cy * g).sum((0, 1))
            out["abs_vx"][r * k + s] = (cx * g).abs().sum((0, 1))
            out["abs_vy"][r * k + s] = (cy * g).abs().sum((0, 1))
    out["b"] = g.sum((0, 1))
    out["abs_b"] = g.abs().sum((0, 1))
    return out


# ----------------------------------------------------------------------------- sums
def batch_sum(d, co):
    """d [n][pix][ldo] -> [pix][co] fp64."""
    return d[:, :, :co].double().sum(0)


def col_sum(d, co):
    """d [rows][ldo] -> [co] fp64."""
    return d[:, :co].double().sum(0)


def col_sum_blocks(rows, co):
    """(tx, nb) of ups_col_sum: row blocks of 16 trips of the 256 / tx row lanes, at most 1024."""
    tx = 32
    while tx < co and tx < 256:
        tx *= 2
    return tx, max(1, min(1024, cdiv(rows, (256 // tx) * 16)))


# ----------------------------------------------------------------------------- inputs
def edge_weights(shape, seed, dtype):
    """N(0, 1) / 4 with the values a conversion can get wrong planted at the front: +-0, fp32 denormals and (fp16) +-1e5."""
    V = torch.randn(shape, generator=gen(seed)) * 0.25
    flat = V.view(-1)
    plant = [0.0, -0.0, 1e-40, -1e-40, 1.1754942e-38, -3e-39]
    if dtype == F16:
        plant += [1e5, -1e5, 65504.0, 65520.0, -65520.0, 7e4]
    n = min(len(plant), flat.numel())
    flat[:n] = torch.tensor(plant[:n], dtype=torch.float32)
    return V


def int_weights(shape, seed, amp=3):
    return torch.randint(-amp, amp + 1, shape, generator=gen(seed)).float()


# per-layer cases: (name, k, ci_log, coords, co); ci_pad = round8(ci_log), drows = ci_log, dk = round8(co), as ops.ConvLayer passes
PREP_CASES = [("k3_16c_16", 3, 16, True, 16), ("k3_20_10", 3, 20, False, 10), ("k1_40c_72", 1, 40, True, 72), ("k3_8_3", 3, 8, False, 3)]
PREP_BIG = ("k3_512_512", 3, 512, False, 512)             # 4.7 M elements > 8192 x 256: the grid-stride loop's second and third trip

Item = collections.namedtuple("Item", "name k ci_log coords co lead fwd dgrad tab hw stride")


def item(name, k, ci_log, coords, co, lead=0, fwd=True, dgrad=True, hw=(16, 16), stride=1):
    return Item(name, k, ci_log, coords, co, lead, fwd, dgrad, coords and fwd, hw, stride)


# The batched list (issue order): with 16 chunks per block, item "co64_coord" starts at chunk 206 = 12 * 16 + 14.
BATCH_ITEMS = [
    item("co64_aligned", 1, 32, False, 64),               # 16 chunks: the 4-chunk unit from c0i = 0 and 4; twin of co64_view
    item("coord16", 3, 16, True, 16),                     # 40 chunks (18 + 18 + 4 of the table)
    item("co10", 3, 20, False, 10),                       # 34 chunks, the last ragged: scalar path
    item("co64_view", 1, 32, False, 64, lead=1),          # 16 chunks: src 4 bytes off a 16-byte boundary
    item("co24", 3, 40, False, 24),                       # 99 chunks: the 8-channel LDS-turned path, two k-chunks
    item("no_fwd", 1, 8, False, 8, fwd=False),            # 1 chunk
    item("co64_coord", 1, 32, True, 64, hw=(9, 17)),      # 32 chunks (8 + 8 + 16): starts at j = 14
    item("no_dgrad", 1, 8, False, 8, dgrad=False),        # 1 chunk
]
BATCH_PREFIX_16BIT = [0, 16, 56, 90, 106, 205, 206, 238, 239]


def item_geometry(it, dtype):
    """(ntaps, cin_v, ci_pad, drows, dk, nf, nd, nc) of an item, element counts as prep_elems() counts them."""
    bk = bk_of(dtype)
    ntaps, cin_v = it.k * it.k, it.ci_log + (2 if it.coords else 0)
    ci_pad, drows, dk = round8(it.ci_log), it.ci_log, round8(it.co)
    nf = ntaps * cdiv(ci_pad, bk) * it.co * bk if it.fwd else 0
    nd = ntaps * cdiv(dk, bk) * drows * bk if it.dgrad else 0
    nc = 64 * it.co if it.tab else 0
    return ntaps, cin_v, ci_pad, drows, dk, nf, nd, nc


def item_chunks(it, dtype):
    return cdiv(sum(item_geometry(it, dtype)[5:]), 256)


def item_weights(it, seed, dtype):
    """The item's V [k*k][cin_v][co] (edge values planted)."""
    ntaps, cin_v = item_geometry(it, dtype)[:2]
    return edge_weights((ntaps, cin_v, it.co), seed, dtype)


def item_reference(it, V, dtype):
    """{"w_fwd", "w_dgrad", "ctab"} of an item (None where the item has none), the table as fp64 with its bound."""
    ntaps, cin_v, ci_pad, drows, dk = item_geometry(it, dtype)[:5]
    wf, wd = blocked_k(V, ntaps, it.ci_log, it.co, ci_pad, drows, dk, dtype)
    out = {"w_fwd": wf if it.fwd else None, "w_dgrad": wd if it.dgrad else None, "ctab": None, "ctab_abs": None}
    if it.tab:
        hi, wi = it.hw
        dy, dx = taps(hi, it.k, it.stride), taps(wi, it.k, it.stride)
        ax, ay = axy(hi, wi)
        out["ctab"] = coord_table(V, it.k, it.ci_log, it.co, dy, dx, it.stride, ax, ay)
        out["ctab_abs"] = coord_table(V, it.k, it.ci_log, it.co, dy, dx, it.stride, ax, ay, absolute=True)
    return out


def chunk_route(it, c0i, j, b, total, dtype, cpb, src_aligned):
    """Which path of weight_prep_batch_kernel chunk c0i of the item takes when it sits at position j of its block (chunk b of
    `total`): "unit4" (and the three chunks behind it are skipped), "turn8", "scalar" or "table" (a chunk may mix the last two)."""
    bk = bk_of(dtype)
    nf, nd, nc = item_geometry(it, dtype)[5:]
    if dtype != F32 and it.co % 32 == 0 and c0i % 4 == 0 and j + 4 <= cpb and b + 4 <= total and it.fwd and src_aligned \
            and (c0i + 4) * 256 <= nf:
        return "unit4"
    if dtype != F32 and it.co % 8 == 0 and c0i * 256 + 256 <= nf:
        return "turn8"
    return "table" if c0i * 256 >= nf + nd else "scalar"


def batch_routes(items, prefix, dtype, cpb):
    """[(item index, chunk of the item, j, route)] for every chunk of the launch, in the order a block walks them."""
    total = prefix[-1]
    out, b = [], 0
    while b < total:
        i = max(n for n in range(len(items)) if prefix[n] <= b)
        c0i, j = b - prefix[i], b % cpb
        route = chunk_route(items[i], c0i, j, b, total, dtype, cpb, items[i].lead % 4 == 0)
        out.append((i, c0i, j, route))
        b += 4 if route == "unit4" else 1
    return out


# table cases: (hi, wi); each runs at (k, stride) in TABLE_KS
TABLE_DYADIC = [(9, 9), (17, 33), (33, 17)]
TABLE_GAUSS = [(16, 16), (7, 20), (128, 48)]
TABLE_KS = [(1, 1), (3, 1), (3, 2), (1, 2)]

BATCH_SUM_CASES = [(1, 1, 8, 8), (5, 20, 130, 136), (3, 7, 3, 8), (64, 16, 32, 32)]      # n, pix, co, ldo
BATCH_SUM_BIG = (2, 65536, 520, 520)          # bf16: 65536 * ceil(520 / 8) = 4 259 840 > 16384 * 256 = 4 194 304
COL_SUM_CASES = [(1, 1, 8), (37, 130, 136), (20000, 32, 32)]                              # rows, co, ldo

WGRAD_DYADIC = [(9, 9, 3, 1, 16), (17, 33, 3, 1, 16), (17, 17, 3, 2, 16)]                 # hi, wi, k, stride, co
WGRAD_GAUSS = [(1, 1, 1, 1, 72), (4, 4, 3, 1, 16), (5, 3, 3, 1, 3), (9, 7, 3, 2, 8), (16, 32, 3, 1, 130), (128, 48, 3, 1, 40)]

D2S_CASES = [(8, 8, 32), (8, 8, 40), (16, 16, 3), (8, 16, 64)]                            # ci_log, C, co
F8_CASES = [("k3_64c_64", 3, 64, True, 64), ("k3_72_40", 3, 72, False, 40), ("k1_6_5", 1, 6, False, 5)]


def f8_weights(case, seed):
    """Gaussian V [k*k][cin_v][co] with, in both orientations' row 0 / 1 / 2: an all-zero row, a row whose maximum is 2^-100, a row
    that holds its maximum twice with opposite signs.  The coordinate rows of a CoordConv V are 100 times larger than the rest: a
    maximum that looks at them is wrong in every row."""
    name, k, ci_log, coords, co = case
    cin_v = ci_log + (2 if coords else 0)
    V = torch.randn(k * k, cin_v, co, generator=gen(seed)) * 0.05
    if coords:
        V[:, ci_log:, :] *= 100.0
    tiny = 2.0 ** -100
    # forward rows are output channels, transposed rows input channels: plant along both axes (the crossings keep the stronger rule)
    V[:, :ci_log, 1] = torch.randn(k * k, ci_log, generator=gen(seed + 1)).clamp(-7, 7) * 2.0 ** -103
    V[:, 1, :] = torch.randn(k * k, co, generator=gen(seed + 2)).clamp(-7, 7) * 2.0 ** -103
    V[0, 2, 1] = tiny
    V[0, 1, 2] = -tiny
    V[0, 1, 1] = tiny
    big = float(V.abs().max()) * 1.5 if not coords else float(V[:, :ci_log].abs().max()) * 1.5
    V[0, 3, 2], V[k * k - 1, 4, 2] = big, -big          # forward row 2
    V[0, 2, 3], V[k * k - 1, 2, 4] = big, -big          # transposed row 2
    V[:, :ci_log, 0] = 0.0
    V[:, 0, :] = 0.0
    return V


def sum_bound(d, abs_terms):
    """Forward error bound of a d-rounding fp32 summation of exactly given terms, (d + 2) 2^-24 sum |terms|."""
    return (d + 2) * U * abs_terms


def fraction_used(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 = 0: an output without terms must be exact)."""
    err = (got.double() - want).abs()
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(frac.max())
