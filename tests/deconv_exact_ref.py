"""Exact (tolerance-free) reference of the weight-normalised deconvolution (csrc/deconv3x3_s2.hip) on lattice inputs.  CPU only.

The normalisation W = g V / |V| is exact on the right data: every filter of V holds entries in {-1, 0, 1} with exactly 4**k
non-zeros over its 9 * cin_v elements (k = floor(log4(9 * cin_v)); the CoordConv columns count), so deconv_norm_kernel's fmaf sum
is the integer 4**k and its rsqrtf is 2**-k; g is drawn from {0.5, 1, 2}.  W is then an integer times a power of two -- exact in
fp32, bf16 and fp16 -- and with x, dy integers in [-4, 4], b integers in [-3, 3] and dyadic coordinates (hi - 1 and wi - 1 powers
of two) every product, every partial sum, the three terms of the CoordConv table, the epilogue acc + b + tb0 + j tb1 + i tb2, db,
dW, dot = <V, dW>, dg = dot * inv, proj = dot * inv * inv and dV = g inv (dW - V proj) are exact in fp32.  The one rounding left
is the RNE to the stored type, which `.to(dtype)` of the float64 reference reproduces.  `headroom` is the condition of that
argument.  The conventions (gen, ints, rounded, lsb, first_diff, LIMIT) are tests/exact_ref.py's.

Coordinates follow oracle.ref_model.Scope.add_coordinates: channel cin is -1 + column * 2 / (hi - 1), channel cin + 1 is
-1 + row * 2 / (wi - 1) -- each scaled by the OTHER dimension -- as both kernels have it.  The one-launch kernel takes
wi % 16 == 0 only, where 2 / (wi - 1) is not dyadic: such cases (zero_row) carry zero weights in the row-coordinate column and
non-zero ones in the column-coordinate column, so the kernel's table path runs with real coordinate terms.
"""
import math

import torch

import exact_ref as E

LIMIT = E.LIMIT
AXES_V = ("tap_y", "tap_x", "filter", "cin")
G_VALUES = (0.5, 1.0, 2.0)


def round8(c):
    return (c + 7) // 8 * 8


class Case(object):
    """n x h x w input, cin -> nf.  sub: the 16-pixel sub-tiles per block the one-launch kernel's gate lines give (None: it refuses
    the shape); dx: the kernel ups_conv_igemm gives the input gradient; splitk: ups_conv_wgrad_plan of the swapped weight
    gradient per gradient type; dx_force: environment of the extra input-gradient routes the case is there for."""
    def __init__(self, name, n, h, w, cin, nf, dtypes, sub, splitk, coords=False, zero_row=False, dx="generic", dx_force=(),
                 reaches=""):
        self.name, self.n, self.h, self.w, self.cin, self.nf = name, n, h, w, cin, nf
        self.dtypes, self.sub, self.splitk, self.coords, self.zero_row = dtypes, sub, splitk, coords, zero_row
        self.dx, self.dx_force, self.reaches = dx, dx_force, reaches
        self.cin_v = cin + (2 if coords else 0)
        self.k = int(math.floor(math.log(9 * self.cin_v, 4) + 1e-9))
        assert not zero_row or coords

    def __repr__(self):
        return self.name


ALL = ("bf16", "f16", "fp32")
CASES = [
    Case("dc_sub1_thin", 3, 16, 16, 3, 10, ALL, 1, {"bf16": 3, "fp32": 6},
         reaches="one launch, sub = 1; one ragged K chunk (ci = 8); ragged 16-channel N tile; pad channels 10..15"),
    Case("dc_sub2_h1", 2, 1, 32, 40, 34, ("bf16",), 2, {"bf16": 1},
         reaches="one launch, sub = 2; h = 1: row i - 1 is never inside; second K chunk ragged (ci = 40); 6 work items over 4 waves"),
    Case("dc_sub4_two_blocks", 1, 5, 128, 32, 32, ("bf16", "f16"), 4, {"bf16": 2},
         reaches="one launch, sub = 4; two blocks per row: the left halo comes from the neighbouring block; odd h"),
    Case("dc_lds_fallback", 1, 2, 64, 256, 256, ("bf16",), 1, {"bf16": 1},
         reaches="one launch, sub falls to 1 (lds(4), lds(2) > 64 KiB); kc_n = 8; 16 N tiles; channel limits 256 / 256"),
    Case("dc_nf3", 2, 4, 16, 16, 3, ("bf16",), 1, {"bf16": 1},
         reaches="one launch, nf < 8: ldo = 8, five pad channels, a single ragged N tile"),
    Case("dc_coords_x", 2, 9, 16, 32, 34, ("bf16", "f16"), 1, {"bf16": 1}, coords=True, zero_row=True,
         reaches="one launch with ctab; ax = 2/8; row column zero (2/15 is not dyadic); non-square"),
    Case("dc_small_w4", 3, 4, 4, 3, 10, ALL, None, {"bf16": 1, "fp32": 1},
         reaches="the one-launch kernel refuses it (w % 16): class launches"),
    Case("dc_coords_9x17", 2, 9, 17, 10, 3, ("bf16", "fp32"), None, {"bf16": 1, "fp32": 2}, coords=True,
         reaches="class launches; both coordinate columns non-zero (2/8, 2/16); non-square; odd width"),
    Case("dc_coords17", 3, 17, 17, 32, 32, ("bf16", "fp32"), None, {"bf16": 3, "fp32": 6}, coords=True,
         reaches="class launches; both coordinate columns non-zero"),
    Case("dc_wide_k", 2, 8, 8, 128, 32, ("bf16",), None, {"bf16": 1},
         reaches="class launches at K = 128"),
    Case("dc_dx_s2", 1, 32, 32, 128, 64, ("bf16",), 2, {"bf16": 4}, dx="generic; rows_s2 <64,6,9> and conv3x3_s2 under force",
         dx_force=(("rows_s2", "force", "0"), ("conv3x3_s2", "0", "force")),
         reaches="one launch, sub = 2; the input gradient (64 channels of a 64 x 64 gradient -> 128) is the one deconvolution "
                 "shape of at most 64 x 64 output pixels that the stride-2 row stream admits, and conv3x3_s2 admits it too"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def takes_one_launch(case, dtype):
    """ups_deconv3x3_s2_fwd's gate lines: 16-bit tensors, width a multiple of 16, at most 256 input / output channels."""
    return dtype != "fp32" and case.w % 16 == 0 and round8(case.cin) <= 256 and case.nf <= 256


def one_launch_sub(case):
    """The `sub` ups_deconv3x3_s2_fwd chooses (its LDS rule restated), None where the kernel refuses the shape."""
    if not takes_one_launch(case, "bf16"):
        return None
    ci, ldo = round8(case.cin), round8(case.nf)
    xp, yp = -(-ci // 32) * 32 + 8, ldo + 8

    def lds(sub):
        return 2 * (16 * sub + 1) * xp * 2 + 2 * 32 * sub * yp * 2
    for sub in (4, 2):
        if case.w % (16 * sub) == 0 and lds(sub) <= 64 * 1024:
            return sub
    return 1 if lds(1) <= 64 * 1024 else None


# ---------------------------------------------------------------------------------------------------------------------------------
# the lattice
def lattice_V(g, case):
    """[3, 3, nf, cin_v] in {-1, 0, 1}: exactly 4**k non-zeros per filter; at least one in every coordinate column the case says
    is non-zero, none in the row-coordinate column of a zero_row case."""
    nf, cv, cin = case.nf, case.cin_v, case.cin
    nnz = 4 ** case.k
    V = torch.zeros(9, nf, cv, dtype=torch.float64)
    cols = [cin, cin + 1] if case.coords and not case.zero_row else ([cin] if case.coords else [])
    allowed = torch.ones(9, cv, dtype=torch.bool)
    if case.zero_row:
        allowed[:, cin + 1] = False
    for o in range(nf):
        chosen = torch.zeros(9, cv, dtype=torch.bool)
        for c in cols:
            chosen[int(torch.randint(0, 9, (1,), generator=g)), c] = True
        free = (allowed & ~chosen).view(-1).nonzero().view(-1)
        pick = free[torch.randperm(free.numel(), generator=g)[:nnz - int(chosen.sum())]]
        chosen.view(-1)[pick] = True
        sign = torch.randint(0, 2, (9, cv), generator=g).double() * 2 - 1
        V[:, o, :] = sign * chosen.double()
    return V.view(3, 3, nf, cv)


def case_inputs(case):
    """(x [n,h,w,cin], V [3,3,nf,cin_v], g [nf], b [nf], dy [n,2h,2w,nf]) float64 lattice tensors."""
    gn = E.gen(case.name)
    x = E.ints(gn, (case.n, case.h, case.w, case.cin), 4)
    V = lattice_V(gn, case)
    g = torch.tensor(G_VALUES, dtype=torch.float64)[torch.randint(0, 3, (case.nf,), generator=gn)]
    b = E.ints(gn, (case.nf,), 3)
    dy = E.ints(gn, (case.n, 2 * case.h, 2 * case.w, case.nf), 4)
    return x, V, g, b, dy


def coord_scales(h, w):
    """(ax, ay): the column coordinate's step 2 / (hi - 1), the row coordinate's 2 / (wi - 1) (add_coordinates' convention)."""
    return 2.0 / max(1, h - 1), 2.0 / max(1, w - 1)


def add_coordinates(x):
    """Scope.add_coordinates: channel c = column / (hi - 1) * 2 - 1, channel c + 1 = row / (wi - 1) * 2 - 1."""
    from oracle.ref_model import Scope
    return Scope.add_coordinates(x)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plain reference (float64: exact on these values)
WN_EPS = 1e-12


def normalise(V, g, inv=None):
    """(W, inv, ss): W = g V inv, inv = rsqrt(max(sum V^2, 1e-12)) per filter (or the `inv` handed in: the device's)."""
    ss = (V * V).sum(dim=(0, 1, 3))
    if inv is None:
        inv = torch.rsqrt(torch.clamp(ss, min=WN_EPS))
    return V * (g * inv).view(1, 1, -1, 1), inv, ss


def _crop(full, h, w):
    """TF 'SAME' for stride 2 on an even size: pad 0 before, 1 after -- the taps that land on row / column 2H are dropped."""
    return full[:, :2 * h, :2 * w]


def deconv_taps(xa, W, b):
    """y[n, 2i+ky, 2j+kx, o] += sum_c xa[n, i, j, c] W[ky, kx, o, c] (the kernel file's header formula), one matrix product per tap
    into a (2h + 1) x (2w + 1) map whose last row and column are then dropped; + b."""
    n, h, w, c = xa.shape
    nf = W.shape[2]
    full = torch.zeros(n, 2 * h + 1, 2 * w + 1, nf, dtype=xa.dtype)
    for ky in range(3):
        for kx in range(3):
            full[:, ky:ky + 2 * h:2, kx:kx + 2 * w:2] += (xa.reshape(-1, c) @ W[ky, kx].t()).view(n, h, w, nf)
    return _crop(full, h, w) + b


def _tap_views(dy, h, w):
    """dy[n, 2i+ky, 2j+kx, :] as [n, h, w, nf] per tap, zero where the tap lands on row / column 2H."""
    dyp = torch.nn.functional.pad(dy, (0, 0, 0, 1, 0, 1))
    return [[dyp[:, ky:ky + 2 * h:2, kx:kx + 2 * w:2] for kx in range(3)] for ky in range(3)]


def reference(x, V, g, b, dy, coords, inv=None):
    """The layer and its gradients by closed forms, float64:
        y  = deconv_taps(x (+ coordinates), W) + b
        db = sum dy;  dx[n,i,j,c] = sum_taps dy[n,2i+ky,2j+kx,:] . W[ky,kx,:,c] (c < cin);  dW[ky,kx,o,c] = sum_pixels dy_tap[.., o] xa[.., c]
        dot = <V_o, dW_o>;  dg = dot inv;  proj = dot inv^2 (0 where the norm is clamped);  dV = g inv (dW - V proj)
    Zeros are +0 (a sum that starts at +0 never gives -0; g > 0)."""
    n, h, w, cin = x.shape
    nf = V.shape[2]
    xa = add_coordinates(x) if coords else x
    W, inv, ss = normalise(V, g, inv)
    y = deconv_taps(xa, W, b)
    taps = _tap_views(dy, h, w)
    dx = torch.zeros(n * h * w, cin, dtype=x.dtype)
    dW = torch.zeros_like(V)
    for ky in range(3):
        for kx in range(3):
            t = taps[ky][kx].reshape(-1, nf)
            dx += t @ W[ky, kx, :, :cin]
            dW[ky, kx] = t.t() @ xa.reshape(-1, xa.shape[-1])
    dW = dW + 0.0
    dot = (V * dW).sum(dim=(0, 1, 3)) + 0.0
    proj = torch.where(ss >= WN_EPS, dot * inv * inv, torch.zeros_like(dot))
    dV = (g * inv).view(1, 1, -1, 1) * (dW - V * proj.view(1, 1, -1, 1))
    return {"y": y + 0.0, "dx": dx.view(n, h, w, cin) + 0.0, "db": dy.sum(dim=(0, 1, 2)) + 0.0, "dW": dW, "dot": dot,
            "dg": dot * inv + 0.0, "dV": dV + 0.0, "W": W, "inv": inv, "ss": ss}


def headroom(case, inputs=None):
    """The condition of exactness, each sum in units of its own LSB, every one to stay below 2**24:
      fwd   sum of |x_aug| |W| + |b| of an output (a coordinate counts |-1| + |a j|, the two pieces the table keeps apart)
      dx    sum of |dy| |W| of an input-gradient element
      dW    sum of |dy| |x_aug| of a weight-gradient element
      db    sum of |dy| of a channel
      dot   sum of |V| |dW| of a filter (dW itself: exact by the line above)
      dV    |dW ss - V dot|: the one difference dW - V proj of two exact operands, in units of proj's LSB (ss = 4**k of them make
            one LSB of dW); it is exact when it is representable
    The row-coordinate column of a zero_row case is left out: its weights are zero and its dW entries are not claimed exact."""
    x, V, g, b, dy = inputs if inputs is not None else case_inputs(case)
    n, h, w, cin = x.shape
    W, inv, ss = normalise(V, g)
    A = x.abs()
    if case.coords:
        ax, ay = coord_scales(h, w)
        cj = (1.0 + ax * torch.arange(w, dtype=x.dtype)).view(1, 1, w, 1).expand(n, h, w, 1)
        ci = (1.0 + ay * torch.arange(h, dtype=x.dtype)).view(1, h, 1, 1).expand(n, h, w, 1)
        A = torch.cat([A, cj] if case.zero_row else [A, cj, ci], dim=-1)
    cv = A.shape[-1]
    Wa, Va = W[..., :cv].abs(), V[..., :cv].abs()
    u_x, u_w, u_g = E.lsb(A), E.lsb(Wa), E.lsb(dy)
    out = {"fwd": float(deconv_taps(A, Wa, b.abs()).max()) / min(u_x * u_w, E.lsb(b))}
    taps = _tap_views(dy.abs(), h, w)
    gx = torch.zeros(n * h * w, cin, dtype=x.dtype)
    gW = torch.zeros_like(Va)
    for ky in range(3):
        for kx in range(3):
            t = taps[ky][kx].reshape(-1, case.nf)
            gx += t @ Wa[ky, kx, :, :cin]
            gW[ky, kx] = t.t() @ A.reshape(-1, cv)
    u_dw = u_x * u_g
    Ax = add_coordinates(x)[..., :cv] if case.coords else x
    dW = torch.stack([torch.stack([tp.reshape(-1, case.nf).t() @ Ax.reshape(-1, cv) for tp in row]) for row in _tap_views(dy, h, w)])
    Vs = V[..., :cv]
    out["dx"] = float(gx.max()) / (u_g * u_w)
    out["dW"] = float(gW.max()) / u_dw
    out["db"] = float(dy.abs().sum(dim=(0, 1, 2)).max()) / u_g
    out["dot"] = float((Va * dW.abs()).sum(dim=(0, 1, 3)).max()) / u_dw
    dot = (Vs * dW).sum(dim=(0, 1, 3))
    out["dV"] = float((dW * ss.view(1, 1, -1, 1) - Vs * dot.view(1, 1, -1, 1)).abs().max()) / u_dw
    return out


_REF = {}


def case_reference(case):
    """(inputs, reference dict, headroom dict), computed once per process and shared; callers must not modify it."""
    if case.name not in _REF:
        ins = case_inputs(case)
        x, V, g, b, dy = ins
        _REF[case.name] = (ins, reference(x, V, g, b, dy, case.coords), headroom(case, ins))
    return _REF[case.name]


def exact_mask_dV(case):
    """[3, 3, nf, cin_v] bool: the entries of dV held by bits (all but the row-coordinate column of a zero_row case, whose dW
    entries are sums of dy * (-1 + i * 2/15))."""
    m = torch.ones(3, 3, case.nf, case.cin_v, dtype=torch.bool)
    if case.zero_row:
        m[..., case.cin + 1] = False
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# the operand layouts, from the layout comments of deconv3x3_s2.hip
def layout_w_fwd(W, cin, bk):
    """wf[t][kc][o][BK] = W[t][o][kc * BK + j], zero for c >= cin (the coordinate columns are not in it) and in the K padding."""
    nf = W.shape[2]
    kc_n = -(-round8(cin) // bk)
    Wt = W.reshape(9, nf, -1)
    out = torch.zeros(9, kc_n, nf, bk, dtype=W.dtype)
    for c in range(cin):
        out[:, c // bk, :, c % bk] = Wt[:, :, c]
    return out


def layout_w_dx(W, cin, bk):
    """wd[t][ko][c][BK] = W[t][ko * BK + j][c], zero for o >= nf."""
    nf = W.shape[2]
    ko_n = -(-round8(nf) // bk)
    Wt = W.reshape(9, nf, -1)
    out = torch.zeros(9, ko_n, cin, bk, dtype=W.dtype)
    for o in range(nf):
        out[:, o // bk, :, o % bk] = Wt[:, o, :cin]
    return out


def layout_ctab(W, cin, h, w):
    """ctab[cls = 2 py + px][mask = 8 ym + xm][3][nf]: over the class's taps whose bit is set in ym / xm (an even class has the
    taps k = 0 at offset 0 and k = 2 at offset -1, an odd class k = 1 at offset 0),
        k0 = sum (ax d_x - 1) W[.., cin] + (ay d_y - 1) W[.., cin + 1],   kj = sum ax W[.., cin],   ki = sum ay W[.., cin + 1]
    with ax, ay as the float32 values the host code computes."""
    nf = W.shape[2]
    ax = float(torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(max(1, h - 1)), dtype=torch.float32))
    ay = float(torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(max(1, w - 1)), dtype=torch.float32))
    taps = {0: ((0, 0), (2, -1)), 1: ((1, 0),)}
    out = torch.zeros(4, 64, 3, nf, dtype=torch.float64)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        for m in range(64):
            ym, xm = m >> 3, m & 7
            for a, (ky, dy_) in enumerate(taps[py]):
                if not (ym >> a) & 1:
                    continue
                for b_, (kx, dx_) in enumerate(taps[px]):
                    if not (xm >> b_) & 1:
                        continue
                    vx, vy = W[ky, kx, :, cin], W[ky, kx, :, cin + 1]
                    out[cls, m, 0] += (ax * dx_ - 1.0) * vx + (ay * dy_ - 1.0) * vy
                    out[cls, m, 1] += ax * vx
                    out[cls, m, 2] += ay * vy
    return out + 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the clamped filters (tolerance cases on dc_sub1_thin's shape)
def clamped_inputs(kind):
    """dc_sub1_thin's lattice with filter 0 all zero ("zero"), or with filter 1 scaled to |V_1| = 1e-7, below the clamp at
    sqrt(1e-12) ("below": g_1 = 0.5 and b_1 = 0 keep that channel's outputs below 0.6, so that the stored type's own rounding of
    them -- 2**-9 of the weight, 2**-9 of the output -- stays under the 1e-3 bar on the tensor's max norm in bf16 too)."""
    case = BY_NAME["dc_sub1_thin"]
    x, V, g, b, dy = (t.clone() for t in case_inputs(case))
    if kind == "zero":
        V[:, :, 0, :] = 0.0
    else:
        assert kind == "below"
        V[:, :, 1, :] *= 1e-7 / 2.0 ** case.k
        g[1], b[1] = 0.5, 0.0
    return case, (x, V, g, b, dy)
