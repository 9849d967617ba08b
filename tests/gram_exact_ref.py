"""Exact (tolerance-free) reference of the Gram kernels (csrc/gram.hip) on integer maps.  CPU only.

With maps of integers in [-2, 2] every product and every partial sum of D_b = F_g[b]^T F_g[b] - F_t[b]^T F_t[b] is an integer, in any
order, split or wave, so `sign` must be sign(D) over the whole [n, cp, cp] array -- the entries with D == 0 and the pad included --
and `partial` the integer per-tile sums of |D| in the order the kernel file's header states: a diagonal tile counts i <= j only
(the diagonal once, the rest twice), an off-diagonal tile (ti < tj) every entry twice.  The backward with coef = 2**-10 and a
device scale of 2 onto a prefill of small integers is pre + 2**-9 act'(y) (F_g S): exact in fp32, one RNE to the stored type.
`headroom` is the condition; the conventions (gen, ints, rounded, first_diff, LIMIT) are tests/exact_ref.py's.
"""
import torch

import exact_ref as E
import gram_ref as G

LIMIT = E.LIMIT
GT = 32
COEF, DEV_SCALE = 2.0 ** -10, 2.0
PAD_GARBAGE = 1000.0


class Case(object):
    """n maps of h x w pixels, c channels.  tie: None, "block" (F_t = F_g on channels 0..7: D == 0 on that 8 x 8 block) or "all"
    (F_t = F_g with its pixels permuted per image: D == 0 everywhere while the inputs differ).  splits: ups_gram_plan per type."""
    def __init__(self, name, n, c, h, w, splits, tie=None, reaches=""):
        self.name, self.n, self.c, self.h, self.w, self.splits, self.tie, self.reaches = name, n, c, h, w, splits, tie, reaches
        self.hw = h * w
        self.ld = (c + 7) // 8 * 8
        self.cp = (c + GT - 1) // GT * GT
        self.tiles = self.cp // GT

    def __repr__(self):
        return self.name


ONE = {"bf16": 1, "fp32": 1}
HW35 = {"bf16": 1, "fp32": 2}          # (35 pixels: 3 k-steps of 16, or 18 of 2 -- two splits)
CASES = [
    Case("gm_ragged_40", 3, 40, 5, 7, HW35, reaches="a ragged 32-channel tile with pad rows in S; hw = 35 is no multiple of the K step"),
    Case("gm_33", 2, 33, 6, 6, {"bf16": 1, "fp32": 2}, reaches="one channel in the second tile (fp32: 18 k-steps, two splits)"),
    Case("gm_1x1", 3, 3, 1, 1, ONE, reaches="one pixel, three channels"),
    Case("gm_offdiag", 2, 64, 16, 16, {"bf16": 1, "fp32": 8}, reaches="one off-diagonal tile pair (fp32: 128 k-steps, 8 splits)"),
    Case("gm_split_bf16", 2, 64, 1, 257, {"bf16": 2, "fp32": 9},
         reaches="hw = 257: the smallest at c = 64 with two splits in bf16 (17 k-steps of 16): gram_fwd_reduce_kernel"),
    Case("gm_split_fp32", 2, 64, 3, 11, {"bf16": 1, "fp32": 2},
         reaches="hw = 33: the smallest at c = 64 with two splits in fp32 (17 k-steps of 2)"),
    Case("gm_tie_block", 3, 40, 5, 7, HW35, tie="block", reaches="D exactly 0 on an 8 x 8 block and its mirror: the sign = 0 branch"),
    Case("gm_tie_all", 3, 40, 5, 7, HW35, tie="all", reaches="D identically 0 with different inputs: all signs 0, every partial +0"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
DTYPES = ("bf16", "fp32")


def case_maps(case):
    """(target, generated) [n, h, w, ld] float64: integers in [-2, 2] in the c logical channels (about half of them zero where
    hw * c is large), garbage in the pad channels."""
    g = E.gen(case.name)
    dens = 0.5 if case.hw * case.c > 4096 else 1.0
    shape = (case.n, case.h, case.w, case.ld)
    a, b = E.ints(g, shape, 2, dens), E.ints(g, shape, 2, dens)
    if case.tie == "block":
        a[..., :8] = b[..., :8]
    elif case.tie == "all":
        for i in range(case.n):
            perm = torch.randperm(case.hw, generator=g)
            a[i] = b[i].reshape(case.hw, case.ld)[perm].view(case.h, case.w, case.ld)
        assert not torch.equal(a, b)
    a[..., case.c:] = PAD_GARBAGE
    b[..., case.c:] = -PAD_GARBAGE
    return a, b


def pair_tiles(p, tiles):
    ti = 0
    while p >= tiles - ti:
        p -= tiles - ti
        ti += 1
    return ti, ti + p


def reference(case, a, b, relu):
    """D [n, c, c] (integers), sign [n, cp, cp] int8 (pad 0), partial [n * pairs] float32 in the kernel's (image, pair) order."""
    Ft, Fg = G.as_F(a, case.c, relu), G.as_F(b, case.c, relu)
    D = Fg.transpose(1, 2) @ Fg - Ft.transpose(1, 2) @ Ft
    cp, tiles = case.cp, case.tiles
    Dp = torch.zeros(case.n, cp, cp, dtype=torch.float64)
    Dp[:, :case.c, :case.c] = D
    sign = torch.sign(Dp).to(torch.int8)
    pairs = tiles * (tiles + 1) // 2
    partial = torch.zeros(case.n, pairs, dtype=torch.float64)
    for p in range(pairs):
        ti, tj = pair_tiles(p, tiles)
        t = Dp[:, ti * GT:(ti + 1) * GT, tj * GT:(tj + 1) * GT].abs()
        if ti == tj:
            partial[:, p] = torch.diagonal(t, dim1=1, dim2=2).sum(-1) + 2.0 * torch.triu(t, diagonal=1).sum(dim=(1, 2))
        else:
            partial[:, p] = 2.0 * t.sum(dim=(1, 2))
    return {"D": D, "sign": sign, "partial": partial.view(-1), "Ft": Ft, "Fg": Fg}


def backward_reference(case, b, sign, pre, relu):
    """pre + COEF * DEV_SCALE * act'(y) * (F_g S) on the c logical channels, float64; channels [c, ld) are pre's."""
    Fg = G.as_F(b, case.c, relu)
    grad = COEF * DEV_SCALE * (Fg @ sign[:, :case.c, :case.c].double())
    if relu:
        grad = grad * (Fg > 0).double()
    out = pre.clone()
    out[..., :case.c] = pre[..., :case.c] + grad.view(case.n, case.h, case.w, case.c)
    return out


def prefill(case):
    """gb before the launch: small integers, no negative zero; recognisable values in the pad channels."""
    pre = E.ints(E.gen(case.name + "/gb"), (case.n, case.h, case.w, case.ld), 3) + 0.0
    pre[..., case.c:] = 77.0
    return pre


def headroom(case, a, b, relu):
    """{"D": the largest sum |F_g F_g| + |F_t F_t| of a D entry, "partial": the largest per-(image, tile) sum of (weighted) |D|,
    "bwd": the largest sum of |F_g| |S| of a gradient element plus the prefill, in units of COEF * DEV_SCALE}: all < 2**24."""
    Ft, Fg = G.as_F(a, case.c, relu).abs(), G.as_F(b, case.c, relu).abs()
    ref = reference(case, a, b, relu)
    top = Fg.transpose(1, 2) @ Fg + Ft.transpose(1, 2) @ Ft
    bwd = Fg @ ref["sign"][:, :case.c, :case.c].double().abs() + 3.0 / (COEF * DEV_SCALE)
    return {"D": float(top.max()), "partial": float(ref["partial"].max()), "bwd": float(bwd.max())}
