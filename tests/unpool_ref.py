"""fp64 restatement of the backward of unpool_features + concat (ups_unpool_bwd, csrc/partpath.hip) and of mask_parts, the cases
that reach every route of its two kernels, and their inputs (parity_ledger.md, section 10, has the branch -> case table).

    g_hard[b, px, p] = sum_f g[b, px, f] feat[b, p, f] + g[b, px, F + p]
    g_feat[b, p, f]  = sum_px hard[b, px, p] g[b, px, f]

A case names the route it is there for -- form (0: unpool_bwd_kernel, 1: unpool_bwd_mfma_kernel), blocks per image, tiles per
block, pixels per tile, whether the direct-copy loop past the five register pieces of a gradient tile is reached -- and
test_host_unpool.py holds that claim to ups_unpool_bwd_plan, the function the launch itself reads.  Inputs are pure functions of
(case, regime):

  lattice01   hard is a 0 / 1 map (one-hot rows, with a tie, an all-parts row and an all-zero row planted in the first tile, the
              last tile and the middle of every image), feat and g hold integers in [-4, 4]
  lattice22   the same with hard holding integers in [-2, 2] (exact in bf16: the lo half of the matrix-core form's hi + lo pair is 0)
  gauss       the inputs of test_gpu_kernels.py::test_unpool_backward_on_the_matrix_cores: one-hot hard, a tie, eight arbitrary
              fp32 rows; feat the float view of a bf16 tensor when the gradient is bf16; g Gaussian in the gradient's type
  gauss_f32feat   gauss with a feat that is NOT bf16-representable: the kernels round it to bf16, so does the reference

In the lattice regimes every product and every partial sum is an integer below 2^24 (``headroom``), so any order of summation in
fp32 gives the fp64 result exactly and the comparison is torch.equal.  The padding channels [F + P, ldo) of g hold +-3 in every
regime: nothing may read them into a result."""
import collections
import zlib

import torch

LATTICE = ("lattice01", "lattice22")
REGIMES = LATTICE + ("gauss",)
KG_PIECES = 5 * 256            # 16-byte pieces of a gradient tile that travel through registers (unpool_bwd_kernel: KG = 5)

Case = collections.namedtuple("Case", "name dtype B H W P F ldo form bpi tpb tpx direct regimes env hard_lead ghard_lead reaches")


def round8(n):
    return (n + 7) // 8 * 8


def _case(name, dtype, B, H, W, P, F, form, bpi, tpb, tpx, direct, reaches, ldo=None, regimes=REGIMES, env=None, hard_lead=0,
          ghard_lead=0):
    return Case(name, dtype, B, H, W, P, F, ldo or round8(F + P), form, bpi, tpb, tpx, direct, regimes, env, hard_lead, ghard_lead,
                reaches)


# ----------------------------------------------------------------------------- matrix-core form: bf16, F = 64, ldo = round8(64 + P)
# (B, H, W, tiles per image, blocks per image, tiles per block, what it reaches)
MFMA_SHAPES = [
    (1, 8, 16, 1, 1, 1, "a single tile: issue(1) skipped, the tail wait at t = 0"),
    (1, 16, 16, 2, 2, 1, "two blocks of one tile, the second block's px0"),
    (1, 16, 24, 3, 1, 3, "all three ring slots, none reused"),
    (1, 16, 40, 5, 1, 5, "first slot reuse, the steady wait count, the tail"),
    (1, 24, 32, 6, 2, 3, "the second block starts mid-image"),
    (1, 28, 32, 7, 1, 7, "t % 3 through two wraps"),
    (1, 34, 64, 17, 1, 17, "longer than the benchmark's 16 tiles per block"),
    (3, 20, 32, 5, 1, 5, "image offsets of gsrc / hsrc / the partial records"),
    (2, 40, 32, 10, 2, 5, "image offsets and a second block together"),
]
MFMA_P = (10, 16, 20, 25)
MFMA_CASES = [_case("mfma_{}x{}x{}_P{}".format(B, H, W, P), "bf16", B, H, W, P, 64, 1, bpi, tpb, 128, False, why)
              for (B, H, W, tiles, bpi, tpb, why) in MFMA_SHAPES for P in MFMA_P]
# the B bpi < 512 cap stops the doubling at 2 blocks per image: an even count of tiles per block, 21 MB of gradient at P = 25
MFMA_BIG = [_case("mfma_256x16x32_P{}".format(P), "bf16", 256, 16, 32, P, 64, 1, 2, 2, 128, False,
                  "the B bpi < 512 cap; an even tile count", regimes=LATTICE) for P in (10, 25)]

# ----------------------------------------------------------------------------- one matrix-core shape, each change alone -> generic form
FALL_CASES = [
    _case("fall_f32", "f32", 1, 16, 40, 10, 64, 0, 32, 1, 64, False, "an fp32 gradient (tpx = 64: exactly the 1280 register pieces)"),
    _case("fall_ldo88", "bf16", 1, 16, 40, 10, 64, 0, 32, 1, 128, True, "ldo = 88 is not P = 10's pitch", ldo=88),
    _case("fall_F56", "bf16", 1, 16, 40, 10, 56, 0, 32, 1, 128, False, "F = 56 (in the same 80-channel rows)", ldo=80),
    _case("fall_P12", "bf16", 1, 16, 40, 12, 64, 0, 32, 1, 128, False, "P = 12 has no instance"),
    _case("fall_env", "bf16", 1, 16, 40, 10, 64, 0, 32, 1, 128, False, "UPS_UNPOOL_MFMA=0", env="0"),
    _case("fall_hard_view", "bf16", 1, 16, 40, 10, 64, 0, 32, 1, 128, False,
          "hard one float into a larger buffer: the scalar path of tile_request / tile_commit (nv == 0)", hard_lead=1),
    _case("fall_ghard_view", "bf16", 1, 16, 40, 10, 64, 0, 32, 1, 128, False,
          "g_hard one float into a larger buffer: the scalar tail of tile_store_f32", ghard_lead=1),
]

# ----------------------------------------------------------------------------- generic form
GENERIC_CASES = [
    _case("gen_2x17x19_P10_bf16", "bf16", 2, 17, 19, 10, 64, 0, 32, 1, 128, False, "323 pixels: slabs of 128, 128 and 67, 29 empty"),
    _case("gen_2x17x19_P10_f32", "f32", 2, 17, 19, 10, 64, 0, 32, 1, 64, False, "tpx = 64: slabs of 5 x 64 and 3 pixels, 26 empty"),
    _case("gen_1x75x75_P10_bf16", "bf16", 1, 75, 75, 10, 64, 0, 32, 2, 128, False,
          "slab_px = 256: two tiles per slab, a last slab of 128 + 121 with the ragged tile prefetched"),
    _case("gen_3x7x7_P3_F8_bf16", "bf16", 3, 7, 7, 3, 8, 0, 32, 1, 128, False, "odd hw, odd P: images 1, 2 have a 4-byte-aligned hard base"),
    _case("gen_3x7x7_P3_F8_f32", "f32", 3, 7, 7, 3, 8, 0, 32, 1, 128, False, "odd hw, odd P: images 1, 2 have a 4-byte-aligned hard base"),
    _case("gen_2x16x24_P3_f32", "f32", 2, 16, 24, 3, 64, 0, 32, 1, 128, True, "tpx = 128, 2304 pieces per tile: the direct-copy loop"),
    _case("gen_2x16x24_P5_ldo96_bf16", "bf16", 2, 16, 24, 5, 64, 0, 32, 1, 128, True,
          "the direct-copy loop for 2-byte rows (1536 pieces); padding channels 69 to 95", ldo=96),
    _case("gen_2x12x20_P25_bf16", "bf16", 2, 12, 20, 25, 64, 0, 32, 1, 32, False, "tpx = 32; PL = 10 pixel lanes, 6 idle threads"),
    _case("gen_2x12x20_P25_f32", "f32", 2, 12, 20, 25, 64, 0, 32, 1, 32, False, "tpx = 32; PL = 10 pixel lanes, 6 idle threads"),
    _case("gen_1x12x20_P64_bf16", "bf16", 1, 12, 20, 64, 64, 0, 32, 1, 32, False,
          "PL = 4; every lane of phase 2 carries a part; LDS above the 64 KB default"),
    _case("gen_2x9x31_P1_F8_bf16", "bf16", 2, 9, 31, 1, 8, 0, 32, 1, 128, False, "one part, one 8-channel group"),
    _case("gen_2x9x31_P1_F8_f32", "f32", 2, 9, 31, 1, 8, 0, 32, 1, 128, False, "one part, one 8-channel group"),
    _case("gen_2x16x16_P10_F40_bf16", "bf16", 2, 16, 16, 10, 40, 0, 32, 1, 128, False, "ff < F inside the unrolled group of 64; f < F lanes idle"),
    _case("gen_2x16x16_P10_F40_f32", "f32", 2, 16, 16, 10, 40, 0, 32, 1, 128, True,
          "ff < F inside the unrolled group of 64; 1792 pieces per tile"),
]
# through ops.UnpoolFn with a non-contiguous incoming gradient
FN_CASE = _case("fn_1x16x16_P10_F16", "bf16", 1, 16, 16, 10, 16, 0, 32, 1, 128, False, "the .contiguous() in UnpoolFn.backward")

# bf16 gradient with a feat that is not bf16-representable: both forms round it
F32FEAT_CASE = _case("mfma_1x16x40_P10_f32feat", "bf16", 1, 16, 40, 10, 64, 1, 1, 5, 128, False,
                     "feat rounded to bf16 by both forms", regimes=("gauss_f32feat",))

ALL_CASES = MFMA_CASES + MFMA_BIG + FALL_CASES + GENERIC_CASES + [FN_CASE, F32FEAT_CASE]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# the shapes of test_gpu_kernels.py::test_mask_parts_forward_over_tiles
MASK_PARTS_SHAPES = [(3, 16, 10), (2, 24, 25), (1, 10, 16), (2, 32, 20), (1, 7, 3)]


def torch_dtype(case):
    return torch.bfloat16 if case.dtype == "bf16" else torch.float32


def esz(case):
    return 2 if case.dtype == "bf16" else 4


def hw_of(case):
    return case.H * case.W


def direct_copy_reached(case, tpx):
    """The largest tile of the case has more 16-byte pieces than the request registers hold."""
    cnt = min(tpx, hw_of(case))
    return cnt * case.ldo * esz(case) // 16 > KG_PIECES


def headroom(case, regime):
    """(max |g_hard|, max |g_feat|) any lattice input of the case can give: sums of integers, each below 2^24."""
    assert regime in LATTICE
    hmax = 1 if regime == "lattice01" else 2
    return 4 * 4 * case.F + 4, hmax * 4 * hw_of(case)


def planted(case):
    """[(pixel, kind)] planted in every image in the lattice regimes: first 128-pixel tile, last one, and the middle."""
    hw = hw_of(case)
    assert hw >= 12
    # (the first and the last pixel of an image carry a tie, not the all-zero row: a pixel dropped there must show in g_feat)
    kinds = ("tie", "all", "zero", "zero", "tie", "all", "all", "zero", "tie")
    at = [0, 1, 2, hw // 2 - 1, hw // 2, hw // 2 + 1, hw - 3, hw - 2, hw - 1]
    return list(zip(at, kinds))


def planted_row(kind, P):
    row = torch.zeros(P)
    if kind == "tie":
        row[:min(2, P)] = 1.0
    elif kind == "all":
        row[:] = 1.0
    return row


def _gen(case, regime):
    return torch.Generator().manual_seed(zlib.crc32("{}/{}".format(case.name, regime).encode()))


def inputs(case, regime):
    """-> hard [B, hw, P] fp32, feat [B, P, F] fp32, g [B, hw, ldo] in the case's gradient type."""
    gen = _gen(case, regime)
    B, hw, P, F, ld = case.B, hw_of(case), case.P, case.F, case.ldo
    dt = torch_dtype(case)
    one_hot = torch.nn.functional.one_hot(torch.randint(0, P, (B, hw), generator=gen), P).float()
    if regime in LATTICE:
        hard = one_hot if regime == "lattice01" else torch.randint(-2, 3, (B, hw, P), generator=gen).float()
        for px, kind in planted(case):
            hard[:, px] = planted_row(kind, P)
        feat = torch.randint(-4, 5, (B, P, F), generator=gen).float()
        g = torch.randint(-4, 5, (B, hw, ld), generator=gen).float()
    else:
        hard = one_hot
        hard[0, 0] = planted_row("tie", P)
        assert hw >= case.W + 8
        hard[0, case.W:case.W + 8] = torch.randn(8, P, generator=gen)
        feat = torch.randn(B, P, F, generator=gen)
        if case.dtype == "bf16" and regime != "gauss_f32feat":
            feat = feat.bfloat16().float()                       # bf16 mode: the float view of a bf16 tensor
        g = torch.randn(B, hw, ld, generator=gen)
    if ld > F + P:
        g[..., F + P:] = 3.0 * (2.0 * torch.randint(0, 2, (B, hw, ld - F - P), generator=gen).float() - 1.0)
    return hard, feat, g.to(dt)


def reference(hard, feat, g, F, P, chunk=16):
    """fp64 g_hard [B, hw, P] and g_feat [B, P, F], over `chunk` images at a time."""
    want_h, want_f = [], []
    for b0 in range(0, hard.shape[0], chunk):
        gd = g[b0:b0 + chunk].double()
        want_h.append(torch.einsum("bxf,bpf->bxp", gd[..., :F], feat[b0:b0 + chunk].double()) + gd[..., F:F + P])
        want_f.append(torch.einsum("bxp,bxf->bpf", hard[b0:b0 + chunk].double(), gd[..., :F]))
    return torch.cat(want_h), torch.cat(want_f)


def reference_of(case, regime, hard, feat, g):
    """The reference the kernels are held to: a bf16 gradient contracts with feat as bf16."""
    if regime == "gauss_f32feat":
        feat = feat.bfloat16().float()
    return reference(hard, feat, g, case.F, case.P)


def first_difference(got, want, rows="pixel"):
    """Where two [B, R, C] tensors first differ by value (row-major; a NaN differs from everything): image, row (a pixel of g_hard
    with its 128-pixel tile, a part of g_feat), channel, both values.  None when they are equal."""
    bad = ~(got == want)
    if not bool(bad.any()):
        return None
    b, r, c = [int(v) for v in bad.nonzero()[0]]
    where = "pixel {} (128-pixel tile {}, row {} of it)".format(r, r // 128, r % 128) if rows == "pixel" else "{} {}".format(rows, r)
    return "{} of {} differ; first at image {}, {}, channel {}: got {!r}, want {!r}".format(
        int(bad.sum()), bad.numel(), b, where, c, float(got[b, r, c]), float(want[b, r, c]))


# ----------------------------------------------------------------------------- mask_parts backward
def mask_parts_inputs(B, S, P, dtype, lattice):
    """view [B, S, S, 3], hard [B, S, S, P], and the gradient of MaskPartsFn's output [P * B, S, S, 8] in `dtype`: channels 3 to 7 are
    padding and hold +-3."""
    gen = torch.Generator().manual_seed(zlib.crc32("mask_parts/{}/{}/{}/{}/{}".format(B, S, P, dtype, lattice).encode()))
    hard = torch.nn.functional.one_hot(torch.randint(0, P, (B, S, S), generator=gen), P).float()
    if lattice:
        view = torch.randint(-4, 5, (B, S, S, 3), generator=gen).float()
        g = torch.randint(-4, 5, (P * B, S, S, 8), generator=gen).float()
    else:
        view = torch.rand(B, S, S, 3, generator=gen) * 2 - 1
        hard[0, 0, 0] = torch.randn(P, generator=gen)           # an arbitrary fp32 row
        g = torch.randn(P * B, S, S, 8, generator=gen)
    g[..., 3:] = 3.0 * (2.0 * torch.randint(0, 2, (P * B, S, S, 5), generator=gen).float() - 1.0)
    return view, hard, g.to(dtype)


def mask_parts_bwd_reference(view, g, B, P):
    """g_hard[b, y, x, p] = sum_c g[p B + b, y, x, c] view[b, y, x, c], c < 3, in fp64."""
    S = view.shape[1]
    g5 = g.double().view(P, B, S, S, 8)[..., :3]
    return torch.einsum("pbyxc,byxc->byxp", g5, view.double())
