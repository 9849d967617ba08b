"""Mask priors on trained-regime masks: the cases, their premises and the fp64 reference (parity_ledger.md, section 7).

`tests/test_gpu_kernels.py::test_mask_priors_forward_and_backward` draws every case from `2 * smooth + N(0, 1)` logits: high
entropy, no tied pixel, every part present, every rectangle mid-image.  The three regimes here are what a trained mask decoder gives:

  confident       the smooth field scaled until the mean per-pixel entropy is <= 0.25 nats (soft-max saturation: exp underflow,
                  m == 0 exactly in fp32, g == 0 exactly), unit noise on top
  lattice_ties    integer logits, round(3 * smooth) + eps with eps in {-1, 0, 1} (or no eps at all): equal logits give equal
                  probabilities in fp32 and in fp64, logits that differ do so by >= 1, so `hard` is multi-hot on a third of
                  the pixels and the tie decision never depends on rounding
  border_absent   every part a blob centred ON the image border (all four borders occur), one part absent (logit -50) from one
                  view-0 image and another from one view-1 image; run with the kernels' own centres and again with four centres
                  planted in the four image corners

Every regime is a pure function of (variant, P, S, B) and the seed those give.  The reference is `_prior_oracle` of
test_gpu_kernels.py restated with two differences: the inputs are the float32 numbers the kernels see (`l` is the float32 sum),
and the rectangle centres are an argument, drawn with `R.draw_rect`, as `Trainer._prior` takes `px` as an argument.

What the cases rest on is asserted, not assumed: `premises` measures, `check_premises` asserts (test_host_prior_edges.py for every
case without a GPU; the GPU tests assert the cheap ones again before they launch)."""
import collections
import functools
import math

import numpy as np
import torch

from oracle import np_ops
from oracle import ref_model as R

GAMMA, PATCH = 10.0, 8
HALF = PATCH // 2
# non-trivial weights on every term, as in test_mask_priors_forward_and_backward
WEIGHTS = {"kl": 0.7, "entropy": 1.3, "ms": 0.05, "area": 2.0e-3, "patch": 0.02, "gmrf": 0.3, "var": 1.7, "msl": 0.4}
MS = {0: (1.0, 1.0e-2), 1: (1.5, 0.05)}          # (alpha, lambda): hard-coded for variant 0, the yaml schedules' values for SB_model48c

# variant, P, S, B, entropy_func: the smallest shapes that reach every form of priors.hip (ledger section 7 for what each reaches)
SHAPES = [(0, 3, 16, 3, "entropy"), (0, 25, 20, 2, "cross_entropy"), (1, 10, 32, 3, "cross_entropy"),
          (0, 10, 128, 2, "entropy"), (1, 10, 128, 2, "cross_entropy"), (0, 16, 128, 2, "cross_entropy"),
          (1, 20, 128, 2, "cross_entropy"), (0, 25, 128, 2, "entropy"), (0, 10, 256, 1, "cross_entropy"),
          (0, 25, 256, 1, "entropy")]
REGIMES = ("confident", "lattice_ties", "lattice_ties_noeps", "border_absent")
NOEPS_SHAPES = [(1, 10, 32, 3, "cross_entropy"), (0, 10, 128, 2, "entropy")]       # eps all zeros: l == l_mean
# seeds that put an element at the Mumford-Shah threshold, an undecided pixel or too many unstable centres move here
SEED_SHIFT = {}

Inputs = collections.namedtuple("Inputs", "regime variant P S B entropy_func")


class Case(collections.namedtuple("Case", "regime variant P S B entropy_func px_bpi planted")):
    @property
    def inputs(self):
        return Inputs(*self[:6])

    @property
    def id(self):
        s = "{}-v{}-P{}-S{}-{}".format(self.regime, self.variant, self.P, self.S, "ce" if self.entropy_func == "cross_entropy" else "ent")
        return s + ("-planted" if self.planted else "") + ("-bpi{}".format(self.px_bpi) if self.px_bpi else "")


def _cases():
    out = []
    for sh in SHAPES:
        out.append(Case("confident", *sh, 0, False))
        out.append(Case("lattice_ties", *sh, 0, False))
        if sh in NOEPS_SHAPES:
            out.append(Case("lattice_ties_noeps", *sh, 0, False))
        for planted in (False, True):
            out.append(Case("border_absent", *sh, 0, planted))
            if sh[:3] == (0, 10, 128):       # UPS_PRIOR_PX_BPI: the multi-tile loops of the pixel-per-lane kernels
                out += [Case("border_absent", *sh, b, planted) for b in (4, 1)]
    return out


CASES = _cases()
INPUTS = list(collections.OrderedDict((c.inputs, None) for c in CASES))


def inputs_id(i):
    return "{}-v{}-P{}-S{}".format(i.regime, i.variant, i.P, i.S)


# ------------------------------------------------------------------------------------------------ the regimes
def _smooth(g, n, P, S):
    """The existing test's field before its factor 2: low-resolution noise, bilinearly interpolated -> [n, S, S, P] fp64."""
    low = torch.randn(n, P, S // 4, S // 4, generator=g, dtype=torch.float64)
    return torch.nn.functional.interpolate(low, size=(S, S), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous()


def mean_entropy(l):
    ls = torch.log_softmax(l.double(), -1)
    return float(-(ls.exp() * ls).sum(-1).mean())


def gap_to_second(l):
    """Per pixel, the largest logit minus the largest one below it (inf where all are equal); exact equality is a tie, not a gap."""
    mx = l.max(dim=-1, keepdim=True).values
    second = torch.where(l < mx, l, torch.full_like(l, -math.inf)).max(dim=-1).values
    return mx[..., 0] - second


def undecided_bar(l):
    return 1e-5 * max(1.0, float(l.abs().max()))


def _decide(lm, eps):
    """Noise is continuous, so a few pixels per million have their two top logits closer than the bar of `premises`: there the
    first maximum's eps is raised by 1/64 (part of the regime: the same function of the seed every time).  -> eps, pixels moved."""
    moved = 0
    for _ in range(8):
        l = lm + eps
        bad = gap_to_second(l) < 2.0 * undecided_bar(l)
        if not bool(bad.any()):
            break
        moved += int(bad.sum())
        first = l.argmax(dim=-1)
        eps = eps.clone()
        eps[bad] = eps[bad] + torch.nn.functional.one_hot(first[bad], l.shape[-1]).to(eps.dtype) / 64.0
    return eps, moved


def _border_blobs(g, n, P, S):
    """Every part a blob of peak 12 centred on the border at a random position along it; image i, part p sits on border
    (i + p) % 4 (top, bottom, left, right), so rows and columns swap roles and all four borders occur in every image.
    Even parts: isotropic, sigma S / 5.  Odd parts: the same sigma along the border but 3 pixels across it, on a floor of -6
    (18 * G - 6): a ridge that hugs the border.  The patch is 8 pixels at every image size, and with unit noise no part of an
    isotropic sigma-S/5 blob lies within 4 pixels of the border of a 128- or 256-wide image; the floor keeps the ridge parts from
    collecting the noise-decided pixels of the interior, which would pull their centres to the middle."""
    sig = S / 5.0
    ii = torch.arange(S, dtype=torch.float64)
    t = torch.rand(n, P, generator=g, dtype=torch.float64) * (S - 1)
    lm = torch.empty(n, S, S, P, dtype=torch.float64)
    for i in range(n):
        for p in range(P):
            side = (i + p) % 4
            across = ii if side in (0, 2) else (S - 1) - ii               # distance from the part's border
            along = ii - t[i, p]
            if p % 2 == 0:
                ga, gb, amp, floor = torch.exp(-across ** 2 / (2 * sig * sig)), torch.exp(-along ** 2 / (2 * sig * sig)), 12.0, 0.0
            else:
                ga, gb, amp, floor = torch.exp(-across ** 2 / (2 * 3.0 * 3.0)), torch.exp(-along ** 2 / (2 * sig * sig)), 18.0, -6.0
            blob = amp * (ga.view(S, 1) * gb.view(1, S)) + floor         # rows = across, columns = along: a top / bottom border
            lm[i, :, :, p] = blob if side < 2 else blob.t()
    return lm


def absent_parts(i):
    """(image, part) of the part forced absent in view 0 and in view 1 (image index within all 2 B images)."""
    return (i.B - 1, i.P - 1), (2 * i.B - 1, max(i.P - 2, 0))


@functools.lru_cache(maxsize=4)
def build(i):
    """-> dict: lm, eps, g_hard float32 [2 B, S, S, P] (views 0 and 1 stacked), `moved` pixels of _decide, `scale` of the confident field."""
    ri = REGIMES.index(i.regime)
    g = torch.Generator().manual_seed(1000 * (ri + 1) + 100 * i.variant + i.P + i.S + SEED_SHIFT.get(i, 0))
    n, P, S = 2 * i.B, i.P, i.S
    info = {"scale": None}
    if i.regime == "confident":
        sm = 2.0 * _smooth(g, n, P, S)
        eps = torch.randn(n, S, S, P, generator=g, dtype=torch.float64).float()
        scale = 20.0
        while mean_entropy((scale * sm).float() + eps) > 0.25:
            scale *= 1.25
        lm, info["scale"] = (scale * sm).float(), scale
    elif i.regime in ("lattice_ties", "lattice_ties_noeps"):
        lm = torch.round(3.0 * _smooth(g, n, P, S)).float()
        eps = torch.randint(-1, 2, (n, S, S, P), generator=g).float()
        if i.regime == "lattice_ties_noeps":
            eps = torch.zeros_like(eps)
    else:
        lm = _border_blobs(g, n, P, S)
        eps = torch.randn(n, S, S, P, generator=g, dtype=torch.float64).float()
        for img, part in absent_parts(i):
            lm[img, :, :, part] = -50.0
        lm = lm.float()
    g_hard = torch.randn(n, S, S, P, generator=g, dtype=torch.float64).float()
    eps, info["moved"] = _decide(lm, eps)
    info.update(lm=lm, eps=eps, g_hard=g_hard, l=lm + eps)
    return info


# ------------------------------------------------------------------------------------------------ centres
CORNERS = lambda S: [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]          # (row, column)


def plant(px, S):
    """The first four (image, part) slots of a view's [B, P, 2] (row, column) centres -- parts 0..3 of image 0 where P >= 4 -- moved
    into the four corners."""
    px = px.clone()
    flat = px.view(-1, 2)
    for k, c in enumerate(CORNERS(S)):
        flat[k, 0], flat[k, 1] = c
    return px


def oracle_centres(hard, S):
    """R.patch_mask on a (multi-hot) hard map: rectangles [n, S, S, P], (row, column) centres of the boxes drawn [n, P, 2], and
    which centres are stable: both fractional positions more than 1e-3 from an integer, so that truncation cannot go either way."""
    rect, rc = R.patch_mask(hard, GAMMA, PATCH, "xy")
    mu, _ = R.probs_to_mu_sigma(R.spatial_softmax(hard * GAMMA))
    frac = mu * S / 2.0 + S / 2.0
    stable = ((frac - frac.round()).abs() > 1e-3).all(-1)
    return rect, rc, stable


def is_clipped(px, S):
    """A box of half-width HALF around the centre leaves the image."""
    return ((px - HALF < 0) | (px + HALF > S - 1)).any(-1)


# ------------------------------------------------------------------------------------------------ the reference
def rects(px, S, dtype=torch.float64):
    """[B, P, 2] (row, column) centres -> [B, S, S, P] rectangles, drawn by the oracle's draw_rect."""
    B, P, _ = px.shape
    r = R.draw_rect(px.reshape(-1, 2).to(torch.int64), PATCH, PATCH, S, S, dtype, order="yx")
    return r.reshape(B, P, S, S).permute(0, 2, 3, 1)


def reference(i, inp, px0, px1, dtype=torch.float64, grads=True):
    """The mask priors of Trainer.make_loss_ops from the oracle's building blocks (semantics of `_prior_oracle`), on the float32
    inputs the kernels see and with the rectangle centres handed in ((row, column) [B, P, 2] per view; ignored by variant 1).
    -> (dict of the logged forward quantities, dict of the gradient maps d_tot0, d_tot1, d_rec0, d_rec1 w.r.t. l_mean)."""
    B, S, P, variant = i.B, i.S, i.P, i.variant
    w = dict(WEIGHTS)
    if variant == 1:       # SB_model48c has no Mumford-Shah-on-masks / area / patch terms
        w.update({"ms": 0.0, "area": 0.0, "patch": 0.0})
    ms_alpha, ms_lambda = MS[variant]
    lm = inp["lm"].to(dtype)
    off = inp["l"].to(dtype) - lm          # l = l_mean + off is the float32 sum the kernels hold, exactly (premise "l exact")
    gh = inp["g_hard"].to(dtype)
    lm0, lm1 = lm[:B].clone().requires_grad_(True), lm[B:].clone().requires_grad_(True)
    l0, l1 = lm0 + off[:B], lm1 + off[B:]
    m0, m1 = torch.softmax(l0, -1), torch.softmax(l1, -1)
    h0, h1 = R.ste(R.hard_max(m0), m0), R.ste(R.hard_max(m1), m1)
    q = {}
    kl0 = (m0 * torch.log(P * m0 + 1e-20)).sum(-1).mean()
    kl1 = (m1 * torch.log(P * m1 + 1e-20)).sum(-1).mean()
    q["mask0_kl"] = kl0 + kl1
    labels = h0 if (variant == 1 or i.entropy_func == "cross_entropy") else m0
    q["weakly"] = (-(labels * torch.log_softmax(l0, -1)).sum(-1)).mean()
    dy, dx = lm0[:, 1:] - lm0[:, :-1], lm0[:, :, 1:] - lm0[:, :, :-1]
    q["gmrf"] = 0.5 * ((dy ** 2).sum(dim=(1, 2, 3)) + (dx ** 2).sum(dim=(1, 2, 3))).mean()
    sq = lambda t: (t.sum(dim=(1, 2)) ** 2).sum(dim=1).mean()
    if variant == 0:
        rect0, rect1 = rects(px0, S, dtype), rects(px1, S, dtype)
        g = R.squared_grad(m0)
        r = torch.clamp(g, max=1.0e-2)
        q["ms"], q["area"] = sq(r), sq(m0)
        q["smooth"] = sq(torch.where(g < 1.0e-2, r, torch.zeros_like(r)))
        q["contour"] = sq(torch.where(g >= 1.0e-2, r, torch.zeros_like(r)))
        q["patch"] = (h0 * (1 - rect0)).sum(dim=(1, 2, 3)).mean()
        c1 = R.spatial_softmax(m1 * GAMMA) * (1 - rect1)
        _, sig = R.probs_to_mu_sigma(c1)
        q["var"] = (sig[:, :, 0, 0] + sig[:, :, 1, 1]).sum(dim=1).mean()
        t0 = (w["kl"] * kl0 + w["entropy"] * q["weakly"] + w["ms"] * q["ms"] + w["area"] * q["area"] + w["patch"] * q["patch"]
              + w["gmrf"] * q["gmrf"])
    else:
        q["msl"] = torch.clamp(ms_alpha * R.squared_grad(lm0), max=ms_lambda).sum(dim=(1, 2, 3)).mean()
        c1 = R.spatial_softmax(m1)
        c1 = c1 / c1.sum(dim=(1, 2), keepdim=True)
        _, sig = R.probs_to_mu_sigma(c1)
        q["var"] = (sig[:, :, 0, 0] ** 2 + sig[:, :, 1, 1] ** 2).sum(dim=1).mean()
        t0 = w["kl"] * kl0 + w["entropy"] * q["weakly"] + w["gmrf"] * q["gmrf"] + w["msl"] * q["msl"]
    t1 = w["kl"] * kl1 + w["var"] * q["var"]
    r0, r1 = (gh[:B] * h0).sum(), (gh[B:] * h1).sum()
    d = {}
    if grads:
        d["d_tot0"], = torch.autograd.grad(t0 + r0, lm0, retain_graph=True)
        d["d_tot1"], = torch.autograd.grad(t1 + r1, lm1, retain_graph=True)
        d["d_rec0"], = torch.autograd.grad(r0, lm0, retain_graph=True)
        d["d_rec1"], = torch.autograd.grad(r1, lm1)
    return {k: v.detach() for k, v in q.items()}, d


def variance_per_part(m1, rect1, gamma):
    """The masked variance of view 1 per (image, part): the variant-0 `var` term before its sums."""
    _, sig = R.probs_to_mu_sigma(R.spatial_softmax(m1 * gamma) * (1 - rect1))
    return sig[:, :, 0, 0] + sig[:, :, 1, 1]


# ------------------------------------------------------------------------------------------------ premises
def premises(i, inp, cheap=False):
    """Measures what the cases rest on.  cheap: what needs no softmax in two precisions and no oracle centres."""
    B, S, P = i.B, i.S, i.P
    l = inp["l"]
    mx = l.max(dim=-1, keepdim=True).values
    nmax = (l == mx).sum(-1)
    p = {"entropy": mean_entropy(l), "tied": float((nmax >= 2).double().mean()), "triple": int((nmax >= 3).sum()),
         "min_gap": float(gap_to_second(l).min()), "gap_bar": undecided_bar(l), "moved": inp["moved"],
         "l_exact": bool(torch.equal((inp["lm"].double() + (l.double() - inp["lm"].double())), l.double()))}
    alpha, lam = MS[i.variant]
    md = torch.softmax(l.double(), -1)
    t = alpha * R.squared_grad(inp["lm"][:B].double()) if i.variant == 1 else R.squared_grad(md[:B])
    p["ms_at_threshold"] = int(((t - lam).abs() <= 5 * 2.0 ** -24 * lam).sum())
    hard = R.hard_max(md)
    owned = hard.sum(dim=(1, 2)) > 0                          # [2 B, P]
    p["absent"] = (int((~owned[:B]).sum()), int((~owned[B:]).sum()))
    p["owned"] = owned
    if cheap:
        return p
    m32 = torch.softmax(l, -1)
    p["hard_f32_equal"] = bool(torch.equal((m32 == m32.max(dim=-1, keepdim=True).values), hard.bool()))
    # saturation as float32 sees it: probabilities that are exactly 0, Mumford-Shah gradients that are exactly 0
    p["m_zero"] = float((m32 == 0).double().mean())
    p["g_zero"] = float((R.squared_grad(m32[:B]) == 0).double().mean())
    _, rc, stable = oracle_centres(hard, S)
    p["centres"], p["stable"] = rc, stable
    p["stable_share"] = float(stable[owned].double().mean())       # an absent part's centre is exactly S / 2: asserted on its own
    p["clipped"] = int(is_clipped(rc, S).sum())
    p["clipped_share"] = p["clipped"] / float(rc.shape[0] * rc.shape[1])
    return p


def check_premises(i, p):
    """Every failure here is a failure of the premise: of the case, not of a kernel."""
    what = "premise of {}: ".format(inputs_id(i))
    assert p["l_exact"], what + "l_mean + (l - l_mean) is not the float32 sum in fp64"
    assert p["min_gap"] >= p["gap_bar"], what + "an undecided pixel: top logits {} apart, bar {}".format(p["min_gap"], p["gap_bar"])
    assert p["ms_at_threshold"] == 0, what + "{} element(s) at the Mumford-Shah threshold: shift this case's seed (SEED_SHIFT)".format(p["ms_at_threshold"])
    if i.regime == "confident":
        assert p["entropy"] <= 0.25, what + "mean entropy {} nats > 0.25".format(p["entropy"])
    if i.regime.startswith("lattice_ties"):
        assert p["tied"] >= 0.10, what + "only {:.1%} tied pixels".format(p["tied"])
        assert p["triple"] >= 1, what + "no pixel with three or more maxima"
    if i.regime == "border_absent":
        (i0, p0), (i1, p1) = absent_parts(i)
        assert not p["owned"][i0, p0] and not p["owned"][i1, p1], what + "the parts forced absent own pixels"
        assert p["absent"][0] >= 1 and p["absent"][1] >= 1, what + "absent parts per view {}".format(p["absent"])
    if "hard_f32_equal" in p:
        assert p["hard_f32_equal"], what + "soft-max in float32 and float64 give different multi-hot maps"
        assert p["stable_share"] >= 0.95, what + "only {:.1%} of the natural centres are stable".format(p["stable_share"])
        if i.regime == "confident":
            assert p["m_zero"] > 0.0 and p["g_zero"] > 0.0, what + "no float32 probability / squared gradient is exactly 0: not saturated"
        if i.regime == "border_absent":
            assert p["clipped_share"] >= 0.20, what + "only {:.1%} of the natural centres within {} of a border".format(p["clipped_share"], HALF)
            for v in (0, 1):
                planted = plant(p["centres"][v * i.B:(v + 1) * i.B], i.S).view(-1, 2)[:4].tolist()
                assert [tuple(c) for c in planted] == CORNERS(i.S), what + "planted corners {}".format(planted)


# ------------------------------------------------------------------------------------------------ NumPy restatement
def np_forward(i, inp, px0):
    """The forward terms np_ops restates, from the same float32 inputs: -> dict comparable with reference()'s."""
    B, S, P = i.B, i.S, i.P
    l = inp["l"].double().numpy()
    lm = inp["lm"].double().numpy()
    m0, m1 = np_ops.softmax_lastdim(l[:B]), np_ops.softmax_lastdim(l[B:])
    out = {"mask0_kl": np_ops.categorical_kl(m0) + np_ops.categorical_kl(m1), "gmrf": np_ops.kl_improper_gmrf(lm[:B])}
    sq = lambda t: float(((t.sum(axis=(1, 2)) ** 2).sum(axis=1)).mean())
    if i.variant == 0:
        r, smooth, contour = np_ops.mumford_shah(m0, 1.0, 1.0e-2)
        out.update({"ms": sq(r), "smooth": sq(smooth), "contour": sq(contour), "area": sq(m0)})
        rect = np_ops.draw_rect(px0.reshape(-1, 2).numpy(), PATCH, PATCH, S, S, np.float64, order="yx").reshape(B, P, S, S).transpose(0, 2, 3, 1)
        out["patch"] = float((np_ops.hard_max(m0) * (1 - rect)).sum(axis=(1, 2, 3)).mean())
    else:
        alpha, lam = MS[1]
        r, _, _ = np_ops.mumford_shah(lm[:B], alpha, lam)
        out["msl"] = float(r.sum(axis=(1, 2, 3)).mean())
    return out
