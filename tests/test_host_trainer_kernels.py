"""The restatements of trainer_kernels_ref.py against independent statements of the same operations, and the premises of the cases
the GPU tests launch (test_gpu_trainer_kernels.py), without a GPU.  A failure here is a failure of a reference or of a case, not
of a kernel."""
import math

import numpy as np
import pytest
import torch

import trainer_kernels_ref as T
from oracle import np_ops
from oracle import tps as OT


# ----------------------------------------------------------------------------- Philox / randn
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert tuple(int(w[0]) for w in T.philox4x32_10(ctr, key)) == want


def test_philox_is_elementwise():
    ctrs = [(0, 0, 0, 0), (5, 1, 0, 0), (0xffffffff, 0xffffffff, 0, 0)]
    both = T.philox4x32_10(tuple(np.array([c[i] for c in ctrs], dtype=np.uint64) for i in range(4)), (7, 9))
    for j, c in enumerate(ctrs):
        assert [int(w[j]) for w in both] == [int(w[0]) for w in T.philox4x32_10(c, (7, 9))]


def test_randn_ref_mapping():
    z = T.randn_ref(8, 0, 0)
    words = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]          # counter 0, key 0: the first group by hand
    u = [((x >> 8) + 0.5) / 16777216.0 for x in words]
    exp = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
           math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3]), math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])]
    assert np.abs(z[:4] - np.array(exp)).max() < 1e-14
    # the carry of offset + group into the second counter word: group 2 of offset 2^32 - 2 is counter (0, 1, 0, 0)
    carry = T.randn_ref(16, 1234, (1 << 32) - 2)
    w = T.philox4x32_10((0, 1, 0, 0), (1234, 0))
    assert np.array_equal(carry[8:12], T.randn_ref(4, 1234, 1 << 32)) and not np.array_equal(carry[8:12], T.randn_ref(4, 1234, 0))
    u1 = ((int(w[0][0]) >> 8) + 0.5) / 16777216.0
    u2 = ((int(w[1][0]) >> 8) + 0.5) / 16777216.0
    assert abs(carry[8] - math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2)) < 1e-14
    # the high key word
    seed = 0x0123456789abcdef
    assert not np.array_equal(T.randn_ref(16, seed, 0), T.randn_ref(16, seed & 0xffffffff, 0))
    assert np.array_equal(T.randn_ref(4, seed, 0)[:1], T.randn_ref(1, seed, 0))
    # the stream property
    for n, s, o in ((4099, seed, 0), (64, 1234, (1 << 40) + 5), (21, (1 << 64) - 1, 7)):
        assert np.array_equal(T.randn_ref(n, s, o)[4:], T.randn_ref(n - 4, s, o + 1))
    x = T.randn_ref(1 << 16, 99, 0)
    assert np.isfinite(x).all() and abs(x.mean()) < 0.02 and abs(x.var() - 1.0) < 0.03


# ----------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("b1,b2", [(0.5, 0.9), (0.9, 0.999)])
def test_adam_ref_is_tf_adam(b1, b2):
    r = np.random.RandomState(3)
    p, g, m, v = r.randn(257), r.randn(257), 0.1 * r.randn(257), 0.1 * r.rand(257)
    t, lr = 3, 2e-4
    want = np_ops.tf_adam_step(p, g, m, v, t, lr, b1, b2)
    got = T.adam_ref(p, g, m, v, T.lr_t_of(lr, b1, b2, t), b1, b2, 1e-8, 1.0)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    scaled = T.adam_ref(p, g, m, v, T.lr_t_of(lr, b1, b2, t), b1, b2, 1e-8, 0.25)
    pre = T.adam_ref(p, 0.25 * g, m, v, T.lr_t_of(lr, b1, b2, t), b1, b2, 1e-8, 1.0)
    for a, b in zip(scaled, pre):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- critic head
def test_critic_head_ref_gradients_by_finite_difference():
    """2 rows x 8 channels (B = 1), K = 6: central differences of the reference's own loss and mean joint logit."""
    B, K, ld = 1, 6, 8
    hp, ha = T.head_inputs(torch.float64, B, K, ld, seed=5, scale=0.8)
    r = T.critic_head_ref(hp, ha, B, K)
    assert r.logits.shape == (2,) and abs(float(r.logits[0]) - float((hp[0, :K] * ha[0, :K]).sum())) < 1e-14
    h = 1e-6
    for wl, wm in T.HEAD_WEIGHTINGS:
        ghp, gha = r.grads(wl, wm)
        assert float(ghp[:, K:].abs().max()) == 0.0 and float(gha[:, K:].abs().max()) == 0.0
        f = lambda a, b: (lambda q: wl * q.loss + wm * q.mim)(T.critic_head_ref(a, b, B, K))
        for which, grad in ((0, ghp), (1, gha)):
            for row in range(2):
                for k in range(ld):
                    d = torch.zeros(2, ld, dtype=torch.float64)
                    d[row, k] = h
                    args = ((hp + d, ha), (hp - d, ha)) if which == 0 else ((hp, ha + d), (hp, ha - d))
                    fd = (f(*args[0]) - f(*args[1])) / (2 * h)
                    assert abs(fd - float(grad[row, k])) < 1e-8, (wl, wm, which, row, k, fd, float(grad[row, k]))


def test_critic_head_ref_zero_logit_and_padding():
    """A zero logit is wrong on both sides and has gradient -+0.5 sigmoid(0) / B; the padding channels change nothing."""
    B, K = 2, 8
    hp, ha = T.head_inputs(torch.float64, B, K, K, seed=6, zero_rows=(0, 2))
    r = T.critic_head_ref(hp, ha, B, K)
    assert float(r.logits[0]) == 0.0 and float(r.logits[2]) == 0.0
    want = (int(r.logits[1] > 0) + int(r.logits[3] < 0)) / 4.0
    assert r.acc == want
    ghp, _ = r.grads(1.0, 0.0)
    assert torch.allclose(ghp[0], -0.125 * ha[0], rtol=1e-14, atol=0) and torch.allclose(ghp[2], 0.125 * ha[2], rtol=1e-14, atol=0)
    hq, hb = T.head_inputs(torch.float64, B, K, K + 8, seed=6, zero_rows=(0, 2))
    assert float(hq[:, K:].abs().min()) == T.HEAD_JUNK
    q = T.critic_head_ref(hq, hb, B, K)
    assert torch.equal(q.logits, r.logits) and q.loss == r.loss and q.mim == r.mim


def test_saturated_head_case_spans_the_ends():
    """The saturated case of the GPU test: fp64 logits beyond +-150 on both sides, four rows exactly zero, no other logit so close
    to zero that the accuracy would depend on the order of an fp32 sum."""
    c = T.SATURATED
    hp, ha = T.head_inputs(c["dtype"], c["B"], c["K"], c["ld"], c["seed"], c["scale"], c["zero_rows"])
    r = T.critic_head_ref(hp, ha, c["B"], c["K"])
    assert float(r.logits.min()) <= -150.0 and float(r.logits.max()) >= 150.0
    zero = torch.zeros(2 * c["B"], dtype=torch.bool)
    zero[list(c["zero_rows"])] = True
    assert bool((r.logits[zero] == 0).all()) and float(r.logits[~zero].abs().min()) > 1e-2
    assert math.isfinite(r.loss) and all(bool(torch.isfinite(t).all()) for t in r.grads(0.7, -2.5))


# ----------------------------------------------------------------------------- latent
@pytest.mark.parametrize("Z,B,S", [(1, 2, 1), (5, 3, 12), (65, 2, 2)])
def test_latent_ref_is_the_numpy_restatement(Z, B, S):
    params, eps, gs = T.latent_inputs(Z, B, S, seed=9)
    samples, kl_rows, gp = T.latent_ref(params, eps, T.LEVELS[:S], gs, 1.7)
    mean, L, ld = np_ops.full_latent(params.double().numpy(), Z)
    kl = np_ops.full_latent_kl(mean, L, ld)
    assert abs(float(kl_rows.sum(1).mean()) - kl) <= 1e-12 * max(1.0, abs(kl))
    want = mean[None] + np.einsum("bij,sbj->sbi", L, eps.double().numpy() * np.array(T.LEVELS[:S]).reshape(S, 1, 1))
    assert np.abs(samples.numpy() - want).max() <= 1e-12
    # d / d mean of sum(samples * gs) + w kl: sum_s gs + w mean / B
    want_gm = gs.double().sum(0) + 1.7 * params.double()[:, :Z] / B
    assert float((gp[:, :Z] - want_gm).abs().max()) <= 1e-12
    _, _, g0 = T.latent_ref(params, eps, T.LEVELS[:S], gs, 0.0)
    assert float((g0[:, :Z] - gs.double().sum(0)).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------- thin-plate-spline warp
def test_tps_warp_ref_is_the_oracle_on_solved_parameters():
    g = torch.Generator().manual_seed(2)
    img = torch.rand(2, 12, 20, 3, generator=g, dtype=torch.float64)
    coord = T.tps_control_points(2, 9, g).double()
    vector = (torch.rand(2, 9, 2, generator=g).double() - 0.5) * 0.3
    out, px, py = T.tps_warp_ref(img, OT.solve_system(coord, vector), coord)
    assert torch.equal(out, OT.thin_plate_spline(img, coord, vector))
    assert px.shape == py.shape == (2, 12, 20)


@pytest.mark.parametrize("kind", T.TPS_KINDS)
@pytest.mark.parametrize("shape", T.TPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tps_case_premises(shape, kind):
    """What the GPU comparison rests on, from the reference alone: the masked share stays under the cap, every affine case has
    source positions beyond each of the four borders, the image tells rows, columns and channels apart, and a one-row or
    one-column image warps to zero (the clamped corners coincide and their weights cancel)."""
    n, h, w, c, K = shape
    img, Tm, coord = T.tps_case(shape, kind)
    assert img.shape == (n, h, w, c) and Tm.shape == (n, 2, K + 3) and coord.shape == (n, K, 2)
    assert all(t.dtype == torch.float32 for t in (img, Tm, coord))
    out, px, py = T.tps_warp_ref(img, Tm, coord)
    keep = T.tps_edge_mask(px, py, h, w)
    assert 1.0 - float(keep.double().mean()) <= T.TPS_MASK_CAP
    if kind == "affine":
        counts = T.tps_border_counts(px, py, h, w)
        assert all(v > 0 for v in counts.values()), counts
        assert float(Tm[:, :, 3:].abs().max()) == 0.0
    else:
        assert float(Tm[:, :, 3:].abs().max()) > 0.0
    flat = img.reshape(n, h * w, c)
    if h > 1:
        assert float((img[:, 1:] - img[:, :-1]).abs().amax(dim=(0, 2, 3)).min()) > 1e-3
    if w > 1:
        assert float((img[:, :, 1:] - img[:, :, :-1]).abs().amax(dim=(0, 1, 3)).min()) > 1e-3
    if c > 1:
        assert float((flat[..., 1:] - flat[..., :-1]).abs().amax(dim=(0, 1)).min()) > 1e-3
    if h == 1 or w == 1:
        assert float(out.abs().max()) <= 1e-12 * float(img.abs().max())
    else:
        assert float(out.abs().max()) > 0.5
