"""Edge parity of the trainer-side kernels -- ups_randn, ups_adam / ups_adam_dev, ups_critic_head_fwd / _bwd, ups_latent_fwd / _bwd,
ups_tps_warp, ups_gauss_hm / _hm3 -- against the fp64 / integer restatements of trainer_kernels_ref.py, at the sizes where each
kernel takes another path: tails, unaligned pointers, grid-stride trips, clamped rows, refusals (parity_ledger.md, section 8, has
the branch -> case table).  Every test is one comparison with its reference; the figures are printed before they are asserted."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import trainer_kernels_ref as T
from util import assert_close

pytestmark = pytest.mark.gpu

SENT = -777.0           # sentinel of the guard bands: not a value any of these kernels writes


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _refused(lib, name, *args):
    """The call is refused by the entry point's argument check (which is before any launch), not by the runtime."""
    with pytest.raises(lib.UpsError) as e:
        lib.call(name, *args)
    assert "argument check failed" in str(e.value), str(e.value)


# ----------------------------------------------------------------------------- randn
RANDN_BAR = 2e-5        # absolute; the bar of test_gpu_kernels.test_randn_philox_stream's known-answer check


def _randn_into(lib, n, seed, offset, dev, lead=0):
    """ups_randn into elements [lead, lead + n) of a sentinel-filled buffer (the buffer itself is 16-byte aligned)."""
    buf = torch.full((lead + n + 8,), SENT, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    lib.call("ups_randn", lib.ptr(buf[lead:lead + n]), n, seed, offset, lib.stream())
    return buf


@pytest.mark.parametrize("seed,offset,n", [
    (0x0123456789abcdef, 0, 4099), ((1 << 64) - 1, 7, 1024), (1234, (1 << 32) - 2, 16), (1234, (1 << 40) + 5, 64),
    (99, 0, 1), (99, 0, 2), (99, 0, 3), (99, 0, 5), (99, 0, 1023)])
def test_randn_values(seed, offset, n, dev):
    """Both key words, the carry of offset + group into the second counter word, the scalar tail store (n % 4 != 0): every value
    against randn_ref, the 8 values behind the n-th untouched."""
    lib, ops = _mods()
    buf = _randn_into(lib, n, seed, offset, dev).cpu()
    err = float(np.abs(buf[:n].double().numpy() - T.randn_ref(n, seed, offset)).max())
    print("randn seed {:#x} offset {} n {}: max |z - ref| {:.3e}".format(seed, offset, n, err))
    assert err <= RANDN_BAR
    assert bool((buf[n:] == SENT).all()), buf[n:].tolist()


def test_randn_store_path(dev):
    """Views at elements 1, 2, 3 of a 16-byte aligned buffer take the scalar stores for every group: the same bits as the float4
    path, and nothing written on either side."""
    lib, ops = _mods()
    n, seed, offset = 1027, 0x0123456789abcdef, 3
    want = _randn_into(lib, n, seed, offset, dev)[:n].clone()
    assert float(np.abs(want.cpu().double().numpy() - T.randn_ref(n, seed, offset)).max()) <= RANDN_BAR
    for lead in (1, 2, 3):
        buf = _randn_into(lib, n, seed, offset, dev, lead=lead)
        assert torch.equal(buf[lead:lead + n], want), lead
        assert bool((buf[:lead] == SENT).all()) and bool((buf[lead + n:] == SENT).all()), lead


def test_randn_stream_contract_with_ragged_draws(dev):
    """A draw of n values advances the stream by ceil(n / 4) groups: 5, then 1023, then 4096 values."""
    lib, ops = _mods()
    seed = 0x0123456789abcdef
    ns = ops.NoiseStream(seed)
    start = 0
    for n, after in ((5, 2), (1023, 258), (4096, 1282)):
        z = ns.randn(n, device=dev)
        assert ns.offset == after
        err = float(np.abs(z.cpu().double().numpy() - T.randn_ref(n, seed, start)).max())
        print("stream chunk n {} at offset {}: max |z - ref| {:.3e}".format(n, start, err))
        assert err <= RANDN_BAR
        start = after


def test_randn_grid_stride_loop(dev):
    """More groups than 65536 blocks x 256 threads: the second trip of the grid-stride loop.  One call == three calls, each below
    the cap, at the matching offsets (the counter's carry into its second word falls inside the range)."""
    lib, ops = _mods()
    cap = 65536 * 256 * 4
    n = cap + 4003
    seed, offset = (1 << 64) - 12345, (1 << 32) - (1 << 23) - 3
    whole = torch.empty(n, dtype=torch.float32, device=dev)
    parts = torch.empty(n, dtype=torch.float32, device=dev)
    lib.call("ups_randn", lib.ptr(whole), n, seed, offset, lib.stream())
    at = 0
    for m in (1 << 25, 1 << 25, 4003):
        assert m < cap and at % 4 == 0
        lib.call("ups_randn", lib.ptr(parts[at:at + m]), m, seed, offset + at // 4, lib.stream())
        at += m
    assert at == n
    same = torch.equal(whole, parts)
    head = float(np.abs(whole[:8].cpu().double().numpy() - T.randn_ref(8, seed, offset)).max())
    tail = float(np.abs(whole[n - 3:].cpu().double().numpy() - T.randn_ref(4, seed, offset + (n - 3) // 4)[:3]).max())
    del whole, parts
    torch.cuda.empty_cache()
    assert same and head <= RANDN_BAR and tail <= RANDN_BAR, (same, head, tail)


# ----------------------------------------------------------------------------- Adam
ADAM_CAP = 8192 * 256
LR, EPS, STEP_T = 2e-4, 1e-8, 3


def _adam_inputs(count, seed, aligned):
    """p, g ~ N(0, 1), m ~ 0.1 |N(0, 1)|, v ~ 0.1 U(0, 1).  aligned: m has the sign of g (an average of past gradients that agrees
    with this one): beta1 m + (1 - beta1) g then has no cancellation and the step is good to a few fp32 roundings."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(count, generator=g)
    gr = torch.randn(count, generator=g)
    m = torch.randn(count, generator=g) * 0.1
    v = torch.rand(count, generator=g) * 0.1
    if aligned:
        gr = torch.where(gr == 0, torch.ones_like(gr), gr)          # (six million draws do hold an exact zero: the step would be 0 / 0 in `rel`)
        m = m.abs() * torch.sign(gr)
    return p, gr, m, v


def _adam_run(ops, dev, p, gr, m, v, lr_t, b1, b2, gscale):
    pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
    ops.adam_step(pd, gr.to(dev), md, vd, lr_t, b1, b2, EPS, gscale)
    return pd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()


@pytest.mark.parametrize("b1,b2", [(0.5, 0.9), (0.9, 0.999)])
@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("count", [1, 255, 257, ADAM_CAP + 257, 3 * ADAM_CAP + 1])
def test_adam_against_fp64(count, gscale, b1, b2, dev):
    """Element-wise over the whole array (above 8192 x 256 elements the grid-stride loop runs: an element skipped keeps its old
    m, v, p, one visited twice moves all three again).

    m, v: rtol 1e-5 / atol 1e-7, the bars of test_adam_and_gauss.
    The update as an update: p = 0, so p_new = -step, held to rtol 1e-5 with no absolute term (on inputs whose m agrees in sign with
    g: where beta1 m + (1 - beta1) g cancels, m's own absolute bar is all that can be asked of the step).
    Random p and m: |p_new - p_ref| <= one fp32 ulp of the larger of |p|, |p_ref| (the rounding of the subtraction; an element
    with |p| below the step ends at the step's magnitude, so it is the larger of the two whose ulp counts) + 1e-5 |step| + the
    step's share of m's absolute bar, lr_t 1e-7 / (sqrt(v) + eps)."""
    lib, ops = _mods()
    lr_t = float(np.float32(T.lr_t_of(LR, b1, b2, STEP_T)))        # the number the kernel gets
    # (1) the update alone
    p, gr, m, v = _adam_inputs(count, 100 + count % 1000, aligned=True)
    p.zero_()
    want = T.adam_ref(p.numpy(), gr.numpy(), m.numpy(), v.numpy(), lr_t, b1, b2, EPS, gscale)
    got = _adam_run(ops, dev, p, gr, m, v, lr_t, b1, b2, gscale)
    rel = float(np.max(np.abs(got[0] - want[0]) / np.abs(want[0])))
    print("adam count {} scale {} betas ({}, {}): step max rel err {:.3e}".format(count, gscale, b1, b2, rel))
    assert np.all(np.abs(want[0]) > 0) and rel <= 1e-5
    assert np.allclose(got[1], want[1], rtol=1e-5, atol=1e-7) and np.allclose(got[2], want[2], rtol=1e-5, atol=1e-7)
    # (2) the usual random state
    p, gr, m, v = _adam_inputs(count, 200 + count % 1000, aligned=False)
    want = T.adam_ref(p.numpy(), gr.numpy(), m.numpy(), v.numpy(), lr_t, b1, b2, EPS, gscale)
    got = _adam_run(ops, dev, p, gr, m, v, lr_t, b1, b2, gscale)
    assert np.allclose(got[1], want[1], rtol=1e-5, atol=1e-7), "m"
    assert np.allclose(got[2], want[2], rtol=1e-5, atol=1e-7), "v"
    p64 = p.double().numpy()
    ulp = np.spacing(np.maximum(np.abs(p.numpy()), np.abs(want[0]).astype(np.float32))).astype(np.float64)
    bound = ulp + 1e-5 * np.abs(want[0] - p64) + lr_t * 1e-7 / (np.sqrt(want[2]) + EPS)
    excess = float(np.max(np.abs(got[0] - want[0]) / bound))
    moved = float(np.mean(got[0] != p.numpy()))
    print("  random p: max |p_new - p_ref| / bound {:.3f}; share of elements moved {:.4f}".format(excess, moved))
    assert excess <= 1.0


@pytest.mark.parametrize("s", [0.25, 4.0])
def test_adam_grad_scale_is_a_product_with_g(s, dev):
    """grad_scale = s on g == grad_scale = 1 on g * s, bit for bit, for s a power of two (g * s is exact)."""
    lib, ops = _mods()
    p, gr, m, v = _adam_inputs(ADAM_CAP + 1000, 7, aligned=False)
    lr_t = T.lr_t_of(LR, 0.5, 0.9, STEP_T)
    a = _adam_run(ops, dev, p, gr, m, v, lr_t, 0.5, 0.9, s)
    b = _adam_run(ops, dev, p, gr * s, m, v, lr_t, 0.5, 0.9, 1.0)
    for x, y, name in zip(a, b, "pmv"):
        assert np.array_equal(x, y), name
    assert not np.array_equal(a[1], _adam_run(ops, dev, p, gr, m, v, lr_t, 0.5, 0.9, 1.0)[1])


def test_adam_dev_reads_the_device_scalar_at_run_time(dev):
    """ups_adam_dev == ups_adam at the same lr_t; after the scalar is changed in place the next call uses the new value."""
    lib, ops = _mods()
    p, gr, m, v = _adam_inputs(ADAM_CAP + 257, 8, aligned=False)
    lr_dev = torch.tensor([T.lr_t_of(LR, 0.5, 0.9, 3)], dtype=torch.float32, device=dev)
    pd, md, vd, gd = p.to(dev), m.to(dev), v.to(dev), gr.to(dev)
    ph, mh, vh = p.to(dev), m.to(dev), v.to(dev)
    for t in (3, 4):
        lr_t = T.lr_t_of(LR, 0.5, 0.9, t)
        lr_dev.fill_(lr_t)
        ops.adam_step(pd, gd, md, vd, lr_dev, 0.5, 0.9, EPS, 0.5)
        ops.adam_step(ph, gd, mh, vh, lr_t, 0.5, 0.9, EPS, 0.5)
        assert torch.equal(pd, ph) and torch.equal(md, mh) and torch.equal(vd, vh), t
    one = p.to(dev), m.to(dev), v.to(dev)                  # (and the second step did not reuse the first step's rate)
    ops.adam_step(one[0], gd, one[1], one[2], T.lr_t_of(LR, 0.5, 0.9, 3), 0.5, 0.9, EPS, 0.5)
    ops.adam_step(one[0], gd, one[1], one[2], T.lr_t_of(LR, 0.5, 0.9, 3), 0.5, 0.9, EPS, 0.5)
    assert not torch.equal(one[0], pd)


def test_adam_degenerate_elements_and_empty_key(dev):
    """g = m = v = 0: the step is 0 / (0 + eps) = 0, p stays as it is.  count = 0 returns without a launch."""
    lib, ops = _mods()
    p0 = torch.randn(300, generator=torch.Generator().manual_seed(9))
    p, g, m, v = p0.to(dev), torch.zeros(300, device=dev), torch.zeros(300, device=dev), torch.zeros(300, device=dev)
    ops.adam_step(p, g, m, v, T.lr_t_of(LR, 0.5, 0.9, 1), 0.5, 0.9, EPS, 1.0)
    assert torch.equal(p.cpu(), p0) and bool(torch.isfinite(p).all())
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    g.fill_(1.0)
    lr_dev = torch.tensor([1.0], device=dev)
    lib.call("ups_adam", lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), 0, 1.0, 0.5, 0.9, EPS, 1.0, lib.stream())
    lib.call("ups_adam_dev", lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), 0, lib.ptr(lr_dev), 0.5, 0.9, EPS, 1.0, lib.stream())
    assert torch.equal(p.cpu(), p0) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


# ----------------------------------------------------------------------------- critic head
BF, F32 = torch.bfloat16, torch.float32
HEAD_ROWS = [(BF, B, 512, 512, 0) for B in (1, 3, 40, 100, 4096)] + [(F32, B, 512, 512, 0) for B in (1, 100)]
HEAD_WIDTHS = [(BF, 40, K, ld, 0) for K, ld in ((8, 8), (504, 512), (500, 504), (520, 520), (1024, 1024))] + [(F32, 40, 500, 504, 0), (BF, 40, 512, 512, 4)]


def _head_id(c):
    return "{}-B{}-K{}-ld{}{}".format("bf16" if c[0] == BF else "fp32", c[1], c[2], c[3], "-lead{}".format(c[4]) if c[4] else "")


def _head_compare(dev, dtype, B, K, ld, lead, hp, ha, rows=True):
    lib, ops = _mods()
    r = T.critic_head_ref(hp, ha, B, K)
    hpd = T.device_view(hp, dev, lead).requires_grad_(True)
    had = T.device_view(ha, dev, lead).requires_grad_(True)
    if lead:
        assert hpd.data_ptr() % 16 == 8 and had.data_ptr() % 16 == 8 and hpd.is_contiguous()
    # the entry point itself, for `logits`: a guard band behind row 2B - 1 (a clamped row past the end is read and dropped)
    logits = torch.full((2 * B + 64,), SENT, dtype=torch.float32, device=dev)
    out4 = torch.full((4,), SENT, dtype=torch.float32, device=dev)
    with torch.no_grad():
        lib.call("ups_critic_head_fwd", lib.ptr(hpd), lib.ptr(had), lib.dt(hpd), B, K, ld, lib.ptr(logits), lib.ptr(out4), lib.stream())
    logits = logits.cpu()
    assert bool((logits[2 * B:] == SENT).all()), "written behind row 2B - 1"
    if rows:
        e = (logits[:2 * B].double() - r.logits).abs() / r.logits.abs().clamp(min=1.0)
        print("head {}: logits max err {:.3e} (row {})".format(_head_id((dtype, B, K, ld, lead)), float(e.max()), int(e.argmax())))
        assert float(e.max()) <= 1e-5
    loss, acc, mim = ops.CriticHeadFn.apply(hpd, had, B, K)
    assert torch.equal(torch.stack([loss, acc, mim]).detach().cpu(), out4[:3].cpu())
    lossv, accv, mimv = (float(t.detach()) for t in (loss, acc, mim))
    print("  loss {} / {}  acc {} / {}  mim {} / {}".format(lossv, r.loss, accv, r.acc, mimv, r.mim))
    assert math.isfinite(lossv) and abs(lossv - r.loss) <= 1e-5 * max(1.0, abs(r.loss))
    assert abs(mimv - r.mim) <= 1e-5 * max(1.0, abs(r.mim))
    assert abs(accv - r.acc) <= 1e-6 and round(accv * 2 * B) == round(r.acc * 2 * B)
    gtol = 1e-5 if dtype == F32 else 1e-2
    for wl, wm in T.HEAD_WEIGHTINGS:
        go = r.grads(wl, wm)
        gh = torch.autograd.grad(wl * loss + wm * mim, [hpd, had], retain_graph=True)
        for got, want, name in zip(gh, go, ("h_pi", "h_alpha")):
            got = got.float().cpu()
            assert bool(torch.isfinite(got).all())
            assert_close(got[:, :K], want[:, :K].float(), gtol, "d / d {} ({}, {})".format(name, wl, wm))
            if ld > K:
                assert float(got[:, K:].abs().max()) == 0.0, "gradient in the padding channels of " + name


@pytest.mark.parametrize("case", HEAD_ROWS + HEAD_WIDTHS, ids=_head_id)
def test_critic_head_rows_and_widths(case, dev):
    """Row counts that leave a wave's four rows in flight partly past the end (2B not a multiple of 64: the clamped-row branch and
    its store guard), one row per class, the B <= 4096 bound; K < ld with junk in the padding channels, K not a multiple of 8
    (the scalar form in bf16), K > 512 (a second trip over a row's 16-byte pieces), a base pointer 8 bytes off a 16-byte
    boundary.  `logits` row by row, the three scalars and the gradients of the three weightings."""
    dtype, B, K, ld, lead = case
    hp, ha = T.head_inputs(dtype, B, K, ld, seed=300 + B + K + ld)
    _head_compare(dev, dtype, B, K, ld, lead, hp, ha)


def test_critic_head_saturated(dev):
    """Logits beyond +-150 on both sides and four rows exactly zero: softplus_f and sigmoid_f at their ends (exp overflows to inf on
    one side, underflows on the other).  Loss and gradients finite and inside the usual bars, the accuracy exact with a zero logit
    wrong on both sides.  (`logits` themselves are not compared here: a sum of 512 products of size 4 is not good to 1e-5 of a
    logit near 1; test_host_trainer_kernels shows the span and that no other logit is within 1e-2 of zero.)"""
    c = T.SATURATED
    hp, ha = T.head_inputs(c["dtype"], c["B"], c["K"], c["ld"], c["seed"], c["scale"], c["zero_rows"])
    _head_compare(dev, c["dtype"], c["B"], c["K"], c["ld"], 0, hp, ha, rows=False)


def test_critic_head_refusals(dev):
    lib, ops = _mods()
    h = torch.zeros(64, dtype=BF, device=dev)
    f = torch.zeros(64, dtype=F32, device=dev)
    _refused(lib, "ups_critic_head_fwd", lib.ptr(h), lib.ptr(h), lib.BF16, 4097, 512, 512, lib.ptr(f), lib.ptr(f), lib.stream())
    _refused(lib, "ups_critic_head_fwd", lib.ptr(h), lib.ptr(h), lib.BF16, 2, 16, 8, lib.ptr(f), lib.ptr(f), lib.stream())
    _refused(lib, "ups_critic_head_bwd", lib.ptr(h), lib.ptr(h), lib.ptr(f), lib.ptr(f), None, lib.BF16, 2, 16, 8, lib.ptr(h), None, lib.stream())
    _refused(lib, "ups_critic_head_fwd", lib.ptr(h), lib.ptr(h), lib.BF16, 0, 8, 8, lib.ptr(f), lib.ptr(f), lib.stream())
    assert float(f.abs().max()) == 0.0


# ----------------------------------------------------------------------------- latent
LATENT_CASES = [(1, 2, 1), (2, 3, 12), (65, 2, 9), (130, 1, 7), (300, 2, 2), (16, 64, 7)]         # Z, B, S
W_KL = 1.7


@pytest.mark.parametrize("Z,B,S", LATENT_CASES)
def test_latent_against_fp64(Z, B, S, dev):
    """Z = 1, a row's second and third lane trip (65, 130), Z > 256, S = MAXS = 12 and the model's S = 9, a batch of 64; noise
    levels that are not all 1.  Samples at 2e-5, the gradient at 5e-5 (the bars of test_latent), the rows of the KL at 2e-5 and
    their mean at test_latent's 1e-4.  want_kl=False (a NULL kl_rows) gives the same samples bit for bit; the trainer's view-1
    backward (no device scalar, scale 0) is the gradient of the sample term alone; no device scalar and scale c is the device
    scalar 1 with scale c."""
    lib, ops = _mods()
    params, eps, gs = T.latent_inputs(Z, B, S, seed=500 + Z)
    levels = T.LEVELS[:S]
    so, klo, gpo = T.latent_ref(params, eps, levels, gs, W_KL)
    pd, ed, gd = params.to(dev), eps.to(dev), gs.to(dev)
    samples, kl_rows = ops.latent_fwd(pd, ed, levels, True)
    assert_close(samples.cpu(), so.float(), 2e-5, "latent samples")
    assert_close(kl_rows.cpu(), klo.float(), 2e-5, "latent kl rows")
    kl = float(klo.sum(1).mean())
    assert abs(float(kl_rows.sum(1).mean()) - kl) < 1e-4 * max(1.0, abs(kl))
    only, none = ops.latent_fwd(pd, ed, levels, False)
    assert none is None and torch.equal(only, samples)
    scale = torch.tensor([W_KL], device=dev)
    gp = ops.latent_bwd(pd, ed, levels, gd, scale, 1.0 / B)
    assert_close(gp.cpu(), gpo.float(), 5e-5, "latent bwd")
    _, _, g0 = T.latent_ref(params, eps, levels, gs, 0.0)
    gp0 = ops.latent_bwd(pd, ed, levels, gd, None, 0.0)
    assert_close(gp0.cpu(), g0.float(), 5e-5, "latent bwd, sample term alone")
    one = torch.tensor([1.0], device=dev)
    assert torch.equal(ops.latent_bwd(pd, ed, levels, gd, None, 0.37), ops.latent_bwd(pd, ed, levels, gd, one, 0.37))


def test_latent_refusals(dev):
    """S = 13 > MAXS, and an empty batch or width in the backward (its forward always refused those), before any launch."""
    lib, ops = _mods()
    params, eps, gs = (t.to(dev) for t in T.latent_inputs(4, 2, 13, seed=1))
    with pytest.raises(lib.UpsError, match="argument check failed"):
        ops.latent_fwd(params, eps, [1.0] * 13, True)
    with pytest.raises(lib.UpsError, match="argument check failed"):
        ops.latent_bwd(params, eps, [1.0] * 13, gs, None, 0.0)
    lv = (C.c_float * 2)(1.0, 1.0)
    gp = torch.full_like(params, SENT)
    for B, Z in ((0, 4), (2, 0), (-1, 4)):
        _refused(lib, "ups_latent_bwd", lib.ptr(params), lib.ptr(eps), lv, lib.ptr(gs), None, 0.0, 2, B, Z, lib.ptr(gp), lib.stream())
        _refused(lib, "ups_latent_fwd", lib.ptr(params), lib.ptr(eps), lv, 2, B, Z, lib.ptr(gp), None, lib.stream())
    assert bool((gp == SENT).all())


# ----------------------------------------------------------------------------- thin-plate-spline warp
def _tps_launch(lib, img, Tm, coord, dev):
    n, h, w, c = img.shape
    out = torch.full((img.numel() + 8,), SENT, dtype=torch.float32, device=dev)
    imgd, Td, cd = img.to(dev), Tm.to(dev), coord.to(dev)          # (named: the three stay alive, and apart, until the kernel has run)
    lib.call("ups_tps_warp", lib.ptr(imgd), lib.ptr(Td), lib.ptr(cd), lib.ptr(out), n, h, w, c, coord.shape[1], lib.stream())
    out = out.cpu()
    assert bool((out[img.numel():] == SENT).all())
    return out[:img.numel()].view(n, h, w, c)


@pytest.mark.parametrize("kind", T.TPS_KINDS)
@pytest.mark.parametrize("shape", T.TPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tps_warp_against_fp64(shape, kind, dev):
    """h != w (an h / w mix-up in the index arithmetic), K = 1 and K = TPS_MAXK = 32, c = 1 and 8, h w not a multiple of 256, one
    row and one column; affine maps whose source positions leave the image across all four borders, and splines.

    The bilinear form jumps where a source coordinate crosses 0 or size - 1 (the clamped-corner weights collapse), and fp32 and
    fp64 may floor on different sides: output pixels whose fp64 px or py is within 1e-3 of those lines are left out, at most 2 %
    of a case (asserted here and, for the reference alone, in test_host_trainer_kernels).  The rest is held to test_tps_warp's
    2e-4 through assert_close.

    A one-row or one-column image is the exception in the metric, not in the bar: both clamped corners of the pinned axis are pixel
    0, their weights are (0 - p) and (p - 0), and the form is identically zero -- in fp64 to 1e-12 of the image (host test), in the
    kernel to the rounding of products that cancel.  assert_close measures against max |ref|, which is that rounding noise, so
    there the same 2e-4 is taken of the image's own maximum, the scale the warped image of any other shape has."""
    lib, ops = _mods()
    n, h, w, c, K = shape
    img, Tm, coord = T.tps_case(shape, kind)
    want, px, py = T.tps_warp_ref(img, Tm, coord)
    keep = T.tps_edge_mask(px, py, h, w)
    masked = 1.0 - float(keep.double().mean())
    assert masked <= T.TPS_MASK_CAP
    if kind == "affine":
        counts = T.tps_border_counts(px, py, h, w)
        assert all(v > 0 for v in counts.values()), counts
    got = _tps_launch(lib, img, Tm, coord, dev)
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - want)[keep].abs().max())
    print("tps {} {}: masked {:.4f}, max |got - ref| {:.3e}, max |ref| {:.3e}, max |got| {:.3e}".format(
        shape, kind, masked, err, float(want.abs().max()), float(got.abs().max())))
    if h == 1 or w == 1:
        assert err <= 2e-4 * float(img.abs().max())
    else:
        assert_close(got[keep], want[keep].float(), 2e-4, "tps {} {}".format(shape, kind))


def test_tps_warp_refusals(dev):
    lib, ops = _mods()
    img = torch.zeros(1, 4, 4, 3, device=dev)
    out = torch.full_like(img, SENT)
    Tm, coord = torch.zeros(1, 2, 36, device=dev), torch.zeros(1, 33, 2, device=dev)
    for K in (33, 0):
        _refused(lib, "ups_tps_warp", lib.ptr(img), lib.ptr(Tm), lib.ptr(coord), lib.ptr(out), 1, 4, 4, 3, K, lib.stream())
    assert bool((out == SENT).all())


# ----------------------------------------------------------------------------- heat maps
def _hm_inputs(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    return g, torch.rand(B, K, 2, generator=g), torch.rand(B, K, 2, generator=g)


def test_gauss_hm(dev):
    lib, ops = _mods()
    from oracle import np_ops
    B, h, w, K = 2, 9, 31, 5
    g, a, b = _hm_inputs(B, K, 21)
    pts, sd = a * torch.tensor([w, h]), b * 2 + 1
    hm = ops.gauss_hm(pts.to(dev), sd.to(dev), h, w)
    assert np.allclose(hm.cpu().numpy(), np_ops.tf_hm(pts.numpy(), h, w, sd.numpy()), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("B,h,w,K", [(2, 9, 31, 5), (1, 1, 7, 2), (1, 7, 1, 2)])
def test_gauss_hm3(B, h, w, K, dev):
    """h != w, and the one-row / one-column grid (linspace(-1, 1, 1) = [-1])."""
    lib, ops = _mods()
    from oracle import np_ops
    g, a, b = _hm_inputs(B, K, 22 + h)
    mu = a - 0.5
    Lt = torch.zeros(B, K, 2, 2)
    Lt[..., 0, 0] = 0.3 + b[..., 0]
    Lt[..., 1, 1] = 0.3 + b[..., 1]
    Lt[..., 1, 0] = torch.randn(B, K, generator=g) * 0.2
    hm3 = ops.gauss_hm3(mu.to(dev), Lt.to(dev), h, w)
    assert np.allclose(hm3.cpu().numpy(), np_ops.tf_hm3(h, w, mu.numpy(), Lt.numpy()), rtol=1e-4, atol=1e-6)


def test_gauss_hm_refusals(dev):
    lib, ops = _mods()
    a = torch.ones(2, 5, 4, device=dev)
    out = torch.full((64,), SENT, device=dev)
    for name in ("ups_gauss_hm", "ups_gauss_hm3"):
        for dims in ((0, 2, 2, 2), (1, 0, 2, 2), (1, 2, 0, 2), (1, 2, 2, 0)):
            _refused(lib, name, lib.ptr(a), lib.ptr(a), lib.ptr(out), *dims, lib.stream())
    assert bool((out == SENT).all())
