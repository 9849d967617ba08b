"""CPU tests of the fp64 restatements the point-wise GPU tests compare against (tests/pointwise_ref.py): each one against an
independent form -- an element loop, a torch.nn.functional operation, the NumPy oracle, fp64 autograd -- and the inverse pairs
against the identity."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as P


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


@pytest.mark.parametrize("n,h,w,C,ldx", [(2, 3, 2, 3, 16), (1, 1, 1, 5, 20), (2, 2, 5, 8, 40)])
def test_depth_to_space_element_formula_and_pixel_shuffle(n, h, w, C, ldx):
    x = _rand((n, h, w, ldx), 1)
    y = P.depth_to_space(x, C)
    assert y.shape == (n, 2 * h, 2 * w, C)
    for b in range(n):
        for i in range(h):
            for j in range(w):
                for di in range(2):
                    for dj in range(2):
                        for c in range(C):
                            assert y[b, 2 * i + di, 2 * j + dj, c] == x[b, i, j, (2 * di + dj) * C + c]
    # pixel_shuffle reads channel c * 4 + (2 di + dj): reorder the channel axis from [q, c] to [c, q]
    xs = x[..., :4 * C].reshape(n, h, w, 4, C).transpose(3, 4).reshape(n, h, w, 4 * C)
    assert torch.equal(y, _nhwc(F.pixel_shuffle(_nchw(xs), 2)))
    # inverse pair, and the backward is the inverse gather
    assert torch.equal(P.space_to_depth(y, C), x[..., :4 * C])
    g = _rand(y.shape, 2)
    gx = P.vjp(lambda t: P.depth_to_space(t, C), x, g)
    assert torch.equal(gx[..., :4 * C], P.space_to_depth(g, C)) and float(gx[..., 4 * C:].abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(2, 3, 5, 4), (1, 1, 1, 8), (2, 1, 4, 3)])
def test_nearest2x_and_sum_of_four(shape):
    x = _rand(shape, 3)
    y = P.nearest2x(x)
    assert torch.equal(y, _nhwc(F.interpolate(_nchw(x), scale_factor=2, mode="nearest")))
    g = _rand(y.shape, 4)
    assert torch.allclose(P.sum_of_four(g), P.vjp(P.nearest2x, x, g), rtol=1e-14, atol=1e-14)     # (four terms, another order)
    assert torch.equal(P.sum_of_four(y), 4 * x)


@pytest.mark.parametrize("h,w,ho,wo", [(6, 5, 3, 2), (4, 7, 4, 7), (5, 5, 1, 1)])
def test_crop_clamps_its_corner_and_inverts(h, w, ho, wo):
    x = _rand((2, h, w, 3), 5)
    for y0, x0 in [(0, 0), (h - ho, w - wo), (1, 1), (-3, 2), (2, -1), (h, w), (10 ** 6, -10 ** 6)]:
        oy, ox = P.clamp_corner(h, w, ho, wo, y0, x0)
        assert 0 <= oy <= h - ho and 0 <= ox <= w - wo
        y = P.crop(x, y0, x0, ho, wo)
        assert y.shape == (2, ho, wo, 3)
        for i in range(ho):
            for j in range(wo):
                assert torch.equal(y[:, i, j], x[:, oy + i, ox + j])
        g = _rand(y.shape, 6)
        gx = P.crop_inverse(g, h, w, y0, x0)
        assert torch.equal(gx, P.vjp(lambda t: P.crop(t, y0, x0, ho, wo), x, g))
        assert torch.equal(P.crop(gx, y0, x0, ho, wo), g)
        assert int((gx != 0).sum()) == int((g != 0).sum())            # nothing outside the window


def test_bilinear_matches_the_numpy_oracle_at_degenerate_extents():
    from oracle import np_ops
    for shape in [(2, 6, 5, 3), (1, 1, 1, 2), (2, 1, 4, 2), (1, 5, 1, 3)]:
        x = _rand(shape, 7)
        assert np.allclose(P.bilinear_up2(x).numpy(), np_ops.bilinear_up2(x.numpy()), rtol=0, atol=1e-14)


def _tie_inputs():
    gen = torch.Generator().manual_seed(8)
    relu = torch.relu(torch.randn((2, 8, 6, 8), generator=gen) - 1.5).to(torch.bfloat16).double()      # sparse, as a ReLU'd feature map
    quant = torch.randint(-1, 2, (2, 4, 6, 8), generator=gen).double() * 0.25
    equal = torch.full((1, 4, 4, 8), 1.5, dtype=torch.float64)
    small = (torch.randn((2, 6, 4, 8), generator=gen) * 0.004 + 1.0).to(torch.bfloat16).double()
    return {"relu": relu, "quantised": quant, "all_equal": equal, "bf16_small": small}


def test_maxpool_tie_rule_against_torch():
    """torch's CPU max_pool2d backward gives the gradient to the first maximum in row-major window order on this build (its scan
    replaces the running maximum only on `>`), the rule the kernel documents; so the comparison with F.max_pool2d + autograd runs on
    the tied inputs themselves.  The rule itself is also pinned without torch, by a loop over windows."""
    inputs = _tie_inputs()
    counts = {k: (P.tied_windows(v), v.numel() // 4) for k, v in inputs.items()}
    assert counts["relu"][0] > counts["relu"][1] // 2, counts            # a majority of the ReLU'd windows tie
    assert counts["all_equal"][0] == counts["all_equal"][1]
    assert counts["quantised"][0] > counts["quantised"][1] // 4 and counts["bf16_small"][0] > counts["bf16_small"][1] // 4, counts
    for name, x in inputs.items():
        g = _rand((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3]), 9)
        xo = x.clone().requires_grad_(True)
        yo = _nhwc(F.max_pool2d(_nchw(xo), 2, 2))
        assert torch.equal(P.maxpool2(x), yo.detach()), name
        yo.backward(g)
        got = P.maxpool2_grad(x, g)
        assert torch.equal(got, xo.grad), name
        # the rule, element by element
        n, h, w, c = x.shape
        want = torch.zeros_like(x)
        for b in range(n):
            for i in range(h // 2):
                for j in range(w // 2):
                    for ch in range(c):
                        win = [(0, 0), (0, 1), (1, 0), (1, 1)]
                        vals = [float(x[b, 2 * i + di, 2 * j + dj, ch]) for di, dj in win]
                        di, dj = win[vals.index(max(vals))]
                        want[b, 2 * i + di, 2 * j + dj, ch] = g[b, i, j, ch]
        assert torch.equal(got, want), name
        nz = P._windows(got != 0).sum(dim=-1)
        assert int(nz.max()) <= 1 and torch.equal(P._windows(got).sum(dim=-1), g)


def test_maxpool_signed_zeros_and_negative_windows():
    x = torch.tensor([[-0.0, 0.0], [0.0, -0.0]], dtype=torch.float64).reshape(1, 2, 2, 1)
    g = torch.tensor(3.0, dtype=torch.float64).reshape(1, 1, 1, 1)
    assert P.maxpool2_grad(x, g).flatten().tolist() == [3.0, 0.0, 0.0, 0.0]       # -0.0 == +0.0: the first one wins
    x = torch.tensor([[-4.0, -2.0], [-2.0, -3.0]], dtype=torch.float64).reshape(1, 2, 2, 1)
    assert float(P.maxpool2(x)) == -2.0
    assert P.maxpool2_grad(x, g).flatten().tolist() == [0.0, 3.0, 0.0, 0.0]


@pytest.mark.parametrize("kind", [P.ACT_NONE, P.ACT_LRELU, P.ACT_RELU, P.ACT_ELU])
def test_activations_and_their_derivatives(kind):
    x = _rand((3, 4, 5, 6), 10)
    ref = {P.ACT_NONE: lambda t: t, P.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2), P.ACT_RELU: torch.relu, P.ACT_ELU: F.elu}[kind]
    assert torch.allclose(P.act(x, kind), ref(x), rtol=1e-15, atol=0)
    g = _rand(x.shape, 11)
    assert torch.allclose(g * P.dact(x, kind), P.vjp(ref, x, g), rtol=1e-14, atol=0)
    assert torch.allclose(P.act_mean(x, kind), ref(x).mean(dim=(1, 2), keepdim=True), rtol=1e-14, atol=0)


def test_elu_is_expm1_below_zero():
    x = torch.tensor([-1e-9, -1.0, -30.0, 0.0, 2.0], dtype=torch.float64)
    assert torch.equal(P.elu(x), torch.tensor([np.expm1(-1e-9), np.expm1(-1.0), np.expm1(-30.0), 0.0, 2.0], dtype=torch.float64))
    assert torch.equal(P.elu_grad(x), torch.tensor([np.exp(-1e-9), np.exp(-1.0), np.exp(-30.0), 1.0, 1.0], dtype=torch.float64))


@pytest.mark.parametrize("kind", [P.ACT_NONE, P.ACT_RELU])
@pytest.mark.parametrize("c,ld", [(6, 8), (8, 8), (13, 16)])
def test_l1_gradient_matches_autograd(c, ld, kind):
    a, b = _rand((3, 5, 5, ld), 12), _rand((3, 5, 5, ld), 13)
    want = P.vjp(lambda t: 3.0 * P.l1_mean(a, t, c, kind), b, torch.tensor(1.0))
    got = P.l1_mean_grad(a, b, c, kind, scale=3.0)
    assert torch.allclose(got, want, rtol=1e-14, atol=0) and float(got[..., c:].abs().sum()) == 0.0
    assert abs(float(P.l1_mean(a, b, c, kind)) - float((P.act(a, kind) - P.act(b, kind))[..., :c].abs().sum() / (75 * c))) < 1e-15


def test_vgg_preprocess_and_pad_convert():
    x = torch.rand((2, 3, 4, 5), generator=torch.Generator().manual_seed(14), dtype=torch.float64) * 2 - 1
    y = P.vgg_preprocess(x)
    assert y.shape == (2, 3, 4, 8) and float(y[..., 3:].abs().sum()) == 0.0
    for k, (src, mean) in enumerate(zip((2, 1, 0), P.VGG_BGR_MEAN)):
        assert torch.allclose(y[..., k], x[..., src] * 127.5 + 127.5 - mean, rtol=1e-15, atol=1e-13)
    g = _rand(y.shape, 15)
    gx = P.vjp(P.vgg_preprocess, x, g)
    assert torch.allclose(gx[..., :3], 127.5 * torch.flip(g[..., :3], dims=[-1]), rtol=1e-15, atol=0) and float(gx[..., 3:].abs().sum()) == 0.0
    s = _rand((7, 3), 16)
    d = P.pad_convert(s, 8)
    assert d.shape == (7, 8) and torch.equal(d[:, :3], s) and float(d[:, 3:].abs().sum()) == 0.0


def test_rounds_once_bound_has_teeth():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    S = ref.abs()
    P.assert_rounds_once(ref.to(torch.bfloat16), ref, S, torch.bfloat16, 0)
    P.assert_rounds_once(ref * (1 + 2.0 ** -8), ref, S, torch.bfloat16, 0)             # one unit round-off: inside
    for bad in (ref * (1 + 2.0 ** -6), ref + torch.tensor([0.0, 0.0, 1e-30]), torch.tensor([1.0, float("nan"), 0.0])):
        with pytest.raises(AssertionError):
            P.assert_rounds_once(bad, ref, S, torch.bfloat16, 0)
    with pytest.raises(AssertionError):                                  # fp32, k = 4: the bound is (2^-23 + 2^-21) |ref| < 2^-20 |ref|
        P.assert_rounds_once(ref * (1 + 2.0 ** -20), ref, S, torch.float32, 4)
    P.assert_rounds_once(ref * (1 + 2.0 ** -22), ref, S, torch.float32, 4)
