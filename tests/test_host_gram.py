"""CPU tests of the Gram-matrix perceptual terms (`gram_weight`): the fp64 restatement the GPU tests compare against (tests/gram_ref.py)
against its direct einsum form, the kernels' single K-concatenated accumulator, fp64 autograd and padded channels; the patched oracle
is unchanged for weights <= 0; the trainer's validation of the key."""
import warnings

import pytest
import torch

import gram_ref as G


def _maps(n, hw, c, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn((n, hw, c), generator=gen, dtype=torch.float64),
            torch.randn((n, hw, c), generator=gen, dtype=torch.float64))


@pytest.mark.parametrize("n,hw,c", [(2, 35, 3), (3, 16, 40), (1, 1, 8)])
def test_restatement_matches_einsum(n, hw, c):
    Ft, Fg = _maps(n, hw, c, n + hw + c)
    gt = torch.einsum("bki,bkj->bij", Ft, Ft) / (4.0 * hw)
    gg = torch.einsum("bki,bkj->bij", Fg, Fg) / (4.0 * hw)
    assert torch.allclose(G.gram(Ft), gt, rtol=1e-13, atol=0)
    w = 0.3
    assert abs(float(G.gram_l1(Ft, Fg, w)) - float(w * (gt - gg).abs().sum() / (n * c * c))) <= 1e-12 * float(w * (gt - gg).abs().mean())


@pytest.mark.parametrize("n,hw,c", [(2, 35, 3), (3, 16, 40)])
def test_concatenated_accumulator_is_the_gram_difference(n, hw, c):
    Ft, Fg = _maps(n, hw, c, 7)
    D = G.concat_d(Ft, Fg) / (G.GRAM_DIV * hw)
    assert torch.allclose(D, G.gram(Fg) - G.gram(Ft), rtol=1e-12, atol=1e-12)
    assert torch.equal(torch.sign(D), torch.sign(D).transpose(1, 2))       # the mirrored sign matrix is the true one


@pytest.mark.parametrize("n,hw,c", [(2, 35, 3), (3, 16, 40), (1, 64, 33)])
def test_closed_form_gradient_matches_autograd(n, hw, c):
    Ft, Fg = _maps(n, hw, c, 11)
    Fg = Fg.clone().requires_grad_(True)
    w = 0.7
    (g,) = torch.autograd.grad([G.gram_l1(Ft, Fg, w)], [Fg])
    assert torch.allclose(G.gram_l1_grad(Ft, Fg.detach(), w), g, rtol=1e-12, atol=1e-15)


def test_padded_channels_change_nothing():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((2, 5, 7, 8), generator=gen, dtype=torch.float64)
    y = torch.randn((2, 5, 7, 8), generator=gen, dtype=torch.float64)
    x2, y2 = x.clone(), y.clone()
    x2[..., 3:] = 1e3 * torch.randn((2, 5, 7, 5), generator=gen, dtype=torch.float64)
    y2[..., 3:] = -7.0
    for relu in (False, True):
        a = G.gram_l1(G.as_F(x, 3, relu), G.as_F(y, 3, relu), 0.5)
        b = G.gram_l1(G.as_F(x2, 3, relu), G.as_F(y2, 3, relu), 0.5)
        assert torch.equal(a, b)


def _perceptual_inputs():
    from oracle import ref_model as R
    gen = torch.Generator().manual_seed(5)
    vp = R.vgg_params(7, widths=(8, 8, 16, 16, 16))
    t = torch.rand((2, 16, 16, 3), generator=gen, dtype=torch.float64) * 2 - 1
    g = torch.rand((2, 16, 16, 3), generator=gen, dtype=torch.float64) * 2 - 1
    vp = {k: v.double() for k, v in vp.items()}
    return R, vp, t, g


@pytest.mark.parametrize("w", [0.0, -0.5])
def test_nonpositive_weight_leaves_the_oracle_bit_identical(monkeypatch, w):
    R, vp, t, g = _perceptual_inputs()
    ref = R.perceptual_loss(vp, t, g)
    G.patch_oracle(monkeypatch, w)
    assert torch.equal(R.perceptual_loss(vp, t, g), ref)


def test_positive_weight_adds_the_six_terms(monkeypatch):
    R, vp, t, g = _perceptual_inputs()
    ref = R.perceptual_loss(vp, t, g)
    ft, fg = R.vgg_features(vp, t), R.vgg_features(vp, g)
    assert len(ft) == 6 and ft[0].shape[-1] == 3
    extra = sum(G.gram_l1(a.reshape(2, -1, a.shape[-1]), b.reshape(2, -1, b.shape[-1]), 0.25) for a, b in zip(ft, fg))
    G.patch_oracle(monkeypatch, 0.25)
    got = R.perceptual_loss(vp, t, g)
    assert float(extra) > 0
    assert abs(float(got) - float(ref + extra)) <= 1e-12 * float(got)


def test_trainer_validates_gram_weight():
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import gram_weight_of
    assert gram_weight_of({}) == 0.0
    assert gram_weight_of({"gram_weight": 0}) == 0.0
    assert gram_weight_of({"gram_weight": 0.1}) == 0.1
    assert gram_weight_of({"gram_weight": 2}) == 2.0
    with pytest.warns(UserWarning, match="gram_weight"):
        assert gram_weight_of({"gram_weight": -0.5}) == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        gram_weight_of({"gram_weight": 0.0})
    for bad in ({"var_type": "linear", "options": {}}, "0.1", [0.1], True):
        with pytest.raises(ValueError, match="gram_weight"):
            gram_weight_of({"gram_weight": bad})
