"""CPU tests of `upsample: conv_transposed` (weight-normalised deconv2d): the fp64 restatement the GPU tests compare against is
pinned to TF's conv2d_transpose by the adjoint identity with the oracle's TF-pinned conv2d_same; variable names, shapes and init
kinds of the dry run; the TF checkpoint split keeps deconv2d's g."""
import copy

import numpy as np
import pytest
import torch

import deconv_ref as D


@pytest.mark.parametrize("cin,nf,h", [(3, 5, 4), (8, 10, 6), (7, 4, 5)])
def test_restatement_is_the_adjoint_of_the_stride2_same_convolution(cin, nf, h):
    """tf.nn.conv2d_transpose is the gradient of tf.nn.conv2d w.r.t. its input: <conv2d_same(u, W, 0, 2), v> = <u, deconv(v, W)>."""
    from oracle import ref_model as R
    gen = torch.Generator().manual_seed(cin * 100 + nf)
    W = torch.randn((3, 3, nf, cin), generator=gen, dtype=torch.float64)
    u = torch.randn((2, 2 * h, 2 * h + 2, nf), generator=gen, dtype=torch.float64)
    v = torch.randn((2, h, h + 1, cin), generator=gen, dtype=torch.float64)
    lhs = (R.conv2d_same(u, W, torch.zeros(cin, dtype=torch.float64), 2) * v).sum()
    y = D.deconv(v, W)
    assert y.shape == u.shape
    rhs = (u * y).sum()
    assert abs(float(lhs - rhs)) <= 1e-10 * max(1.0, abs(float(lhs)))


def test_restatement_taps_and_normalisation():
    """y[2i+ky, 2j+kx] = x[i, j] W[ky, kx] for a single input pixel; the taps on row / column 2H are dropped; W = g V / ||V_o||."""
    V = torch.randn((3, 3, 2, 1), dtype=torch.float64)
    g = torch.tensor([2.0, 0.5], dtype=torch.float64)
    W = D.weight(V, g)
    for o in range(2):
        assert abs(float(W[:, :, o, :].norm()) - float(g[o])) < 1e-12
    x = torch.zeros((1, 3, 3, 1), dtype=torch.float64)
    x[0, 1, 2, 0] = 1.0
    y = D.deconv(x, W)
    assert y.shape == (1, 6, 6, 2)
    for ky in range(3):
        for kx in range(3):
            yy, xx = 2 + ky, 4 + kx
            if yy < 6 and xx < 6:
                assert torch.equal(y[0, yy, xx], W[ky, kx, :, 0])
    assert int((y != 0).any(-1).sum()) == 6        # (4, 6) and (y, 6) taps fall off the image
    # an all-zero filter: the clamp keeps W finite (zero)
    Wz = D.weight(torch.zeros((3, 3, 2, 4), dtype=torch.float64), g)
    assert torch.isfinite(Wz).all() and float(Wz.abs().max()) == 0.0


def _nets(cfg):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import nets
    return nets, nets.Nets(cfg, torch.device("cpu"), seed=0)


def _deconv_config():
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg["final_hour"]["upsample_method"] = "conv_transposed"
    cfg["dv"]["upsample_config"] = ["conv_transposed", "linear"]
    return cfg


def test_dry_run_specs_of_deconv2d():
    from oracle import configs
    nets, n = _nets(_deconv_config())
    _, base = _nets(copy.deepcopy(configs.tiny_config()))
    sp = n.specs
    # hourglass final_hour [8, 16]: 16 -> 8 channels at 8x8 -> 16x16; no coordinates there.  dv [8, 16, 16] with coords: the
    # up-sampling nearest the 4x4 start (the LAST entry of upsample_config) is linear, the next one (16 -> 8 channels) a deconv
    assert sp["decoder_delta/deconv2d_0/V"] == ((3, 3, 8, 16), 0.05, "normal")
    assert sp["decoder_delta/deconv2d_0/g"] == ((8,), 1.0, "ones")
    assert sp["decoder_delta/deconv2d_0/b"] == ((8,), 0.0, "zeros")
    assert sp["decoder_visualize/deconv2d_0/V"] == ((3, 3, 8, 18), 0.05, "normal")
    assert "decoder_delta/deconv2d_1/V" not in sp and "decoder_visualize/deconv2d_1/V" not in sp
    # the conv2d_k counter is independent of deconv2d_k: the convolutions keep their names, and their (uniform) initial values
    # wherever the shape is the same (a linear up-sampling keeps the channel count, a deconvolution maps it to nf)
    conv = [k for k in sp if "/conv2d_" in k]
    assert conv == [k for k in base.specs]
    same = [k for k in conv if sp[k] == base.specs[k]]
    assert len(same) >= len(conv) - 8
    for k in same:
        assert torch.equal(n.bank.params[k], base.bank.params[k]), k
    # init kinds, seeded per name
    V = n.bank.params["decoder_delta/deconv2d_0/V"]
    assert torch.equal(V, (torch.randn((3, 3, 8, 16), generator=nets._rng(0, "decoder_delta/deconv2d_0/V"),
                                       dtype=torch.float64) * 0.05).float())
    assert torch.equal(n.bank.params["decoder_delta/deconv2d_0/g"], torch.ones(8))
    assert torch.equal(n.bank.params["decoder_delta/deconv2d_0/b"], torch.zeros(8))
    # the variables belong to their sub-network's optimizer key
    assert "decoder_visualize/deconv2d_0/g" in n.bank.groups["decoder_visualize"]["names"]
    assert "decoder_delta/deconv2d_0/g" in n.bank.groups["decoder_delta"]["names"]


def test_tf_checkpoint_split_keeps_deconv_scale():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import tfckpt
    bundle = {"decoder_visualize/deconv2d_0/g": np.ones(4, np.float32), "decoder_visualize/deconv2d_0/V": np.zeros((3, 3, 4, 6), np.float32),
              "decoder_visualize/deconv2d_0/g/Adam": np.ones(4, np.float32), "global_step": np.int64(3), "Variable": np.float32(0)}
    params, m, v, other = tfckpt.to_trainer_state(bundle)
    assert sorted(params) == ["decoder_visualize/deconv2d_0/V", "decoder_visualize/deconv2d_0/g"]
    assert "decoder_visualize/deconv2d_0/g" in m
    assert sorted(other) == ["Variable", "global_step"]


def test_unknown_upsample_method_still_raises():
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    cfg["final_hour"]["upsample_method"] = "gram_weight"
    with pytest.raises(NotImplementedError):
        _nets(cfg)
