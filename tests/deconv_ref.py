"""fp64 restatement of `upsample(x, nf, "conv_transposed")` (weight-normalised deconv2d, cub/code/nn.py:818-822, 938-1039) for the
deconvolution tests, and a patch that teaches the oracle's Scope.upsample the method (in-test only: oracle/ is not edited)."""
import torch
import torch.nn.functional as F


def weight(V, g):
    """W = g * tf.nn.l2_normalize(V, [0, 1, 3]) (x * rsqrt(max(sum x^2, 1e-12))); V [3,3,nf,Cin] = [kh, kw, out, in]."""
    ss = (V * V).sum(dim=(0, 1, 3), keepdim=True)
    return g.view(1, 1, -1, 1) * (V * torch.rsqrt(torch.clamp(ss, min=1e-12)))


def deconv(x, W, b=None):
    """tf.nn.conv2d_transpose(x, W, [n, 2H, 2W, nf], stride 2, 'SAME') (+ b): x NHWC, W [3,3,nf,Cin].  The transposed convolution
    without padding is 2H+1 tall; 'SAME' on an even size pads 0 before and 1 after, so the last row / column is cropped."""
    n, h, w, _ = x.shape
    y = F.conv_transpose2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), stride=2)[:, :, :2 * h, :2 * w]
    if b is not None:
        y = y + b.view(1, -1, 1, 1)
    return y.permute(0, 2, 3, 1)


def layer(x, V, g, b, coords, add_coordinates):
    """The whole layer: CoordConv channels at the input's resolution, normalisation, transposed convolution, bias."""
    if coords:
        x = add_coordinates(x)
    return deconv(x, weight(V.to(x.dtype), g.to(x.dtype)), b.to(x.dtype))


def init(seed, name, shape, kind, rng):
    """The package's init kinds (nets.init_variable): V ~ N(0, 0.05), g = 1, b = 0, seeded per name."""
    if kind == "normal":
        return (torch.randn(shape, generator=rng(seed, name), dtype=torch.float64) * 0.05).to(torch.float32)
    return (torch.ones if kind == "ones" else torch.zeros)(shape, dtype=torch.float32)


def patch_oracle(monkeypatch):
    """oracle.ref_model.Scope.upsample learns "conv_transposed" (its own deconv2d_k counter, variables created on first use)."""
    from oracle import ref_model as R
    orig = R.Scope.upsample

    def upsample(self, x, num_units, method="subpixel"):
        if method != "conv_transposed":
            return orig(self, x, num_units, method)
        k = self.__dict__.get("dcounter", 0)
        self.dcounter = k + 1
        name = "{}/deconv2d_{}".format(self.prefix, k)
        cin = x.shape[-1] + (2 if self.coords else 0)
        if name + "/V" not in self.params:
            assert self.seed is not None, "missing variable " + name
            self.params[name + "/V"] = init(self.seed, name + "/V", (3, 3, num_units, cin), "normal", R.param_rng)
            self.params[name + "/g"] = init(self.seed, name + "/g", (num_units,), "ones", R.param_rng)
            self.params[name + "/b"] = init(self.seed, name + "/b", (num_units,), "zeros", R.param_rng)
        return layer(x, self.params[name + "/V"], self.params[name + "/g"], self.params[name + "/b"], self.coords,
                     self.add_coordinates)
    monkeypatch.setattr(R.Scope, "upsample", upsample)
