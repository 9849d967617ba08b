"""fp64 restatement of the Gram-matrix (style) terms of edflow's VGG19Features(default_gram=gram_weight).make_loss_op (edflow source
absent: the recalled reading, UNVERIFIED, like the rest of the perceptual trunk) for the Gram tests, and a patch that adds the terms
to the oracle's perceptual loss (in-test only: oracle/ is not edited).

    G(F)[b] = F[b]^T F[b] / (GRAM_DIV * h * w),   F = act(feature)[..., :c] as [n, h*w, c]
    term    = gram_weight * mean_{b,i,j} |G(F_t)[b,i,j] - G(F_g)[b,i,j]|
"""
import torch

GRAM_DIV = 4.0          # the normalisation of G (UNVERIFIED); the package's copy is ops.GRAM_DIV


def as_F(x, c, relu):
    """A feature map [n,h,w,ld] as the Gram operand [n, h*w, c] (logical channels only; relu = the term's activation)."""
    f = x[..., :c]
    if relu:
        f = torch.relu(f)
    return f.reshape(f.shape[0], -1, c)


def gram(F):
    return F.transpose(1, 2) @ F / (GRAM_DIV * F.shape[1])


def gram_l1(Ft, Fg, w):
    return w * (gram(Ft) - gram(Fg)).abs().mean()


def concat_d(Ft, Fg):
    """The kernel's single accumulator: [F_g; F_t]^T [F_g; -F_t] along K = 2 h w (unnormalised G(F_g) - G(F_t))."""
    return torch.cat([Fg, Ft], 1).transpose(1, 2) @ torch.cat([Fg, -Ft], 1)


def gram_l1_grad(Ft, Fg, w):
    """Closed form of d term / d F_g: 2 w / (n c c) / (GRAM_DIV h w) * F_g[b] S_b, S_b = sign(G(F_g)[b] - G(F_t)[b])."""
    n, hw, c = Fg.shape
    S = torch.sign(gram(Fg) - gram(Ft))
    return 2.0 * w / (n * c * c) / (GRAM_DIV * hw) * (Fg @ S)


def patch_oracle(monkeypatch, gram_weight):
    """oracle.ref_model.perceptual_loss gains sum_l gram_l1(f_l(target), f_l(generated)) over the same six feature maps it compares
    (after the same resize / crop: the maps are captured from its own vgg_features calls).  gram_weight <= 0: nothing changes."""
    from oracle import ref_model as R
    orig, orig_features = R.perceptual_loss, R.vgg_features
    if not gram_weight > 0:
        return

    def perceptual_loss(vp, target, generated, mode="native", depths=R.VGG_DEPTHS, crop=None):
        seen = []

        def features(*a, **k):
            f = orig_features(*a, **k)
            seen.append(f)
            return f
        monkeypatch.setattr(R, "vgg_features", features)
        try:
            l1 = orig(vp, target, generated, mode, depths, crop=crop)
        finally:
            monkeypatch.setattr(R, "vgg_features", orig_features)
        ft, fg = seen
        terms = [gram_l1(a.reshape(a.shape[0], -1, a.shape[-1]), b.reshape(b.shape[0], -1, b.shape[-1]), gram_weight)
                 for a, b in zip(ft, fg)]
        return l1 + sum(terms)
    monkeypatch.setattr(R, "perceptual_loss", perceptual_loss)
