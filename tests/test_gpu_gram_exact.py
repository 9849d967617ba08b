"""Bit-exact parity of the Gram kernels (csrc/gram.hip) on integer maps (tests/gram_exact_ref.py).

Maps of integers in [-2, 2]: D = F_g^T F_g - F_t^T F_t is an integer matrix in any order of summation, so `sign` is held to sign(D)
over the whole [n, cp, cp] array by bits -- the D == 0 entries, which tests/test_gpu_gram.py skips, and the pad included -- and
`partial` to the integer per-tile sums.  The backward runs with coef = 2**-10 and a device scale of 2 onto a prefill of small
integers: exact in fp32, one RNE to bf16, compared by bits, channels [c, ld) untouched.  Two cases make D exactly zero: on an
8 x 8 block (F_t = F_g on eight channels) and everywhere (F_t = F_g with its pixels permuted).  The one tolerance is the loss
through ups_sum_scale at the 1e-4 of tests/test_gpu_gram.py: that scale is not dyadic.  The headroom is asserted before launch."""
import pytest
import torch

import exact_ref as E
import gram_exact_ref as X
import gram_ref as G

pytestmark = pytest.mark.gpu


def _lib():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _cmp(errs, got, want, what, axes=None):
    msg = E.first_diff(got.contiguous(), want.contiguous(), axes)
    if msg is not None:
        errs.append("{}: {}".format(what, msg))


def _params():
    return [pytest.param(c, d, r, id="{}-{}-{}".format(c.name, d, "relu" if r else "plain"))
            for c in X.CASES for d in X.DTYPES for r in (False, True)]


@pytest.mark.parametrize("case,dtype,relu", _params())
def test_gram_exact(case, dtype, relu, dev):
    lib, ops = _lib()
    a, b = X.case_maps(case)
    for name, v in X.headroom(case, a, b, relu).items():
        assert v < X.LIMIT, "{} {}: headroom {:.0f} >= 2**24".format(case, name, v)
    ref = X.reference(case, a, b, relu)
    T = E.TORCH_T[dtype]
    n, c, hw, ld, cp = case.n, case.c, case.hw, case.ld, case.cp
    ad, bd = a.to(T).to(dev), b.to(T).to(dev)
    splits, npart, nws, nsign = ops.gram_plan(n, hw, c, lib.dt(bd))
    assert splits == case.splits[dtype], (case, dtype, splits)
    part = torch.empty(npart, dtype=torch.float32, device=dev)
    part.view(torch.uint8).fill_(0xFF)
    sign = torch.full((nsign,), 0x55, dtype=torch.int8, device=dev)
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws else None
    if ws is not None:
        ws.view(torch.uint8).fill_(0xFF)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    act = lib.ACT_RELU if relu else lib.ACT_NONE
    lib.call("ups_gram_l1_fwd", lib.ptr(ad), lib.ptr(bd), lib.dt(bd), n, hw, c, ld, act, lib.ptr(part), lib.ptr(sign), lib.ptr(ws),
             lib.stream())
    lib.call("ups_sum_scale", lib.ptr(part), npart, 1.0 / (ops.GRAM_DIV * hw) / (n * c * c), lib.ptr(loss), 0, lib.stream())
    pre = X.prefill(case)
    gb = pre.to(T).to(dev)
    scale_dev = torch.tensor(X.DEV_SCALE, dtype=torch.float32, device=dev)
    lib.call("ups_gram_l1_bwd", lib.ptr(bd), lib.ptr(sign), lib.ptr(gb), lib.dt(bd), n, hw, c, ld, act, lib.ptr(scale_dev), X.COEF,
             lib.stream())
    torch.cuda.synchronize()
    errs = []
    S = sign.view(n, cp, cp).cpu()
    _cmp(errs, S, ref["sign"], "{} sign".format(case), ("image", "row", "column"))
    _cmp(errs, part.cpu(), ref["partial"].float(), "{} partial (image * pairs + pair)".format(case))
    want_loss = float(G.gram_l1(ref["Ft"], ref["Fg"], 1.0))
    if not abs(float(loss) - want_loss) <= 1e-4 * want_loss:
        errs.append("{} loss {!r} want {!r}".format(case, float(loss), want_loss))
    # the backward reference uses the reference's S: a wrong sign entry has been reported above and shows here again
    want = X.backward_reference(case, b, ref["sign"], pre, relu)
    _cmp(errs, gb.cpu(), E.rounded(want, dtype), "{} backward".format(case))
    if ld > c:
        _cmp(errs, gb.cpu()[..., c:], pre.to(T)[..., c:], "{} backward, channels [c, ld)".format(case))
    if case.tie == "block":
        blk = S[:, :8, :8]
        if int(blk.abs().sum()) != 0:
            errs.append("{}: S is not zero on the tied block".format(case))
        nz = ref["D"] != 0
        if not bool((S[:, :c, :c][nz] != 0).all()):
            errs.append("{}: S is zero where D is not".format(case))
    if case.tie == "all":
        if int(S.abs().sum()) != 0:
            errs.append("{}: S is not all zero".format(case))
        _cmp(errs, part.cpu(), torch.zeros(npart), "{} partial is not +0".format(case))
        if float(loss) != 0.0:
            errs.append("{}: loss {!r}".format(case, float(loss)))
        _cmp(errs, gb.cpu(), pre.to(T), "{} backward changed gb".format(case))
    assert not errs, "\n".join(errs)
