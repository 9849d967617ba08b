"""Bit-exact weight and bias gradient of the wide 3x3 weight-gradient kernel (conv_wgrad3x3_kernel<64,128,8>, pipelined unit loop) on
lattice inputs (tests/exact_ref.py), at the smallest shapes that take that instance and reach the edges of its unit loop.

The loop stages the following units inside the MFMA rows of the current one, walks the units incrementally and runs as one of
eight copies (bias sum yes / no, activation on load yes / no, bf16 / fp16 input).  The cases below pick every copy:
  A  two units in one block: the prologue and the last-unit paths only (the walkers never move past the second unit)
  B  six units in one split: the steady state; ragged channel tails on both sides (72 -> 136)
  C  four splits x four (ci, co) tile pairs: the XCD block order; the bias is summed only by the blocks of the first ci tile;
     a stored-activation input (no activation on load)
  D  eight splits of seven units, the last of five: the unit walk across tile-row and image boundaries, starting mid-image
fp16 storage is a forward format; the gradient operand stays bf16 and the kernel converts the staged input (in_f16).
There is no tolerance: every sum is exact in fp32 (the headroom is asserted), so the result is the integer reference's bits, and
each case runs twice in the process with identical bits required (a miscounted wait reads a buffer a moment too early)."""
import pytest
import torch

import exact_ref as E

pytestmark = pytest.mark.gpu

LR = E.LR
CASES = [
    E.Case("wide_a_two_units", "conv", 1, 16, 16, 64, 128, act=LR, dtypes=("bf16", "f16")),
    E.Case("wide_b_one_split_ragged", "conv", 1, 16, 48, 72, 136, act=LR, dtypes=("bf16",)),
    E.Case("wide_c_splits_pairs_post", "conv", 2, 32, 32, 128, 256, act=LR, in_post=True, out_act=True, dtypes=("bf16", "f16")),
    E.Case("wide_d_unit_walk", "conv", 3, 48, 48, 64, 128, act="relu", dtypes=("bf16",)),
]
PARAMS = [pytest.param(c, d, id="{}-{}".format(c.name, d)) for c in CASES for d in c.dtypes]


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops
    return lib, ops


def _ff(shape, dtype, dev):
    """A caller buffer pre-filled with 0xFF bytes (NaN in every float type): an element the kernel does not write shows."""
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _grads(case, dtype, inputs, dev):
    """One forward + weight / bias gradient of the case through ops.conv and torch.autograd.grad, into 0xFF-filled buffers."""
    lib, ops = _mods()
    x, V, b, go = inputs
    f16 = dtype == "f16"
    lay = ops.ConvLayer("exact/conv2d_0", V.float().to(dev).requires_grad_(True), b.float().to(dev).requires_grad_(True), case.k,
                        case.stride, case.coords, case.act, slope=E.SLOPE)
    lay.in_post = case.in_post
    lay.out_act = lib.ACT_LRELU if case.out_act else lib.ACT_NONE
    lay.f16 = f16
    lay.grad_V, lay.grad_b = _ff(lay.V.shape, torch.float32, dev), _ff(lay.b.shape, torch.float32, dev)
    if f16:
        xd = x.to(torch.float16).to(dev).view(torch.bfloat16)          # fp16 lives in bf16 containers
    else:
        xd = x.to(torch.bfloat16).to(dev)
    y = ops.conv(xd, lay, fmt=lib.F16 if f16 else None)
    gd = torch.zeros(y.shape, dtype=torch.bfloat16, device=dev)       # the gradient of an fp16 layer is bf16 too
    gd[..., :case.cout] = go.to(torch.bfloat16).to(dev)
    gV, gb = torch.autograd.grad([y], [lay.V, lay.b], grad_outputs=[gd])
    ops.Streams.join(dev)
    torch.cuda.synchronize()
    return gV.cpu().clone(), gb.cpu().clone()


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_wide_wgrad_exact(case, dtype, dev):
    inputs, ref, hr = E.case_reference(case)
    print("{}: headroom {:.0f}".format(case, hr))
    assert hr < E.LIMIT, "{}: headroom {:.0f} >= 2**24".format(case, hr)
    want_V, want_b = ref["gV"].float(), ref["gb"].float()
    runs = [_grads(case, dtype, inputs, dev) for _ in range(2)]
    for i, (gV, gb) in enumerate(runs):
        msg = E.first_diff(gV, want_V, E.AXES_HWIO)
        assert msg is None, "{} {} run {}: weight gradient: {}".format(case, dtype, i, msg)
        msg = E.first_diff(gb, want_b)
        assert msg is None, "{} {} run {}: bias gradient: {}".format(case, dtype, i, msg)
    msg = E.first_diff(runs[0][0], runs[1][0], E.AXES_HWIO)
    assert msg is None, "{} {}: weight gradient differs between two runs: {}".format(case, dtype, msg)
    msg = E.first_diff(runs[0][1], runs[1][1])
    assert msg is None, "{} {}: bias gradient differs between two runs: {}".format(case, dtype, msg)
