"""CPU checks of tests/exact_ref.py: every case of the exact-parity table meets the headroom condition (so an ill-chosen case fails
without a GPU), and the plain reference equals the oracle's fp64 convolution and autograd exactly on the same lattice inputs."""
import pytest
import torch

import exact_ref as E
from oracle import ref_model as R


@pytest.mark.parametrize("case", E.CASES, ids=repr)
def test_case_meets_the_headroom_condition(case):
    _, _, hr = E.case_reference(case)
    assert hr < E.LIMIT, "{}: sum of |products| is {:.0f} LSBs (2**{:.2f}) >= 2**24".format(case, hr, torch.log2(torch.tensor(hr)).item())


def _oracle(case, x_stored, V, b, go):
    """The same layer through oracle.ref_model (conv2d_same = F.conv2d in fp64), slope 0.25."""
    x_pre = (E.act_inverse(x_stored) if case.in_post else x_stored).clone().requires_grad_(True)
    Vr, br = V.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xa = x_pre
    if case.act == "leaky_relu":
        xa = torch.nn.functional.leaky_relu(x_pre, E.SLOPE)
    elif case.act == "relu":
        xa = torch.relu(x_pre)
    if case.coords:
        xa = R.Scope.add_coordinates(xa)
    pre = R.conv2d_same(xa, Vr, br, case.stride)
    if case.res_self:
        pre = pre + x_pre
    y = torch.nn.functional.leaky_relu(pre, E.SLOPE) if case.out_act else pre
    grads = torch.autograd.grad([pre], [x_pre, Vr, br], grad_outputs=[go])
    return y.detach(), grads


# (not the case whose coordinates are not dyadic: its CoordConv weight-gradient rows are not exact, and no test reads them)
@pytest.mark.parametrize("case", [c for c in E.CASES if not c.extra.get("zero_coord_rows")], ids=repr)
def test_reference_equals_the_oracle_exactly(case):
    (x, V, b, go), ref, _ = E.case_reference(case)
    xin = E.part_images(x, E.part_bits(case)[1]) if case.family == "mask" else x
    if "gx" not in ref:             # (a forward-only family: its table entry holds no gradients)
        ref = E.conv_block(xin, V, b, go, **case.kw())
    y, (gx, gV, gb) = _oracle(case, xin, V, b, go)
    for name, a, want in (("y", ref["y"], y), ("gx", ref["gx"], gx), ("gV", ref["gV"], gV), ("gb", ref["gb"], gb)):
        if name == "gx" and case.act == "relu":
            # exact_ref applies act' as a factor, as the kernels do, so a zero gradient carries its sum's sign; torch writes +0
            assert torch.equal(a, want), "{} gx: {}".format(case, E.first_diff(a, want))
        else:
            assert E.first_diff(a, want) is None, "{} {}: {}".format(case, name, E.first_diff(a, want))


@pytest.mark.parametrize("case", E.TOWER_CASES, ids=repr)
def test_tower_case_meets_the_headroom_condition_and_equals_autograd(case):
    """Every sum of the six layers, forward and backward, stays below 2**24 LSBs; and the hand-written backward equals fp64 autograd
    through the same chain with straight-through roundings wherever no gradient was rounded (the last layer's and, from its
    rounded inputs, every layer's weight and bias gradient formula)."""
    ref, hr = E.tower_case_reference(case)
    assert hr < E.LIMIT, "{}: {:.0f} LSBs".format(case, hr)
    for (x0, Ws, bs, g), r in ref:
        Ln = len(Ws)
        assert all(torch.equal(a, E.bf16_round(a)) for a in r["acts"])
        # autograd on one layer at a time from the reference's own stored tensors: d <v_l, g_l> / d (W_l, b_l, input)
        gl = g
        for l in range(Ln - 1, -1, -1):
            X = (x0 if l == 0 else r["acts"][l - 1]).clone()
            xp = (E.act_inverse(X) if l > 0 else X).requires_grad_(True)
            W, b = Ws[l].clone().requires_grad_(True), bs[l].clone().requires_grad_(True)
            v = (E.lrelu(xp) if l > 0 else xp) @ W + b + (xp if 0 < l < Ln - 1 else 0)
            gin, gW, gb = torch.autograd.grad([v], [xp, W, b], grad_outputs=[gl])
            assert torch.equal(gW, r["gW"][l]) and torch.equal(gb, r["gb"][l]), (case, l)
            want_act = r["acts"][l] if l == Ln - 1 else None
            if want_act is not None:
                assert torch.equal(E.bf16_round(v.detach()), want_act)
            gl = E.bf16_round(gin)
        assert torch.equal(gl, r["gx0"])


def test_lattice_values_are_exact_in_every_stored_type():
    g = E.gen("lattice")
    for t in (E.activations(g, (64,)), E.weights(g, (64,), 2), E.biases(g, 64), E.out_grads(g, (64,)),
              E.lrelu(E.activations(g, (64,))), E.act_inverse(E.activations(g, (64,)))):
        for T in ("bf16", "f16", "fp32"):
            assert torch.equal(E.rounded(t, T).double(), t)
    assert float(E.activations(g, (4096,)).abs().max()) == 4 and float(E.weights(g, (4096,)).abs().max()) == 1
    assert 0.3 < float((E.weights(g, (4096,), 1, 0.5) != 0).double().mean()) < 0.4       # 2/3 non-zero x density 1/2


def test_coordinates_are_dyadic_only_at_power_of_two_plus_one():
    for H in (9, 17, 33, 65):
        c = R.Scope.add_coordinates(torch.zeros(1, H, H, 1, dtype=torch.float64))[..., 1:]
        assert E.lsb(c) == 2.0 / (H - 1)
    with pytest.raises(ValueError):
        E.lsb(R.Scope.add_coordinates(torch.zeros(1, 16, 16, 1, dtype=torch.float64)))


def test_headroom_counts_lsbs_and_flags_an_ill_chosen_case():
    x = torch.full((1, 4, 4, 8), 4.0, dtype=torch.float64)
    V = torch.ones(3, 3, 8, 8, dtype=torch.float64)
    b = torch.zeros(8, dtype=torch.float64)
    assert E.headroom(x, V, b) == 9 * 8 * 4                                    # interior pixel: 72 products of 4
    assert E.headroom(-x / 4, V, b, act="leaky_relu") == 9 * 8                 # act(-1) = -1/4: 72 products of one LSB
    assert E.headroom(x, V, b, out_act=True) == 9 * 8 * 4 * 4                  # the stored activation adds two bits
    g = torch.ones(1, 4, 4, 8, dtype=torch.float64)
    assert E.headroom(x, V, b, g) == max(9 * 8 * 4, 16 * 4, 16)                # forward / weight-gradient / bias sums
    deep = torch.full((1, 16, 16, 4096), 4.0 * 2 ** 10, dtype=torch.float64)
    assert E.headroom(deep, torch.ones(3, 3, 4096, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)) >= E.LIMIT


def test_first_diff_decodes_the_index_and_sees_signed_zero_and_nan():
    a = torch.zeros(2, 3, 4, 8, dtype=torch.bfloat16)
    b = a.clone()
    assert E.first_diff(a, b) is None
    b[1, 2, 3, 5] = -0.0
    msg = E.first_diff(a, b)
    assert msg.startswith("1 of 192 elements differ") and "image=1, y=2, x=3, channel=5" in msg
    n = torch.full((4,), float("nan"))
    assert E.first_diff(n, n.clone()) is None and E.first_diff(n, torch.zeros(4)) is not None
