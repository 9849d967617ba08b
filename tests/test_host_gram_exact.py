"""CPU checks of tests/gram_exact_ref.py: on every case the headroom is below 2**24, the integer reference equals
tests/gram_ref.py (the single-accumulator form, the normalised Gram matrices, autograd of the term), the tie cases are ties,
every rounded backward reference is representable, and the split counts are what ups_gram_plan gives (host code)."""
import ctypes as C

import pytest
import torch

import exact_ref as E
import gram_exact_ref as X
import gram_ref as G


def _params():
    return [pytest.param(c, r, id="{}-{}".format(c.name, "relu" if r else "plain")) for c in X.CASES for r in (False, True)]


@pytest.mark.parametrize("case,relu", _params())
def test_case_meets_the_headroom_condition_and_equals_gram_ref(case, relu):
    a, b = X.case_maps(case)
    for name, v in X.headroom(case, a, b, relu).items():
        assert v < X.LIMIT, "{} {}: {:.0f} >= 2**24".format(case, name, v)
    assert float(a[..., :case.c].abs().max()) <= 2 and torch.equal(a[..., :case.c], a[..., :case.c].round())
    assert float(a[..., case.c:].abs().min()) == X.PAD_GARBAGE if case.ld > case.c else True
    for T in X.DTYPES:
        assert torch.equal(E.rounded(a, T).double(), a) and torch.equal(E.rounded(b, T).double(), b)
    ref = X.reference(case, a, b, relu)
    Ft, Fg = ref["Ft"], ref["Fg"]
    assert torch.equal(ref["D"], G.concat_d(Ft, Fg))
    scale = G.GRAM_DIV * case.hw
    assert float((ref["D"] / scale - (G.gram(Fg) - G.gram(Ft))).abs().max()) <= 1e-12 * max(1.0, float(ref["D"].abs().max()) / scale)
    # the partials add up to the term: sum |D| over the whole symmetric matrix
    assert float(ref["partial"].sum()) == float(ref["D"].abs().sum())
    assert torch.equal(ref["partial"].float().double(), ref["partial"])
    S = ref["sign"]
    assert torch.equal(S, S.transpose(1, 2)) and int(S[:, case.c:].abs().sum()) == 0 and int(S[:, :, case.c:].abs().sum()) == 0
    # backward: the closed form is autograd of the term (torch's |.| has gradient 0 at 0, the kernel's sign = 0 branch)
    Fr = Fg.clone().requires_grad_(True)
    term = G.gram_l1(Ft, Fr, 1.0)
    gF, = torch.autograd.grad([term], [Fr])
    const = 2.0 / (case.n * case.c * case.c) / scale
    FS = Fg @ S[:, :case.c, :case.c].double()
    assert float((gF - const * FS).abs().max()) <= 1e-12 * max(1e-30, float((const * FS).abs().max()))
    assert float((G.gram_l1_grad(Ft, Fg, 1.0) - const * FS).abs().max()) <= 1e-12 * max(1e-30, float((const * FS).abs().max()))
    pre = X.prefill(case)
    assert not bool(torch.signbit(pre[pre == 0]).any()) and float(pre[..., :case.c].abs().max()) <= 3
    want = X.backward_reference(case, b, S, pre, relu)
    assert torch.equal(want.float().double(), want)                     # exact in fp32: bf16 is its one RNE
    assert torch.equal(want[..., case.c:], pre[..., case.c:])


@pytest.mark.parametrize("relu", [False, True])
def test_tie_cases_are_ties(relu):
    blk, al = X.BY_NAME["gm_tie_block"], X.BY_NAME["gm_tie_all"]
    a, b = X.case_maps(blk)
    ref = X.reference(blk, a, b, relu)
    assert float(ref["D"][:, :8, :8].abs().max()) == 0 and int(ref["sign"][:, :8, :8].abs().sum()) == 0
    rest = ref["D"].clone()
    rest[:, :8, :8] = 1.0
    assert float((rest != 0).double().mean()) > 0.9            # (elsewhere D is mostly non-zero: the block is what is special)
    assert torch.equal(ref["sign"][:, :blk.c, :blk.c].double(), torch.sign(ref["D"]))
    a, b = X.case_maps(al)
    assert not torch.equal(a[..., :al.c], b[..., :al.c])
    ref = X.reference(al, a, b, relu)
    assert float(ref["D"].abs().max()) == 0 and int(ref["sign"].abs().sum()) == 0 and float(ref["partial"].abs().max()) == 0
    pre = X.prefill(al)
    assert torch.equal(X.backward_reference(al, b, ref["sign"], pre, relu), pre)


def _plan(lib, n, hw, c, T):
    out = (C.c_int64 * 4)()
    assert lib.load().ups_gram_plan(n, hw, c, lib.F32 if T == "fp32" else lib.BF16, out) == 0
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_split_counts_are_the_plans(case):
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    pairs = case.tiles * (case.tiles + 1) // 2
    for T in X.DTYPES:
        splits, npart, nws, nsign = _plan(lib, case.n, case.hw, case.c, T)
        assert splits == case.splits[T], (case, T, splits)
        assert npart == case.n * pairs and nsign == case.n * case.cp * case.cp
        assert nws == (case.n * pairs * splits * X.GT * X.GT if splits > 1 else 0)


def test_split_cases_are_the_smallest_with_two_splits():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    for name, T in (("gm_split_bf16", "bf16"), ("gm_split_fp32", "fp32")):
        case = X.BY_NAME[name]
        assert case.c == 64 and _plan(lib, case.n, case.hw, 64, T)[0] == 2
        assert all(_plan(lib, case.n, hw, 64, T)[0] == 1 for hw in range(1, case.hw))
    assert any(c.splits["bf16"] > 1 for c in X.CASES) and any(c.splits["fp32"] == 1 for c in X.CASES)
