"""CPU checks of the fp8 lattice of tests/exact_ref.py: on every case each quantisation round-trips through the torch fp8 types,
every scale the kernels will derive is a power of two, every sum stays below 2**24 LSBs in the quantised domain, and the fp8
emulation equals the plain integer convolution bit for bit -- so tests/test_gpu_exact_fp8.py may hold the fp8 kernels to the
integers.  Also: the outputs of the emitting launches are arranged to a maximum of 7 * 2**k, and the split-K of every
weight-gradient case is what ups_conv_wgrad_plan gives."""
import ctypes as C

import pytest
import torch

import exact_ref as E

F32 = torch.float32


def _lossless_dyadic_and_within_headroom(case, inputs, ref, hr):
    x, V, b, go = inputs
    assert ref["lossless"], "{}: a quantisation does not round-trip".format(case)
    Vm = V[:, :, :case.cin]
    assert float(V[:, :, case.cin:].abs().sum()) == 0.0
    xa = E.act_fn(x, case.act)
    for q, t, s in ((E.E4M3, xa, E.F8_SA), (E.E4M3, Vm, E.F8_SW), (E.E5M2, go, E.F8_SG)):
        assert torch.equal((t * s).float().to(q).double() / s, t)
    # the scales as the kernels derive them, in float32: weight_prep_f8_kernel per column (forward) and per row (input gradient),
    # the primed scale (from |x|, |g|) and the delayed one (from the recorded max |act(x)|, |g|)
    for m in (Vm.abs().amax(dim=(0, 1, 2)).to(F32), Vm.abs().amax(dim=(0, 1, 3)).to(F32)):
        sc, deq = torch.tensor(448.0, dtype=F32) / m, m / torch.tensor(448.0, dtype=F32)
        assert E.is_pow2(sc) and E.is_pow2(deq) and E.is_pow2(1.0 / sc) and E.is_pow2(1.0 / deq)
        assert bool((sc == E.F8_SW).all()) and bool((deq == 1.0 / E.F8_SW).all())
    half = torch.tensor(E.F8_MARGIN, dtype=F32)
    for fmax, amaxes, want in ((E.E4M3_MAX, (x.abs().max(), xa.abs().max()), E.F8_SA), (E.E5M2_MAX, (go.abs().max(),), E.F8_SG)):
        for amax in amaxes:
            s = torch.tensor(fmax, dtype=F32) * half / amax.to(F32)
            assert E.is_pow2(s) and E.is_pow2(1.0 / s) and float(s) == want
    assert E.is_pow2(1.0 / torch.tensor(E.F8_SA * E.F8_SG, dtype=F32))
    for name, v in hr.items():
        assert v < E.LIMIT, "{} {}: sum of |products| is {:.0f} LSBs >= 2**24".format(case, name, v)
    assert set(hr) == set(case.dirs) | ({"bgrad"} if "wgrad" in case.dirs else set())


@pytest.mark.parametrize("case", E.FP8_CASES, ids=repr)
def test_fp8_case_is_lossless_dyadic_within_headroom_and_equals_the_integer_reference(case):
    """Round trips, power-of-two scales, headroom, a dyadic output scale where the launch emits a copy; and, since no information
    is lost on this lattice, the fp8 emulation IS the bf16 / fp32 reference: tap loop for every case, conv_block + autograd in
    float64 for the small ones.  (One test: the large cases' references are not kept.)"""
    inputs, ref, hr = E.fp8_case_reference(case)
    _lossless_dyadic_and_within_headroom(case, inputs, ref, hr)
    _emitting_launches_have_a_dyadic_output_scale(case, inputs, ref)
    x, V, b, go = inputs
    big = E._big(case)
    assert not big or max(hr.values()) < E.LIMIT
    plain = E.plain_reference(case, inputs, ref, torch.float32 if big else torch.float64)
    for k, want in plain.items():
        assert E.first_diff(ref[k], want, E.AXES_HWIO if k == "gV" else None) is None, "{} {}: {}".format(case, k, E.first_diff(ref[k], want))
    if big:
        return
    blk = E.conv_block(x, V[:, :, :case.cin], ref["b"], go, act=case.act, res_self=case.res_self)
    if "fwd" in case.dirs:
        assert E.first_diff(ref["y"], blk["y"]) is None
    if "dgrad" in case.dirs:
        gx = blk["gx"] + (ref["res_g"] if ref["res_g"] is not None else 0.0)
        assert E.first_diff(ref["gx"], gx) is None
    if "wgrad" in case.dirs:
        assert E.first_diff(ref["gV"], blk["gV"], E.AXES_HWIO) is None and E.first_diff(ref["gb"], blk["gb"]) is None


def _emitting_launches_have_a_dyadic_output_scale(case, inputs, ref):
    """Every emitting case arranges it (none needs the GPU test's skip): the stored bf16 output's act-maximum is 7 * 2**k."""
    x, V, b, go = inputs
    if "fwd" in case.emit:
        ya = E.lrelu(E.rounded(ref["y"], "bf16").double())
        assert float(ya.abs().max()) == ref["y_top"] and float(ya.max()) == ref["y_top"]
        s = torch.tensor(E.E4M3_MAX * E.F8_MARGIN, dtype=F32) / torch.tensor(ref["y_top"], dtype=F32)
        assert E.is_pow2(s) and E.f8_quantise(ya, float(s), E.E4M3)[0].double().abs().max() == 224.0
        assert float(ref["b"].abs().max()) < 2 ** 24 and torch.equal(ref["b"], ref["b"].float().double())
    if "dgrad" in case.emit:
        assert ref["res_g"] is not None, "{}: no element with a zero sum to carry the arranged maximum".format(case)
        gq = E.rounded(ref["gx"], "bf16").double()
        assert float(gq.abs().max()) == ref["gx_top"]
        s = torch.tensor(E.E5M2_MAX * E.F8_MARGIN, dtype=F32) / torch.tensor(ref["gx_top"], dtype=F32)
        assert E.is_pow2(s)
        res = (go if case.res_self else 0.0) + ref["res_g"]
        assert torch.equal(E.rounded(res, "bf16").double(), res)


def _wgrad_desc(lib, case, dout_f8):
    d = lib.WgradDesc()
    d.dtype = lib.BF16
    d.n, d.hi, d.wi, d.ci, d.ldi = case.n, case.h, case.w, case.cin, case.cin
    d.ci_log, d.cin_v = case.cin, case.cin + (2 if case.coords else 0)
    d.ho, d.wo, d.co, d.ldo = case.h, case.w, case.cout, case.cout
    d.in_sy = d.in_sx = 1
    for t in range(9):
        d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = t // 3 - 1, t % 3 - 1, t
    d.ntaps = 9
    d.dout_f8 = dout_f8
    return d


@pytest.mark.parametrize("case", [c for c in E.FP8_CASES if c.route == "wgrad"], ids=repr)
def test_fp8_wgrad_case_split_k_is_the_plans(case):
    """The plan is host code: with an e5m2 copy in the descriptor the fp8 kernel's split, without one the bf16 kernel's."""
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib
    buf = C.create_string_buffer(64)
    sk, wsb = C.c_int32(0), C.c_size_t(0)
    d = _wgrad_desc(lib, case, C.cast(buf, C.c_void_p).value)
    assert lib.load().ups_conv_wgrad_plan(C.byref(d), C.byref(sk), C.byref(wsb)) == 0
    assert sk.value == case.splitk, (case, sk.value)
    assert wsb.value == sk.value * (9 * d.cin_v * d.co + d.co) * 4


def test_fp8_wgrad_cases_cover_both_sides_of_the_multiple_of_8_rule():
    sks = [c.splitk for c in E.FP8_CASES if c.route == "wgrad"]
    assert any(s < 8 for s in sks) and any(s >= 8 for s in sks)
    assert sorted((c.f16, c.act is not None) for c in E.FP8_CASES if c.route == "wgrad") == [(False, False), (False, True), (True, False), (True, True)]


def test_fp8_generators_guarantee_their_conditions():
    g = E.gen("fp8 lattice")
    V = E.f8_weights(g, 3, 64, 136, density=0.1)
    assert bool((V.abs().amax(dim=(0, 1, 2)) == 7).all()) and bool((V.abs().amax(dim=(0, 1, 3)) == 7).all())
    assert float((V != 0).double().mean()) < 0.2 and float(V.abs().max()) == 7
    x = E.f8_activations(g, (2, 4, 4, 8), density=0.0)
    assert float(x.max()) == 7 and float(x.min()) == -7 and float(E.lrelu(x).abs().max()) == 7
    # every lattice value is an fp8 value at its scale; 0.25 * odd * 32 is one too (8 ... 56), but act(x) * 64 would not need to be
    ints = torch.arange(-7, 8).double()
    assert E.f8_quantise(ints, E.F8_SW, E.E4M3)[1] and E.f8_quantise(E.lrelu(ints), E.F8_SA, E.E4M3)[1] and E.f8_quantise(ints, E.F8_SG, E.E5M2)[1]
    assert not E.f8_quantise(ints, 1024.0, E.E4M3)[1]                       # saturates: not lossless
    assert not E.f8_quantise(torch.tensor([9.0]), E.F8_SG, E.E5M2)[1]       # 1001b needs three mantissa bits
    assert E.is_pow2(torch.tensor([0.5, 4096.0, 2.0 ** -17])) and not E.is_pow2(torch.tensor([3.0])) and not E.is_pow2(torch.tensor([0.0]))
    assert E.lsb(torch.tensor([512.0, 1536.0]), 20) == 512.0 and E.lsb(torch.tensor([512.0, 1536.0])) == 1.0
    a, b_ = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    b_[2] = 0x80
    assert E.first_diff(a, a.clone()) is None and "1 of 4" in E.first_diff(a, b_)
