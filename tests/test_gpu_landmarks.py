"""GPU tests of the landmark regression evaluation: ups_part_moments, ups_landmark_gram, ups_landmark_solve and ups_landmark_predict
(csrc/landmarks.hip, through the C ABI) against the NumPy float64 restatement of landmarks_ref.py -- integer sums with ==, float
outputs bit for bit, the float sums also within (n - 1) 2^-53 sum|term| of an independent sum and exactly on lattice inputs -- then
TrainModel.part_centres and the runner's --landmarks end to end.  Every output and scratch buffer sits between sentinel guard bands and
is pre-filled, so that "written completely" is visible; every kernel is launched twice and gives the same bits."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import landmarks_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FSENT = -7.0e77
ISENT = -0x5A5A5A5B
BSENT, BFILL = 0xA5, 7
IFILL = 0x01234567
VGG_W = (8, 8, 16, 16, 16)
E_ARG, E_UNSUPPORTED = -1, -2
MCH, CH = R.MOMENTS_CHUNK, R.LANDMARK_CHUNK      # = ups_part_moments_chunk(), ups_landmark_chunk() (asserted below)


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, landmarks
    return lib, ops, landmarks


@pytest.fixture(autouse=True)
def _keep_rng_state(dev):
    """Building a model seeds torch's generators; later test files draw unseeded device tensors.  They see the state they saw before
    this file existed."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu, dev)


class _Guarded(object):
    """`n` elements inside a sentinel-filled buffer with GUARD elements on each side."""

    def __init__(self, dev, n, dtype, inside):
        self.sent = {torch.int32: ISENT, torch.uint8: BSENT, torch.float64: FSENT}[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.sent, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n]
        self.view.fill_(inside)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def numpy(self):
        return self.view.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return all(torch.equal(a[k].view.view(torch.int64) if a[k].view.dtype == torch.float64 else a[k].view,
                           b[k].view.view(torch.int64) if b[k].view.dtype == torch.float64 else b[k].view) for k in a if k != "scratch")


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _geometry(L):
    h = L.load()
    assert (h.ups_part_moments_chunk(), h.ups_landmark_chunk()) == (MCH, CH)


# ---------------------------------------------------------------------------------------------- ups_part_moments
def _moments(L, dev, soft, pred, min_mass):
    N, h, w, P = soft.shape
    lib = L.load()
    nbytes = lib.ups_part_moments_scratch_bytes(N, h, w, P)
    assert nbytes == N * (-(-h * w // MCH)) * 3 * P * 8
    o = {"mass": _Guarded(dev, N * P, torch.float64, float("nan")), "centre": _Guarded(dev, N * P * 2, torch.float64, float("nan")),
         "valid": _Guarded(dev, N * P, torch.uint8, BFILL), "hard": _Guarded(dev, N * P * 3, torch.int32, 0),
         "invalid": _Guarded(dev, 1, torch.int32, 0), "scratch": _Guarded(dev, nbytes // 8, torch.float64, FSENT)}
    ts, tp = _to(dev, soft), None if pred is None else _to(dev, pred)
    rc = lib.ups_part_moments(L.ptr(ts), L.ptr(tp), N, h, w, P, C.c_double(min_mass), o["mass"].ptr(), o["centre"].ptr(), o["valid"].ptr(),
                              o["hard"].ptr() if pred is not None else None, o["invalid"].ptr() if pred is not None else None,
                              o["scratch"].ptr(), L.stream())
    torch.cuda.synchronize(dev)
    return rc, o


def _check_moments(L, dev, soft, pred, min_mass):
    N, h, w, P = soft.shape
    want = R.part_moments(soft, pred, min_mass)
    rc, o = _moments(L, dev, soft, pred, min_mass)
    assert rc == 0, L.load().ups_last_error().decode()
    for name, g in o.items():
        assert g.intact(), "wrote outside " + name
    assert not (o["scratch"].view == FSENT).any(), "a scratch element was left unwritten"
    mass, centre, valid = o["mass"].numpy().reshape(N, P), o["centre"].numpy().reshape(N, P, 2), o["valid"].numpy().reshape(N, P)
    assert not np.isnan(mass).any() and not np.isnan(centre).any() and not (valid == BFILL).any(), "an output was not written completely"
    # the float sums against an independently ordered sum: the issue's bound, (n - 1) 2^-53 sum|term|; the numerators are read back
    # as centre * mass, which adds one division's and one multiplication's rounding (2 * 2^-53 relative)
    s = soft.reshape(N, h * w, P).astype(np.float64)
    ux, uy, _, _ = R.pixel_units(h, w)
    ind = np.stack([s.sum(1), (s * ux[None, :, None]).sum(1), (s * uy[None, :, None]).sum(1)], axis=-1)
    bound = R.reordered_sum_bound(h * w, want["terms"])
    print("moments", soft.shape, "mass max |diff| / bound", (np.abs(mass - ind[..., 0]) / np.maximum(bound[..., 0], 1e-300)).max())
    assert (np.abs(mass - ind[..., 0]) <= bound[..., 0]).all()
    ok = valid != 0
    for c in (0, 1):
        num = centre[..., c] * mass
        assert (np.abs(num - ind[..., 1 + c])[ok] <= (bound[..., 1 + c] + 2.0 ** -51 * np.abs(ind[..., 1 + c]))[ok]).all()
    # and the restatement's order gives the kernel's bits
    assert np.array_equal(valid, want["valid"])
    assert np.array_equal(_bits(mass), _bits(want["mass"])), "mass differs in bits"
    assert np.array_equal(_bits(centre), _bits(want["centre"])), "centre differs in bits"
    assert (centre[~ok] == 0).all()
    if pred is not None:
        assert np.array_equal(o["hard"].numpy().reshape(N, P, 3), want["hard"]) and int(o["invalid"].numpy()[0]) == want["invalid"]
    else:
        assert bool((o["hard"].view == 0).all()) and int(o["invalid"].numpy()[0]) == 0
    rc, o2 = _moments(L, dev, soft, pred, min_mass)
    assert rc == 0 and _same(o, o2), "two calls differ"
    return want, ind


@pytest.mark.parametrize("P", [1, 3, 10, 32])
@pytest.mark.parametrize("hw", [(16, 16), (5, 51), (1, 257), (12, 12)], ids=lambda s: "x".join(map(str, s)))
def test_moments_random_input(hw, P, dev):
    L, _, _ = _mods()
    _geometry(L)
    h, w = hw
    rng = np.random.RandomState(h * 1000 + w + P)
    soft = rng.rand(3, h, w, P).astype(np.float32) ** 4
    soft /= soft.sum(-1, keepdims=True)
    pred = soft.argmax(-1).astype(np.int64)
    pred[0].reshape(-1)[0], pred[2].reshape(-1)[-1], pred[1].reshape(-1)[h * w // 2] = -1, P, 2 ** 40      # out of range
    soft[1, :, :, P - 1] = 0
    soft[1, 0, 0, P - 1] = 0.25                              # a part whose mass is below min_mass
    want, _ = _check_moments(L, dev, soft, pred, 0.5)
    assert want["invalid"] == 3 and want["valid"][1, P - 1] == 0 and want["mass"][1, P - 1] == 0.25
    assert want["valid"].sum() >= 1
    _check_moments(L, dev, soft, None, 0.0)                  # no arg-max map: hard and invalid are not touched


@pytest.mark.parametrize("P", [1, 3, 10, 32])
@pytest.mark.parametrize("hw", [(16, 16), (4, 128), (1, 256), (2, 64)], ids=lambda s: "x".join(map(str, s)))
def test_moments_lattice_input_is_exact(hw, P, dev):
    """Soft values multiples of 2^-8 and power-of-two sizes: every product and every partial sum is exact, so the kernel, the
    restatement and a sum in any other order agree in bits."""
    L, _, _ = _mods()
    h, w = hw
    rng = np.random.RandomState(h * 1000 + w + P)
    soft = (rng.randint(0, 257, size=(3, h, w, P)) / 256.0).astype(np.float32)
    soft[2, :, :, 0] = 0                                     # mass 0: not valid, also at min_mass 0
    pred = rng.randint(0, P, size=(3, h, w)).astype(np.int64)
    want, ind = _check_moments(L, dev, soft, pred, 0.0)
    assert np.array_equal(want["sums"], ind), "the lattice sums are exact in any order"      # (values: a zero sum's sign is the order's)
    assert want["valid"][2, 0] == 0 and (want["centre"][2, 0] == 0).all()
    assert (want["hard"][..., 0].sum(-1) == h * w).all()


def test_moments_refusals_launch_nothing(dev):
    L, _, _ = _mods()
    lib = L.load()
    N, h, w, P = 2, 5, 7, 3
    soft = _to(dev, np.random.RandomState(0).rand(N, h, w, 40).astype(np.float32))
    pred = torch.zeros((N, h, w), dtype=torch.int64, device=dev)
    o = {"mass": _Guarded(dev, N * 40, torch.float64, float("nan")), "centre": _Guarded(dev, N * 80, torch.float64, float("nan")),
         "valid": _Guarded(dev, N * 40, torch.uint8, BFILL), "hard": _Guarded(dev, N * 120, torch.int32, IFILL),
         "invalid": _Guarded(dev, 1, torch.int32, IFILL), "scratch": _Guarded(dev, 4096, torch.float64, FSENT)}
    full = dict(soft=L.ptr(soft), pred=L.ptr(pred), N=N, h=h, w=w, P=P, min_mass=0.5, mass=o["mass"].ptr(), centre=o["centre"].ptr(),
                valid=o["valid"].ptr(), hard=o["hard"].ptr(), invalid=o["invalid"].ptr(), scratch=o["scratch"].ptr())

    def call(**kw):
        a = dict(full, **kw)
        return lib.ups_part_moments(a["soft"], a["pred"], a["N"], a["h"], a["w"], a["P"], C.c_double(a["min_mass"]), a["mass"], a["centre"],
                                    a["valid"], a["hard"], a["invalid"], a["scratch"], L.stream())
    assert call(P=33) == E_UNSUPPORTED and b"P <= 32" in lib.ups_last_error()
    for kw in ({"soft": None}, {"mass": None}, {"centre": None}, {"valid": None}, {"scratch": None}, {"hard": None}, {"invalid": None},
               {"N": 0}, {"h": 0}, {"w": 0}, {"P": 0}, {"N": -1}, {"min_mass": float("nan")}, {"h": 1024, "w": 1025}, {"h": 1, "w": 1 << 17}):
        assert call(**kw) == E_ARG, kw
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(o["mass"].view).all()) and bool(torch.isnan(o["centre"].view).all()) and bool((o["valid"].view == BFILL).all())
    assert bool((o["hard"].view == IFILL).all()) and bool((o["invalid"].view == IFILL).all()) and bool((o["scratch"].view == FSENT).all())
    assert all(g.intact() for g in o.values())
    # the complete call is accepted, and `hard` / `invalid` are added to
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert int(o["invalid"].numpy()[0]) == IFILL and int(o["hard"].numpy()[0]) == IFILL + h * w and all(g.intact() for g in o.values())


def test_part_moments_through_ops(dev):
    L, ops, _ = _mods()
    rng = np.random.RandomState(5)
    soft = rng.rand(2, 12, 12, 3).astype(np.float32)
    pred = soft.argmax(-1).astype(np.int64)
    want = R.part_moments(soft, pred, 2.0)
    r = ops.part_moments(_to(dev, soft), _to(dev, pred), min_mass=2.0)
    assert sorted(r) == ["centre", "hard", "invalid", "mass", "valid"]
    assert np.array_equal(_bits(r["centre"].cpu().numpy()), _bits(want["centre"])) and np.array_equal(r["hard"].cpu().numpy(), want["hard"])
    assert np.array_equal(r["valid"].cpu().numpy(), want["valid"]) and r["centre"].dtype == torch.float64 and int(r["invalid"]) == 0
    assert sorted(ops.part_moments(_to(dev, soft))) == ["centre", "mass", "valid"]
    with pytest.raises(L.UpsError):
        ops.part_moments(_to(dev, soft).double())
    with pytest.raises(L.UpsError):
        ops.part_moments(_to(dev, soft), _to(dev, pred[:1]))
    with pytest.raises(L.UpsError):
        ops.part_moments(torch.zeros((1, 4, 4, 33), device=dev))


# ---------------------------------------------------------------------------------------------- ups_landmark_gram
def _gram(L, dev, feat, target, vis):
    N, D, K = feat.shape[0], feat.shape[1] + 1, vis.shape[1]
    lib = L.load()
    E = D * D + 2 * D + 1
    nbytes = lib.ups_landmark_gram_scratch_bytes(N, D, K)
    assert nbytes == (-(-N // CH)) * K * E * 8
    o = {"G": _Guarded(dev, K * D * D, torch.float64, float("nan")), "R": _Guarded(dev, K * D * 2, torch.float64, float("nan")),
         "cnt": _Guarded(dev, K, torch.int32, IFILL), "scratch": _Guarded(dev, nbytes // 8, torch.float64, FSENT)}
    tf, tt, tv = _to(dev, feat), _to(dev, target), _to(dev, vis)        # (named: a temporary's memory is the next one's)
    rc = lib.ups_landmark_gram(L.ptr(tf), L.ptr(tt), L.ptr(tv), N, D, K, o["G"].ptr(), o["R"].ptr(), o["cnt"].ptr(), o["scratch"].ptr(),
                               L.stream())
    torch.cuda.synchronize(dev)
    return rc, o


def _check_gram(L, dev, feat, target, vis):
    N, D, K = feat.shape[0], feat.shape[1] + 1, vis.shape[1]
    wG, wR, wc = R.gram(feat, target, vis)
    rc, o = _gram(L, dev, feat, target, vis)
    assert rc == 0, L.load().ups_last_error().decode()
    for name, g in o.items():
        assert g.intact(), "wrote outside " + name
    assert not (o["scratch"].view == FSENT).any(), "a scratch element was left unwritten"
    G, Rr, cnt = o["G"].numpy().reshape(K, D, D), o["R"].numpy().reshape(K, D, 2), o["cnt"].numpy()
    assert not np.isnan(G).any() and not np.isnan(Rr).any() and not (cnt == IFILL).any(), "an output was not written completely"
    assert np.array_equal(cnt, wc)
    assert np.array_equal(_bits(G), _bits(wG)), "G differs in bits"
    assert np.array_equal(_bits(Rr), _bits(wR)), "R differs in bits"
    assert np.array_equal(_bits(G), _bits(G.transpose(0, 2, 1))), "G is not symmetric in bits"
    rc, o2 = _gram(L, dev, feat, target, vis)
    assert rc == 0 and _same(o, o2), "two calls differ"
    return G, Rr, cnt


def _gram_inputs(rng, N, P, K, lattice):
    if lattice:
        feat = rng.randint(-64, 65, size=(N, 2 * P)) / 64.0
        target = rng.randint(-64, 65, size=(N, K, 2)) / 64.0
    else:
        feat, target = rng.rand(N, 2 * P) * 2 - 1, rng.rand(N, K, 2) * 2 - 1
    vis = (rng.rand(N, K) < 0.7).astype(np.uint8)
    if K > 1:
        vis[:, 1] = 0                                        # a keypoint that is never visible
    if N == 1:
        vis[0, 0] = 1
    target[vis == 0] = np.nan                                # an invisible target is never read
    return feat, target, vis


GRAM_CASES = [(N, K, P) for N in (1, CH - 1, CH, CH + 1, 2 * CH + 3) for K in (1, 4) for P in (1, 3)] + [(CH + 1, 32, 32)]


@pytest.mark.parametrize("data", ["float", "lattice"])
@pytest.mark.parametrize("case", GRAM_CASES, ids=["x".join(map(str, c)) for c in GRAM_CASES])
def test_gram_equals_the_restatement(case, data, dev):
    L, _, _ = _mods()
    _geometry(L)
    N, K, P = case
    rng = np.random.RandomState(sum(case))
    feat, target, vis = _gram_inputs(rng, N, P, K, data == "lattice")
    G, Rr, cnt = _check_gram(L, dev, feat, target, vis)
    if K > 1:
        assert cnt[1] == 0 and (G[1] == 0).all() and (Rr[1] == 0).all()
    else:                                                    # the only keypoint never visible: zeros, and nothing is read
        G0, R0, c0 = _check_gram(L, dev, feat, np.full_like(target, np.nan), np.zeros_like(vis))
        assert c0[0] == 0 and (G0 == 0).all() and (R0 == 0).all()
    if data == "lattice":                                    # multiples of 2^-12 below 2^53: exact in any order
        f1 = R.with_one(feat)
        for k in range(K):
            m = vis[:, k] != 0
            assert np.array_equal(G[k], np.einsum("na,nb->ab", f1[m], f1[m]))
            assert np.array_equal(Rr[k], np.einsum("na,nc->ac", f1[m], np.where(m[:, None], target[:, k], 0.0)[m]))


# ---------------------------------------------------------------------------------------------- ups_landmark_solve
def _solve(L, dev, G, Rr, cnt, lam, singular_before=5):
    K, D = G.shape[0], G.shape[1]
    o = {"W": _Guarded(dev, K * D * 2, torch.float64, float("nan")), "n_singular": _Guarded(dev, 1, torch.int32, singular_before)}
    tG, tR, tc = _to(dev, G), _to(dev, Rr), _to(dev, cnt.astype(np.int32))
    rc = L.load().ups_landmark_solve(L.ptr(tG), L.ptr(tR), L.ptr(tc), D, K, C.c_double(lam), o["W"].ptr(), o["n_singular"].ptr(), L.stream())
    torch.cuda.synchronize(dev)
    return rc, o


def _check_solve(L, dev, G, Rr, cnt, lam):
    K, D = G.shape[0], G.shape[1]
    wW, bad = R.solve(G, Rr, cnt, lam)
    rc, o = _solve(L, dev, G, Rr, cnt, lam)
    assert rc == 0, L.load().ups_last_error().decode()
    assert o["W"].intact() and o["n_singular"].intact()
    W = o["W"].numpy().reshape(K, D, 2)
    assert not np.isnan(W).any(), "W was not written completely"
    assert int(o["n_singular"].numpy()[0]) == 5 + int(bad.sum())                  # added to, never reset
    assert np.array_equal(_bits(W), _bits(wW)), "W differs in bits"
    rc, o2 = _solve(L, dev, G, Rr, cnt, lam)
    assert rc == 0 and _same(o, o2), "two calls differ"
    return W, bad


@pytest.mark.parametrize("D", [3, 7, 65])
def test_solve_equals_the_restatement(D, dev):
    L, _, _ = _mods()
    rng = np.random.RandomState(D)
    P, N, K = (D - 1) // 2, 3 * D + 5, 4
    feat, target, vis = _gram_inputs(rng, N, P, K, False)
    G, Rr, cnt = R.gram(feat, target, vis)
    W, bad = _check_solve(L, dev, G, Rr, cnt, 1e-6)
    assert bad.tolist() == [False, True, False, False] and (W[1] == 0).all()     # cnt = 0: W_k = 0, counted
    A = G[0] + 1e-6 * np.diag([1.0] * (D - 1) + [0.0])
    assert np.abs(A @ W[0] - Rr[0]).max() <= 1e-9 * max(1.0, np.abs(Rr[0]).max()) * D
    W0, bad0 = _check_solve(L, dev, G, Rr, cnt, 0.0)
    assert bad0.tolist() == [False, True, False, False]
    # an always-absent part: a zero column.  Without the ridge its pivot is 0 (W_k = 0, counted), with it the system is solved
    feat[:, 0] = 0.0
    G, Rr, cnt = R.gram(feat, target, vis)
    Wz, badz = _check_solve(L, dev, G, Rr, cnt, 0.0)
    assert badz.all() and (Wz == 0).all()
    rc, one = _solve(L, dev, G[:1], Rr[:1], cnt[:1], 0.0, singular_before=0)
    assert rc == 0 and int(one["n_singular"].numpy()[0]) == 1 and (one["W"].numpy() == 0).all()
    Wr, badr = _check_solve(L, dev, G, Rr, cnt, 1e-6)
    assert badr.tolist() == [False, True, False, False] and (Wr[0, 0] == 0).all() and np.abs(Wr[0]).max() > 0


def test_solve_and_predict_refusals_launch_nothing(dev):
    L, _, _ = _mods()
    lib = L.load()
    K, D, N = 2, 3, 4
    G, Rr = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous(), torch.ones((K, D, 2), dtype=torch.float64, device=dev)
    cnt = torch.ones(K, dtype=torch.int32, device=dev)
    W, ns = _Guarded(dev, 40 * 70 * 2, torch.float64, float("nan")), _Guarded(dev, 1, torch.int32, 0)
    s = L.stream()

    def solve(G_=L.ptr(G), R_=L.ptr(Rr), c_=L.ptr(cnt), D_=D, K_=K, lam=0.0, W_=W.ptr(), n_=ns.ptr()):
        return lib.ups_landmark_solve(G_, R_, c_, D_, K_, C.c_double(lam), W_, n_, s)
    assert solve(D_=66) == E_UNSUPPORTED and solve(K_=33) == E_UNSUPPORTED
    for kw in ({"G_": None}, {"R_": None}, {"c_": None}, {"W_": None}, {"n_": None}, {"D_": 0}, {"K_": 0}, {"lam": -1.0},
               {"lam": float("nan")}, {"lam": float("inf")}):
        assert solve(**kw) == E_ARG, kw
    feat, tgt = torch.zeros((N, D - 1), dtype=torch.float64, device=dev), torch.zeros((N, K, 2), dtype=torch.float64, device=dev)
    vis = torch.ones((N, K), dtype=torch.uint8, device=dev)
    pred, d2 = _Guarded(dev, N * 40 * 2, torch.float64, float("nan")), _Guarded(dev, N * 40, torch.float64, float("nan"))
    Wp = torch.ones((K, D, 2), dtype=torch.float64, device=dev)

    def predict(f=L.ptr(feat), W_=L.ptr(Wp), N_=N, D_=D, K_=K, t=L.ptr(tgt), v=L.ptr(vis), p=pred.ptr(), d=d2.ptr()):
        return lib.ups_landmark_predict(f, W_, N_, D_, K_, t, v, p, d, s)
    assert predict(D_=66) == E_UNSUPPORTED and predict(K_=33) == E_UNSUPPORTED
    for kw in ({"f": None}, {"W_": None}, {"p": None}, {"N_": 0}, {"D_": 0}, {"K_": 0}, {"t": None}, {"v": None}, {"d": None},
               {"t": None, "v": None}, {"N_": 2 ** 30, "K_": 32}):
        assert predict(**kw) == E_ARG, kw
    Gg, Rg = _Guarded(dev, 4096, torch.float64, float("nan")), _Guarded(dev, 4096, torch.float64, float("nan"))
    cg, sg = _Guarded(dev, 40, torch.int32, IFILL), _Guarded(dev, 4096, torch.float64, FSENT)

    def gram(f=L.ptr(feat), t=L.ptr(tgt), v=L.ptr(vis), N_=N, D_=D, K_=K, G_=Gg.ptr(), R_=Rg.ptr(), c_=cg.ptr(), s_=sg.ptr()):
        return lib.ups_landmark_gram(f, t, v, N_, D_, K_, G_, R_, c_, s_, s)
    assert gram(D_=66) == E_UNSUPPORTED and gram(K_=33) == E_UNSUPPORTED
    for kw in ({"f": None}, {"t": None}, {"v": None}, {"G_": None}, {"R_": None}, {"c_": None}, {"s_": None}, {"N_": 0}, {"D_": 0}, {"K_": 0}):
        assert gram(**kw) == E_ARG, kw
    torch.cuda.synchronize(dev)
    for g in (W, pred, d2, Gg, Rg):
        assert bool(torch.isnan(g.view).all()) and g.intact()
    assert int(ns.numpy()[0]) == 0 and bool((cg.view == IFILL).all()) and bool((sg.view == FSENT).all()) and cg.intact() and sg.intact()
    assert solve() == 0 and predict() == 0 and gram() == 0 and predict(t=None, v=None, d=None) == 0
    torch.cuda.synchronize(dev)
    assert (W.numpy()[:K * D * 2] == 1).all() and (pred.numpy()[:N * K * 2] == 1).all() and (d2.numpy()[:N * K] == 2).all()


# ---------------------------------------------------------------------------------------------- ups_landmark_predict
@pytest.mark.parametrize("case", [(1, 1, 1), (CH + 3, 4, 3), (300, 32, 32), (257, 15, 10)], ids=lambda c: "x".join(map(str, c)))
def test_predict_equals_the_restatement(case, dev):
    L, ops, _ = _mods()
    N, K, P = case
    D = 2 * P + 1
    rng = np.random.RandomState(sum(case))
    feat, target, vis = _gram_inputs(rng, N, P, K, False)
    W = rng.standard_normal((K, D, 2))
    want_p, want_d = R.predict(feat, W, target, vis)
    lib = L.load()
    outs = []
    tf, tW, tt, tv = _to(dev, feat), _to(dev, W), _to(dev, target), _to(dev, vis)
    for _ in range(2):
        pred, d2 = _Guarded(dev, N * K * 2, torch.float64, float("nan")), _Guarded(dev, N * K, torch.float64, float("nan"))
        rc = lib.ups_landmark_predict(L.ptr(tf), L.ptr(tW), N, D, K, L.ptr(tt), L.ptr(tv), pred.ptr(), d2.ptr(), L.stream())
        torch.cuda.synchronize(dev)
        assert rc == 0 and pred.intact() and d2.intact()
        outs.append((pred.numpy().reshape(N, K, 2), d2.numpy().reshape(N, K)))
    got_p, got_d = outs[0]
    assert not np.isnan(got_p).any() and not np.isnan(got_d).any(), "an output was not written completely"
    assert np.array_equal(_bits(got_p), _bits(want_p)) and np.array_equal(_bits(got_d), _bits(want_d))
    assert (got_d[vis == 0] == -1).all() and (got_d[vis != 0] >= 0).all()
    assert np.array_equal(_bits(outs[1][0]), _bits(got_p)) and np.array_equal(_bits(outs[1][1]), _bits(got_d))
    p_only, none = ops.landmark_predict(tf, tW)
    assert none is None and np.array_equal(_bits(p_only.cpu().numpy()), _bits(want_p))


def test_regressor_fit_predict_evaluate(dev):
    L, ops, LM = _mods()
    rng = np.random.RandomState(17)
    N, P, K = 2 * CH + 9, 3, 4
    centre = rng.rand(N, P, 2) * 2 - 1
    valid = (rng.rand(N, P) < 0.9).astype(np.uint8)
    target, vis = rng.rand(N, K, 2) * 2 - 1, (rng.rand(N, K) < 0.7).astype(np.uint8)
    vis[:, 2] = 0
    feat = R.features(centre, valid)
    assert (feat.reshape(N, P, 2)[valid == 0] == 0).all()
    wG, wR, wc = R.gram(feat, target, vis)
    wW, bad = R.solve(wG, wR, wc, 1e-6)
    reg = LM.LandmarkRegressor(device=dev).fit(centre, valid, target, vis, ridge=1e-6)
    assert np.array_equal(_bits(reg.W), _bits(wW)) and np.array_equal(reg.cnt, wc) and reg.n_singular == int(bad.sum()) == 1
    assert np.array_equal(_bits(reg.predict(centre[:5], valid[:5])), _bits(R.predict(feat[:5], wW)[0]))
    res = reg.evaluate(centre, valid, target, vis, pck=(0.05, 0.1, 0.5))
    want = R.metrics(R.predict(feat, wW, target, vis)[1], (0.05, 0.1, 0.5))
    assert res["mean_error"] == want["mean_error"] and res["mean_error_instances"] == want["mean_error_instances"] and res["n_singular"] == 1
    assert [r["n_visible"] for r in res["keypoints"]] == want["n_visible"].tolist() and res["keypoints"][2]["mean_error"] is None
    for k in (0, 1, 3):
        assert res["keypoints"][k]["mean_error"] == want["mean_error_k"][k] and res["keypoints"][k]["pck@0.5"] == want["pck@0.5"][k]
    G, Rr, cnt = ops.landmark_gram(_to(dev, feat), _to(dev, target), _to(dev, vis))
    assert np.array_equal(_bits(G.cpu().numpy()), _bits(wG)) and cnt.dtype == torch.int32
    W, ns = ops.landmark_solve(G, Rr, cnt, 1e-6)
    assert np.array_equal(_bits(W.cpu().numpy()), _bits(wW)) and int(ns) == 1
    with pytest.raises(L.UpsError):
        ops.landmark_gram(_to(dev, feat).float(), _to(dev, target), _to(dev, vis))
    with pytest.raises(L.UpsError):
        ops.landmark_solve(G, Rr[:, :2], cnt, 1e-6)
    with pytest.raises(ValueError):
        reg.predict(centre[:, :2], valid[:, :2])
    with pytest.raises(ValueError):
        LM.LandmarkRegressor(device=dev).predict(centre, valid)


# ---------------------------------------------------------------------------------------------- the model and the runner
def _decode(path, S):
    from PIL import Image
    im = Image.open(path).convert("RGB")
    return np.asarray(im.resize((S, S), Image.BILINEAR), dtype=np.uint8), (im.size[1], im.size[0])


def test_runner_landmarks_end_to_end(dev, tmp_path):
    import yaml
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import landmarks as LM, runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    S, P, K = cfg["spatial_size"], cfg["n_parts"], 3
    data_root = tmp_path / "images"
    rng = np.random.RandomState(7)
    files = ["a/{}.png".format(i) for i in range(7)] + ["b/c/{}.png".format(i) for i in range(5)]
    sizes = [(19 + i, 23 + 2 * (i % 4)) for i in range(len(files))]                  # (h, w): unequal
    rows = []
    for rel, (h, w) in zip(files, sizes):
        os.makedirs(os.path.dirname(str(data_root / rel)), exist_ok=True)
        small = rng.randint(0, 256, size=(4, 5, 3)).astype(np.uint8)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(str(data_root / rel))
        xy = rng.rand(K, 2) * [w - 1, h - 1]
        v = (rng.rand(K) < 0.8).astype(int)
        rows.append(rel + "," + ",".join("{!r},{!r},{}".format(float(x), float(y), int(f)) for (x, y), f in zip(xy, v)))
    fit_csv, test_csv = tmp_path / "fit.csv", tmp_path / "test.csv"
    fit_csv.write_text("\n".join(rows[:7]) + "\n")
    test_csv.write_text("\n".join(rows[7:]) + "\n")
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(data_root), "landmark_fit_csv": str(fit_csv),
                "landmark_test_csv": str(test_csv), "landmark_pck": [0.1, 0.25], "landmark_names": ["beak", "crown", "tail"]})
    ypath = tmp_path / "landmarks.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    res = runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "run")])
    odir = str(tmp_path / "run" / "landmarks" / "0")
    assert res["dir"] == odir
    assert sorted(os.listdir(odir)) == ["landmarks.csv", "predictions.npz", "regressor.npz", "summary.yml"]
    model = res["model"]
    # part_centres equals the restatement fed with segment_soft's output: both sources, a ragged last pass
    views, src_sizes = zip(*[_decode(str(data_root / rel), S) for rel in files])
    assert list(src_sizes) == sizes
    v = torch.from_numpy(np.stack(views).astype(np.float32) / 127.5 - 1.0)
    hard, soft = model.segment_soft(v[:7])
    want = R.part_moments(soft.cpu().numpy(), hard.cpu().numpy(), 0.005 * S * S)
    got = model.part_centres(v[:7])
    assert sorted(got) == ["centre", "mass", "out_parts_hard", "valid"] and got["centre"].device.type == "cuda"
    assert tuple(got["centre"].shape) == (7, P, 2) and got["centre"].dtype == torch.float64 and got["valid"].dtype == torch.uint8
    assert np.array_equal(_bits(got["centre"].cpu().numpy()), _bits(want["centre"])) and torch.equal(got["out_parts_hard"], hard)
    assert np.array_equal(_bits(got["mass"].cpu().numpy()), _bits(want["mass"])) and np.array_equal(got["valid"].cpu().numpy(), want["valid"])
    hc, hm, hv = R.hard_centres(want["hard"], S, S, int(np.ceil(0.2 * S * S)))
    goth = model.part_centres(v[:7], source="hard", min_part_area=0.2)
    assert np.array_equal(_bits(goth["centre"].cpu().numpy()), _bits(hc)) and np.array_equal(goth["valid"].cpu().numpy(), hv)
    assert np.array_equal(goth["mass"].cpu().numpy(), hm) and (hm.sum(-1) == S * S).all()
    with pytest.raises(Exception):
        model.part_centres(v[:2], source="mean")
    # the files against the restatement of the whole route
    fit_c, fit_v = want["centre"], want["valid"]
    hard_t, soft_t = model.segment_soft(v[7:])
    test_m = R.part_moments(soft_t.cpu().numpy(), None, 0.005 * S * S)
    _, fit_xy, fit_vis = LM.read_landmark_csv(str(fit_csv))
    _, test_xy, test_vis = LM.read_landmark_csv(str(test_csv))
    fit_t, test_t = LM.normalise_targets(fit_xy, sizes[:7]), LM.normalise_targets(test_xy, sizes[7:])
    assert np.abs(fit_t[fit_vis != 0]).max() < 1
    G, Rr, cnt = R.gram(R.features(fit_c, fit_v), fit_t, fit_vis)
    W, bad = R.solve(G, Rr, cnt, 1e-6)
    pred, d2 = R.predict(R.features(test_m["centre"], test_m["valid"]), W, test_t, test_vis)
    reg = LM.LandmarkRegressor.load(os.path.join(odir, "regressor.npz"))
    assert np.array_equal(_bits(reg.W), _bits(W)) and np.array_equal(reg.cnt, cnt) and reg.n_singular == int(bad.sum())
    assert reg.options == {"ridge": 1e-6, "source": "soft", "min_part_area": 0.005, "pck": [0.1, 0.25]}
    m = R.metrics(d2, [0.1, 0.25])
    summary = yaml.safe_load(open(os.path.join(odir, "summary.yml")))
    assert summary == res["summary"]
    assert summary["split"] == "test" and summary["error"] == "test error" and (summary["n_fit"], summary["n_test"]) == (7, 5)
    assert summary["mean_error"] == m["mean_error"] and summary["mean_error_instances"] == m["mean_error_instances"]
    assert summary["n_singular"] == int(bad.sum()) and summary["n_visible"] == int(m["n_visible"].sum()) and summary["n_keypoints"] == K
    for k in range(K):
        row = summary["keypoints"][k]
        assert row["name"] == ["beak", "crown", "tail"][k] and row["n_visible"] == int(m["n_visible"][k])
        if row["n_visible"]:
            assert row["mean_error"] == m["mean_error_k"][k] and row["pck@0.1"] == m["pck@0.1"][k] and row["pck@0.25"] == m["pck@0.25"][k]
    dev_reg = LM.LandmarkRegressor.load(os.path.join(odir, "regressor.npz"), device=dev)
    again = dev_reg.evaluate(test_m["centre"], test_m["valid"], test_t, test_vis, pck=[0.1, 0.25])
    assert again["mean_error"] == summary["mean_error"] and again["keypoints"] == [
        {c: r[c] for c in r if c != "name"} for r in summary["keypoints"]]
    lines = open(os.path.join(odir, "landmarks.csv")).read().splitlines()
    assert lines[0] == "keypoint,name,n_fit,n_visible,mean_error,pck@0.1,pck@0.25" and len(lines) == 1 + K
    assert lines[1].split(",")[:4] == ["0", "beak", str(int(cnt[0])), str(int(m["n_visible"][0]))]
    with np.load(os.path.join(odir, "predictions.npz")) as z:
        assert sorted(z.files) == ["centre", "files", "pred", "valid"] and z["files"].tolist() == files[7:]
        assert np.array_equal(_bits(z["centre"]), _bits(test_m["centre"])) and np.array_equal(z["valid"], test_m["valid"])
        assert np.array_equal(_bits(z["pred"]), _bits(LM.to_source_pixels(pred, sizes[7:]))) and z["pred"].shape == (5, K, 2)
    # a second run: the same bytes
    runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "again")])
    for name in ("regressor.npz", "landmarks.csv", "summary.yml", "predictions.npz"):
        assert (open(os.path.join(odir, name), "rb").read() ==
                open(str(tmp_path / "again" / "landmarks" / "0" / name), "rb").read()), name
    # no test csv: evaluated on the fit split, and the summary says so
    del cfg["landmark_test_csv"]
    cfg.update({"landmark_source": "hard"})
    del cfg["landmark_names"]
    ypath.write_text(yaml.safe_dump(cfg))
    res = runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "run3")])
    assert res["summary"]["split"] == "fit" and res["summary"]["error"] == "fit error" and res["summary"]["n_test"] == 7
    assert res["summary"]["keypoints"][0]["name"] == "keypoint_0" and res["summary"]["source"] == "hard"
    # a wrong key raises before the model is built
    ypath.write_text(yaml.safe_dump(dict(cfg, landmark_rigde=1e-3, model="no.such.Model")))
    with pytest.raises(ValueError, match="landmark_rigde"):
        runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "run4")])
    # the two files disagree about K
    test_csv.write_text("a/0.png,1,2,1\n")
    ypath.write_text(yaml.safe_dump(dict(cfg, landmark_test_csv=str(test_csv))))
    with pytest.raises(ValueError, match="keypoints"):
        runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "run5")])
    # a missing image raises; nothing synthetic stands in, nothing is written
    fit_csv.write_text(rows[0] + "\nnot/there.png" + rows[1][len(files[1]):] + "\n")
    ypath.write_text(yaml.safe_dump(cfg))
    with pytest.raises(FileNotFoundError):
        runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "run6")])
    assert not os.path.exists(str(tmp_path / "run6" / "landmarks"))
    cfg["landmark_fit_csv"] = str(tmp_path / "nope.csv")
    ypath.write_text(yaml.safe_dump(cfg))
    with pytest.raises(FileNotFoundError):
        runner.main(["--landmarks", str(ypath), "-p", str(tmp_path / "run7")])
