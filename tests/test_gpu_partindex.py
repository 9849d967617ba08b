"""GPU tests of the part-appearance index: ups_part_knn and ups_part_kmeans_step (csrc/partindex.hip, through the C ABI) against the
NumPy float64 restatement of partindex_ref.py -- indices, labels and counts with ==, distances bit for bit, the reordered float sums
within (n - 1) 2^-53 sum|term| (exactly on the lattice bank) -- then PartIndex.kmeans end to end, TrainModel.encode_parts and the
runner's --index.  Every output and scratch buffer sits between sentinel guard bands."""
import copy
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import partindex_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
ISENT = -0x5A5A5A5B
FSENT = -7.0e77
IFILL = 0x01234567              # what an int32 output holds before the call: "written completely" means none is left
VGG_W = (8, 8, 16, 16, 16)
E_ARG, E_UNSUPPORTED = -1, -2
T, CH = 64, 256                 # = ups_part_knn_tile(), ups_part_kmeans_chunk() (asserted below)


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, ops, partindex
    return lib, ops, partindex


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
        self.sent = ISENT if dtype == torch.int32 else FSENT
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


def _dev_bank(dev, feat, valid):
    return torch.from_numpy(np.ascontiguousarray(feat)).to(dev), torch.from_numpy(np.ascontiguousarray(valid)).to(dev)


def _geometry(L):
    h = L.load()
    assert (h.ups_part_knn_tile(), h.ups_part_kmeans_chunk()) == (T, CH)


# ---------------------------------------------------------------------------------------------- ups_part_knn
def _knn(L, dev, q, qv, g, gv, K, exclude):
    tq, tqv = _dev_bank(dev, q, qv)
    tg, tgv = (tq, tqv) if g is q else _dev_bank(dev, g, gv)
    Nq, P, A = q.shape
    idx = _Guarded(dev, Nq * P * K, torch.int32, IFILL)
    dist = _Guarded(dev, Nq * P * K, torch.float64, float("nan"))
    rc = L.load().ups_part_knn(L.ptr(tq), L.ptr(tqv), Nq, L.ptr(tg), L.ptr(tgv), g.shape[0], P, A, K, int(exclude), idx.ptr(), dist.ptr(),
                               L.stream())
    torch.cuda.synchronize(dev)
    return rc, idx, dist


def _check_knn(L, dev, q, qv, g, gv, K, exclude):
    want_i, want_d = R.knn(q, qv, g, gv, K, exclude)
    rc, idx, dist = _knn(L, dev, q, qv, g, gv, K, exclude)
    assert rc == 0, L.load().ups_last_error().decode()
    got_i, got_d = idx.numpy().reshape(want_i.shape), dist.numpy().reshape(want_d.shape)
    assert idx.intact() and dist.intact(), "wrote outside idx / dist"
    assert not (got_i == IFILL).any() and not np.isnan(got_d).any(), "an output was not written completely"
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_d), _bits(want_d)), "dist differs in bits"
    rc, idx2, dist2 = _knn(L, dev, q, qv, g, gv, K, exclude)
    assert rc == 0 and torch.equal(idx2.view, idx.view) and torch.equal(dist2.view.view(torch.int64), dist.view.view(torch.int64))
    return want_i, want_d


#            Nq          Ng         P   A   K
KNN_CASES = [(1,         1,         1,  1,  1),
             (T - 1,     T + 1,     3,  5,  8),
             (T,         T,         1,  8,  32),
             (T + 1,     2 * T + 1, 10, 64, 8),
             (2 * T + 1, T - 1,     25, 65, 1),
             (5,         3 * T,     3,  8,  32)]


@pytest.mark.parametrize("bank", ["float", "lattice"])
@pytest.mark.parametrize("case", KNN_CASES, ids=["x".join(map(str, c)) for c in KNN_CASES])
def test_knn_query_bank_against_another_gallery(case, bank, dev):
    L, _, _ = _mods()
    _geometry(L)
    Nq, Ng, P, A, K = case
    rng = np.random.RandomState(sum(case))
    gen = (lambda n: R.float_bank(rng, n, P, A)) if bank == "float" else (lambda n: R.lattice_bank(rng, n, P, A, 3))
    (q, qv), (g, gv) = gen(Nq), gen(Ng)
    if Nq == 1:
        qv[:], gv[:] = 1, 1
    else:
        qv[0, 0] = 0                             # an invalid query
    if P >= 3:
        gv[:, 1] = 0                             # a part with no valid gallery entry at all
        gv[:, 2] = 0
        gv[:min(Ng, 5), 2] = 1                   # fewer eligible items than K (for K > 5): padding
    want_i, _ = _check_knn(L, dev, q, qv, g, gv, K, False)
    if P >= 3:
        assert (want_i[:, 1] == -1).all()
        if K > 5:
            assert (want_i[qv[:, 2] != 0, 2, 5:] == -1).all() and (want_i[qv[:, 2] != 0, 2, 4] >= 0).all()
    # the definition of exclude_same_index is on indices: with another bank it still drops gallery item n from query n's candidates
    _check_knn(L, dev, q, qv, g, gv, K, True)


@pytest.mark.parametrize("bank", ["float", "lattice"])
@pytest.mark.parametrize("shape", [(2 * T + 1, 3, 8, 8), (T + 1, 10, 64, 8), (T - 1, 2, 5, 32)], ids=lambda s: "x".join(map(str, s)))
def test_knn_self_query_with_duplicates(shape, bank, dev):
    L, _, _ = _mods()
    N, P, A, K = shape
    rng = np.random.RandomState(sum(shape))
    feat, valid = R.float_bank(rng, N, P, A) if bank == "float" else R.lattice_bank(rng, N, P, A, 3)
    third = N // 3
    feat[2 * third:3 * third] = feat[:third]     # a third of the codes are exact duplicates of another third
    with_self_i, with_self_d = _check_knn(L, dev, feat, valid, feat, valid, K, False)
    excl_i, excl_d = _check_knn(L, dev, feat, valid, feat, valid, K, True)
    # the restatement's ties are real: equal finite distances next to each other, in index order
    tie = np.isfinite(excl_d[..., 1:]) & (excl_d[..., 1:] == excl_d[..., :-1])
    if K > 1:
        assert tie.any() and (excl_i[..., 1:][tie] > excl_i[..., :-1][tie]).all()
    v = valid != 0
    n_idx = np.arange(N)[:, None]
    assert (with_self_d[..., 0][v] == 0).all() and (with_self_i[..., 0][v] <= np.broadcast_to(n_idx, v.shape)[v]).all()
    assert (excl_i != n_idx[..., None]).all()


def test_knn_through_ops_and_part_index(dev):
    L, ops, PI = _mods()
    rng = np.random.RandomState(11)
    feat, valid = R.float_bank(rng, T + 7, 3, 8)
    qf, qvalid = R.float_bank(rng, 9, 3, 8)
    index, queries = PI.PartIndex(feat, valid), PI.PartIndex(qf, qvalid)
    i0, d0 = index.neighbours(4)
    w0 = R.knn(feat, valid, feat, valid, 4, True)
    assert np.array_equal(i0, w0[0]) and np.array_equal(_bits(d0), _bits(w0[1])) and i0.dtype == np.int32
    i1, d1 = index.neighbours(4, queries)
    w1 = R.knn(qf, qvalid, feat, valid, 4, False)
    assert np.array_equal(i1, w1[0]) and np.array_equal(_bits(d1), _bits(w1[1]))
    # cosine ranking: the same kernel on the normalised bank
    ni, nd = PI.PartIndex(feat, valid, normalize=True).neighbours(4)
    nf, nv = R.normalize(feat, valid)
    wn = R.knn(nf, nv, nf, nv, 4, True)
    assert np.array_equal(ni, wn[0]) and np.array_equal(_bits(nd), _bits(wn[1]))
    tf, tv = _dev_bank(dev, feat, valid)
    with pytest.raises(L.UpsError):
        ops.part_knn(tf, tv, K=33)
    with pytest.raises(L.UpsError):
        ops.part_knn(tf, tv, tf[:, :2].contiguous(), tv[:, :2].contiguous())
    with pytest.raises(L.UpsError):
        ops.part_knn(tf.double(), tv)


# ---------------------------------------------------------------------------------------------- ups_part_kmeans_step
def _centroids(rng, feat, valid, k):
    """k centroids per part near the data (items, perturbed) -- and, for k >= 3, one far away: an empty cluster."""
    N, P, A = feat.shape
    cent = feat[rng.randint(0, N, size=(k, P)), np.arange(P)[None, :]].transpose(1, 0, 2).astype(np.float64)
    cent = cent + rng.randint(-8, 9, size=cent.shape) / 32.0
    if k >= 3:
        cent[:, 1] = 1.0e4
    return np.ascontiguousarray(cent)


def _step(L, dev, feat, valid, cent, prev, accumulate=True):
    N, P, A = feat.shape
    k = cent.shape[1]
    lib = L.load()
    tf, tv = _dev_bank(dev, feat, valid)
    tc = torch.from_numpy(cent).to(dev)
    tp = None if prev is None else torch.from_numpy(prev).to(dev)
    nbytes = lib.ups_part_kmeans_scratch_bytes(N, P, A, k)
    assert nbytes % 8 == 0 and nbytes > 0
    o = {"label": _Guarded(dev, N * P, torch.int32, IFILL), "mind": _Guarded(dev, N * P, torch.float64, float("nan")),
         "changed": _Guarded(dev, 1, torch.int32, 0), "scratch": _Guarded(dev, nbytes // 8, torch.float64, FSENT)}
    if accumulate:
        o.update(counts=_Guarded(dev, P * k, torch.int32, 0), sums=_Guarded(dev, P * k * A, torch.float64, float("nan")),
                 inertia=_Guarded(dev, P, torch.float64, float("nan")))
    rc = lib.ups_part_kmeans_step(L.ptr(tf), L.ptr(tv), N, P, A, L.ptr(tc), k, L.ptr(tp), o["label"].ptr(), o["mind"].ptr(),
                                  o["counts"].ptr() if accumulate else None, o["sums"].ptr() if accumulate else None,
                                  o["inertia"].ptr() if accumulate else None, o["changed"].ptr(), o["scratch"].ptr(), L.stream())
    torch.cuda.synchronize(dev)
    return rc, o


#               N           P   A   k
STEP_CASES = [(1,          1,  1,  1),
              (CH - 1,     3,  5,  2),
              (CH,         2,  8,  7),
              (CH + 1,     3,  64, 64),
              (2 * CH + 1, 10, 65, 7),
              (2 * CH + 1, 2,  16, 9)]


@pytest.mark.parametrize("bank", ["float", "lattice"])
@pytest.mark.parametrize("case", STEP_CASES, ids=["x".join(map(str, c)) for c in STEP_CASES])
def test_kmeans_step_equals_the_restatement(case, bank, dev):
    L, _, _ = _mods()
    _geometry(L)
    N, P, A, k = case
    rng = np.random.RandomState(sum(case))
    feat, valid = R.float_bank(rng, N, P, A) if bank == "float" else R.lattice_bank(rng, N, P, A, 3)
    if N == 1:
        valid[:] = 1
    cent = _centroids(rng, feat, valid, k)
    prev = rng.randint(-1, k, size=(N, P)).astype(np.int32)
    want = R.kmeans_step(feat, valid, cent, prev)
    if k >= 3:
        assert (want["counts"][:, 1] == 0).all(), "an empty cluster"
    rc, o = _step(L, dev, feat, valid, cent, prev)
    assert rc == 0, L.load().ups_last_error().decode()
    for name, g in o.items():
        assert g.intact(), "wrote outside " + name
    assert not (o["scratch"].view == FSENT).any(), "a scratch element was left unwritten"
    assert np.array_equal(o["label"].numpy().reshape(N, P), want["label"])
    assert np.array_equal(_bits(o["mind"].numpy().reshape(N, P)), _bits(want["mind"])), "mind differs in bits"
    assert np.array_equal(o["counts"].numpy().reshape(P, k), want["counts"])
    assert int(o["changed"].numpy()[0]) == want["changed"] and (want["changed"] > 0 or N == 1)
    sums, inertia = o["sums"].numpy().reshape(P, k, A), o["inertia"].numpy()
    assert not np.isnan(sums).any() and not np.isnan(inertia).any(), "an output was not written completely"
    n_valid = (valid != 0).sum(axis=0)
    print("kmeans_step", case, bank, "sums max abs diff", np.abs(sums - want["sums"]).max(), "inertia rel",
          (np.abs(inertia - want["inertia"]) / np.maximum(want["inertia_terms"], 1e-300)).max())
    if bank == "lattice":
        assert np.array_equal(_bits(sums), _bits(want["sums"])), "sums differ in bits on the lattice"
    else:
        for p in range(P):
            for j in range(k):
                bound = R.reordered_sum_bound(int(want["counts"][p, j]), want["sum_terms"][p, j])
                assert (np.abs(sums[p, j] - want["sums"][p, j]) <= bound).all(), (p, j)
    for p in range(P):
        assert abs(inertia[p] - want["inertia"][p]) <= R.reordered_sum_bound(int(n_valid[p]), want["inertia_terms"][p]), p
    # two calls: the same bytes
    rc, o2 = _step(L, dev, feat, valid, cent, prev)
    assert rc == 0
    for name in ("label", "mind", "counts", "sums", "inertia", "changed"):
        a, b = o[name].view, o2[name].view
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), name
    # assignment only: NULL counts / sums / inertia (and no prev_label: changed stays), the scratch untouched
    rc, o3 = _step(L, dev, feat, valid, cent, None, accumulate=False)
    assert rc == 0
    assert torch.equal(o3["label"].view, o["label"].view) and torch.equal(o3["mind"].view.view(torch.int64), o["mind"].view.view(torch.int64))
    assert int(o3["changed"].numpy()[0]) == 0 and bool((o3["scratch"].view == FSENT).all())
    assert all(g.intact() for g in o3.values())


def test_kmeans_step_through_ops(dev):
    L, ops, _ = _mods()
    rng = np.random.RandomState(21)
    feat, valid = R.lattice_bank(rng, CH + 9, 3, 8, 3)
    cent = _centroids(rng, feat, valid, 4)
    tf, tv = _dev_bank(dev, feat, valid)
    tc = torch.from_numpy(cent).to(dev)
    want = R.kmeans_step(feat, valid, cent, np.full((CH + 9, 3), -2, np.int32))
    r = ops.part_kmeans_step(tf, tv, tc, torch.full((CH + 9, 3), -2, dtype=torch.int32, device=dev))
    assert sorted(r) == ["changed", "counts", "inertia", "label", "mind", "sums"]
    assert np.array_equal(r["label"].cpu().numpy(), want["label"]) and int(r["changed"]) == want["changed"] == (CH + 9) * 3
    assert np.array_equal(r["counts"].cpu().numpy(), want["counts"]) and np.array_equal(_bits(r["sums"].cpu().numpy()), _bits(want["sums"]))
    a = ops.part_kmeans_step(tf, tv, tc, accumulate=False)
    assert sorted(a) == ["changed", "label", "mind"] and np.array_equal(_bits(a["mind"].cpu().numpy()), _bits(want["mind"]))
    with pytest.raises(L.UpsError):
        ops.part_kmeans_step(tf, tv, tc.float())
    with pytest.raises(L.UpsError):
        ops.part_kmeans_step(tf, tv, torch.zeros((3, 65, 8), dtype=torch.float64, device=dev))


# ---------------------------------------------------------------------------------------------- PartIndex.kmeans
LLOYD_CASES = [(97, 3, 8, 4, 4), (300, 2, 64, 5, 3), (65, 1, 5, 2, 2), (130, 3, 8, 7, 4)]
_LLOYD_BANKS = {}


def _lloyd_bank(case):
    if case not in _LLOYD_BANKS:
        N, P, A, k, blobs = case
        _LLOYD_BANKS[case] = R.lattice_bank(np.random.RandomState(sum(case)), N, P, A, blobs)
    return _LLOYD_BANKS[case]


@pytest.mark.parametrize("init", ["kmeans++", "random"])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", LLOYD_CASES, ids=["x".join(map(str, c)) for c in LLOYD_CASES])
def test_part_index_kmeans_end_to_end(case, seed, init, dev):
    _, _, PI = _mods()
    N, P, A, k, blobs = case
    feat, valid = _lloyd_bank(case)
    want = R.lloyd(feat, valid, k, seed=seed, init=init)
    print("lloyd", case, seed, init, "iterations", want["iterations"], "min relative gap", want["min_gap"])
    assert want["min_gap"] >= 1e-9, "a last-bit difference could move a label: not a case for exact comparison"
    assert 1 <= want["iterations"] < 100
    index = PI.PartIndex(feat, valid)
    assert np.array_equal(index.seed_centres(k, seed, init), R.seed_centres(feat, valid, k, seed, init))
    got = index.kmeans(k, seed=seed, init=init)
    assert sorted(got) == ["clusters", "counts", "inertia", "iterations", "labels"]
    assert got["iterations"] == want["iterations"]
    assert got["labels"].shape == (P, N) and got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["counts"], want["counts"])
    assert got["clusters"].shape == (P, k, A) and np.array_equal(_bits(got["clusters"]), _bits(want["clusters"]))
    n_valid = (valid != 0).sum(axis=0)
    for p in range(P):
        assert abs(got["inertia"][p] - want["inertia"][p]) <= R.reordered_sum_bound(int(n_valid[p]), want["inertia"][p])
    label, mind = index.assign(got["clusters"])
    assert np.array_equal(label.T, want["labels"])


def test_part_index_kmeans_refusals(dev):
    _, _, PI = _mods()
    feat, valid = _lloyd_bank(LLOYD_CASES[0])
    valid = valid.copy()
    valid[:, 1] = 0
    valid[:2, 1] = 1
    index = PI.PartIndex(feat, valid)
    with pytest.raises(ValueError, match="part 1"):
        index.kmeans(3)
    with pytest.raises(ValueError):
        index.kmeans(65)
    with pytest.raises(ValueError):
        index.kmeans(2, init="pca")
    with pytest.raises(ValueError):
        index.kmeans(2, max_iter=0)
    assert index.kmeans(2, max_iter=1)["iterations"] == 1


# ---------------------------------------------------------------------------------------------- error codes
def test_error_codes_launch_nothing(dev):
    L, _, _ = _mods()
    lib = L.load()
    rng = np.random.RandomState(31)
    N, P, A, K, k = 9, 2, 5, 3, 3
    feat, valid = R.float_bank(rng, N, P, A)
    tf, tv = _dev_bank(dev, feat, valid)
    tc = torch.zeros((P, k, A), dtype=torch.float64, device=dev)
    tprev = torch.zeros((N, P), dtype=torch.int32, device=dev)
    idx, dist = _Guarded(dev, N * P * 40, torch.int32, IFILL), _Guarded(dev, N * P * 40, torch.float64, float("nan"))
    s = L.stream()
    f, v = L.ptr(tf), L.ptr(tv)

    def knn(q=f, qv=v, Nq=N, g=f, gv=v, Ng=N, P_=P, A_=A, K_=K, i=idx.ptr(), d=dist.ptr()):
        return lib.ups_part_knn(q, qv, Nq, g, gv, Ng, P_, A_, K_, 1, i, d, s)
    assert knn(K_=33) == E_UNSUPPORTED and knn(A_=513) == E_UNSUPPORTED
    for kw in ({"q": None}, {"qv": None}, {"g": None}, {"gv": None}, {"i": None}, {"d": None}, {"Nq": 0}, {"Ng": 0}, {"P_": 0},
               {"A_": 0}, {"K_": 0}, {"Nq": -3}, {"Nq": 2 ** 31 - 1, "P_": 64}, {"Ng": 2 ** 30, "A_": 512}, {"Nq": 2 ** 30, "K_": 32}):
        assert knn(**kw) == E_ARG, kw
    label, mind = _Guarded(dev, N * P, torch.int32, IFILL), _Guarded(dev, N * P, torch.float64, float("nan"))
    counts, sums = _Guarded(dev, P * 64, torch.int32, 0), _Guarded(dev, P * 64 * A, torch.float64, float("nan"))
    inertia, changed = _Guarded(dev, P, torch.float64, float("nan")), _Guarded(dev, 1, torch.int32, 0)
    scratch = _Guarded(dev, 4096, torch.float64, FSENT)
    full = dict(feat=f, valid=v, N=N, P=P, A=A, cent=L.ptr(tc), k=k, prev=L.ptr(tprev), label=label.ptr(), mind=mind.ptr(),
                counts=counts.ptr(), sums=sums.ptr(), inertia=inertia.ptr(), changed=changed.ptr(), scratch=scratch.ptr())

    def step(**kw):
        a = dict(full, **kw)
        return lib.ups_part_kmeans_step(a["feat"], a["valid"], a["N"], a["P"], a["A"], a["cent"], a["k"], a["prev"], a["label"], a["mind"],
                                        a["counts"], a["sums"], a["inertia"], a["changed"], a["scratch"], s)
    assert step(k=65) == E_UNSUPPORTED and step(A=513) == E_UNSUPPORTED
    for kw in ({"feat": None}, {"valid": None}, {"cent": None}, {"label": None}, {"mind": None}, {"N": 0}, {"P": 0}, {"A": 0}, {"k": 0},
               {"counts": None}, {"sums": None}, {"inertia": None}, {"counts": None, "sums": None}, {"sums": None, "inertia": None},
               {"scratch": None}, {"changed": None}, {"N": 2 ** 30, "A": 512}, {"N": 2 ** 31 - 1, "P": 64, "A": 1}):
        assert step(**kw) == E_ARG, kw
    torch.cuda.synchronize(dev)
    assert bool((idx.view == IFILL).all()) and bool(torch.isnan(dist.view).all()) and bool((label.view == IFILL).all())
    assert bool(torch.isnan(mind.view).all()) and bool((counts.view == 0).all()) and bool(torch.isnan(sums.view).all())
    assert bool(torch.isnan(inertia.view).all()) and int(changed.numpy()[0]) == 0 and bool((scratch.view == FSENT).all())
    for g in (idx, dist, label, mind, counts, sums, inertia, changed, scratch):
        assert g.intact()
    # and the complete calls are accepted
    assert knn() == 0 and step() == 0
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------------------------------------- the model
def _model(precision, dev):
    import upsparts_amd  # noqa: F401
    from upsparts_amd.model import TrainModel
    from oracle import configs, ref_model
    cfg = copy.deepcopy(configs.tiny_config())
    cfg.update(precision=precision, vgg_widths=VGG_W)
    return cfg, TrainModel(cfg, device=dev, seed=0), ref_model


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_encode_parts(precision, dev):
    cfg, model, RM = _model(precision, dev)
    B, S, P, A = cfg["batch_size"], cfg["spatial_size"], cfg["n_parts"], cfg.get("local_app_size", 64)
    views = RM.synthetic_views(cfg)
    gen = torch.Generator().manual_seed(5)
    v = torch.cat([views["view0"], views["view1"], torch.rand(B + 1, S, S, 3, generator=gen) * 2 - 1], 0)      # 3B + 1: an odd count
    n = v.shape[0]
    r = model.encode_parts(v)
    assert sorted(r) == ["area", "feat", "out_parts_hard"]
    assert tuple(r["feat"].shape) == (n, P, A) and r["feat"].dtype == torch.float32 and r["feat"].device.type == "cuda"
    assert tuple(r["area"].shape) == (n, P) and r["area"].dtype == torch.int32
    assert tuple(r["out_parts_hard"].shape) == (n, S, S) and r["out_parts_hard"].dtype == torch.int64
    vd = v.to(dev)
    a, b = model._encode((vd[:B], True), (vd[B:2 * B], True))
    assert torch.equal(r["feat"][:B], a["feat"]) and torch.equal(r["feat"][B:2 * B], b["feat"])
    assert torch.equal(r["out_parts_hard"][:B], a["out_parts_hard"])
    hard = r["out_parts_hard"].cpu().numpy()
    assert np.array_equal(r["area"].cpu().numpy(), np.stack([np.bincount(hard[i].reshape(-1), minlength=P) for i in range(n)]))
    assert torch.equal(r["out_parts_hard"], model.segment(v))
    # the ragged pass: its images encoded with the padding segment uses
    pad = torch.cat([vd[2 * B:], vd[2 * B:2 * B + 1].expand(2 * B - (n - 2 * B), S, S, 3)], 0)
    c, d = model._encode((pad[:B], True), (pad[B:], True))
    assert torch.equal(r["feat"][2 * B:3 * B], c["feat"]) and torch.equal(r["feat"][3 * B:], d["feat"][:n - 3 * B])
    again = model.encode_parts(v)
    assert all(torch.equal(again[k], r[k]) for k in r)


# ---------------------------------------------------------------------------------------------- the runner
def test_runner_index_end_to_end(dev, tmp_path):
    import yaml
    from PIL import Image
    import upsparts_amd  # noqa: F401
    from upsparts_amd import partindex as PI, runner
    from oracle import configs
    cfg = copy.deepcopy(configs.tiny_config())
    S, P, A = cfg["spatial_size"], cfg["n_parts"], cfg.get("local_app_size", 64)
    data_root = tmp_path / "images"
    rng = np.random.RandomState(7)
    files = ["a/{}.png".format(i) for i in range(4)] + ["b/c/{}.png".format(i) for i in range(3)]
    for rel in files:
        os.makedirs(os.path.dirname(str(data_root / rel)), exist_ok=True)
        small = rng.randint(0, 256, size=(4, 5, 3)).astype(np.uint8)
        Image.fromarray(small).resize((23, 19), Image.BILINEAR).save(str(data_root / rel))
    csv_path = tmp_path / "list.csv"
    csv_path.write_text("\n".join(files) + "\n")
    K, k, n_vis = 3, 2, 4
    cfg.update({"precision": "bf16", "vgg_widths": list(VGG_W), "data_root": str(data_root), "index_csv": str(csv_path),
                "index_neighbours": K, "index_clusters": k, "index_min_part_area": 0.0, "index_n_vis": n_vis})
    ypath = tmp_path / "index.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    res = runner.main(["--index", str(ypath), "-p", str(tmp_path / "run")])
    odir = str(tmp_path / "run" / "index" / "0")
    assert res["dir"] == odir
    listed = sorted(os.path.relpath(os.path.join(d, f), odir) for d, _, fs in os.walk(odir) for f in fs)
    want_files = sorted(["features.npz", "index.csv", "neighbours.npz", "clusters.p"] +
                        ["neighbours/part{:02}.png".format(p) for p in range(P)] +
                        ["clusters/part{:02}_cluster{:02}.png".format(p, j) for p in range(P) for j in range(k)])
    assert listed == want_files
    with np.load(os.path.join(odir, "features.npz")) as z:
        feat, area, valid = z["feat"], z["area"], z["valid"]
    assert feat.shape == (7, P, A) and feat.dtype == np.float32 and area.shape == (7, P) and (area.sum(axis=1) == S * S).all()
    assert np.array_equal(valid != 0, area >= 0) and valid.all()                 # index_min_part_area 0: ceil(0) = 0 pixels
    lines = open(os.path.join(odir, "index.csv")).read().splitlines()
    assert lines[0] == "file," + ",".join("area_{}".format(p) for p in range(P))
    assert [ln.split(",")[0] for ln in lines[1:]] == files and lines[1].split(",")[1:] == [str(a) for a in area[0]]
    with np.load(os.path.join(odir, "neighbours.npz")) as z:
        idx, dist = z["idx"], z["dist"]
    want_i, want_d = R.knn(feat, valid, feat, valid, K, True)
    assert np.array_equal(idx, want_i) and np.array_equal(_bits(dist), _bits(want_d))
    with open(os.path.join(odir, "clusters.p"), "rb") as f:
        clusters = pickle.load(f)
    assert sorted(clusters) == ["clusters", "counts", "inertia", "iterations", "labels"]
    assert clusters["clusters"].shape == (P, k, A) and clusters["clusters"].dtype == np.float64
    assert clusters["labels"].shape == (P, 7) and clusters["labels"].dtype == np.int32 and clusters["labels"].min() >= 0
    assert clusters["counts"].shape == (P, k) and (clusters["counts"].sum(axis=1) == 7).all() and clusters["inertia"].shape == (P,)
    for p in range(P):
        assert Image.open(os.path.join(odir, "neighbours", "part{:02}.png".format(p))).size == ((K + 1) * S, n_vis * S)
        for j in range(k):
            assert Image.open(os.path.join(odir, "clusters", "part{:02}_cluster{:02}.png".format(p, j))).size == (n_vis * S, S)
    # the first tile of a neighbour sheet is the first query's part crop, from the image decoded as the runner decodes it
    sheet = np.asarray(Image.open(os.path.join(odir, "neighbours", "part00.png")))
    first_pass = np.stack([np.asarray(Image.open(str(data_root / rel)).convert("RGB").resize((S, S), Image.BILINEAR), dtype=np.uint8)
                           for rel in files[:4]])
    hard = res["model"].encode_parts(torch.from_numpy(first_pass.astype(np.float32) / 127.5 - 1.0))["out_parts_hard"].cpu().numpy()
    assert np.array_equal(sheet[:S, :S], PI.part_crop(first_pass[0], hard[0].astype(np.uint8), 0))
    # a second run: the same bytes
    runner.main(["--index", str(ypath), "-p", str(tmp_path / "again")])
    for name in ("features.npz", "neighbours.npz", "clusters.p", "index.csv"):
        assert (open(os.path.join(odir, name), "rb").read() ==
                open(str(tmp_path / "again" / "index" / "0" / name), "rb").read()), name
    # the default area threshold, a query list of its own, no sheets, no clusters
    q_path = tmp_path / "queries.csv"
    q_path.write_text("\n".join(files[4:]) + "\n")
    cfg.update({"index_query_csv": str(q_path), "index_clusters": 0, "index_sheets": False})
    del cfg["index_min_part_area"]
    ypath.write_text(yaml.safe_dump(cfg))
    res = runner.main(["--index", str(ypath), "-p", str(tmp_path / "run3")])
    assert sorted(os.listdir(res["dir"])) == ["features.npz", "index.csv", "neighbours.npz"]
    with np.load(os.path.join(res["dir"], "features.npz")) as z:
        assert np.array_equal(z["feat"], feat) and np.array_equal(z["valid"] != 0, z["area"] >= R.part_area_threshold(0.005, S))
        gvalid = z["valid"]
    with np.load(os.path.join(res["dir"], "neighbours.npz")) as z:
        assert z["idx"].shape == (3, P, K)
        qi = z["idx"]
    # (the query bank's own codes: the gallery's rows 4..6, so with self NOT excluded every valid query finds itself first)
    for n in range(3):
        for p in range(P):
            if gvalid[4 + n, p]:
                assert qi[n, p, 0] == 4 + n or (feat[qi[n, p, 0], p] == feat[4 + n, p]).all()
    # both numeric outputs and the sheets off: nothing to do
    cfg.update({"index_neighbours": 0})
    ypath.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="index"):
        runner.main(["--index", str(ypath), "-p", str(tmp_path / "run4")])
    # a missing file raises; nothing synthetic stands in
    cfg.update({"index_neighbours": 2})
    csv_path.write_text("a/0.png\nnot/there.png\n")
    ypath.write_text(yaml.safe_dump(cfg))
    with pytest.raises(FileNotFoundError):
        runner.main(["--index", str(ypath), "-p", str(tmp_path / "run5")])
    assert not os.path.exists(str(tmp_path / "run5" / "index"))
