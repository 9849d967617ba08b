"""Host tests of the evaluators' shared accumulator (evalutil._Accumulator) and of the host routes of PartUsageEvaluator and
PartEvaluator on CPU tensors: growth that keeps the filled rows and zeroes fresh count rows, the one copy to the host with int32
counts riding in the float64 transfer, and the evaluators against their NumPy restatements.  Everything short of a kernel call."""
import numpy as np
import pytest
import torch

CPU = torch.device("cpu")
I32_MAX = 2 ** 31 - 1


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import evalutil, lib
    return lib, evalutil


def _accumulator(E):
    return E._Accumulator("Test", CPU, (("counts", 3, torch.int32, True), ("sums", 2, torch.float64, False)))


# ---------------------------------------------------------------------------------------------- the accumulator
def test_accumulator_grows_keeps_rows_and_fetches_every_bit():
    _, E = _mods()
    acc = _accumulator(E)
    rng = np.random.RandomState(0)
    want_c, want_s, capacity = [], [], []
    special = np.array([0.1, -0.0, 1e300, np.inf])
    for n in (1, 63, 1, 200):
        counts, sums = acc.take(n)
        capacity.append(acc.capacity)
        assert tuple(counts.shape) == (n, 3) and counts.dtype == torch.int32 and counts.is_contiguous()
        assert tuple(sums.shape) == (n, 2) and sums.dtype == torch.float64 and sums.is_contiguous()
        assert int(counts.abs().sum()) == 0, "a fresh count row is not zero"
        c = rng.randint(0, I32_MAX, (n, 3)).astype(np.int32)
        c[0, 0] = I32_MAX
        s = rng.standard_normal((n, 2))
        s.reshape(-1)[:min(4, 2 * n)] = special[:min(4, 2 * n)]
        counts.copy_(torch.from_numpy(c))
        sums.copy_(torch.from_numpy(s))
        want_c.append(c), want_s.append(s)
    assert capacity == [64, 64, 128, 265]       # 1 + 63 fill the first 64 rows; then twice as many; then what is needed
    acc.invalid.fill_(I32_MAX)
    (c, s), invalid = acc.fetch()
    want_c, want_s = np.concatenate(want_c), np.concatenate(want_s)
    assert acc.n == 265 and c.shape == (265, 3) and s.shape == (265, 2)
    assert c.dtype == np.int32 and np.array_equal(c, want_c)
    assert s.dtype == np.float64 and np.array_equal(s.view(np.uint64), want_s.view(np.uint64))
    assert np.signbit(s[0, 1]) and s[0, 1] == 0.0 and (want_c == I32_MAX).sum() >= 4
    assert type(invalid) is int and invalid == I32_MAX
    acc.reset()
    assert acc.n == 0 and acc.capacity == 64 and int(acc.invalid) == 0
    counts, _ = acc.take(70)
    assert tuple(counts.shape) == (70, 3) and int(counts.abs().sum()) == 0 and acc.n == 70


def test_accumulator_makes_one_copy(monkeypatch):
    _, E = _mods()
    acc = _accumulator(E)
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    counts, sums = acc.take(5)
    sums.zero_()
    assert calls == []
    acc.fetch()
    assert len(calls) == 1


# ---------------------------------------------------------------------------------------------- the evaluators' host routes
def _usage_inputs(seed, n, HW=7, P=33):
    rng = np.random.RandomState(seed)
    soft = rng.uniform(0.0, 1.0, (n, HW, P)).astype(np.float32)
    soft /= soft.sum(axis=2, keepdims=True)
    return soft, rng.randint(0, P, (n, HW)).astype(np.int64)


def test_part_usage_evaluator_host_route(caplog):
    import logging
    L, E = _mods()
    P, HW = 33, 7
    with caplog.at_level(logging.INFO, logger="upsparts"):
        ev = E.PartUsageEvaluator(CPU, P)
    assert not ev.on_device and sum("on the host" in r.getMessage() for r in caplog.records) == 1
    with pytest.raises(ValueError):
        ev.result()                                             # nothing evaluated
    soft, pred = _usage_inputs(1, 5)
    ts, tp = torch.from_numpy(soft), torch.from_numpy(pred)
    ev.update(ts[:3], tp[:3])
    ev.update(ts[3:], tp[3:], valid=1)
    want_c, want_bad, want_s = E.part_usage_host(soft[:4], pred[:4], P)
    c, s, bad = ev.sums()
    assert ev.n == 4 and ev.HW == HW and bad == want_bad == 0
    assert c.dtype == np.int32 and np.array_equal(c, want_c) and np.array_equal(s, want_s)
    with pytest.raises(ValueError):
        ev.update(ts[:2, :5], tp[:2, :5])                       # maps of 5 pixels after maps of 7
    # part ids outside [0, P): counted as invalid, and result() says how many
    planted = pred.copy()
    planted[0, 0], planted[1, 3], planted[4, 6] = -1, 33, 33
    ev.reset()
    assert ev.n == 0
    ev.update(ts, torch.from_numpy(planted))
    c, s, bad = ev.sums()
    assert bad == 3 and np.array_equal(c, E.part_usage_host(soft, planted, P)[0]) and c.sum() == 5 * HW - 3
    with pytest.raises(L.UpsError, match=r"\b3\b"):
        ev.result()
    ev.reset()
    ev.update(ts, tp)
    want_c, _, want_s = E.part_usage_host(soft, pred, P)
    assert ev.result() == E.usage_from_counts(want_c, want_s, HW, ev.min_area)


class _SegmentStub(object):
    """What PartEvaluator needs of a model, on the host: `segment` hands out prepared int64 maps, one array per call."""
    n_parts = 3

    def __init__(self, maps, device=CPU):
        self.device, self.maps = device, [torch.from_numpy(m).to(device) for m in maps]

    def segment(self, views):
        return self.maps.pop(0)[:len(views)]


def test_part_evaluator_host_route():
    _, E = _mods()
    rng = np.random.RandomState(2)
    P, G = 3, 33
    pred = [rng.randint(0, P, (3, 4, 4)).astype(np.int64), rng.randint(0, P, (4, 4, 4)).astype(np.int64)]
    gt = [rng.randint(0, G, (3, 4, 4)).astype(np.uint8), rng.randint(0, G, (4, 4, 4)).astype(np.uint8)]
    ev = E.PartEvaluator(_SegmentStub(pred), G)
    assert not ev.on_device
    views = np.zeros((4, 4, 4, 3), np.float32)
    ev.update(views[:3], gt[0])
    ev.update(views, gt[1], valid=2)
    counts, invalid = ev.counts()
    want = E.confusion_counts(np.concatenate([pred[0], pred[1][:2]]), np.concatenate([gt[0], gt[1][:2]]), P, G)
    assert ev.n == 5 and invalid == 0 and counts.shape == (5, P, G) and counts.dtype == np.int32 and np.array_equal(counts, want)
    assert ev.result() == E.evaluate_from_counts(want)
