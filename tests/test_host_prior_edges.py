"""The premises of the trained-regime mask-prior cases (prior_edge_ref.py), without a GPU: every regime has the property it is
named for, no pixel's tie decision and no Mumford-Shah threshold element depends on rounding, the oracle's centres are stable,
and the fp64 reference agrees with the independent NumPy restatement and has finite gradients.  A failure here is a failure of
a case, not of a kernel."""
import numpy as np
import pytest
import torch

import prior_edge_ref as E


def _rel(a, b):
    return abs(float(a) - float(b)) / max(1.0, abs(float(b)))


def test_case_table():
    """Every shape in every regime; the blocks-per-image variants for border_absent at 0-10-128 only; ids are unique."""
    ids = [c.id for c in E.CASES]
    assert len(set(ids)) == len(ids)
    for sh in E.SHAPES:
        got = set((c.regime, c.planted) for c in E.CASES if tuple(c[1:6]) == sh)
        assert {("confident", False), ("lattice_ties", False), ("border_absent", False), ("border_absent", True)} <= got, sh
    assert sum(c.regime == "lattice_ties_noeps" for c in E.CASES) >= 1
    bpi = [c for c in E.CASES if c.px_bpi]
    assert sorted(set(c.px_bpi for c in bpi)) == [1, 4] and all(c.regime == "border_absent" and c[1:4] == (0, 10, 128) for c in bpi)


@pytest.mark.parametrize("i", E.INPUTS, ids=E.inputs_id)
def test_premises_and_oracle_agreement(i):
    inp = E.build(i)
    assert inp["lm"].dtype == inp["eps"].dtype == inp["g_hard"].dtype == torch.float32
    assert torch.equal(E.build.__wrapped__(i)["l"], inp["l"]), "the regime is not a pure function of its arguments"
    p = E.premises(i, inp)
    print({k: v for k, v in p.items() if not torch.is_tensor(v)})
    E.check_premises(i, p)
    if i.regime.startswith("lattice_ties"):          # integer logits: the float32 sum is exact, eps in {-1, 0, 1}
        assert torch.equal(inp["l"], inp["l"].round()) and float(inp["eps"].abs().max()) <= 1.0
        assert (i.regime == "lattice_ties_noeps") == (float(inp["eps"].abs().max()) == 0.0)
    B, S = i.B, i.S
    centre_sets = [p["centres"]]
    if i.regime == "border_absent":
        rc = p["centres"]
        centre_sets.append(torch.cat([E.plant(rc[:B], S), E.plant(rc[B:], S)]))
        # all four borders carry a clipped natural centre somewhere in the case
        c = rc.view(-1, 2)
        assert bool((c[:, 0] < E.HALF).any() and (c[:, 0] > S - 1 - E.HALF).any() and (c[:, 1] < E.HALF).any() and (c[:, 1] > S - 1 - E.HALF).any())
    for rc in centre_sets:
        q, d = E.reference(i, inp, rc[:B], rc[B:])
        for k, v in q.items():
            assert bool(torch.isfinite(v)), k
        for k, v in d.items():
            assert bool(torch.isfinite(v).all()), "fp64 gradient {} is not finite".format(k)
            assert float(v.abs().max()) > 0.0, k
        nq = E.np_forward(i, inp, rc[:B])
        assert set(nq) == set(q) - {"weakly", "var"}
        for k, v in nq.items():
            assert _rel(v, q[k]) <= 1e-9, "oracle {} {} vs NumPy restatement {}".format(k, float(q[k]), v)
        # the rectangles themselves: ref_model.draw_rect == np_ops.draw_rect on these centres, clipped boxes included
        r_t = E.rects(rc, S).permute(0, 3, 1, 2).reshape(-1, S, S).numpy()
        r_n = E.np_ops.draw_rect(rc.reshape(-1, 2).numpy(), E.PATCH, E.PATCH, S, S, np.float64, order="yx")
        assert np.array_equal(r_t, r_n)
    if i.regime == "border_absent":
        # a planted corner box is clipped to (HALF + 1)^2 pixels
        assert float(E.rects(centre_sets[1][:1, :1], S).sum()) == (E.HALF + 1) ** 2
