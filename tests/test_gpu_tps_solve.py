"""ups_tps_solve / ups_tps_params (csrc/tps.hip) against oracle/tps.py (CPU, fp64): the (K+3) x (K+3) solve on the kernel's own fp32
inputs, the parameter chain from the uniforms, the singular fallback, and make_tps's one solve for the view and its target.

Tolerance of the solve (derived, not tuned): |got - want| <= 2^-23 |want| + 1e-9 max|want| per sample -- one fp32 ulp for the single
final rounding, 1e-9 for fp64 round-off amplified by the conditioning the tests assert (cond(W) <= 1e4 on the drawn points; the
augmentation's own systems reach 6.8e4 and are held to the same bound)."""
import numpy as np
import pytest
import torch

from util import rel_err

pytestmark = pytest.mark.gpu

P = dict(scal=0.8, tps_scal=0.15, rot_scal=0.2, off_scal=0.2, scal_var=0.1, augm_scal=1.0)      # the shipped CUB yaml's tps_parameters


def _mods():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import lib, tps as PT
    from oracle import tps as OT
    return lib, PT, OT


def _W(coord):
    """The system matrix of oracle.tps.solve_system (for its condition number)."""
    c = coord.double()
    n, K, _ = c.shape
    p = torch.cat([torch.ones(n, K, 1, dtype=c.dtype), c], dim=2)
    d2 = ((p.unsqueeze(2) - p.unsqueeze(1)) ** 2).sum(dim=3)
    r = d2 * torch.log(d2 + 1e-6)
    return torch.cat([torch.cat([p, r], dim=2), torch.cat([torch.zeros(n, 3, 3, dtype=c.dtype), p.transpose(1, 2)], dim=2)], dim=1)


def _points(n, K, seed):
    """Control points uniform in [-0.7, 0.7]^2 as fp32, redrawn per sample until the closest pair is >= 0.05 apart (K = 3: and the
    triangle's determinant is >= 0.05); vectors uniform in +-0.3."""
    g = torch.Generator().manual_seed(seed)
    coord = torch.empty(n, K, 2, dtype=torch.float32)
    for i in range(n):
        while True:
            c = (torch.rand(K, 2, generator=g) * 1.4 - 0.7).float()
            d = torch.cdist(c.double(), c.double()) + torch.eye(K, dtype=torch.float64) * 10
            ok = float(d.min()) >= 0.05
            if ok and K == 3:
                a, b = (c[1] - c[0]).double(), (c[2] - c[0]).double()
                ok = abs(float(a[0] * b[1] - a[1] * b[0])) >= 0.05
            if ok:
                break
        coord[i] = c
    vector = (torch.rand(n, K, 2, generator=g) * 0.6 - 0.3).float()
    return coord, vector


def _solve_excess(got, want):
    """max over elements of |got - want| / (2^-23 |want| + 1e-9 max|want| of the sample); <= 1 passes."""
    got, want = got.double().cpu(), want.double()
    bound = 2.0 ** -23 * want.abs() + 1e-9 * want.abs().amax(dim=(1, 2), keepdim=True)
    return float(((got - want).abs() / bound).max())


def _counter(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("n", [1, 5, 130])
@pytest.mark.parametrize("K", [3, 9, 32])
def test_solve_matches_oracle_on_its_own_inputs(K, n, dev):
    lib, PT, OT = _mods()
    coord, vector = _points(n, K, seed=1000 * K + n)
    cond = float(np.linalg.cond(_W(coord).numpy()).max())
    print("K = {} n = {}: max cond(W) {:.1f}".format(K, n, cond))
    assert cond <= 1e4
    want = OT.solve_system(coord.double(), vector.double())
    ns = _counter(dev)
    got = PT.solve_system(coord.to(dev), vector.to(dev), n_singular=ns)
    assert got.dtype == torch.float32 and got.shape == (n, 2, K + 3)
    ex = _solve_excess(got, want)
    print("worst ratio to the bound {:.3f}".format(ex))
    assert ex <= 1.0
    assert int(ns.item()) == 0
    again = PT.solve_system(coord.to(dev), vector.to(dev), n_singular=ns)
    assert torch.equal(got, again)


def test_solve_refuses_what_it_does_not_take(dev):
    lib, PT, OT = _mods()
    for K in (2, 33):
        coord, vector = _points(1, K, seed=K)
        with pytest.raises(lib.UpsError):
            PT.solve_system(coord.to(dev), vector.to(dev))


def _uniforms(OT):
    u = torch.rand(2048, OT.N_UNIFORMS, generator=torch.Generator().manual_seed(2024))
    top = 1.0 - 2.0 ** -24
    alt = (torch.arange(OT.N_UNIFORMS) % 2).float() * top
    extreme = torch.stack([torch.zeros(OT.N_UNIFORMS), torch.full((OT.N_UNIFORMS,), top), alt, top - alt])
    return torch.cat([u, extreme.float()], dim=0)


@pytest.fixture(scope="module")
def params_run(dev):
    """ups_tps_params on 2048 seeded uniforms + four extreme rows, and the oracle's chain on the same uniforms in fp64 (computed once)."""
    lib, PT, OT = _mods()
    u = _uniforms(OT)
    ns = _counter(dev)
    coord, vector, T = PT.tps_system(u.to(dev), P, n_singular=ns)
    co, vo = OT.make_input_tps_param(OT.uniforms_to_params(u.double(), **P))
    return {"u": u, "coord": coord.cpu(), "vector": vector.cpu(), "T": T.cpu(), "ns": int(ns.item()), "co": co, "vo": vo}


def test_params_stage1_coord_and_vector(params_run):
    r = params_run
    assert r["coord"].dtype == torch.float32 and r["vector"].dtype == torch.float32
    ec = float((r["coord"].double() - r["co"]).abs().max())
    ev = float((r["vector"].double() - r["vo"]).abs().max())
    print("coord max abs error {:.3e}, vector {:.3e}".format(ec, ev))
    assert ec <= 2.0 ** -23
    assert ev <= 2.5e-7


def test_params_stage2_solve(params_run):
    lib, PT, OT = _mods()
    r = params_run
    assert r["ns"] == 0
    own = OT.solve_system(r["coord"].double(), r["vector"].double())
    print("max cond(W) {:.3e}".format(float(np.linalg.cond(_W(r["coord"]).numpy()).max())))
    ex = _solve_excess(r["T"], own)
    print("worst ratio to the bound {:.3f}".format(ex))
    assert ex <= 1.0
    loose = rel_err(r["T"], OT.solve_system(r["co"], r["vo"]))
    print("against the unrounded oracle T: rel_err {:.3e}".format(loose))
    assert loose <= 1e-5


def test_singular_systems_get_the_identity(dev):
    lib, PT, OT = _mods()
    K, n = 9, 5
    coord, vector = _points(n, K, seed=77)
    ns = _counter(dev)
    clean = PT.solve_system(coord.to(dev), vector.to(dev), n_singular=ns)
    assert int(ns.item()) == 0
    dup = coord.clone()
    for i in (1, 3):
        dup[i, 4] = dup[i, 0]
    got = PT.solve_system(dup.to(dev), vector.to(dev), n_singular=ns).cpu()
    assert int(ns.item()) == 2
    ident = torch.zeros(2, K + 3)
    ident[0, 1] = ident[1, 2] = 1.0
    for i in range(n):
        if i in (1, 3):
            assert torch.equal(got[i], ident), i
        else:
            assert torch.equal(got[i], clean[i].cpu()), i


def test_make_tps_is_deterministic_and_solves_the_target_once(dev):
    lib, PT, OT = _mods()
    g = torch.Generator().manual_seed(5)
    B, S = 3, 24
    views = [(torch.rand(B, S, S, 3, generator=g) * 2 - 1).to(dev) for _ in range(3)]
    u = torch.rand(2 * B, OT.N_UNIFORMS, generator=g).to(dev)
    a = PT.make_tps(views, P, uniforms=u)
    b = PT.make_tps(views, P, uniforms=u)
    assert len(a) == 3
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    coord, vector, T = PT.tps_system(u, P)
    assert torch.equal(T, PT.solve_system(coord, vector))       # one device function: the fused launch and the solve alone
    for i, (lo, hi) in enumerate(((0, B), (B, 2 * B), (0, B))):
        want, _ = PT.ThinPlateSpline(views[i], coord[lo:hi], vector[lo:hi])
        assert torch.equal(a[i], want), i
