"""In-graph thin-plate-spline augmentation of the CUB model (cub/code/SB_model48i/model.py:282-311).

The reference imports it from the un-vendored ``eddata.utils.tps`` (the yaml block says "adapted from
https://github.com/CompVis/unsupervised-disentangling", train_cub_subset_tps.yaml:188); the three entry points keep
their names and argument meaning -- ``tps_parameters``, ``make_input_tps_param``, ``ThinPlateSpline`` -- but the
arithmetic is re-derived from the published algorithm (Lorenz et al., CVPR 2019): UNVERIFIED, parity unpinned.
A training step draws its uniforms on the device and runs ``ups_tps_params`` -- the parameter chain and the (K+3)x(K+3) fp64 solve
of every sample in one launch (csrc/tps.hip) -- then ``ups_tps_warp`` per view: no library call, no host check, capturable.
``tps_parameters`` / ``make_input_tps_param`` remain as the torch restatement of the chain (tests, tools/bench_tps.py).
"""
import torch

from . import lib as L

# control points (x, y) in [-1, 1]^2 of unsupervised-disentangling's tps_parameters (UNVERIFIED)
CONTROL_POINTS = [(-.5, -.5), (.5, -.5), (-.5, .5), (.5, .5), (.2, -.2), (-.2, .2), (.2, .2), (-.2, -.2), (0., 0.)]
N_UNIFORMS = 2 * len(CONTROL_POINTS) * 2 + 2 + 2 + 2 + 1


def tps_parameters(batch_size, scal, tps_scal, rot_scal, off_scal, scal_var, augm_scal=1.0, uniforms=None, generator=None,
                   device=None):
    """Random scale / rotation / offsets + jittered control points and TPS vectors for ``batch_size`` samples.
    ``uniforms`` [batch_size, N_UNIFORMS] in [0,1) may be passed explicitly (tests); otherwise drawn on ``device``."""
    K = len(CONTROL_POINTS)
    if uniforms is None:
        uniforms = torch.rand(batch_size, N_UNIFORMS, generator=generator, device=device, dtype=torch.float32)
    u = uniforms.to(torch.float32)
    n = u.shape[0]
    rng = lambda t, lo, hi: lo + (hi - lo) * t
    base = torch.tensor(CONTROL_POINTS, dtype=torch.float32, device=u.device).view(1, K, 2)
    i = 0
    coord = base + rng(u[:, i:i + 2 * K].reshape(n, K, 2), -0.2, 0.2); i += 2 * K
    vector = rng(u[:, i:i + 2 * K].reshape(n, K, 2), -tps_scal, tps_scal); i += 2 * K
    offset = rng(u[:, i:i + 2].reshape(n, 1, 2), -off_scal, off_scal); i += 2
    offset_2 = rng(u[:, i:i + 2].reshape(n, 1, 2), -off_scal, off_scal); i += 2
    t_scal = rng(u[:, i:i + 2], scal * (1.0 - scal_var), scal * (1.0 + scal_var)) * augm_scal; i += 2
    rot = rng(u[:, i:i + 1], -rot_scal, rot_scal)
    rot_mat = torch.stack([torch.cos(rot), -torch.sin(rot), torch.sin(rot), torch.cos(rot)], dim=-1).reshape(n, 2, 2)
    return {"coord": coord, "vector": vector, "offset": offset, "offset_2": offset_2, "t_scal": t_scal, "rot_mat": rot_mat}


def make_input_tps_param(p):
    scaled = p["t_scal"].unsqueeze(1) * (p["coord"] + p["vector"] - p["offset"]) + p["offset"]
    t_vector = torch.einsum("blk,bck->bcl", p["rot_mat"], scaled - p["offset_2"]) + p["offset_2"] - p["coord"]
    return p["coord"], t_vector


_BASE, _SINGULAR = {}, {}       # device index -> tensor


def _index(device):
    idx = torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


def base_points(device):
    """CONTROL_POINTS as the [K, 2] fp64 device tensor ``ups_tps_params`` reads (one per device, made on first use)."""
    idx = _index(device)
    if idx not in _BASE:
        _BASE[idx] = torch.tensor(CONTROL_POINTS, dtype=torch.float64, device=torch.device("cuda", idx))
    return _BASE[idx]


def singular_counter(device):
    """The int32 device counter the solve kernel adds to for every sample it gave the identity transform (a singular system) when the
    caller passes none of its own: one per device, never reset."""
    idx = _index(device)
    if idx not in _SINGULAR:
        _SINGULAR[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return _SINGULAR[idx]


def solve_system(coord, vector, n_singular=None):
    """T [n, 2, K+3] fp32 with f(c_i) = c_i + v_i: ``ups_tps_solve`` (fp64 elimination with partial pivoting on the fp32 inputs, one
    launch, no host check).  A singular system -- coincident control points -- gets the identity transform and counts in
    ``n_singular`` (int32 [1] on the device; default ``singular_counter``) instead of raising as torch.linalg.solve did."""
    cd, vc = coord.contiguous().float(), vector.contiguous().float()
    n, K, _ = cd.shape
    T = torch.empty(n, 2, K + 3, dtype=torch.float32, device=cd.device)
    ns = singular_counter(cd.device) if n_singular is None else n_singular
    L.call("ups_tps_solve", L.ptr(cd), L.ptr(vc), L.ptr(T), L.ptr(ns), n, K, L.stream())
    return T


def tps_system(uniforms, tps_params, n_singular=None):
    """(coord, vector, T) of ``uniforms`` [n, N_UNIFORMS] fp32 in [0,1): ``tps_parameters`` + ``make_input_tps_param`` +
    ``solve_system`` as ONE launch of ``ups_tps_params`` (parameter arithmetic in fp64, coord / vector rounded to fp32 once, T solved
    from those rounded values)."""
    u = uniforms.contiguous().float()
    n, K = u.shape[0], len(CONTROL_POINTS)
    assert u.shape[1] == N_UNIFORMS, "uniforms [n, {}] expected".format(N_UNIFORMS)
    p = dict(tps_params)
    coord, vector = (torch.empty(n, K, 2, dtype=torch.float32, device=u.device) for _ in range(2))
    T = torch.empty(n, 2, K + 3, dtype=torch.float32, device=u.device)
    ns = singular_counter(u.device) if n_singular is None else n_singular
    L.call("ups_tps_params", L.ptr(u), L.ptr(base_points(u.device)), K, float(p["scal"]), float(p["tps_scal"]), float(p["rot_scal"]),
           float(p["off_scal"]), float(p["scal_var"]), float(p.get("augm_scal", 1.0)), L.ptr(coord), L.ptr(vector), L.ptr(T), L.ptr(ns),
           n, L.stream())
    return coord, vector, T


def _warp(U, T, coord):
    n, h, w, c = U.shape
    out = torch.empty_like(U)
    L.call("ups_tps_warp", L.ptr(U), L.ptr(T), L.ptr(coord), L.ptr(out), n, h, w, c, coord.shape[1], L.stream())
    return out


def ThinPlateSpline(U, coord, vector, out_size=None, n_c=None):
    """U [n,H,W,C] fp32 -> (warped images, None); out_size / n_c are implied by U (kept for signature compatibility)."""
    U = U.contiguous().float()
    cd = coord.contiguous().float()
    return _warp(U, solve_system(cd, vector), cd), None


def make_tps(views, tps_params, uniforms=None, generator=None, n_singular=None):
    """model.py:282-311: views 0 and 1 get independent transforms, the target (if any) gets view0's.  Uniforms drawn on the device
    (or given), ``ups_tps_params`` once for the 2 B samples, then ``ups_tps_warp`` per view -- the target with T[:B], coord[:B] of
    that one solve.  No library call and no host check: the same launches run eagerly and inside a captured step."""
    B, dev = views[0].shape[0], views[0].device
    if uniforms is None:
        uniforms = torch.rand(2 * B, N_UNIFORMS, generator=generator, device=dev, dtype=torch.float32)
    coord, _, T = tps_system(uniforms, tps_params, n_singular=n_singular)
    out = [_warp(views[0].contiguous().float(), T[:B], coord[:B]), _warp(views[1].contiguous().float(), T[B:], coord[B:])]
    if len(views) > 2:
        out.append(_warp(views[2].contiguous().float(), T[:B], coord[:B]))
    return out
