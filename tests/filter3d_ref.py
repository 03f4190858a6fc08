"""Restatement of the 3D smoothing filter of Mip-Splatting for the tests (tests/test_filter3d_*.py), from the paper's
formulas and include/lsr_filter3d.h / include/lsr_scene.h: the (Gaussians x cameras) pass as the published loop over
cameras in float64 NumPy, both modes; the filtered activation on float64 torch tensors so that autograd gives the
gradients; the fused parameters; the bars both are held to; and the input builders the tests share."""
from __future__ import annotations

import numpy as np
import torch

from tests import scene_params_ref as sref

PARAMS = sref.PARAMS
VIEW_FLOATS = 44
NEAR = 0.2                     # the rasterizer's near-plane cull, in the scaled space
U = 2.0 ** -24                 # the unit roundoff of float32
THRESHOLD_REL = 1e-4           # a (point, camera) pair closer than this (relative) to a threshold is "near" it


# ---- the pass ----

def _usable(r: np.ndarray) -> bool:
    s, tx, ty = r[40], r[35], r[36]
    return bool(np.isfinite([s, tx, ty]).all() and s > 0 and tx > 0 and ty > 0)


def project(xyz: np.ndarray, r: np.ndarray):
    """p = W (s x, 1) in float64 for one view record (W transposed in slots 0..15, s = slot 40): (px, py, pz) and
    T = |r2 s x| + |r6 s y| + |r10 s z| + |r14|, the magnitude the rounding of p.z is relative to."""
    sx = r[40] * xyz
    with np.errstate(invalid="ignore", over="ignore"):
        p = [r[c] * sx[:, 0] + r[4 + c] * sx[:, 1] + r[8 + c] * sx[:, 2] + r[12 + c] for c in range(3)]
        T = np.abs(r[2] * sx[:, 0]) + np.abs(r[6] * sx[:, 1]) + np.abs(r[10] * sx[:, 2]) + np.abs(r[14])
    return p[0], p[1], p[2], T


def filter_ref(xyz: np.ndarray, views: np.ndarray, width: int, margin: float = 0.15, variance: float = 0.2,
               per_view: bool = False) -> dict:
    """The pass in float64 from the float32 inputs: ``filter (n,)``, ``seen (n,)`` bool, ``F`` the largest focal length,
    ``bound (n,)`` = 8 u max_v(T_v / s_v) sqrt(variance) / F (three FMAs and the operations after them), and ``near``,
    the number of (point, camera) pairs within THRESHOLD_REL of one of the three thresholds."""
    x = np.asarray(xyz, np.float64)
    n = x.shape[0]
    spread = 1.0 + 2.0 * float(np.float32(margin))
    dist, rate = np.full(n, np.inf), np.zeros(n)
    seen, tmax = np.zeros(n, bool), np.zeros(n)
    F, near = 0.0, 0
    for rec in np.asarray(views):                              # the published loop over the training cameras
        r = rec.astype(np.float64)
        if not _usable(r):
            continue
        px, py, pz, T = project(x, r)
        lx, ly = spread * r[35] * pz, spread * r[36] * pz
        with np.errstate(invalid="ignore"):
            valid = (pz > NEAR) & (np.abs(px) <= lx) & (np.abs(py) <= ly)          # a NaN compares false
            near += int((np.abs(pz - NEAR) <= THRESHOLD_REL * NEAR).sum())
            near += int((np.abs(np.abs(px) - lx) <= THRESHOLD_REL * np.abs(lx)).sum())
            near += int((np.abs(np.abs(py) - ly) <= THRESHOLD_REL * np.abs(ly)).sum())
        z, focal = pz / r[40], width / (2.0 * r[35])
        F = max(F, focal)
        dist = np.where(valid, np.minimum(dist, z), dist)
        with np.errstate(divide="ignore", invalid="ignore"):
            rate = np.where(valid, np.maximum(rate, focal / z), rate)
        seen |= valid
        tmax = np.fmax(tmax, T / r[40])
    seen &= np.isfinite(dist)                                  # an infinite coordinate: unseen
    sd = np.sqrt(float(np.float32(variance)))
    with np.errstate(divide="ignore", invalid="ignore"):
        filt = sd / rate if per_view else dist / F * sd
    filt = np.where(seen, filt, filt[seen].max() if seen.any() else 0.0)
    bound = 8.0 * U * tmax * sd / F if F > 0 else np.zeros(n)
    return dict(filter=filt, seen=seen, F=F, bound=bound, near=near)


# ---- cameras and points ----

def view_records(extrinsics: np.ndarray, tanfovx, tanfovy, scale=1.0) -> np.ndarray:
    """(V, 44) float32 view records from camera-to-world matrices (V, 4, 4): the slots the filter reads (the transposed
    world->view matrix of the scaled scene in 0..15, tanfov in 35 / 36, the scene scale in 40); the others are 0."""
    ext = np.asarray(extrinsics, np.float64)
    V = ext.shape[0]
    scale = np.broadcast_to(np.asarray(scale, np.float64), (V,))
    out = np.zeros((V, VIEW_FLOATS), np.float32)
    for v in range(V):
        c2w = ext[v].copy()
        c2w[:3, 3] *= scale[v]
        out[v, :16] = np.linalg.inv(c2w).T.reshape(16)
        out[v, 40] = scale[v]
    out[:, 35], out[:, 36] = tanfovx, tanfovy
    return out


def circle_extrinsics(V: int, radius: float = 4.0, seed: int = 0) -> np.ndarray:
    """Camera-to-world matrices (x right, y down, z forward) on a circle around the origin, looking at it."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(V) + rng.uniform(0, 1)) / V
    ext = np.zeros((V, 4, 4))
    for v, a in enumerate(ang):
        offset = np.array([np.cos(a), 0.0, np.sin(a)])
        forward, down = -offset, np.array([0.0, 1.0, 0.0])
        ext[v, :3, 0], ext[v, :3, 1], ext[v, :3, 2] = np.cross(down, forward), down, forward
        ext[v, :3, 3] = radius * offset
        ext[v, 3, 3] = 1.0
    return ext


def circle_views(V: int, seed: int = 0, scale=1.0, radius: float = 4.0) -> np.ndarray:
    """View records of V cameras on a circle with differing tanfov (so differing focal lengths)."""
    rng = np.random.default_rng(1000 + seed)
    return view_records(circle_extrinsics(V, radius, seed), rng.uniform(0.25, 0.6, V), rng.uniform(0.25, 0.6, V), scale)


def draw_points(n: int, views: np.ndarray, seed: int, margin: float = 0.15, extent: float = 6.0) -> np.ndarray:
    """n float32 points in a cube wide enough that some fall behind the near plane of some camera, some outside its
    frustum and some only inside the margin.  Any point that has a pair within THRESHOLD_REL of a threshold (judged by the
    float64 restatement) is drawn again, so that no comparison of the kernel is decided by rounding."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    for _ in range(100):
        bad = _near_rows(pts, views, margin)
        if not bad.any():
            return pts
        pts[bad] = rng.uniform(-extent, extent, (int(bad.sum()), 3)).astype(np.float32)
    raise AssertionError("could not draw points away from the thresholds")


def _near_rows(pts: np.ndarray, views: np.ndarray, margin: float) -> np.ndarray:
    x = pts.astype(np.float64)
    spread = 1.0 + 2.0 * float(np.float32(margin))
    bad = np.zeros(len(pts), bool)
    for rec in views:
        r = rec.astype(np.float64)
        px, py, pz, _ = project(x, r)
        lx, ly = spread * r[35] * pz, spread * r[36] * pz
        bad |= np.abs(pz - NEAR) <= THRESHOLD_REL * NEAR
        bad |= np.abs(np.abs(px) - lx) <= THRESHOLD_REL * np.abs(lx)
        bad |= np.abs(np.abs(py) - ly) <= THRESHOLD_REL * np.abs(ly)
    return bad


def world_point(rec: np.ndarray, p) -> np.ndarray:
    """The float32 world point whose p = W (s x, 1) is ``p`` for the view record ``rec`` (up to rounding)."""
    r = rec.astype(np.float64)
    W = r[:16].reshape(4, 4).T
    return (np.linalg.solve(W[:3, :3], np.asarray(p, np.float64) - W[:3, 3]) / r[40]).astype(np.float32)


def threshold_points(rec: np.ndarray, margin: float = 0.15, depth: float = 3.0):
    """Points 1 % either side of each threshold of one camera, as (points (k, 3) float32, valid (k,) bool for that camera):
    the near plane, the widened frustum in x and in y on both sides, and the margin band itself (outside the image,
    inside the widened frustum)."""
    spread = 1.0 + 2.0 * margin
    lx, ly = spread * float(rec[35]) * depth, spread * float(rec[36]) * depth
    cases = [((0, 0, NEAR * 1.01), True), ((0, 0, NEAR * 0.99), False)]
    for sign in (1, -1):
        cases += [((sign * lx * 0.99, 0, depth), True), ((sign * lx * 1.01, 0, depth), False),
                  ((0, sign * ly * 0.99, depth), True), ((0, sign * ly * 1.01, depth), False),
                  ((sign * (1 + margin) * float(rec[35]) * depth, 0, depth), True),
                  ((0, sign * (1 + margin) * float(rec[36]) * depth, depth), True)]
    return np.stack([world_point(rec, p) for p, _ in cases]), np.array([ok for _, ok in cases])


# ---- the filtered activation ----

def make_filter(n: int, seed: int) -> np.ndarray:
    """(n, 1) float32 filters, log-uniform in [1e-4, 1], with exact zeros in every seventh row."""
    rng = np.random.default_rng(seed)
    f = np.exp(rng.uniform(np.log(1e-4), 0.0, (n, 1))).astype(np.float32)
    f[::7] = 0.0
    return f


def forward64(p: dict, filt, scale_modifier: float = 1.0) -> dict:
    """The filtered forward on float64 torch tensors (differentiable in ``p``): v = s^2 + f^2, scales = m sqrt(v), cov3D
    = R diag(m^2 v) R^T, opacities = sigmoid(opacity) prod_k s_k / sqrt(v_k); shs and rotations as unfiltered."""
    shs = torch.cat([p["features_dc"], p["features_rest"]], 1)
    s = torch.exp(p["scaling"])
    root = torch.sqrt(s * s + filt * filt)
    opac = (1.0 / (1.0 + torch.exp(-p["opacity"]))) * (s / root).prod(1, keepdim=True)
    scales = scale_modifier * root
    q = p["rotation"] / torch.linalg.norm(p["rotation"], dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * scales[:, None, :]
    S = M @ M.transpose(1, 2)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    return dict(shs=shs, opacities=opac, scales=scales, rotations=q, cov3D=cov)


def _t64(p: dict, grad: bool = False) -> dict:
    return {k: torch.from_numpy(np.asarray(p[k], np.float64)).requires_grad_(grad) for k in PARAMS}


def _f64(filt) -> torch.Tensor:
    return torch.from_numpy(np.asarray(filt, np.float64).reshape(-1, 1))


def expected(p: dict, filt, scale_modifier: float = 1.0) -> dict:
    """The filtered forward's outputs in float64 (numpy)."""
    with torch.no_grad():
        out = forward64(_t64(p), _f64(filt), scale_modifier)
    return {k: v.numpy() for k, v in out.items()}


def gradients(p: dict, filt, upstream: dict, scale_modifier: float = 1.0) -> dict:
    """float64 autograd through :func:`forward64`: the gradients of the five raw tensors for the upstream gradients given
    (a missing or ``None`` entry is zero), and the float64 ``cov3D`` the bars are scaled by."""
    t = _t64(p, grad=True)
    out = forward64(t, _f64(filt), scale_modifier)
    loss = sum((out[k] * torch.from_numpy(np.asarray(g, np.float64))).sum() for k, g in upstream.items() if g is not None)
    got = torch.autograd.grad(loss, [t[k] for k in PARAMS], allow_unused=True)
    res = {k: (np.zeros(t[k].shape) if g is None else g.numpy()) for k, g in zip(PARAMS, got)}
    res["cov3D"] = out["cov3D"].detach().numpy()
    return res


def fused64(opacity, scaling, filt):
    """The fused parameters in float64: ``logit(o c)`` and ``log(sqrt(v_k))``."""
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity, np.float64)))
    s, f = np.exp(np.asarray(scaling, np.float64)), np.asarray(filt, np.float64).reshape(-1, 1)
    root = np.sqrt(s * s + f * f)
    oc = o * (s / root).prod(1, keepdims=True)
    return np.log(oc) - np.log1p(-oc), np.log(root)


def assert_forward_matches(got: dict, want: dict, show: str = "") -> None:
    """The bars of the filtered forward against float64 ``want``: shs bit-equal; scales and rotations at rtol = atol =
    2e-5; cov3D within 2e-5 of the Gaussian's largest entry; opacities at rtol 2e-5 with NO absolute floor (o c is
    legitimately tiny: an absolute 2e-5 would hide it)."""
    if "shs" in got:
        assert np.array_equal(got["shs"], want["shs"].astype(np.float32))
    for k in ("scales", "rotations"):
        if k in got:
            np.testing.assert_allclose(got[k], want[k], rtol=2e-5, atol=2e-5, err_msg=k)
    if "cov3D" in got:
        bound = 2e-5 * np.abs(want["cov3D"]).max(1, keepdims=True)
        err = np.abs(got["cov3D"].astype(np.float64) - want["cov3D"])
        print(f"{show} cov3D: worst err / largest entry {np.max(err / np.maximum(bound / 2e-5, 1e-300), initial=0.0):.3e} (bar 2e-5)")
        assert (err <= bound).all(), "cov3D"
    if "opacities" in got:
        err = np.abs(got["opacities"].astype(np.float64) - want["opacities"])
        print(f"{show} opacities: worst relative err {np.max(err / np.maximum(np.abs(want['opacities']), 1e-300), initial=0.0):.3e} "
              f"(bar 2e-5), smallest value {np.min(want['opacities'], initial=1.0):.3e}")
        assert (err <= 2e-5 * np.abs(want["opacities"])).all(), "opacities"


def assert_backward_matches(got: dict, p: dict, filt, upstream: dict, scale_modifier: float = 1.0, show: str = "") -> None:
    """The bars of the filtered backward, per Gaussian, against :func:`gradients`: SH gradients bit-equal to the re-layout
    of the upstream gradient; ``|d_opacity err| <= 2e-5 |g_o|``; each d_scaling row within ``2e-5 (max|cov_g| max|g_cov,g|
    + |g_o,g|)`` (the opacity coefficient's term is bounded by |g_o|); each d_rotation row within ``2e-5 max|cov_g|
    max|g_cov,g| / |q_g|``."""
    want = gradients(p, filt, upstream, scale_modifier)
    n = p["opacity"].shape[0]
    g_shs, g_o, g_cov = (upstream.get(k) for k in ("shs", "opacities", "cov3D"))
    if "features_dc" in got:
        assert np.array_equal(got["features_dc"], np.zeros((n, 1, 3), np.float32) if g_shs is None else g_shs[:, :1, :])
    if "features_rest" in got:
        K = p["features_rest"].shape[1] + 1
        assert np.array_equal(got["features_rest"], np.zeros((n, K - 1, 3), np.float32) if g_shs is None else g_shs[:, 1:, :])
    abs_go = np.abs(np.zeros((n, 1)) if g_o is None else g_o.astype(np.float64))
    if "opacity" in got:
        err = np.abs(got["opacity"].astype(np.float64) - want["opacity"])
        print(f"{show} d_opacity: worst err / |g_o| {np.max(err / np.maximum(abs_go, 1e-300), initial=0.0):.3e} (bar 2e-5)")
        assert (err <= 2e-5 * abs_go).all(), "opacity"
    scale = np.abs(want["cov3D"]).max(1, keepdims=True) * \
        (np.zeros((n, 1)) if g_cov is None else np.abs(g_cov.astype(np.float64)).max(1, keepdims=True))
    norm = np.linalg.norm(p["rotation"].astype(np.float64), axis=1, keepdims=True)
    for k, s in (("scaling", scale + abs_go), ("rotation", scale / norm)):
        if k in got:
            assert got[k].shape == want[k].shape
            err = np.abs(got[k].astype(np.float64) - want[k])
            print(f"{show} d_{k}: worst err / scale {np.max(err / np.maximum(s, 1e-300), initial=0.0):.3e} (bar 2e-5)")
            assert (err <= 2e-5 * s).all(), k
