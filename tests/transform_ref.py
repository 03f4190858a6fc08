"""Float64 restatement of the similarity transform of a 3DGS scene (latentsplat_amd.transform, csrc/scene_transform.hip)
for tests/test_scene_transform_*.py.  It shares nothing with the library's tables: the band matrices come from their
DEFINITION,

    B_l(R d) = T_l(R) . B_l(d)      for every unit d,  B the "3dgs" basis (scene_export_ref.basis = sh_basis of lsr_sh.h),

by least squares over a few hundred directions (the residual is asserted); R (the rotation nearest to the linear part
over s), s, t and q_R come from the 4x4 matrix; the
map and its adjoint are written out; and the per-element rounding bounds of a float32 evaluation follow from the arithmetic
(u = 2^-24: one rounding for each float32 table entry and one for each operation of an n-term dot product; they hold with
or without FMA contraction):

    positions    6 u (sum_j |sR_kj| |x_j| + |t_k|)
    quaternion   6 u  sum_j |L(q_R)_kj| |q_j|          (the four products of the component)
    log-scales   2 u (|scaling| + |log s|)
    band l       (2 l + 3) u sum_j |T_ij| |c_j|

Everything is torch float64 on the CPU, so that autograd of :func:`forward` is the reference of the backward."""
from __future__ import annotations

from math import isqrt

import numpy as np
import torch

from tests import scene_export_ref as sref

U = 2.0 ** -24
FIT_RESIDUAL = 1e-12
_DIRS = sref.unit_directions(300, 4242)


def band_matrix(l: int, R: np.ndarray):
    """T_l(R) ((2l+1) x (2l+1), float64) from the definition, and the fit's largest residual."""
    R = np.asarray(R, dtype=np.float64)
    s = slice(l * l, (l + 1) ** 2)
    B = sref.basis(_DIRS)[:, s]                                   # (N, n): B(d)
    BR = sref.basis(_DIRS @ R.T)[:, s]                            # (N, n): B(R d)
    Tt, *_ = np.linalg.lstsq(B, BR, rcond=None)                   # B Tt = BR  <=>  BR^T = T B^T
    res = float(np.abs(B @ Tt - BR).max())
    assert res < FIT_RESIDUAL, (l, res)
    return Tt.T, res


def rest_matrix(degree: int, R: np.ndarray) -> np.ndarray:
    """The block-diagonal matrix of bands 1..degree that multiplies the K - 1 rows of f_rest (each channel)."""
    n = (degree + 1) ** 2 - 1
    T = np.zeros((n, n))
    for l in range(1, degree + 1):
        T[l * l - 1:(l + 1) ** 2 - 1, l * l - 1:(l + 1) ** 2 - 1] = band_matrix(l, R)[0]
    return T


def split(M: np.ndarray):
    """(s, R, t) of a similarity (4, 4): s = cbrt(det) of the linear part A, R the rotation nearest to A / s (the
    orthogonal polar factor: float32 entries make A / s a rotation only to 1e-7, and T_l and q_R are defined for one)."""
    M = np.asarray(M, dtype=np.float64)
    A = M[:3, :3]
    s = float(np.cbrt(np.linalg.det(A)))
    u, _, vt = np.linalg.svd(A / s)
    return s, u @ vt, M[:3, 3].copy()


def quaternion(R: np.ndarray, like=None) -> np.ndarray:
    """A unit quaternion (w,x,y,z) of the rotation R.  R has two (q and -q); ``like`` picks the one on its side."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= max(R[0, 0], R[1, 1], R[2, 2]):
        w = 0.5 * np.sqrt(1 + tr)
        q = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        x = 0.5 * np.sqrt(1 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)]
    elif R[1, 1] >= R[2, 2]:
        y = 0.5 * np.sqrt(1 - R[0, 0] + R[1, 1] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / (4 * y), (R[0, 1] + R[1, 0]) / (4 * y), y, (R[1, 2] + R[2, 1]) / (4 * y)]
    else:
        z = 0.5 * np.sqrt(1 - R[0, 0] - R[1, 1] + R[2, 2])
        q = [(R[1, 0] - R[0, 1]) / (4 * z), (R[0, 2] + R[2, 0]) / (4 * z), (R[1, 2] + R[2, 1]) / (4 * z), z]
    q = np.array(q, dtype=np.float64)
    q /= np.linalg.norm(q)
    if like is not None and float(np.dot(q, np.asarray(like, dtype=np.float64))) < 0:
        q = -q
    return q


def left_matrix(q: np.ndarray) -> np.ndarray:
    """L(q) with q (x) p = L(q) p (Hamilton product, w,x,y,z)."""
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]], dtype=np.float64)


class Constants:
    """What one transform contributes to the map, float64 torch tensors: A = sR, t, log s, L(q_R) and the f_rest matrix."""

    def __init__(self, M, degree: int, like_q=None):
        s, R, t = split(M)
        self.s, self.R = s, R
        self.q = quaternion(R, like_q)
        self.A = torch.from_numpy(np.asarray(M, dtype=np.float64)[:3, :3].copy())
        self.t = torch.from_numpy(t)
        self.log_s = float(np.log(s))
        self.L = torch.from_numpy(left_matrix(self.q))
        self.T = torch.from_numpy(rest_matrix(degree, R))
        self.degree = degree
        # the factor (2 l + 3) of each f_rest row
        self.band_factor = torch.tensor([2 * l + 3 for l in range(1, degree + 1) for _ in range(2 * l + 1)], dtype=torch.float64)


def forward(c: Constants, xyz, rest, scaling, rotation):
    """The map on float64 tensors (n, 3), (n, K - 1, 3), (n, 3), (n, 4)."""
    return (xyz @ c.A.T + c.t, torch.einsum("ij,njc->nic", c.T, rest), scaling + c.log_s, rotation @ c.L.T)


def adjoint(c: Constants, g_xyz, g_rest, g_scaling, g_rotation):
    """The adjoint of the linear part of :func:`forward`."""
    return (g_xyz @ c.A, torch.einsum("ji,njc->nic", c.T, g_rest), g_scaling.clone(), g_rotation @ c.L)


def bounds(c: Constants, xyz, rest, scaling, rotation):
    """Per-element bounds on |float32 evaluation - forward| for float32 inputs."""
    return (6 * U * (xyz.abs() @ c.A.abs().T + c.t.abs()),
            U * c.band_factor[None, :, None] * torch.einsum("ij,njc->nic", c.T.abs(), rest.abs()),
            2 * U * (scaling.abs() + abs(c.log_s)),
            6 * U * (rotation.abs() @ c.L.abs().T))


def adjoint_bounds(c: Constants, g_xyz, g_rest, g_scaling, g_rotation):
    """The same bound forms for the adjoint, the upstream gradient in place of the input."""
    return (6 * U * (g_xyz.abs() @ c.A.abs()),
            U * c.band_factor[None, :, None] * torch.einsum("ji,njc->nic", c.T.abs(), g_rest.abs()),
            2 * U * g_scaling.abs(),
            6 * U * (g_rotation.abs() @ c.L.abs()))


def apply_indexed(fn, consts, idx, tensors):
    """``fn`` (forward, adjoint or one of the bounds) row by row with the constants ``consts[idx[row]]``; rows whose idx is
    out of range: the input itself (pass-through) for the maps, zero for the bounds."""
    is_bound = fn in (bounds, adjoint_bounds)
    outs = [torch.zeros_like(t) if is_bound else t.clone() for t in tensors]
    idx = torch.as_tensor(idx)
    for k, c in enumerate(consts):
        rows = torch.nonzero(idx == k)[:, 0]
        if rows.numel():
            for o, v in zip(outs, fn(c, *(t[rows] for t in tensors))):
                o[rows] = v
    return tuple(outs)


def degree_of(K: int) -> int:
    return isqrt(K) - 1


def random_similarity(rng: np.random.Generator, t_max: float = 1e3, s_range=(0.25, 4.0)) -> np.ndarray:
    """A similarity (4, 4) as the float32 values a caller hands over: a uniform random rotation, s log-uniform in
    ``s_range``, |t| up to ``t_max``."""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    s = float(np.exp(rng.uniform(np.log(s_range[0]), np.log(s_range[1]))))
    t = rng.normal(size=3)
    t *= rng.uniform(0, t_max) / np.linalg.norm(t)
    return matrix(R, t, s)


def matrix(R, t, s) -> np.ndarray:
    M = np.eye(4)
    M[:3, :3] = s * np.asarray(R, dtype=np.float64)
    M[:3, 3] = t
    return M.astype(np.float32)


def random_scene(n: int, K: int, seed: int) -> dict:
    """Seeded float32 raw parameters of a scene's range: positions of a few units, coefficients of order 0.3, log-scales
    around -3, unnormalised quaternions."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    return dict(xyz=3.0 * r(n, 3), features_rest=0.3 * r(n, K - 1, 3), scaling=-3.0 + 0.7 * r(n, 3),
                rotation=r(n, 4) * (0.5 + torch.rand(n, 1, generator=g)))


NAMES = ("xyz", "features_rest", "scaling", "rotation")


def f64(scene: dict):
    return tuple(scene[k].detach().cpu().to(torch.float64) for k in NAMES)
