"""Float64 reference for the SH coefficient rotation (latentsplat_amd.rotate_sh, csrc/sh_rotate.hip).

The rotation matrices are built from their DEFINITION, with a basis table of this file's own:
for the real SH basis ``Y`` below (the reference's ``eval_sh`` polynomials with every constant
positive and index 14 = y (zz - xx); e3nn's basis up to a positive factor per band),

    Y_l(R x) = D_l(R) . Y_l(x)      for every unit x,

so ``D_l`` follows from a least-squares fit over a few hundred directions.  Nothing here shares
code with the kernels or their generated tables.
"""
from __future__ import annotations

from math import isqrt

import numpy as np

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, 1.0925484305920792, 0.31539156525252005, 1.0925484305920792, 0.5462742152960396)
C3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 0.4570457994644658,
      1.445305721320277, 0.5900435899266435)
C4 = (2.5033429417967046, 1.7701307697799304, 0.9461746957575601, 0.6690465435572892, 0.10578554691520431,
      0.6690465435572892, 0.47308734787878004, 1.7701307697799304, 0.6258357354491761)

P = np.diag([-1.0, 1.0, -1.0])     # the sign pattern (-1)^m of eval_sh is the reflection of x and z


def basis(degree: int, d: np.ndarray) -> np.ndarray:
    """(..., 3) float64 -> (..., (degree+1)^2).  Written as homogeneous polynomials (1 -> x.x), so
    it is defined for any vector and equals the usual table on the unit sphere."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    rr = xx + yy + zz
    t = [C0 * np.ones_like(x)]
    if degree >= 1:
        t += [C1 * x, C1 * y, C1 * z]
    if degree >= 2:
        t += [C2[0] * xz, C2[1] * xy, C2[2] * (2 * yy - zz - xx), C2[3] * yz, C2[4] * (zz - xx)]
    if degree >= 3:
        t += [C3[0] * x * (3 * zz - xx), C3[1] * xz * y, C3[2] * x * (4 * yy - zz - xx),
              C3[3] * y * (2 * yy - 3 * zz - 3 * xx), C3[4] * z * (4 * yy - zz - xx),
              C3[5] * y * (zz - xx), C3[6] * z * (zz - 3 * xx)]
    if degree >= 4:
        t += [C4[0] * xz * (zz - xx), C4[1] * xy * (3 * zz - xx), C4[2] * xz * (7 * yy - rr),
              C4[3] * xy * (7 * yy - 3 * rr), C4[4] * (yy * (35 * yy - 30 * rr) + 3 * rr * rr),
              C4[5] * yz * (7 * yy - 3 * rr), C4[6] * (zz - xx) * (7 * yy - rr),
              C4[7] * yz * (zz - 3 * xx), C4[8] * (zz * (zz - 3 * xx) - xx * (3 * zz - xx))]
    return np.stack(t, axis=-1)


def _directions(n: int = 400, seed: int = 12345) -> np.ndarray:
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


_DIRS = _directions()


def band_matrix(degree: int, R: np.ndarray) -> tuple[np.ndarray, float]:
    """D_l(R) ((2l+1) x (2l+1), float64) and the fit's largest residual."""
    R = np.asarray(R, dtype=np.float64)
    lo, hi = degree * degree, (degree + 1) * (degree + 1)
    Y = basis(degree, _DIRS)[:, lo:hi]                   # (N, n):  Y(x)
    YR = basis(degree, _DIRS @ R.T)[:, lo:hi]            # (N, n):  Y(R x)
    Dt, *_ = np.linalg.lstsq(Y, YR, rcond=None)          # Y Dt = YR  <=>  YR^T = D Y^T
    return Dt.T, float(np.abs(Y @ Dt - YR).max())


def rotation_blocks(max_degree: int, R: np.ndarray) -> list[np.ndarray]:
    return [band_matrix(l, R)[0] for l in range(max_degree + 1)]


def packed_table(max_degree: int, R: np.ndarray) -> np.ndarray:
    """The layout of lsr_sh_rotation_matrices: the band blocks, row-major, one after another
    (1 + 9 + 25 + 49 + 81 = 165 entries at degree 4)."""
    return np.concatenate([b.reshape(-1) for b in rotation_blocks(max_degree, R)])


def full_matrix(max_degree: int, R: np.ndarray) -> np.ndarray:
    n = (max_degree + 1) ** 2
    D = np.zeros((n, n))
    for l, b in enumerate(rotation_blocks(max_degree, R)):
        D[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = b
    return D


def rotate(coefficients: np.ndarray, R: np.ndarray) -> np.ndarray:
    """coefficients (..., n) rotated by ONE rotation R (3, 3); n a perfect square <= 25."""
    n = coefficients.shape[-1]
    deg = isqrt(n) - 1
    assert (deg + 1) ** 2 == n and deg <= 4
    return np.asarray(coefficients, dtype=np.float64) @ full_matrix(deg, R).T


def random_rotations(n: int, rng: np.random.Generator) -> np.ndarray:
    """Proper rotations (n, 3, 3), float64, from normalised quaternions."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, s = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s),
                     2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s),
                     2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)


def axis_rotation(axis: int, angle: float) -> np.ndarray:
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i] = c; R[i, j] = -s; R[j, i] = s; R[j, j] = c
    return R


def special_rotations() -> np.ndarray:
    """Identity, half turns about each axis, and matrices within 1e-6 of gimbal lock in e3nn's
    Y-X-Y angle convention (beta -> 0 and beta -> pi: the image of the y axis is +-y)."""
    out = [np.eye(3)] + [axis_rotation(a, np.pi) for a in range(3)]
    for beta in (1e-6, 3e-7, np.pi - 1e-6, np.pi - 2e-7, 0.0, np.pi):
        for alpha, gamma in ((0.3, -1.1), (2.0, 2.5)):
            out.append(axis_rotation(1, alpha) @ axis_rotation(0, beta) @ axis_rotation(1, gamma))
    return np.stack(out)
