"""Restatement of the scene export for the tests (tests/test_scene_export_*.py): numpy, float64.  The SH basis of
csrc/lsr_sh.h, the change of basis "reference" -> "3dgs" solved from its defining equation (independently of the
library's table), seeded inputs of the encoder's range, and the bars a packed row table is held to."""
from __future__ import annotations

from functools import lru_cache

import numpy as np


def basis(d: np.ndarray) -> np.ndarray:
    """sh_basis of csrc/lsr_sh.h at directions d (N, 3) -> (N, 25)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C1 = 0.4886025119029199
    b = [0.28209479177387814 * np.ones_like(x),
         -C1 * y, C1 * z, -C1 * x,
         1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * (2 * zz - xx - yy),
         -1.0925484305920792 * xz, 0.5462742152960396 * (xx - yy),
         -0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z,
         -0.4570457994644658 * y * (4 * zz - xx - yy), 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
         -0.4570457994644658 * x * (4 * zz - xx - yy), 1.445305721320277 * z * (xx - yy),
         -0.5900435899266435 * x * (xx - 3 * yy),
         2.5033429417967046 * xy * (xx - yy), -1.7701307697799304 * yz * (3 * xx - yy),
         0.9461746957575601 * xy * (7 * zz - 1), -0.6690465435572892 * yz * (7 * zz - 3),
         0.10578554691520431 * (zz * (35 * zz - 30) + 3), -0.6690465435572892 * xz * (7 * zz - 3),
         0.47308734787878004 * (xx - yy) * (7 * zz - 1), -1.7701307697799304 * xz * (xx - 3 * yy),
         0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return np.stack(b, axis=-1)


def unit_directions(n: int, seed: int) -> np.ndarray:
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def reference_view(d: np.ndarray) -> np.ndarray:
    """The basis as LSR_SH_AXES_REFERENCE evaluates it: at (d_z, d_x, d_y)."""
    return basis(d[:, [2, 0, 1]])


@lru_cache(maxsize=None)
def axes_matrix() -> np.ndarray:
    """(25, 25) M with basis(d) @ M = reference_view(d): coefficients c under "reference" are M c under "3dgs".  Solved
    band by band (off-block entries are 0 by construction)."""
    d = unit_directions(3000, 99)
    Y, Yp = basis(d), reference_view(d)
    M = np.zeros((25, 25))
    for l in range(5):
        s = slice(l * l, (l + 1) ** 2)
        M[s, s] = np.linalg.lstsq(Y[:, s], Yp[:, s], rcond=None)[0]
    M.setflags(write=False)
    return M


def rotation_matrices(q: np.ndarray) -> np.ndarray:
    """(n, 4) w,x,y,z (any norm) -> (n, 3, 3)."""
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def covariances_from(q: np.ndarray, s: np.ndarray) -> np.ndarray:
    """R diag(s^2) R^T, float64 (n, 3, 3)."""
    R = rotation_matrices(np.asarray(q, np.float64))
    return np.einsum("nik,nk,njk->nij", R, np.asarray(s, np.float64) ** 2, R)


def make_inputs(n: int, K: int, seed: int) -> dict:
    """float32 means (n,3), opacities (n,), shs (n,K,3), cov (n,3,3).  Covariances R diag(s^2) R^T with random unit
    quaternions, overall scale log-uniform in [1e-3, 1] and axis ratios down to 1/30 (the encoder's range); opacities
    cover [1e-4, 1 - 1e-4] with both ends populated; SH bands are drawn around different centres so that a swapped or
    transposed coefficient changes the result."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    overall = np.exp(rng.uniform(np.log(1e-3), 0.0, (n, 1)))
    ratios = np.exp(rng.uniform(np.log(1.0 / 30), 0.0, (n, 3)))
    ratios[:, 0] = 1.0
    cov = covariances_from(q, overall * ratios)
    u = rng.uniform(0.0, 1.0, n)
    ends = np.exp(rng.uniform(np.log(1e-4), np.log(0.5), n))
    opac = np.where(u < 0.25, ends, np.where(u < 0.5, 1.0 - ends, rng.uniform(1e-4, 1 - 1e-4, n)))
    shs = rng.standard_normal((n, K, 3)) * 0.5 + (np.arange(K)[None, :, None] % 7 - 3) + 0.25 * np.arange(3)[None, None, :]
    return dict(means=(rng.standard_normal((n, 3)) * 3).astype(np.float32), opacities=opac.astype(np.float32).clip(1e-4, 1 - 1e-4),
                shs=shs.astype(np.float32), cov=cov.astype(np.float32))


def pack6(cov: np.ndarray) -> np.ndarray:
    return np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1)


def columns(K: int) -> dict:
    """Column ranges of a row of construct_list_of_attributes(3 (K - 1))."""
    o = 6 + 3 * K
    return dict(xyz=slice(0, 3), normals=slice(3, 6), f_dc=slice(6, 9), f_rest=slice(9, o), opacity=o,
                scale=slice(o + 1, o + 4), rot=slice(o + 4, o + 8), stride=o + 8)


def stored_shs(rows: np.ndarray, K: int) -> np.ndarray:
    """(n, K, 3) from the channel-major columns."""
    col = columns(K)
    n = rows.shape[0]
    rest = rows[:, col["f_rest"]].reshape(n, 3, K - 1).transpose(0, 2, 1)
    return np.concatenate([rows[:, col["f_dc"]][:, None, :], rest], axis=1)


def rebuilt_covariances(rows: np.ndarray, K: int) -> np.ndarray:
    """R S^2 R^T in float64 from the stored log-scales and quaternion (normalised, as every loader does)."""
    col = columns(K)
    return covariances_from(rows[:, col["rot"]].astype(np.float64), np.exp(rows[:, col["scale"]].astype(np.float64)))


def reconstruction_error(rows: np.ndarray, K: int, cov: np.ndarray) -> np.ndarray:
    """Per Gaussian: max |rebuilt - cov| / max |cov| (0 where cov is the zero matrix and the rebuilt one is tiny)."""
    cov = np.asarray(cov, np.float64).reshape(-1, 3, 3)
    err = np.abs(rebuilt_covariances(rows, K) - cov).reshape(-1, 9).max(1)
    big = np.abs(cov).reshape(-1, 9).max(1)
    return np.where(big > 0, err / np.where(big > 0, big, 1.0), 0.0)


def assert_rows(rows: np.ndarray, inp: dict, K_out: int, convention: str, what: str = "") -> float:
    """Every bar of the issue on one packed table; `inp` as make_inputs (shs (n, K_in, 3)).  Returns the worst
    reconstruction error relative to the Gaussian's largest |cov| entry."""
    col = columns(K_out)
    n = inp["means"].shape[0]
    assert rows.shape == (n, col["stride"]) and rows.dtype == np.float32, what
    assert np.array_equal(rows[:, col["xyz"]].view(np.uint32), inp["means"].view(np.uint32)), f"{what}: means"
    assert not rows[:, col["normals"]].view(np.uint32).any(), f"{what}: normals"
    got = stored_shs(rows, K_out)
    src = inp["shs"][:, :K_out, :]
    if convention == "3dgs":
        assert np.array_equal(got.view(np.uint32), src.view(np.uint32)), f"{what}: colour SH re-layout"
    else:
        want = np.einsum("ij,njc->nic", axes_matrix()[:K_out, :K_out], src.astype(np.float64))
        for l in range(int(round(K_out ** 0.5))):
            s = slice(l * l, (l + 1) ** 2)
            bound = 1e-5 * np.maximum(1.0, np.abs(src[:, s, :]).max(axis=1, keepdims=True))      # per Gaussian, channel, band
            err = np.abs(got[:, s, :] - want[:, s, :])
            assert (err <= bound).all(), f"{what}: band {l} worst err / bound {np.max(err / bound):.3f}"
    p = inp["opacities"].astype(np.float64)
    logit = rows[:, col["opacity"]].astype(np.float64)
    assert np.isfinite(logit).all(), f"{what}: logits"
    inside = (p >= 1e-4) & (p <= 1 - 1e-4)
    perr = np.abs(1.0 / (1.0 + np.exp(-logit)) - p)[inside]
    assert perr.size == 0 or perr.max() <= 1e-6, f"{what}: sigmoid(logit) off by {perr.max():.2e}"
    q = rows[:, col["rot"]].astype(np.float64)
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max(initial=0.0) <= 1e-5 and (q[:, 0] >= 0).all(), f"{what}: quaternion"
    ls = rows[:, col["scale"]]
    assert np.isfinite(ls).all() and (ls[:, 0] >= ls[:, 1]).all() and (ls[:, 1] >= ls[:, 2]).all(), f"{what}: log-scales"
    rel = reconstruction_error(rows, K_out, inp["cov"])
    worst = float(rel.max(initial=0.0))
    assert worst <= 1e-5, f"{what}: R S^2 R^T off by {worst:.2e} of the largest covariance entry"
    return worst
