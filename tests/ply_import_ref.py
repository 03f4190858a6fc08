"""Restatement of the .ply import for the tests (tests/test_ply_import_*.py): numpy, float64 inside, rounded to float32
at the end.  Also writes the scene files the tests read: the published 3DGS ``point_cloud.ply`` layout, with the
properties in any order and with extra ones."""
from __future__ import annotations

import numpy as np


def standard_names(K: int) -> list:
    """Property order of the published 3DGS trainer's files for K SH coefficients per channel."""
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
    names += [f"f_rest_{i}" for i in range(3 * (K - 1))] + ["opacity"]
    return names + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]


def shuffled_names(K: int, extra: int, seed: int) -> list:
    """The same properties without the normals, with ``extra`` other float properties, in a seeded random order."""
    names = [n for n in standard_names(K) if n not in ("nx", "ny", "nz")] + [f"extra_{i}" for i in range(extra)]
    order = np.random.default_rng(seed).permutation(len(names))
    return [names[i] for i in order]


def make_table(n: int, names: list, seed: int) -> np.ndarray:
    """(n, len(names)) float32.  Log-scales uniform in [-7, 1], opacity logits in [-8, 8], quaternions not normalised
    with norms in [0.1, 10]; every other column is drawn around its own centre, so that no two columns are alike and
    a swapped offset or a transposed coefficient layout changes the result."""
    rng = np.random.default_rng(seed)
    t = np.empty((n, len(names)), np.float64)
    q = rng.standard_normal((n, 4))
    q *= (rng.uniform(0.1, 10.0, (n, 1)) / np.linalg.norm(q, axis=1, keepdims=True))
    for j, name in enumerate(names):
        if name.startswith("scale_"):
            t[:, j] = rng.uniform(-7.0, 1.0, n)
        elif name == "opacity":
            t[:, j] = rng.uniform(-8.0, 8.0, n)
        elif name.startswith("rot_"):
            t[:, j] = q[:, int(name[4:])]
        else:
            t[:, j] = rng.standard_normal(n) * 0.5 + (j % 23) - 11
    return t.astype(np.float32)


def write_ply(path, names: list, table: np.ndarray, comments=(), fmt="binary_little_endian", prop_type="float",
              count=None, tail=b"") -> None:
    lines = ["ply", f"format {fmt} 1.0"] + [f"comment {c}" for c in comments]
    lines += [f"element vertex {table.shape[0] if count is None else count}"]
    lines += [f"property {prop_type} {n}" for n in names] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode())
        f.write(np.ascontiguousarray(table, "<f4").tobytes())
        f.write(tail)


def expected(table: np.ndarray, names: list, opacity: str = "logit") -> dict:
    """means (n,3), shs (n,K,3), opacities (n,1), scales (n,3), rotations (n,4), cov3D (n,6) as float32."""
    t = np.asarray(table, np.float64)
    col = lambda name: t[:, names.index(name)]
    n = t.shape[0]
    K = sum(1 for x in names if x.startswith("f_rest_")) // 3 + 1
    means = np.stack([col(k) for k in "xyz"], 1)
    shs = np.empty((n, K, 3))
    for c in range(3):
        shs[:, 0, c] = col(f"f_dc_{c}")
        for k in range(K - 1):
            shs[:, 1 + k, c] = col(f"f_rest_{c * (K - 1) + k}")      # the file is channel-major
    o = col("opacity")
    opac = (o if opacity == "raw" else 1.0 / (1.0 + np.exp(-o)))[:, None]
    scales = np.exp(np.stack([col(f"scale_{i}") for i in range(3)], 1))
    q = np.stack([col(f"rot_{i}") for i in range(4)], 1)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    M = R * scales[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    f = lambda a: a.astype(np.float32)
    return dict(means=f(means), shs=f(shs), opacities=f(opac), scales=f(scales), rotations=f(q), cov3D=f(cov))


def assert_matches(got: dict, want: dict) -> None:
    """means / shs bit-equal; opacities, scales, rotations within rtol = atol = 2e-5 (the bar the export's logf is
    held to); cov3D within 2e-5 of that Gaussian's largest covariance entry."""
    for k in ("means", "shs"):
        if k in got:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in ("opacities", "scales", "rotations"):
        if k in got:
            assert got[k].shape == want[k].shape
            np.testing.assert_allclose(got[k], want[k], rtol=2e-5, atol=2e-5, err_msg=k)
    if "cov3D" in got:
        assert got["cov3D"].shape == want["cov3D"].shape
        bound = 2e-5 * np.abs(want["cov3D"].astype(np.float64)).max(1, keepdims=True)
        err = np.abs(got["cov3D"].astype(np.float64) - want["cov3D"])
        assert (err <= bound).all(), f"cov3D: worst err / largest entry {np.max(err / bound) * 2e-5:.3e}"
