"""Restatement of the 3DGS activation map for the tests (tests/test_scene_params_*.py): the raw parameters upcast
exactly to float64, the forward of tests/ply_import_ref.py's ``expected`` written in torch so that autograd gives the
gradients, and the bars both directions are held to.  Also the parameter draws and the scene file the tests share."""
from __future__ import annotations

import numpy as np
import torch

from tests import ply_import_ref as ref

PARAMS = ("features_dc", "features_rest", "opacity", "scaling", "rotation")


def split_table(table: np.ndarray, names: list) -> dict:
    """The raw parameter arrays (float32, the table's values) of a row table: xyz (n,3), features_dc (n,1,3),
    features_rest (n,K-1,3) from the channel-major f_rest columns, opacity (n,1), scaling (n,3), rotation (n,4)."""
    n = table.shape[0]
    K = sum(1 for x in names if x.startswith("f_rest_")) // 3 + 1
    col = lambda ks: np.stack([table[:, names.index(k)] for k in ks], 1)
    rest = col([f"f_rest_{i}" for i in range(3 * (K - 1))]).reshape(n, 3, K - 1).transpose(0, 2, 1) if K > 1 \
        else np.zeros((n, 0, 3), np.float32)
    return dict(xyz=col("xyz"), features_dc=col([f"f_dc_{i}" for i in range(3)]).reshape(n, 1, 3),
                features_rest=np.ascontiguousarray(rest), opacity=col(["opacity"]),
                scaling=col([f"scale_{i}" for i in range(3)]), rotation=col([f"rot_{i}" for i in range(4)]))


def make_params(n: int, K: int, seed: int) -> dict:
    """Raw parameters drawn as ``ply_import_ref.make_table`` draws them: log-scales in [-7, 1], logits in [-8, 8],
    quaternion norms in [0.1, 10]."""
    names = ref.standard_names(K)
    return split_table(ref.make_table(n, names, seed), names)


def make_upstream(n: int, K: int, seed: int) -> dict:
    """Seeded normal upstream gradients of shs, opacities and cov3D (float32)."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(shs=f(n, K, 3), opacities=f(n, 1), cov3D=f(n, 6))


def forward64(p: dict, scale_modifier: float = 1.0) -> dict:
    """The forward on float64 torch tensors (differentiable), as ``ply_import_ref.expected`` states it, with the scales
    multiplied by the modifier."""
    shs = torch.cat([p["features_dc"], p["features_rest"]], 1)
    opac = 1.0 / (1.0 + torch.exp(-p["opacity"]))
    scales = scale_modifier * torch.exp(p["scaling"])
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


def expected(p: dict, scale_modifier: float = 1.0) -> dict:
    """The forward's outputs rounded to float32 (numpy), in the shape ``ply_import_ref.assert_matches`` takes."""
    with torch.no_grad():
        out = forward64(_t64(p), scale_modifier)
    return {k: v.numpy().astype(np.float32) for k, v in out.items()}


def gradients(p: dict, upstream: dict, scale_modifier: float = 1.0) -> dict:
    """float64 autograd: the gradients of the five raw tensors for the upstream gradients given (a missing or ``None``
    entry is zero), and the float64 ``cov3D`` the bars are scaled by."""
    t = _t64(p, grad=True)
    out = forward64(t, scale_modifier)
    loss = sum((out[k] * torch.from_numpy(np.asarray(g, np.float64))).sum() for k, g in upstream.items() if g is not None)
    got = torch.autograd.grad(loss, [t[k] for k in PARAMS], allow_unused=True)
    res = {k: (np.zeros(t[k].shape) if g is None else g.numpy()) for k, g in zip(PARAMS, got)}
    res["cov3D"] = out["cov3D"].detach().numpy()
    return res


def assert_backward_matches(got: dict, p: dict, upstream: dict, scale_modifier: float = 1.0, show: str = "") -> None:
    """The bars of the backward, per Gaussian, against :func:`gradients` (``got``: float32 arrays, any subset of the five):
    SH gradients bit-equal to the re-layout of the upstream shs gradient; ``|d_opacity err| <= 2e-5 |g_o|``; each d_scaling
    row within ``2e-5 max|cov_g| max|g_cov,g|``, each d_rotation row within that over ``|q_g|``."""
    want = gradients(p, upstream, scale_modifier)
    n = p["opacity"].shape[0]
    g_shs, g_o, g_cov = (upstream.get(k) for k in ("shs", "opacities", "cov3D"))
    if "features_dc" in got:
        assert np.array_equal(got["features_dc"], np.zeros((n, 1, 3), np.float32) if g_shs is None else g_shs[:, :1, :])
    if "features_rest" in got:
        K = p["features_rest"].shape[1] + 1
        assert np.array_equal(got["features_rest"], np.zeros((n, K - 1, 3), np.float32) if g_shs is None else g_shs[:, 1:, :])
    if "opacity" in got:
        err = np.abs(got["opacity"].astype(np.float64) - want["opacity"])
        bound = 2e-5 * np.abs(np.zeros((n, 1)) if g_o is None else g_o.astype(np.float64))
        print(f"{show} d_opacity: worst err / |g_o| {np.max(err / np.maximum(bound / 2e-5, 1e-300), initial=0.0):.3e}")
        assert (err <= bound).all()
    scale = np.abs(want["cov3D"]).max(1, keepdims=True) * \
        (np.zeros((n, 1)) if g_cov is None else np.abs(g_cov.astype(np.float64)).max(1, keepdims=True))
    for k, s in (("scaling", scale), ("rotation", scale / np.linalg.norm(p["rotation"].astype(np.float64), axis=1, keepdims=True))):
        if k in got:
            assert got[k].shape == want[k].shape
            err = np.abs(got[k].astype(np.float64) - want[k])
            print(f"{show} d_{k}: worst err / scale {np.max(err / np.maximum(s, 1e-300), initial=0.0):.3e} (bar 2e-5)")
            assert (err <= 2e-5 * s).all(), k


def expected_rows(p: dict) -> np.ndarray:
    """The rows of the scene file that holds these raw parameters, in the published property order."""
    n = p["xyz"].shape[0]
    rest = p["features_rest"].transpose(0, 2, 1).reshape(n, -1)
    return np.concatenate([p["xyz"], np.zeros((n, 3), np.float32), p["features_dc"].reshape(n, 3), rest, p["opacity"],
                           p["scaling"], p["rotation"]], 1).astype(np.float32)


def write_scene_file(path, G: int = 2000, W: int = 64, views: int = 2, rest_scale: float = 1.0):
    """A degree-1 scene of G Gaussians in front of ``views`` cameras as a standard scene file (the recipe of
    tests/test_ply_import_gpu.py's ``scene_file``): positions, projected sizes and opacities of the synthetic test
    scenes, orientations and SH coefficients drawn here.  Returns the synthetic scene (cameras) and the table."""
    from tests import util
    sc = util.make_scene(G, image_size=W, views=views, color_sh_degree=1, feature_channels=None)
    rng = np.random.default_rng(5)
    names = ref.standard_names(4)
    table = np.zeros((G, len(names)), np.float32)
    col = names.index
    z = sc.means[:, 2].numpy()
    major = np.exp(rng.uniform(np.log(0.3), np.log(3.0), G)) * z / (0.8 * W)
    table[:, col("x"):col("x") + 3] = sc.means.numpy()
    for k in range(3):
        table[:, col(f"scale_{k}")] = np.log(major * (1.0 if k == 0 else rng.uniform(0.3, 1.0, G)))
    table[:, col("rot_0"):col("rot_0") + 4] = rng.standard_normal((G, 4)) * rng.uniform(0.5, 2.0, (G, 1))
    p = sc.opacities.numpy().astype(np.float64).clip(1e-4, 1 - 1e-4)
    table[:, col("opacity")] = np.log(p / (1 - p))
    sh = sc.color_sh.numpy()                                           # (G, 3, K): channel-major, as the file stores it
    table[:, col("f_dc_0"):col("f_dc_0") + 3] = sh[:, :, 0]
    table[:, col("f_rest_0"):col("f_rest_0") + 9] = sh[:, :, 1:].reshape(G, 9) * rest_scale
    ref.write_ply(path, names, table)
    return sc, table, names
