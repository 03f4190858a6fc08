"""The depth distortion regulariser (include/lsr_distortion.h) restated in torch: one statement of operator A (the depth
moments of the Gaussians) and of operator B (the image-space pair term), evaluated in float64 (the reference) and in float32
(the "stock" composition a user would write with PyTorch: the error yardstick), the pair sum and the 2DGS recurrence written
out literally, the case builders, and the float64 chain through the oracle's rasterizer.

The error rule is the project's standing one (tests/normals_ref.py): per quantity, the kernel's largest error against
float64 is at most ``max(4 x the stock composition's own largest error, 2^-20 x max |want|)`` (:func:`held`); the worst
ratio per quantity goes into :data:`WORST`."""
import numpy as np
import torch

from tests import normals_ref as nref

SPACES = ("linear", "ndc", "disparity")
MARGIN, FLOOR = nref.MARGIN, nref.FLOOR
WORST = {}          # quantity -> worst kernel error / stock error seen
NEAR, FAR = 0.5, 50.0
GRAD_LOSS = 0.75


def held(name: str, got, want: np.ndarray, stock: np.ndarray, show: str = "") -> None:
    """normals_ref.held with this module's table."""
    got = np.asarray(got, np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), (show, name, "not finite")
    err = float(np.abs(got - want).max()) if want.size else 0.0
    err_stock = float(np.abs(stock - want).max()) if want.size else 0.0
    scale = float(np.abs(want).max()) if want.size else 0.0
    bar = max(MARGIN * err_stock, FLOOR * scale)
    ratio = err / err_stock if err_stock > 0 else (0.0 if err == 0 else float("inf"))
    if np.isfinite(ratio):
        WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{show} {name:16s} kernel {err:.3e}  stock {err_stock:.3e}  ratio {ratio:.3f}  scale {scale:.3e}  bar {bar:.3e}")
    assert err <= bar, (show, name, err, err_stock, bar)


# ---- the identity ----

def blend_weights(alphas: np.ndarray) -> np.ndarray:
    """w_i = alpha_i T_i, T_i = prod_{j<i} (1 - alpha_j): a real front-to-back blend, float64."""
    a = np.asarray(alphas, np.float64)
    return a * np.concatenate([[1.0], np.cumprod(1.0 - a)[:-1]])


def pair_sum(w: np.ndarray, m: np.ndarray) -> float:
    """sum_i sum_{j<i} w_i w_j (m_i - m_j)^2, brute force."""
    return float(sum(w[i] * w[j] * (m[i] - m[j]) ** 2 for i in range(len(w)) for j in range(i)))


def moment_form(w: np.ndarray, m: np.ndarray) -> float:
    return float(w.sum() * (w * m * m).sum() - (w * m).sum() ** 2)


def recurrence_2dgs(w: np.ndarray, m: np.ndarray) -> float:
    """The running sums of the 2DGS rasterizer, front to back: per entry ``error = m^2 A + M2 - 2 m M1`` with the sums of the
    entries BEFORE it, ``D += error w``, then the sums take the entry."""
    A = M1 = M2 = D = 0.0
    for wi, mi in zip(w, m):
        D += (mi * mi * A + M2 - 2.0 * mi * M1) * wi
        A += wi
        M1 += wi * mi
        M2 += wi * mi * mi
    return float(D)


# ---- operator A ----

def depths(views: torch.Tensor, xyz: torch.Tensor) -> torch.Tensor:
    """(V, n): the view-space z of the scaled means divided by slot 40, as the definition reads."""
    s = views[:, 40:41]
    tz = (s[:, :, None] * xyz[None]) @ torch.stack([views[:, 2], views[:, 6], views[:, 10]], -1)[:, :, None]
    return (tz[..., 0] + views[:, 14:15]) / s


def depth_moments(views: torch.Tensor, xyz: torch.Tensor, space: str, pivot=None) -> torch.Tensor:
    """Operator A, (V, n, 2), in the dtype of the inputs."""
    z = depths(views, xyz)
    ok = torch.isfinite(z) & (z > 0)
    zs = torch.where(ok, z, torch.ones_like(z))
    if space == "linear":
        m = zs
    elif space == "disparity":
        m = 1.0 / zs
    else:
        n, f = views[:, 42:43], views[:, 43:44]
        m = f / (f - n) * (1.0 - n / zs)
    mp = m - (0.0 if pivot is None else pivot[:, None])
    out = torch.stack([mp, mp * mp], -1)
    ok = ok & torch.isfinite(out).all(-1)
    return torch.where(ok[..., None], out, torch.zeros_like(out))


def pivot_of(views: np.ndarray, point, space: str) -> np.ndarray:
    """depth_pivot by hand in numpy float64, (V,) float32."""
    v = np.asarray(views, np.float64)
    p = np.asarray(point, np.float64)
    z = (v[:, 2] * p[0] + v[:, 6] * p[1] + v[:, 10] * p[2]) + v[:, 14] / v[:, 40]
    m = z if space == "linear" else 1.0 / z if space == "disparity" else v[:, 43] / (v[:, 43] - v[:, 42]) * (1.0 - v[:, 42] / z)
    return m.astype(np.float32)


def scene_case(n: int, V: int, seed: int, scale40=1.0, with_pivot: bool = True, space: str = "ndc") -> dict:
    """float32 ``views`` (near / far in slots 42 / 43), ``xyz`` in front of every camera (z between about 2 and 6), ``pivot``."""
    rng = np.random.default_rng(seed)
    views = nref.make_views(V, seed, offcentre=True, scale=scale40)
    views[:, 42], views[:, 43] = NEAR, FAR
    xyz = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    pivot = pivot_of(views, (0.1, -0.05, 0.2), space) if with_pivot else None
    return dict(views=views, xyz=xyz, pivot=pivot, space=space)


def moments_and_grad(case: dict, upstream: np.ndarray, dt) -> dict:
    views, xyz, up = nref.to(dt, case["views"], case["xyz"], upstream)
    pivot = None if case["pivot"] is None else torch.from_numpy(case["pivot"]).to(dt)
    xyz.requires_grad_(True)
    out = depth_moments(views, xyz, case["space"], pivot)
    (out * up).sum().backward()
    return dict(moments=out.detach().double().numpy(), grad_xyz=xyz.grad.double().numpy())


# ---- operator B ----

def distortion(moment_map: torch.Tensor, alpha: torch.Tensor, weight=None) -> dict:
    """Operator B in the dtype of the inputs: ``loss``, ``per_view (V,)``, ``distortion (V, H, W)``."""
    d = alpha * moment_map[:, 1] - moment_map[:, 0] * moment_map[:, 0]
    per_view = (d if weight is None else weight * d).sum((1, 2)) / (alpha.shape[1] * alpha.shape[2])
    return dict(loss=per_view.mean(), per_view=per_view, distortion=d)


def image_case(V: int, H: int, W: int, seed: int, weighted: bool) -> dict:
    """float32 maps as a render of layers close together leaves them: alpha in (0.1, 1), M1 = alpha (mean + noise), M2 a
    little above M1^2 / alpha; ``weight`` in [0, 1] with zeros."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.1, 0.999, (V, H, W))
    mean = rng.uniform(-0.5, 0.5, (V, H, W))
    var = rng.uniform(0.0, 0.05, (V, H, W))
    mm = np.stack([alpha * mean, alpha * (mean * mean + var)], 1).astype(np.float32)
    weight = None
    if weighted:
        weight = rng.uniform(0.0, 1.0, (V, H, W))
        weight[rng.uniform(size=(V, H, W)) < 0.2] = 0.0
        weight = weight.astype(np.float32)
    return dict(moment_map=mm, alpha=alpha.astype(np.float32), weight=weight)


def distortion_and_grads(case: dict, dt) -> dict:
    mm, alpha = nref.to(dt, case["moment_map"], case["alpha"])
    weight = None if case["weight"] is None else torch.from_numpy(case["weight"]).to(dt)
    mm.requires_grad_(True)
    alpha.requires_grad_(True)
    out = distortion(mm, alpha, weight)
    (out["loss"] * GRAD_LOSS).backward()
    res = {k: v.detach().double().numpy() for k, v in out.items()}
    res["loss"] = res["loss"].reshape(1)
    res.update(grad_moment_map=mm.grad.double().numpy(), grad_alpha=alpha.grad.double().numpy())
    return res


# ---- through the rasterizer ----

def forward_views(V: int, scale40=1.0) -> np.ndarray:
    """V cameras near the origin looking down +z (x right, y down), a little apart and turned: records of depth mode NATIVE
    with near / far in slots 42 / 43."""
    ext = np.tile(np.eye(4), (V, 1, 1))
    for v in range(V):
        a = 0.06 * v
        ext[v, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        ext[v, :3, 3] = (0.15 * v, -0.05 * v, 0.0)
    views = nref.view_records(ext, 0.5, 0.45, scale=scale40)
    views[:, 42], views[:, 43] = NEAR, FAR
    return views


def layered_params(n: int, seed: int, z_lo: float, z_hi: float, K: int = 4) -> dict:
    """Raw scene parameters of n Gaussians between depths z_lo and z_hi inside the frustum of :func:`forward_views`."""
    from tests import scene_params_ref as sref
    p = sref.make_params(n, K, seed=seed)
    rng = np.random.default_rng(seed)
    z = rng.uniform(z_lo, z_hi, n)
    p["xyz"] = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], 1).astype(np.float32)
    p["scaling"] = np.log(rng.uniform(0.05, 0.2, (n, 3)) * (z[:, None] / 4.0)).astype(np.float32)
    p["opacity"] = rng.uniform(-1.0, 2.0, (n, 1)).astype(np.float32)
    return p


def float64_chain(params: dict, views: np.ndarray, H: int, W: int, space: str, pivot=None, weight=None, grads: bool = True):
    """render_with_distortion + distortion_loss in float64 on the host, from the shared chain (tests/surface_chain_ref.py):
    the activation restated (tests/scene_params_ref.py), operator A restated, the oracle's rasterizer per view with the moments
    as features, operator B restated.
    ``(loss, distortion map (V, H, W), moment map, gradients of xyz, scaling, rotation, opacity)``."""
    from tests import surface_chain_ref as chain
    res = chain.chain(params, views, H, W, dict(dist=1.0), space=space, pivot=pivot, dist_weight=weight, grads=grads)
    g = {k: res["grad"][k] for k in ("xyz", "scaling", "rotation", "opacity")} if grads else {}
    return res["terms"]["dist"], res["maps"]["distortion"], res["maps"]["moment_map"], g


def scene_of(params: dict, dev):
    from latentsplat_amd import GaussianScene
    return GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in params.items()}).to(dev)


PLANE = 4.0


def pivot_errors(dev) -> dict:
    """The pivot measured: Gaussians within +-0.01 of the plane z = 4 in front of one camera at the origin, 32 x 32,
    ``space="linear"``.  The distortion map of the float32 pipeline (operator A, the rasterizer, operator B) against the
    float64 chain, once with pivot 0 and once with ``depth_pivot`` at the plane: the largest absolute errors, their ratio
    and the largest value of the map."""
    from latentsplat_amd.distortion import depth_pivot, distortion_map
    n, H, W = 300, 32, 32
    p = layered_params(n, 11, PLANE - 0.01, PLANE + 0.01)
    views = forward_views(1)
    _, want, _, _ = float64_chain(p, views, H, W, "linear", grads=False)
    scene, tv = scene_of(p, dev), torch.from_numpy(views).to(dev)
    res = {}
    with torch.no_grad():
        for name, pivot in (("pivot_0", None), ("pivoted", depth_pivot(tv, (0.0, 0.0, PLANE), "linear"))):
            _, mm, mask, _, _ = scene.render_with_distortion(tv, H, W, space="linear", pivot=pivot)
            res["err_" + name] = float(np.abs(distortion_map(mm, mask).cpu().numpy().astype(np.float64) - want).max())
    res["ratio"] = res["err_pivot_0"] / res["err_pivoted"] if res["err_pivoted"] > 0 else float("inf")
    res["max_distortion"] = float(np.abs(want).max())
    return res
