"""The depth-normal consistency regulariser (include/lsr_normals.h) restated in torch: one statement of operator A (the
normals of the Gaussians) and of operator B (the image-space loss), evaluated in float64 (the reference; B's leading alpha
detached, as the kernels' backward has it) and in float32 (the "stock" composition a user would write with PyTorch: the
error yardstick), and the case builders.

The error rule is that of tests/latent_ref.py: per quantity, the kernel's largest error against float64 is at most
``max(4 x the stock composition's own largest error, 2^-20 x max |want|)`` (:func:`held`).  The floor is 16 roundings of a
float32 output at the quantity's scale: a single lucky stock value does not set a bar below what a float32 result can meet.

The builders guarantee that a float32 kernel and the float64 reference take the same branch everywhere, so NO case is
excluded from comparison (:func:`check_scene_case`, :func:`check_image_case`; tests/test_normals_cpu.py asserts them):
  * the two smallest ``scaling`` entries of a Gaussian differ by at least 1e-3 relative, unless they are exactly equal;
  * |cos| between a Gaussian's axis and its view direction is at least 1e-2 in every view;
  * no pixel has alpha within 1e-3 of ``alpha_min``;
  * no interior stencil has |m| below 1e-6 of |a| |b|, unless m is exactly 0."""
import numpy as np
import torch

VIEW_FLOATS = 44
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
MARGIN, FLOOR = 4.0, 2.0 ** -20
ALPHA_MIN = 0.5
WORST = {}          # quantity -> worst kernel error / stock error seen


# ---- view records ----

def view_records(extrinsics, tanfovx, tanfovy, cx=0.0, cy=0.0, scale=1.0, near=0.1, far=100.0) -> np.ndarray:
    """(V, 44) float32 records from camera-to-world matrices (V, 4, 4) (x right, y down, z forward): the transposed
    world->view matrix of the scaled scene in 0..15, the transposed world->clip matrix in 16..31, the scaled camera
    position in 32..34, tan(fov) in 35 / 36, the scene scale in 40, depth mode NATIVE.  ``cx``, ``cy``: the principal
    point's offset from the image centre in NDC units (0: centred)."""
    ext = np.asarray(extrinsics, np.float64)
    V = ext.shape[0]
    b = lambda x: np.broadcast_to(np.asarray(x, np.float64), (V,))
    tanfovx, tanfovy, cx, cy, scale = b(tanfovx), b(tanfovy), b(cx), b(cy), b(scale)
    out = np.zeros((V, VIEW_FLOATS), np.float32)
    for v in range(V):
        c2w = ext[v].copy()
        c2w[:3, 3] *= scale[v]
        w2c = np.linalg.inv(c2w)
        n, f = near * scale[v], far * scale[v]
        P = np.zeros((4, 4))
        P[0, 0], P[0, 2] = 1.0 / tanfovx[v], cx[v]
        P[1, 1], P[1, 2] = 1.0 / tanfovy[v], cy[v]
        P[2, 2], P[2, 3] = f / (f - n), -f * n / (f - n)
        P[3, 2] = 1.0
        out[v, :16] = w2c.T.reshape(16)
        out[v, 16:32] = (P @ w2c).T.reshape(16)
        out[v, 32:35] = c2w[:3, 3]
        out[v, 35], out[v, 36], out[v, 40] = tanfovx[v], tanfovy[v], scale[v]
    return out


def circle_extrinsics(V: int, radius: float = 4.0, seed: int = 0) -> np.ndarray:
    """Camera-to-world matrices on a circle around the origin, looking at it, rolled a little (x right, y down, z forward)."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(V) + rng.uniform(0, 1)) / V
    ext = np.zeros((V, 4, 4))
    for v, a in enumerate(ang):
        offset = np.array([np.cos(a), 0.3 * np.sin(2 * a + 1.0), np.sin(a)])
        forward = -offset / np.linalg.norm(offset)
        right = np.cross(np.array([0.0, 1.0, 0.0]), forward)
        right /= np.linalg.norm(right)
        ext[v, :3, 0], ext[v, :3, 1], ext[v, :3, 2] = right, np.cross(forward, right), forward
        ext[v, :3, 3] = radius * offset
        ext[v, 3, 3] = 1.0
    return ext


def make_views(V: int, seed: int = 0, offcentre: bool = False, scale=1.0) -> np.ndarray:
    """V cameras on a circle with unequal fields of view; ``offcentre``: principal points away from the centre."""
    rng = np.random.default_rng(2000 + seed)
    cx = rng.uniform(-0.3, 0.3, V) if offcentre else 0.0
    cy = rng.uniform(-0.3, 0.3, V) if offcentre else 0.0
    return view_records(circle_extrinsics(V, 4.0, seed), rng.uniform(0.3, 0.6, V), rng.uniform(0.25, 0.5, V), cx, cy, scale)


# ---- operator A ----

def rotation_matrices(q: torch.Tensor) -> torch.Tensor:
    """(n, 3, 3) of the normalised quaternions (w, x, y, z)."""
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def axes(scaling: torch.Tensor, rotation: torch.Tensor) -> torch.Tensor:
    """(n, 3): the column of R that belongs to the smallest scaling entry (torch.argmin returns the first of equal minima)."""
    k = torch.argmin(scaling, dim=-1)
    return rotation_matrices(rotation)[torch.arange(scaling.shape[0]), :, k]


def view_cosines(views, xyz, scaling, rotation) -> torch.Tensor:
    """(V, n): the cosine between each axis and the direction to each camera, in the dtype of the inputs."""
    a = axes(scaling, rotation)
    to_cam = views[:, None, 32:35] - views[:, None, 40:41] * xyz[None]
    return (a[None] * to_cam).sum(-1) / to_cam.norm(dim=-1)


def gaussian_normals(views: torch.Tensor, xyz: torch.Tensor, scaling: torch.Tensor, rotation: torch.Tensor) -> torch.Tensor:
    """Operator A, (V, n, 3), in the dtype of the inputs."""
    a = axes(scaling, rotation)
    out = []
    for v in range(views.shape[0]):
        W3 = views[v, :16].reshape(4, 4).T[:3, :3]
        c = torch.sqrt((W3 * W3).sum() / 3.0)
        d = (a * (views[v, 32:35] - views[v, 40] * xyz)).sum(-1)
        sign = torch.where(d < 0, -torch.ones_like(d), torch.ones_like(d))
        o = sign[:, None] * (a @ W3.T) / c
        ok = torch.isfinite(d) & torch.isfinite(o).all(-1)
        out.append(torch.where(ok[:, None], o, torch.zeros_like(o)))
    return torch.stack(out)


# ---- operator B ----

def pixel_rays(view: torch.Tensor, H: int, W: int, xs: torch.Tensor, ys: torch.Tensor):
    """(rx, ry) of the camera-space rays with z = 1 through the centres of the pixels (xs, ys): per pixel the 2 x 2 solve of
    Q0 . r = ndc_x Q3 . r, Q1 . r = ndc_y Q3 . r, with Q = rows 0, 1, 3 of the projection matrix times the inverse of the
    view matrix's upper 3 x 3 (no affine shortcut: the kernels' is checked against this)."""
    A = view[:16].reshape(4, 4).T[:3, :3]
    Q = view[16:32].reshape(4, 4).T[[0, 1, 3], :3] @ torch.linalg.inv(A)
    nx, ny = (2 * xs + 1) / W - 1, (2 * ys + 1) / H - 1
    m00, m01, b0 = Q[0, 0] - nx * Q[2, 0], Q[0, 1] - nx * Q[2, 1], nx * Q[2, 2] - Q[0, 2]
    m10, m11, b1 = Q[1, 0] - ny * Q[2, 0], Q[1, 1] - ny * Q[2, 1], ny * Q[2, 2] - Q[1, 2]
    det = m00 * m11 - m01 * m10
    return (b0 * m11 - m01 * b1) / det, (m00 * b1 - b0 * m10) / det


def stencils(depth: torch.Tensor, alpha: torch.Tensor, views: torch.Tensor, alpha_min: float = ALPHA_MIN) -> dict:
    """Everything about the interior stencils of (V, H, W) maps, in their dtype: ``a``, ``b``, ``m`` (V, H-2, W-2, 3), ``norm``,
    ``usable`` (alpha above the threshold and D finite at all five pixels), ``valid``, ``sigma`` (V,)."""
    V, H, W = depth.shape
    dt = depth.dtype
    ok = alpha > alpha_min
    D = torch.where(ok, depth, torch.zeros_like(depth)) / torch.where(ok, alpha, torch.ones_like(alpha))
    ok = ok & torch.isfinite(D)
    D = torch.where(ok, D, torch.zeros_like(D))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    P, sigma = [], []
    for v in range(V):
        rx, ry = pixel_rays(views[v], H, W, xs, ys)
        P.append(D[v][..., None] * torch.stack([rx, ry, torch.ones_like(rx)], -1))
        ox, oy = pixel_rays(views[v], H, W, torch.tensor([0.0, 1.0, 0.0], dtype=dt), torch.tensor([0.0, 0.0, 1.0], dtype=dt))
        det = (ox[1] - ox[0]) * (oy[2] - oy[0]) - (ox[2] - ox[0]) * (oy[1] - oy[0])
        sigma.append(-1.0 if float(det) > 0 else 1.0)
    P = torch.stack(P)
    a = P[:, 1:-1, 2:] - P[:, 1:-1, :-2] if W >= 3 and H >= 3 else P.new_zeros((V, max(H - 2, 0), max(W - 2, 0), 3))
    b = P[:, 2:, 1:-1] - P[:, :-2, 1:-1] if W >= 3 and H >= 3 else a
    m = torch.linalg.cross(a, b, dim=-1)
    norm = m.norm(dim=-1)
    if W >= 3 and H >= 3:
        usable = ok[:, 1:-1, 1:-1] & ok[:, 1:-1, 2:] & ok[:, 1:-1, :-2] & ok[:, 2:, 1:-1] & ok[:, :-2, 1:-1]
    else:
        usable = torch.zeros(norm.shape, dtype=torch.bool)
    valid = usable & (norm >= FLT_MIN) & (norm <= FLT_MAX)
    return dict(a=a, b=b, m=m, norm=norm, usable=usable, valid=valid, sigma=torch.tensor(sigma, dtype=dt))


def consistency(normal_map: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, views: torch.Tensor,
                alpha_min: float = ALPHA_MIN) -> dict:
    """Operator B in the dtype of the inputs: ``loss``, ``per_view (V,)``, ``depth_normals (V, 3, H, W)``, ``valid (V, H, W)``.
    The leading alpha of e is detached."""
    V, H, W = depth.shape
    s = stencils(depth, alpha, views, alpha_min)
    valid = torch.zeros((V, H, W), dtype=torch.bool)
    normals = depth.new_zeros((V, H, W, 3))
    e = depth.new_zeros((V, H, W))
    if H >= 3 and W >= 3:
        valid[:, 1:-1, 1:-1] = s["valid"]
        safe = torch.where(s["valid"], s["norm"], torch.ones_like(s["norm"]))
        n = torch.where(s["valid"][..., None], s["sigma"][:, None, None, None] * s["m"] / safe[..., None], torch.zeros_like(s["m"]))
        normals = torch.nn.functional.pad(n, (0, 0, 1, 1, 1, 1))
        N = normal_map.permute(0, 2, 3, 1)
        e = torch.where(valid, alpha.detach() - (N * normals).sum(-1), torch.zeros_like(alpha))
    per_view = e.sum((1, 2)) / (H * W)
    return dict(loss=per_view.mean(), per_view=per_view, depth_normals=normals.permute(0, 3, 1, 2), valid=valid)


def to(dt, *arrays):
    return [torch.from_numpy(np.asarray(a)).to(dt) for a in arrays]


def normals_and_grad(case: dict, upstream: np.ndarray, dt) -> dict:
    """Operator A and its rotation gradient under ``upstream`` (V, n, 3), in ``dt``, as float64 numpy arrays."""
    views, xyz, scaling, rotation, up = to(dt, case["views"], case["xyz"], case["scaling"], case["rotation"], upstream)
    rotation.requires_grad_(True)
    out = gaussian_normals(views, xyz, scaling, rotation)
    (out * up).sum().backward()
    return dict(normals=out.detach().double().numpy(), grad_rotation=rotation.grad.double().numpy())


def consistency_and_grads(case: dict, grad_loss: float, dt) -> dict:
    """Operator B and its three gradients under the upstream ``grad_loss``, in ``dt``, as float64 numpy arrays."""
    N, depth, alpha, views = to(dt, case["normal_map"], case["depth"], case["alpha"], case["views"])
    for t in (N, depth, alpha):
        t.requires_grad_(True)
    out = consistency(N, depth, alpha, views, case["alpha_min"])
    if out["loss"].requires_grad:            # (an image without an interior has a constant loss of 0)
        (out["loss"] * grad_loss).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = {k: v.detach().double().numpy() for k, v in out.items() if k != "valid"}
    res["valid"] = out["valid"].numpy()
    res["loss"] = res["loss"].reshape(1)
    res.update(grad_normal_map=zero(N).double().numpy(), grad_depth=zero(depth).double().numpy(),
               grad_alpha=zero(alpha).double().numpy())
    return res


def held(name: str, got, want: np.ndarray, stock: np.ndarray, show: str = "") -> None:
    """The rule of the module docstring for one quantity; prints kernel error, stock error and their ratio first."""
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


# ---- case builders ----

def scene_case(n: int, V: int, seed: int, quat_scale: float = 1.0, scale40=1.0, ties: str = "") -> dict:
    """float32 arrays ``views (V, 44)``, ``xyz``, ``scaling`` (log-scales), ``rotation`` (raw, times ``quat_scale``) that meet
    the conditions of the module docstring.  ``ties``: "two" makes the two smallest log-scales of every third Gaussian
    exactly equal (at every pair of indices in turn), "three" all three."""
    rng = np.random.default_rng(seed)
    views = make_views(V, seed, offcentre=True, scale=scale40)
    xyz = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    scaling = np.empty((n, 3), np.float32)
    for g in range(n):                       # distinct log-scales, at least 0.05 apart (far beyond 1e-3 relative)
        while True:
            s = rng.uniform(-4.0, -1.0, 3)
            if np.diff(np.sort(s)).min() >= 0.05:
                break
        scaling[g] = s
    if ties:
        for g in range(0, n, 3):
            order = np.argsort(scaling[g])
            if ties == "three":
                scaling[g] = scaling[g, order[0]]
            else:
                pair = [(0, 1), (0, 2), (1, 2)][(g // 3) % 3]
                low, top = scaling[g, order[0]], scaling[g, order[2]]
                scaling[g] = top
                scaling[g, list(pair)] = low
    rotation = rng.standard_normal((n, 4))
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for _ in range(100):                     # redraw the axes that lie within 1e-2 of perpendicular to a view direction
        q32 = (rotation * quat_scale).astype(np.float32)
        cos = view_cosines(t64(views), t64(xyz), t64(scaling), t64(q32)).abs().min(0).values.numpy()
        bad = cos < 2e-2
        if not bad.any():
            break
        rotation[bad] = rng.standard_normal((int(bad.sum()), 4))
    return dict(views=views, xyz=xyz, scaling=scaling, rotation=(rotation * quat_scale).astype(np.float32))


def check_scene_case(case: dict) -> None:
    s = np.sort(case["scaling"].astype(np.float64), axis=1)
    gap = (s[:, 1] - s[:, 0]) / np.maximum(np.abs(s[:, 0]), np.abs(s[:, 1]))
    assert ((gap >= 1e-3) | (s[:, 1] == s[:, 0])).all()
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    cos = view_cosines(t64(case["views"]), t64(case["xyz"]), t64(case["scaling"]), t64(case["rotation"]))
    assert float(cos.abs().min()) >= 1e-2


def image_case(V: int, H: int, W: int, seed: int, offcentre: bool = False, scale40=1.0, holes: bool = True,
               zero_block: bool = False, alpha_min: float = ALPHA_MIN) -> dict:
    """float32 maps ``normal_map (V, 3, H, W)``, ``depth``, ``alpha`` (V, H, W) and ``views`` that meet the conditions of the
    module docstring: a smooth surface D = plane + ripples under a smooth alpha in [0.6, 1), with holes of alpha 0.1 (one
    pixel wide and wider; inside, across the tile seams at 31 | 32 and 63 | 64, and next to the borders) and, with
    ``zero_block``, a block of zero depth under a solid alpha (m = 0 exactly: invalid)."""
    rng = np.random.default_rng(seed)
    views = make_views(V, seed, offcentre, scale40)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth, alpha, nmap = (np.empty((V, H, W), np.float32), np.empty((V, H, W), np.float32), np.empty((V, 3, H, W), np.float32))
    for v in range(V):
        gx, gy, ph = rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0, 6.28, 2)
        D = 3.0 + gx * xs + gy * ys + 0.05 * np.sin(0.37 * xs + ph[0]) * np.cos(0.29 * ys + ph[1]) + 0.002 * rng.standard_normal((H, W))
        al = 0.8 + 0.19 * np.sin(0.21 * xs + 0.13 * ys + ph[0])
        big = H >= 16 and W >= 16            # (the smallest images keep their few interior pixels)
        if holes and big:
            for (y, x, h, w) in ((H // 2, W // 2, 1, 1), (1, 1, 1, 2), (H - 2, W - 3, 1, 1), (30, 29, 4, 5), (62, 20, 3, 1),
                                 (10, 31, 1, 2), (H // 3, 0, 2, 1)):
                if 0 <= y < H and 0 <= x < W:
                    al[y:y + h, x:x + w] = 0.1
        if zero_block and big:
            D[H // 4:H // 4 + 4, W // 4:W // 4 + 4] = 0.0
            al[H // 4:H // 4 + 4, W // 4:W // 4 + 4] = 0.9
        alpha[v] = al
        depth[v] = (D * float(np.float64(scale40) if np.ndim(scale40) == 0 else scale40[v])) * alpha[v].astype(np.float64)
        n = rng.standard_normal((3, H, W)) * 0.3 + np.array([0.0, 0.0, -1.0])[:, None, None]
        nmap[v] = n / np.linalg.norm(n, axis=0) * alpha[v]
    return dict(normal_map=nmap, depth=depth, alpha=alpha, views=views, alpha_min=alpha_min)


def check_image_case(case: dict) -> None:
    assert (np.abs(case["alpha"].astype(np.float64) - case["alpha_min"]) >= 1e-3).all()
    depth, alpha, views = to(torch.float64, case["depth"], case["alpha"], case["views"])
    s = stencils(depth, alpha, views, case["alpha_min"])
    size = s["a"].norm(dim=-1) * s["b"].norm(dim=-1)
    u = s["usable"]
    assert bool(((s["norm"] == 0) | (s["norm"] >= 1e-6 * size))[u].all())
    assert bool(((s["norm"] == 0) | (s["norm"] >= 1e3 * FLT_MIN))[u].all()) and bool((s["norm"][u] <= 1e-3 * FLT_MAX).all())
