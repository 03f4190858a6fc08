"""Differentiable PyTorch-CPU restatement of the rasterizer (ORACLE — test infrastructure only,
parity unpinned; see raster_oracle.c header for what it follows).

Independent of raster_oracle.c's hand-derived backward: gradients here come from autograd, so
agreement between the two pins the analytic backward:
  (a) straight-through ``min(0.99, .)``; (b) skipped contributions are masked, not branched;
  (c) early termination is a stop mask computed under ``no_grad``; (d) the 1.3*tanfov clamp
  zeroes d/dt.x, d/dt.y and treats the clamped t.x as constant w.r.t. t.z.

Dense (pixels x Gaussians) evaluation: small cases only (G <= ~2k, <= 64x64).
"""
from __future__ import annotations

import torch

from . import oracle as _o  # noqa: F401  (same package; constants shared by value below)

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
         -0.4570457994644658, 1.445305721320277, -0.5900435899266435]
SH_C4 = [2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892,
         0.10578554691520431, -0.6690465435572892, 0.47308734787878004, -1.7701307697799304,
         0.6258357354491761]


def sh_basis(deg: int, d: torch.Tensor) -> torch.Tensor:
    """(G,3) unit dirs -> (G,(deg+1)^2) basis in the upstream axis convention."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    b = [torch.full_like(x, SH_C0)]
    if deg >= 1:
        b += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if deg >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    if deg >= 3:
        b += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
              SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy),
              SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)]
    if deg >= 4:
        b += [SH_C4[0] * xy * (xx - yy), SH_C4[1] * yz * (3 * xx - yy), SH_C4[2] * xy * (7 * zz - 1),
              SH_C4[3] * yz * (7 * zz - 3), SH_C4[4] * (zz * (35 * zz - 30) + 3),
              SH_C4[5] * xz * (7 * zz - 3), SH_C4[6] * (xx - yy) * (7 * zz - 1),
              SH_C4[7] * xz * (xx - 3 * yy), SH_C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(b, dim=-1)


def _clamp_mask(vm, means3D, tanfovx, tanfovy):
    """(inx, iny): the EWA Jacobian clamp decision of the C forward, bit for bit — t in float32 as
    ((a0 b0 + a1 b1) + a2 b2) + b3, the IEEE float ratio t.x / t.z against the float limit 1.3f * tanfov (not the
    matmul's t, nor a ratio or limit in double: within an ulp of the limit those decide differently, and the decision
    switches a whole gradient term)."""
    with torch.no_grad():
        m, p = vm.to(torch.float32), means3D.detach().to(torch.float32)
        t = [((m[0, k] * p[:, 0] + m[1, k] * p[:, 1]) + m[2, k] * p[:, 2]) + m[3, k] for k in range(3)]
        f = lambda x: torch.tensor(x, dtype=torch.float32)
        limx, limy = f(1.3) * f(tanfovx), f(1.3) * f(tanfovy)
        rx, ry = t[0] / t[2], t[1] / t[2]
        return (rx >= -limx) & (rx <= limx), (ry >= -limy) & (ry <= limy)


def _project(dt, H, W, tanfovx, tanfovy, vm, means3D, cov3D, inx, iny):
    """(t (G,3), cov2 (G,2,2)): view-space means and the EWA projection M S M^T (no low-pass) in dtype ``dt``; ``vm`` (4,4)
    as memory has it; (inx, iny) the forward's clamp decision."""
    G = means3D.shape[0]
    ones = torch.ones(G, 1, dtype=dt)
    t = (torch.cat([means3D, ones], 1) @ vm)[:, :3]
    tz = t[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = t[:, 0] / tz, t[:, 1] / tz
    tx = torch.where(inx, t[:, 0], (txtz.clamp(-limx, limx) * tz).detach())
    ty = torch.where(iny, t[:, 1], (tytz.clamp(-limy, limy) * tz).detach())
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], -1),
                     torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], -1)], 1)  # (G,2,3)
    Wr = vm[:3, :3].T  # Wr[r][c] = vm_mem[4c+r] = vm[c, r]
    M = J @ Wr
    S = torch.stack([cov3D[:, 0], cov3D[:, 1], cov3D[:, 2], cov3D[:, 1], cov3D[:, 3], cov3D[:, 4],
                     cov3D[:, 2], cov3D[:, 4], cov3D[:, 5]], -1).reshape(G, 3, 3)
    return t, M @ S @ M.transpose(1, 2)


LOWPASS = 0.3
RHO_FLOOR = 0.000025


def _factor(cov2):
    """sqrt(max(0.000025, det0 / det)) of the undilated (G,2,2) covariance; 1 where det == 0 (culled anyway)."""
    a0, b, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    det0 = a0 * c0 - b * b
    det = (a0 + LOWPASS) * (c0 + LOWPASS) - b * b
    det_s = torch.where(det != 0, det, torch.ones_like(det))
    return torch.sqrt(torch.clamp_min(det0 / det_s, RHO_FLOOR))


def opacity_factor(H, W, tanfovx, tanfovy, viewmatrix, means3D, cov3D, dtype=None):
    """(G,) antialiasing factor rho = sqrt(max(0.000025, det0 / det)) of every Gaussian, det0 / det the determinants of the
    projected covariance before / after the 0.3 low-pass.  Computed in ``dtype`` from casts of the inputs (default: that of
    ``means3D``) and returned in it; differentiable in the view matrix, tan(fov), means and covariances.  The clamp decision
    is the forward's float32 one in every dtype."""
    dt = means3D.dtype if dtype is None else dtype
    c = lambda x: torch.as_tensor(x).to(dt)
    vm = viewmatrix.reshape(4, 4)
    inx, iny = _clamp_mask(vm, means3D, tanfovx, tanfovy)
    return _factor(_project(dt, H, W, c(tanfovx), c(tanfovy), c(vm), c(means3D), c(cov3D), inx, iny)[1])


def rasterize(H, W, tanfovx, tanfovy, bg, viewmatrix, projmatrix, campos, sh_degree, means3D, cov3D,
              opacities, shs=None, colors_precomp=None, features=None, antialiasing: bool = False, rho_dtype=None):
    """Returns (color|None, feature|None, mask(1,H,W), depth(1,H,W), radii). All torch CPU.

    ``antialiasing``: the opacities composited are ``o * sqrt(clamp_min(det0 / det, 0.000025))`` (LSR_FWD_ANTIALIAS), det0
    of the undilated ``cov2`` below and det its own: differentiable.  ``rho_dtype``: None — the factor in the call's dtype;
    ``torch.float32`` — only the factor from float32 casts of the inputs, the rest in the call's dtype (the "stock"
    statement of the 4 x rule, tests/antialias_ref.py); ``"constant"`` — the factor detached: what a backward without its
    term returns."""
    dt = means3D.dtype
    G = means3D.shape[0]
    vm = viewmatrix.reshape(4, 4).to(dt)  # memory [4*col+row] => vm[col,row]
    pm = projmatrix.reshape(4, 4).to(dt)
    ones = torch.ones(G, 1, dtype=dt)
    ph = torch.cat([means3D, ones], 1) @ pm  # (G,4): row-vector convention == transposed matrix
    p_w = 1.0 / (ph[:, 3] + 0.0000001)
    ndc = ph[:, :2] * p_w[:, None]
    inx, iny = _clamp_mask(vm, means3D, tanfovx, tanfovy)
    t, cov2 = _project(dt, H, W, tanfovx, tanfovy, vm, means3D, cov3D, inx, iny)
    tz = t[:, 2]
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    if antialiasing:
        if rho_dtype is None or rho_dtype == "constant" or rho_dtype == dt:
            rho = _factor(cov2)
            rho = rho.detach() if rho_dtype == "constant" else rho
        else:
            rho = opacity_factor(H, W, tanfovx, tanfovy, viewmatrix, means3D, cov3D, dtype=rho_dtype).to(dt)
        opacities = opacities.reshape(-1) * rho
    ok = (tz > 0.2) & (det != 0)
    det_s = torch.where(det != 0, det, torch.ones_like(det))
    conA, conB, conC = c / det_s, -b / det_s, a / det_s
    with torch.no_grad():
        mid = 0.5 * (a + c)
        disc = torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(mid + disc, mid - disc)))
    px = (((ndc[:, 0].double() + 1.0) * W - 1.0) * 0.5).to(dt)
    py = (((ndc[:, 1].double() + 1.0) * H - 1.0) * 0.5).to(dt)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    with torch.no_grad():
        def ti(v):
            return torch.nan_to_num(v / 16.0, nan=0.0, posinf=1e9, neginf=-1e9).to(torch.int64)
        rminx = ti(px - radius).clamp(0, gx)
        rminy = ti(py - radius).clamp(0, gy)
        rmaxx = ti(px + radius + 15).clamp(0, gx)
        rmaxy = ti(py + radius + 15).clamp(0, gy)
        vis = ok & ((rmaxx - rminx) * (rmaxy - rminy) > 0)
        radii = torch.where(vis, radius, torch.zeros_like(radius)).to(torch.int32)

    rgb = None
    if shs is not None:
        d = means3D - campos.to(dt)[None]
        d = d / d.norm(dim=-1, keepdim=True)
        nb = (sh_degree + 1) ** 2
        rgb = torch.einsum("gk,gkc->gc", sh_basis(sh_degree, d), shs[:, :nb]) + 0.5
        rgb = torch.clamp_min(rgb, 0.0)  # autograd: zero grad where clamped (r<0)
    elif colors_precomp is not None:
        rgb = colors_precomp

    # global stable depth order == per-tile order restricted to the tile's members
    with torch.no_grad():
        order = torch.argsort(torch.where(vis, tz, torch.full_like(tz, float("inf"))), stable=True)
        order = order[: int(vis.sum())]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pxf, pyf = xs.reshape(-1).to(dt), ys.reshape(-1).to(dt)
    tile_x, tile_y = (xs.reshape(-1) // 16), (ys.reshape(-1) // 16)
    o = order
    dx = px[o][None] - pxf[:, None]
    dy = py[o][None] - pyf[:, None]
    power = -0.5 * (conA[o][None] * dx * dx + conC[o][None] * dy * dy) - conB[o][None] * dx * dy
    Gv = torch.exp(torch.clamp(power, max=0.0))
    alpha_raw = opacities.reshape(-1)[o][None] * Gv
    alpha = alpha_raw + (torch.clamp(alpha_raw, max=0.99) - alpha_raw).detach()
    with torch.no_grad():
        in_rect = ((tile_x[:, None] >= rminx[o][None]) & (tile_x[:, None] < rmaxx[o][None]) &
                   (tile_y[:, None] >= rminy[o][None]) & (tile_y[:, None] < rmaxy[o][None]))
        valid = in_rect & (power <= 0) & (alpha >= 1.0 / 255.0)
        a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
        T_excl = torch.cumprod(torch.cat([torch.ones_like(a_eff[:, :1]), 1 - a_eff[:, :-1]], 1), 1)
        stop_here = valid & (T_excl * (1 - a_eff) < 0.0001)
        stopped = torch.cumsum(stop_here.to(torch.int32), 1) > 0
        live = valid & ~stopped
    a_live = torch.where(live, alpha, torch.zeros_like(alpha))
    T = torch.cumprod(torch.cat([torch.ones_like(a_live[:, :1]), 1 - a_live[:, :-1]], 1), 1)
    w = a_live * T
    T_final = T[:, -1] * (1 - a_live[:, -1]) if o.numel() else torch.ones(H * W, dtype=dt)
    color = feat = None
    if rgb is not None:
        color = (w @ rgb[o] + T_final[:, None] * bg.to(dt)[None]).T.reshape(3, H, W)
    if features is not None:
        feat = (w @ features[o]).T.reshape(features.shape[1], H, W)
    mask = (1 - T_final).reshape(1, H, W)
    depth = (w @ tz[o]).reshape(1, H, W)
    return color, feat, mask, depth, radii
