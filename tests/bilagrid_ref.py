"""References of the bilateral-grid operator (csrc/bilagrid.hip, include/lsr_bilagrid.h), the case table of
tests/test_bilagrid_{cpu,gpu}.py with seeded inputs, and the error bar.  CPU only; torch operators, nothing else.

  * `restate` / `restate_tv`: the header's formulas in float64, vectorised, written with gathers and explicit gradient
    formulas (no `grid_sample`, no autograd);
  * `stock` / `stock_tv`: the stock composition (`F.grid_sample` of the 5-D parameter, then the affine; the published
    total-variation loop) with autograd, in float64 or float32.  The float32 one is the error yardstick;
  * `held`: the bar of tests/latent_ref.py's resize quantities.  Every element of a quantity is within
    max(4 x the stock float32 error, 2^-20 x max |want|) of float64; kernel error, stock error and their ratio are printed.

The case generator moves every pixel whose luminance coordinate u_z lies within 1e-3 of an integer (0 and L - 1 included)
away from it, so that the one-sided derivative along luminance is the same in every precision; no element is left out of
any comparison."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 4.0
FLOOR = 2.0 ** -20
LUMA = (0.299, 0.587, 0.114)
NUDGE = 1e-3

# case -> ((L, Y, X), (H, W), V, N, grid_idx, kernel path: the tile edge whose footprint is staged in LDS, 0 = direct)
CASES = {
    "affine_1x1": ((1, 1, 1), (1, 1), 2, 2, (1, 0), 32),
    "affine_5x7": ((1, 1, 1), (5, 7), 2, 2, (1, 0), 32),
    "tiny_grid": ((2, 3, 2), (5, 7), 2, 2, (0, 1), 32),
    "shared_grid": ((3, 1, 5), (33, 65), 3, 3, (2, 0, 2), 32),            # two views add into grid 2, grid 1 is not indexed
    "default_64": ((8, 16, 16), (64, 64), 3, 3, (2, -1, 0), 16),          # 10 x 10 x 8 = 800 nodes per 32-tile: over the limit
    "default_33x65": ((8, 16, 16), (33, 65), 3, 3, (2, -1, 0), 16),       # partial tiles both ways, a view without a grid
    "default_256": ((8, 16, 16), (40, 256), 1, 1, (0,), 32),              # 14 x 4 x 8 = 448 nodes: the published grid on 32-tiles
    "grid_wider_than_image": ((8, 16, 16), (8, 8), 1, 1, (0,), 0),        # X > W: every node under one tile, 2048 of them
    "largest_8": ((16, 64, 64), (8, 8), 1, 1, (0,), 0),
    "largest_40": ((16, 64, 64), (40, 40), 1, 1, (0,), 0),
}


def luma_coordinate(image: torch.Tensor, L: int) -> torch.Tensor:
    """Unclamped u_z in float64."""
    p = image.to(torch.float64)
    return (LUMA[0] * p[:, 0] + LUMA[1] * p[:, 1] + LUMA[2] * p[:, 2]) * (L - 1)


def nudge(image: torch.Tensor, L: int) -> torch.Tensor:
    """The float32 image with every pixel whose u_z is within NUDGE of an integer moved 2.5 NUDGE further from it."""
    if L == 1:
        return image            # u_z is 0 everywhere and its derivative carries the factor L - 1 = 0
    u = luma_coordinate(image, L)
    d = u - u.round()
    step = torch.where(d.abs() < NUDGE, torch.where(d < 0, -1.0, 1.0) * 2.5 * NUDGE / (L - 1), torch.zeros_like(d))
    out = (image.to(torch.float64) + step[:, None]).to(torch.float32)
    u = luma_coordinate(out, L)
    assert float((u - u.round()).abs().min()) >= NUDGE
    return out


@functools.lru_cache(maxsize=None)
def make_case(name: str) -> dict:
    """Seeded float32 inputs of one case.  Shared between tests: never modify them.  grids = identity + 0.3 randn, pixels
    in [-0.2, 1.2]: a grey level uniform over that range plus up to 0.1 per channel, so that both luminance clamps occur
    wherever there are a few dozen pixels (independent channels would average them away); grad_out = randn."""
    (L, Y, X), (H, W), V, N, idx, _ = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 4242)
    grids = torch.eye(3, 4).reshape(1, 12, 1, 1, 1) + 0.3 * torch.randn(N, 12, L, Y, X, generator=g)
    grey = torch.rand(V, 1, H, W, generator=g) * 1.4 - 0.2            # the channels share most of their value: a seventh of
    chroma = 0.2 * torch.rand(V, 3, H, W, generator=g) - 0.1          # the pixels is darker than 0 and a seventh brighter than 1
    image = nudge((grey + chroma).clamp(-0.2, 1.2), L)
    return dict(grids=grids, image=image, grid_idx=torch.tensor(idx, dtype=torch.int32), grad_out=torch.randn(V, 3, H, W, generator=g),
                grad_tv=torch.tensor(1.7))


def _split(u: torch.Tensor, size: int):
    """Clamped coordinate -> lower node, upper node, weight of the upper node."""
    u = u.clamp(0, size - 1)
    i0 = u.floor().clamp(max=max(size - 2, 0)).long()
    return i0, (i0 + 1).clamp(max=size - 1), u - i0


def restate(grids: torch.Tensor, image: torch.Tensor, grid_idx: torch.Tensor, grad_out: torch.Tensor = None) -> dict:
    """out (and, with grad_out, grad_image and grad_grids) by the header's formulas in float64."""
    g, p = grids.to(torch.float64), image.to(torch.float64)
    N, _, L, Y, X = g.shape
    V, _, H, W = p.shape
    f64 = torch.float64
    ix0, ix1, fx = _split((torch.arange(W, dtype=f64) + 0.5) / W * (X - 1), X)
    iy0, iy1, fy = _split((torch.arange(H, dtype=f64) + 0.5) / H * (Y - 1), Y)
    uz = luma_coordinate(p, L)                                        # (V, H, W)
    iz0, iz1, fz = _split(uz, L)
    idx = grid_idx.long()
    valid = (idx >= 0) & (idx < N)
    n = idx.clamp(0, N - 1)[:, None, None].expand(V, H, W)
    cells = g.permute(0, 2, 3, 4, 1)                                  # (N, L, Y, X, 12)
    corners = []
    for iz, wz, sz in ((iz0, 1 - fz, -1.0), (iz1, fz, 1.0)):
        for iy, wy in ((iy0, 1 - fy), (iy1, fy)):
            for ix, wx in ((ix0, 1 - fx), (ix1, fx)):
                wxy = (wy[:, None] * wx[None, :])[None].expand(V, H, W)
                corners.append((iz, iy[None, :, None].expand(V, H, W), ix[None, None, :].expand(V, H, W), wz * wxy, sz * wxy))
    A = torch.zeros(V, H, W, 12, dtype=f64)
    D = torch.zeros(V, H, W, 12, dtype=f64)                           # dA/du_z between the two luminance nodes
    for iz, iy, ix, w, dw in corners:
        node = cells[n, iz, iy, ix]
        A += w[..., None] * node
        D += dw[..., None] * node
    if L == 1:
        D.zero_()
    A, D = A.reshape(V, H, W, 3, 4), D.reshape(V, H, W, 3, 4)
    pix = p.permute(0, 2, 3, 1)
    q = torch.cat((pix, torch.ones(V, H, W, 1, dtype=f64)), -1)
    out = torch.einsum("vhwrk,vhwk->vhwr", A, q)
    keep = valid[:, None, None, None]
    res = dict(out=torch.where(keep, out, pix).permute(0, 3, 1, 2).contiguous())
    if grad_out is None:
        return res
    go = grad_out.to(f64).permute(0, 2, 3, 1)
    inside = ((uz > 0) & (uz < L - 1)).to(f64)
    dz = (L - 1) * inside * torch.einsum("vhwr,vhwrk,vhwk->vhw", go, D, q)
    dp = torch.einsum("vhwrk,vhwr->vhwk", A[..., :3], go) + dz[..., None] * torch.tensor(LUMA, dtype=f64)
    res["grad_image"] = torch.where(keep, dp, go).permute(0, 3, 1, 2).contiguous()
    outer = (go[..., :, None] * q[..., None, :]).reshape(V, H, W, 12) * keep.to(f64)
    gg = torch.zeros(N, L, Y, X, 12, dtype=f64)
    for iz, iy, ix, w, _ in corners:
        gg.index_put_((n, iz, iy, ix), w[..., None] * outer, accumulate=True)
    res["grad_grids"] = gg.permute(0, 4, 1, 2, 3).contiguous()
    return res


def stock(grids: torch.Tensor, image: torch.Tensor, grid_idx: torch.Tensor, grad_out: torch.Tensor = None, dtype=torch.float64) -> dict:
    """The stock composition in `dtype`: grid_sample(grids[idx], 2 (x, y, luma) - 1, bilinear, border, align_corners=True),
    the affine, and autograd for the gradients.  Views without a grid pass through.  Results come back as float64."""
    g = grids.to(dtype).clone().requires_grad_(True)
    p = image.to(dtype).clone().requires_grad_(True)
    N = g.shape[0]
    V, _, H, W = p.shape
    idx = grid_idx.long()
    has = ((idx >= 0) & (idx < N)).nonzero()[:, 0]
    out = p
    if len(has):
        ps = p[has]
        x = ((torch.arange(W, dtype=dtype) + 0.5) / W)[None, None, :].expand(len(has), H, W)
        y = ((torch.arange(H, dtype=dtype) + 0.5) / H)[None, :, None].expand(len(has), H, W)
        luma = LUMA[0] * ps[:, 0] + LUMA[1] * ps[:, 1] + LUMA[2] * ps[:, 2]
        coords = torch.stack((x, y, luma), -1)[:, None] * 2 - 1       # (v, 1, H, W, 3)
        A = F.grid_sample(g[idx[has]], coords, mode="bilinear", padding_mode="border", align_corners=True)
        A = A.reshape(len(has), 3, 4, H, W)
        sliced = torch.einsum("vrkhw,vkhw->vrhw", A[:, :, :3], ps) + A[:, :, 3]
        out = p.index_copy(0, has, sliced) if len(has) < V else sliced
    res = dict(out=out.detach().to(torch.float64))
    if grad_out is not None:
        gp, gg = torch.autograd.grad((out * grad_out.to(dtype)).sum(), (p, g), allow_unused=True)
        res["grad_image"] = gp.to(torch.float64)
        res["grad_grids"] = (torch.zeros_like(g) if gg is None else gg).to(torch.float64)
    return res


def restate_tv(grids: torch.Tensor, grad_tv: float = None) -> dict:
    """tv (and, with grad_tv, grad_tv * d tv / d grids) by the header's formula in float64, gradient written out."""
    g = grids.to(torch.float64)
    tv, grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(g)
    for axis in (2, 3, 4):
        size = g.shape[axis]
        if size < 2:
            continue
        d = g.narrow(axis, 1, size - 1) - g.narrow(axis, 0, size - 1)
        tv = tv + (d * d).sum() / d.numel()
        grad.narrow(axis, 1, size - 1).add_(2.0 / d.numel() * d)
        grad.narrow(axis, 0, size - 1).sub_(2.0 / d.numel() * d)
    res = dict(tv=tv.reshape(1))
    if grad_tv is not None:
        res["grad"] = float(grad_tv) * grad
    return res


def stock_tv(grids: torch.Tensor, grad_tv: float = None, dtype=torch.float64) -> dict:
    """The published total-variation loop (index_select both ways, squared difference, sum over the element count; an
    axis of size 1 skipped) in `dtype`, with autograd."""
    x = grids.to(dtype).clone().requires_grad_(True)
    tv = torch.zeros((), dtype=dtype)
    for i in range(2, x.dim()):
        n_res = x.shape[i]
        if n_res < 2:
            continue
        x1 = x.index_select(i, torch.arange(1, n_res))
        x2 = x.index_select(i, torch.arange(0, n_res - 1))
        tv = tv + torch.pow(x1 - x2, 2).sum() / x1.numel()
    res = dict(tv=tv.detach().to(torch.float64).reshape(1))
    if grad_tv is not None:
        grad = torch.autograd.grad(tv, x)[0] if tv.requires_grad else torch.zeros_like(x)
        res["grad"] = float(grad_tv) * grad.to(torch.float64)
    return res


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(float64 restatement, stock float32) of one case, slice and tv together, computed once; numpy float64 arrays."""
    c = make_case(name)
    want = dict(restate(c["grids"], c["image"], c["grid_idx"], c["grad_out"]))
    yard = dict(stock(c["grids"], c["image"], c["grid_idx"], c["grad_out"], torch.float32))
    for d, fn, kw in ((want, restate_tv, {}), (yard, stock_tv, dict(dtype=torch.float32))):
        tv = fn(c["grids"], float(c["grad_tv"]), **kw)
        d["tv"], d["grad_tv"] = tv["tv"], tv["grad"]
    return {k: v.numpy() for k, v in want.items()}, {k: v.numpy() for k, v in yard.items()}


def held(name: str, got, want: np.ndarray, stock_: np.ndarray, show: str = "") -> None:
    """Assert every element of `got` within max(4 x stock error, 2^-20 x max |want|) of `want`; print the figures first."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (show, name, got.shape, want.shape)
    assert np.isfinite(want).all() and np.isfinite(got).all(), (show, name, "not finite")
    diff = np.abs(got - want)
    err, err_stock, scale = float(diff.max()), float(np.abs(stock_ - want).max()), float(np.abs(want).max())
    bar = max(MARGIN * err_stock, FLOOR * scale)
    ratio = err / err_stock if err_stock > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{show} {name:11s} kernel {err:.3e}  stock {err_stock:.3e}  ratio {ratio:.3f}  scale {scale:.3e}  bar {bar:.3e}  "
          f"over the bar {int((diff > bar).sum())}")
    assert not (diff > bar).any(), (show, name, err, err_stock, bar)
