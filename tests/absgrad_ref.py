"""Reference, cases and bars of the absolute view-space gradient (AbsGS; ``means2D_abs``, ``lsr_backward_absgrad``; DESIGN.md
§2.22), for tests/test_absgrad_{cpu,gpu}.py.

Reference.  :func:`composite` restates ``oracle.torch_oracle.rasterize`` (projection through the oracle's own helpers, the
compositing line by line) with ONE change: ``dx = (px[o][None] + dlx) - pxf``, ``dy`` likewise, where ``dlx``, ``dly`` are zero
``(P, n)`` leaves (P pixels, n visible Gaussians in depth order).  ``dlx.grad[p, j]`` is then pixel p's contribution to
dL/d(mean_pix of j), and

    abs_ref = (W / 2 * sum_p |dlx.grad|,  H / 2 * sum_p |dly.grad|)        signed = the same sums without the magnitudes

in float64; "stock" is the same function in float32 (the project's 4 x rule: tests/antialias_ref.py ``MARGIN``).  The torch
oracle has no ``means2D`` leaf, so the restatement is tied to it in three steps (:func:`preconditions`): its images equal
``rasterize``'s to 1e-12, the gradients of its leaves (means, covariances, opacities, payload) equal autograd through
``rasterize`` to 1e-10 relative, and ``signed`` equals W / 2 x its own dL/dpx to 1e-10 relative — px reaches the loss through
dx alone, which is the NDC path of the oracle's mean gradient.  The radii are the C oracle's.

Bars (``hold``), per quantity:  err <= max(CLEAN_TOL x max |want|, 4 x stock error), CLEAN_TOL = 2e-5 of tests/test_parity_gpu.py.

Every case must be able to tell (``preconditions``, CPU only): ``abs_ref >= |signed|`` everywhere, no fragile evaluation of the
C oracle's forward, and two mutants each at least 10 bars from ``abs_ref``: |signed| (the magnitude of the sum) and the
magnitude taken after adding the horizontally adjacent pixel pair (2j, 2j + 1) — the two pixels of a compositing lane.  The
"onepix" case is the opposite: every splat reaches exactly one pixel, so that abs_ref == |signed| and the kernel has to return
the two equal.

Seeds: the first of 400, 401, ... for which the preconditions hold (``python -m tests.absgrad_ref`` searches 400 ... 439 and
prints the table); the pair of the per-view case is (seed, unused) as camera_grad_cases._a5 derives the views' seeds itself.

Measured on the MI355X (all 39 tests of tests/test_absgrad_gpu.py pass).  Worst kernel error / bar over every check: abs 0.252
and means2D 0.252 (both the one-pixel case, whose bar is 8.8e-6: kernel 2.2e-6, stock 2.2e-6; on the other cases abs <= 0.05,
means2D <= 0.11), means 0.143, cov 0.093, opac 0.067, colors_precomp 0.051, shs 0.034, features 0.023, DensityControl's
accumulator 0.012.  Kernel error / stock error lies between 0.8 and 1.1 throughout: the kernels are as good as the float32
statement, and the 4 x stock term of the bar never binds (CLEAN_TOL x max |want| does).  |means2D grad| exceeds abs by at most
4.8e-7 (bars 1e-3); one-pixel splats return the two equal to 1.5e-8.  Under LSR_DETERMINISTIC the ordinary gradients of a call
with ``means2D_abs`` equal those of the call without it bit for bit, in the plain and the list-splitting instance.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.synthetic import make_scene
from oracle import torch_oracle as TO
from tests import antialias_ref as aref
from tests import camera_grad_cases as cases
from tests.test_parity_gpu import CLEAN_TOL

F64 = torch.float64
SEPARATION = 10.0
SUB_PIXEL = dict(sigma_px=(0.05, 0.6), opacity_scale=0.9)
SEEDS = {"V1": 400, "V3": 400, "V5": 400, "aa": 400, "perview": 400, "feat": 400, "onepix": 400}
NAMES = ("V1", "V3", "V5", "aa", "perview", "feat")          # the cases the mutants must be told from


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def composite(H, W, tanfovx, tanfovy, bg, viewmatrix, projmatrix, campos, sh_degree, means3D, cov3D, opacities, shs=None,
              colors_precomp=None, features=None, antialiasing=False):
    """``TO.rasterize`` in the dtype of ``means3D`` with the per-(pixel, Gaussian) offsets.  Returns
    (color | None, feature | None, mask, depth, radii, order, (dlx, dly), (px, py)); px, py retain their gradient."""
    dt = means3D.dtype
    G = means3D.shape[0]
    vm = viewmatrix.reshape(4, 4).to(dt)
    pm = projmatrix.reshape(4, 4).to(dt)
    ones = torch.ones(G, 1, dtype=dt)
    ph = torch.cat([means3D, ones], 1) @ pm
    p_w = 1.0 / (ph[:, 3] + 0.0000001)
    ndc = ph[:, :2] * p_w[:, None]
    inx, iny = TO._clamp_mask(vm, means3D, tanfovx, tanfovy)
    t, cov2 = TO._project(dt, H, W, tanfovx, tanfovy, vm, means3D, cov3D, inx, iny)
    tz = t[:, 2]
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    if antialiasing:
        opacities = opacities.reshape(-1) * TO._factor(cov2)
    ok = (tz > 0.2) & (det != 0)
    det_s = torch.where(det != 0, det, torch.ones_like(det))
    conA, conB, conC = c / det_s, -b / det_s, a / det_s
    with torch.no_grad():
        mid = 0.5 * (a + c)
        disc = torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(mid + disc, mid - disc)))
    px = (((ndc[:, 0].double() + 1.0) * W - 1.0) * 0.5).to(dt)
    py = (((ndc[:, 1].double() + 1.0) * H - 1.0) * 0.5).to(dt)
    px.retain_grad()
    py.retain_grad()
    gx, gy = (W + 15) // 16, (H + 15) // 16
    with torch.no_grad():
        ti = lambda v: torch.nan_to_num(v / 16.0, nan=0.0, posinf=1e9, neginf=-1e9).to(torch.int64)
        rminx, rminy = ti(px - radius).clamp(0, gx), ti(py - radius).clamp(0, gy)
        rmaxx, rmaxy = ti(px + radius + 15).clamp(0, gx), ti(py + radius + 15).clamp(0, gy)
        vis = ok & ((rmaxx - rminx) * (rmaxy - rminy) > 0)
        radii = torch.where(vis, radius, torch.zeros_like(radius)).to(torch.int32)
    rgb = None
    if shs is not None:
        d = means3D - campos.to(dt)[None]
        d = d / d.norm(dim=-1, keepdim=True)
        nb = (sh_degree + 1) ** 2
        rgb = torch.clamp_min(torch.einsum("gk,gkc->gc", TO.sh_basis(sh_degree, d), shs[:, :nb]) + 0.5, 0.0)
    elif colors_precomp is not None:
        rgb = colors_precomp
    with torch.no_grad():
        order = torch.argsort(torch.where(vis, tz, torch.full_like(tz, float("inf"))), stable=True)
        order = order[: int(vis.sum())]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pxf, pyf = xs.reshape(-1).to(dt), ys.reshape(-1).to(dt)
    tile_x, tile_y = (xs.reshape(-1) // 16), (ys.reshape(-1) // 16)
    o = order
    dlx = torch.zeros(H * W, o.numel(), dtype=dt, requires_grad=True)
    dly = torch.zeros(H * W, o.numel(), dtype=dt, requires_grad=True)
    dx = (px[o][None] + dlx) - pxf[:, None]           # THE change: one offset per (pixel, Gaussian)
    dy = (py[o][None] + dly) - pyf[:, None]
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
    return color, feat, mask, depth, radii, order, (dlx, dly), (px, py)


# ---------------------------------------------------------------------------------------------------------------------
# loss, leaves, the reference of a case
# ---------------------------------------------------------------------------------------------------------------------
def weights(c):
    """Per view: float64 image weights of the loss (colour, features, mask, depth), fixed by the case's shape."""
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    return [dict(col=r(3, c.H, c.W), feat=r(max(c.C, 1), c.H, c.W), mask=r(1, c.H, c.W), depth=0.05 * r(1, c.H, c.W))
            for _ in range(c.V)]


def loss(col, feat, mask, depth, w, with_depth=True):
    out = (mask * w["mask"].to(mask)).sum()
    if col is not None:
        out = out + (col * w["col"].to(col)).sum()
    if feat is not None:
        out = out + (feat * w["feat"][: feat.shape[0]].to(feat)).sum()
    if with_depth:
        out = out + (depth * w["depth"].to(depth)).sum()
    return out


def tensors(c):
    """name -> tensor of every differentiable input of the case, in the shapes the op takes them"""
    return dict(means=c.means, cov=c.cov, opac=c.opac, **{k: v for k, v in c.kw.items() if torch.is_tensor(v)})


def _view_call(c, v, L, dt, fn, **mode):
    """One view of the case through ``fn`` (``composite`` or ``TO.rasterize``) on the leaves L (dtype dt)."""
    sidx = v if c.scenes is None else v // (c.V // c.scenes)
    pick = lambda t, base: t if t.dim() == base else t[sidx]
    rec = c.views[v].to(dt)
    s = rec[40]
    m, o = pick(L["means"], 2), pick(L["opac"], 2)
    cv = pick(L["cov"], 2)
    assert cv.shape[-1] == 6
    pl = {}
    if "shs" in L:
        pl["shs"] = pick(L["shs"], 3)
    for k in ("colors_precomp", "features"):
        if k in L:
            pl[k] = pick(L[k], 2)
    return fn(c.H, c.W, rec[35], rec[36], rec[37:40], rec[0:16], rec[16:32], rec[32:35], c.kw.get("sh_degree", 0),
              m * s, cv * s * s, o, **pl, **mode)


def reference(c, dt=F64, with_depth=True):
    """The restatement over the views of the case.  dict: ``abs`` / ``signed`` / ``pair`` (V, G, 2) — abs_ref, the signed sums
    (the means2D gradient, NDC) and the pair mutant; ``hits`` (V, G) pixels with a non-zero contribution; ``m2d_px`` (V, G, 2)
    W / 2 x dL/dpx of the same graph; ``radii``; ``images`` per view; ``grads``: name -> gradient of every input."""
    L = {k: t.detach().to(dt).clone().requires_grad_(True) for k, t in tensors(c).items()}
    w = weights(c)
    mode = dict(antialiasing=True) if c.antialiasing else {}
    z = lambda: torch.zeros(c.V, c.G, 2, dtype=dt)
    out = dict(abs=z(), signed=z(), pair=z(), m2d_px=z(), hits=torch.zeros(c.V, c.G, dtype=torch.int64), radii=[], images=[])
    scale = torch.tensor([0.5 * c.W, 0.5 * c.H], dtype=dt)
    for v in range(c.V):
        col, feat, mask, depth, radii, order, (dlx, dly), (px, py) = _view_call(c, v, L, dt, composite, **mode)
        loss(col, feat, mask, depth, w[v], with_depth).backward()
        g = torch.stack([dlx.grad, dly.grad], -1)                                   # (P, n, 2)
        out["abs"][v, order] = g.abs().sum(0) * scale
        out["signed"][v, order] = g.sum(0) * scale
        pairs = g.reshape(c.H, c.W // 2, 2, -1, 2).sum(2)                            # pixels (2j, 2j + 1) of a row added first
        out["pair"][v, order] = pairs.abs().sum((0, 1)) * scale
        out["hits"][v, order] = (g != 0).any(-1).sum(0)
        out["m2d_px"][v] = torch.stack([px.grad, py.grad], -1) * scale
        out["radii"].append(radii)
        out["images"].append([None if t is None else t.detach() for t in (col, feat, mask, depth)])
    out["radii"] = torch.stack(out["radii"])
    out["grads"] = {k: t.grad for k, t in L.items()}
    return out


def oracle_reference(c, with_depth=True):
    """Autograd through ``TO.rasterize`` itself in float64 under the same loss: (grads, images per view)."""
    L = {k: t.detach().double().clone().requires_grad_(True) for k, t in tensors(c).items()}
    w = weights(c)
    images = []
    for v in range(c.V):
        col, feat, mask, depth, _ = _view_call(c, v, L, F64, TO.rasterize, **(dict(antialiasing=True) if c.antialiasing else {}))
        loss(col, feat, mask, depth, w[v], with_depth).backward()
        images.append([None if t is None else t.detach() for t in (col, feat, mask, depth)])
    return {k: t.grad for k, t in L.items()}, images


@functools.lru_cache(maxsize=None)
def references(name, with_depth=True):
    """(want, stock) of the case: computed once, shared, never modified"""
    c = case(name)
    return reference(c, F64, with_depth), reference(c, torch.float32, with_depth)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _finish(c, name, antialiasing=False):
    c.name, c.antialiasing = name, antialiasing
    return c


def _views(V, seed):
    """V shared views, colour SH of degree 1 alone: what a GaussianScene render hands the rasterizer"""
    return cases._colour_case(make_scene(160, image_size=32, views=V, seed=seed, color_sh_degree=1, feature_channels=None), 1, 32, 32)


def _aa(seed):
    """3 views of sub-pixel splats under antialiasing=True, precomputed colours"""
    sc = make_scene(160, image_size=32, views=3, seed=seed, color_sh_degree=None, feature_channels=None, **SUB_PIXEL)
    cp = torch.rand(160, 3, generator=torch.Generator().manual_seed(seed))
    return cases.Case(cases.cams32(sc), 32, 32, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                      dict(colors_precomp=cp), None, 0)


def _feat(seed):
    """2 views, 3 precomputed colours + 1 direct feature: the 4 padded channels are full"""
    sc = make_scene(160, image_size=32, views=2, seed=seed, color_sh_degree=None, feature_channels=1)
    cp = torch.rand(160, 3, generator=torch.Generator().manual_seed(seed))
    return cases.Case(cases.cams32(sc), 32, 32, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                      dict(colors_precomp=cp, features=sc.feature_sh[..., 0].contiguous()), None, 1)


ONEPIX = 156


def _onepix(seed):
    """One view at the identity (scale slot 1), 156 splats of negligible extent — the 0.3 low-pass alone: conic 1 / 0.3 — and
    opacity 0.01 within 0.15 px of the pixel centres (2 i + 3, 2 j + 4): alpha is 0.01 exp(-d^2 / 0.6) >= 1/255 at the own pixel
    (d <= 0.22) and at most 0.01 exp(-0.85^2 / 0.6) = 0.003 < 1/255 at every other."""
    H = W = 32
    sc = make_scene(1, image_size=32, views=1, seed=seed, color_sh_degree=None, feature_channels=None)
    sc.near = torch.ones(1)
    gen = torch.Generator().manual_seed(seed)
    n = ONEPIX
    tan = 0.5 / float(sc.intrinsics[0, 0, 0])
    z = 2.0 + 2.0 * torch.rand(n, generator=gen, dtype=F64)
    idx = torch.arange(n)
    off = 0.3 * torch.rand(n, 2, generator=gen, dtype=F64) - 0.15
    px, py = 3 + 2 * (idx % 13) + off[:, 0], 4 + 2 * (idx // 13) + off[:, 1]
    sc.means = torch.stack([((2 * px + 1) / W - 1) * tan * z, ((2 * py + 1) / H - 1) * tan * z, z], -1).float()
    sc.covariances = (1e-10 * torch.eye(3))[None].repeat(n, 1, 1)
    sc.opacities = torch.full((n,), 0.01)
    cp = torch.rand(n, 3, generator=gen)
    return cases.Case(cases.cams32(sc), H, W, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                      dict(colors_precomp=cp), None, 0)


def build(name, seed=None):
    seed = SEEDS[name] if seed is None else seed
    if name in ("V1", "V3", "V5"):
        return _finish(_views(int(name[1]), seed), name)
    if name == "aa":
        return _finish(_aa(seed), name, antialiasing=True)
    if name == "perview":
        return _finish(cases._a5(seed=seed), name)
    if name == "feat":
        return _finish(_feat(seed), name)
    if name == "onepix":
        return _finish(_onepix(seed), name)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name)


def payload_of(c):
    from tests.test_camera_grads_gpu import _payload_of
    return _payload_of({k: (v.double() if torch.is_tensor(v) else v) for k, v in c.kw.items()})


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def bar(want, stock):
    """(bar, stock error) of one quantity"""
    es = float((stock.double() - want).abs().max())
    return max(CLEAN_TOL * float(want.abs().max()), aref.MARGIN * es), es


WORST: dict = {}


def hold(what, name, got, want, stock):
    """err <= max(CLEAN_TOL x max |want|, 4 x stock error); prints kernel error, stock error and their ratio"""
    got = got.double()
    assert bool(torch.isfinite(got).all()), (what, name, "non-finite values")
    b, es = bar(want, stock)
    err = float((got - want).abs().max())
    ratio = err / es if es > 0 else (0.0 if err == 0 else float("inf"))
    WORST[name] = max(WORST.get(name, 0.0), err / b)
    print(f"{what:34s} {name:14s} kernel {err:.3e}  stock {es:.3e}  ratio {ratio:9.3f}  bar {b:.3e}  kernel / bar {err / b:.3f}")
    assert err <= b, (what, name, err, es, b)


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def preconditions(c, refs=None, show=True):
    """What holds on the CPU alone, before any GPU run.  Returns the smaller of the two mutants' distances in bars (None for
    the one-pixel case)."""
    want, stock = refs if refs is not None else references(c.name)
    assert 150 <= c.G <= 200 and (c.H, c.W) == (32, 32)
    # 1. the restatement is the oracle: images, the gradients of every leaf, and the signed sums are its NDC mean gradient
    ograds, oimages = oracle_reference(c)
    for v in range(c.V):
        for a, b in zip(want["images"][v], oimages[v]):
            assert (a is None) == (b is None) and (a is None or float((a - b).abs().max()) <= 1e-12)
    for k, g in ograds.items():
        assert rel(want["grads"][k], g) <= 1e-10, (c.name, k, rel(want["grads"][k], g))
    assert rel(want["signed"], want["m2d_px"]) <= 1e-10, (c.name, rel(want["signed"], want["m2d_px"]))
    # 2. magnitudes dominate
    assert bool((want["abs"] >= want["signed"].abs()).all())
    # 3. no fragile evaluation; the C oracle's radii and (float32) means2D agree
    fw = cases.oracle_forwards(c.views, c.H, c.W, c.means, c.cov, c.opac, payload_of(c), c.scenes, antialiasing=c.antialiasing)
    fragile = cases.fragile_counts(None, c.H, c.W, None, None, None, None, forwards=fw)
    assert fragile == [0] * c.V, (c.name, fragile)
    assert np.array_equal(np.stack([f["radii"] for f in fw]), want["radii"].numpy()), c.name
    assert bool((want["abs"][want["radii"] == 0] == 0).all())
    b, es = bar(want["abs"], stock["abs"])
    if c.name == "onepix":
        vis = want["radii"] > 0
        assert int(vis.sum()) == ONEPIX and bool((want["hits"][vis] == 1).all()), (int(vis.sum()), want["hits"][vis])
        assert float((want["abs"] - want["signed"].abs()).abs().max()) <= 1e-12 * float(want["abs"].max())
        assert float(want["abs"].max()) > 0
        if show:
            print(f"{c.name:8s} {ONEPIX} splats of one pixel each; bar {b:.3e} (stock error {es:.3e})")
        return None
    # 4. the mutants can be told
    away = {m: float((want[m].abs() - want["abs"]).abs().max()) / b for m in ("signed", "pair")}
    if show:
        print(f"{c.name:8s} visible {int((want['radii'] > 0).sum())}; bar {b:.3e} (stock error {es:.3e}); |signed| {away['signed']:.0f} bars away, "
              f"magnitude after the pixel pair {away['pair']:.0f} bars away")
    assert min(away.values()) >= SEPARATION, (c.name, away)
    return min(away.values())


def search(names=NAMES + ("onepix",), first=400, last=439):
    """The seed table: per case the first seed of [first, last] for which the preconditions hold."""
    found = {}
    for name in names:
        for seed in range(first, last + 1):
            c = build(name, seed)
            try:
                preconditions(c, refs=(reference(c), reference(c, torch.float32)), show=False)
            except AssertionError as e:
                print(f"{name}: seed {seed} fails: {str(e)[:120]}")
                continue
            found[name] = seed
            break
    print("SEEDS =", found)
    return found


if __name__ == "__main__":
    search()
