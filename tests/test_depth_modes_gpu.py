"""Depth modes on the MI355X: the projection kernels write d(z) = max(0, C0 u(z) + 0.5) into the record slot the
compositing kernels blend into the depth image (view-table slots 41-43 carry the mode and the caller's near / far), so
``render_scenes(depth_mode=m)`` returns in ONE pass what ``render_depth_scenes(mode=m)`` renders with a second one.

Method of tests/test_camera_grads_gpu.py: expectations are autograd through the float64 PyTorch oracle
(oracle/torch_oracle.py), which is handed the payload d — computed by the public helper
``latentsplat_amd.rasterizer.depth_mode_payload`` — as one more feature channel (same weights, no background: exactly the
depth image's blend); the C oracle, fed the same channel, tells which evaluations are fragile.  Scene seeds are chosen
so that no view has a fragile evaluation (asserted)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from latentsplat_amd import rasterizer as R
from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.decoder.geometry import eval_sh
from latentsplat_amd.synthetic import make_scene
from oracle import oracle as orc
from oracle import torch_oracle as TO
from tests import depth_modes_util as du
from tests import util
from tests.test_camera_grads_gpu import _assert_grads_close, _chain64

pytestmark = pytest.mark.gpu
F64 = torch.float64
MODES = du.MODES
GOLD = du.GOLD
IMG_TOL = 1e-4      # of the image's scale: the suite's image bar
GRAD_TOL = 1e-4     # of the tensor's largest magnitude: the suite's gradient bar
BG = (0.2, 0.5, 0.7)

# scene seeds: the C oracle's forward reports no fragile evaluation for any view of the case (asserted in _expect)
SEEDS = dict(fused=(105, 155), plain=6, perview=3, clamp=0, camera=2)


# ---------------------------------------------------------------------------------------------------------------------
# cases: scene-level tensors with a leading slice dimension S (1: shared by the views, b: scenes of V / b views, V: per view)
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, kind, H, W, ext, intr, near, far, means, cov, opac, color, feat, scale_invariant=True):
        self.kind, self.H, self.W = kind, H, W                      # kind: "sh" (harmonics) or "direct" (colors_precomp + features)
        self.ext, self.intr, self.near, self.far = ext, intr, near, far     # (V, ...)
        self.means, self.cov, self.opac, self.color, self.feat = means, cov, opac, color, feat
        self.scale_invariant = scale_invariant
        self.V, self.S = ext.shape[0], means.shape[0]

    def leaves(self):
        return dict(means=self.means, cov=self.cov, opac=self.opac, color=self.color, feat=self.feat)


def fused_case():
    """b = 2 scenes x v = 2 views, G = 600, 64 x 64, colour SH degree 1 + 4 latent channels of SH degree 2: k_preprocess_sh"""
    scs = [make_scene(600, image_size=64, views=2, seed=s, color_sh_degree=1, feature_channels=4, feature_sh_degree=2)
           for s in SEEDS["fused"]]
    st = lambda n: torch.stack([getattr(s, n) for s in scs])
    cat = lambda n: torch.cat([getattr(s, n) for s in scs])
    near = cat("near") * torch.tensor([1.0, 1.25, 1.1, 0.9])         # per-view scene scales
    return Case("sh", 64, 64, cat("extrinsics"), cat("intrinsics"), near, cat("far"), st("means"), st("covariances"),
                st("opacities"), st("color_sh"), st("feature_sh"))


def plain_case():
    """one shared scene, 3 views, G = 500, 48 x 40, colors_precomp + 4 direct features: k_preprocess"""
    sc = make_scene(500, image_size=48, views=3, seed=SEEDS["plain"], color_sh_degree=None, feature_channels=4)
    g = torch.Generator().manual_seed(1)
    cp = torch.rand(1, 500, 3, generator=g)
    return Case("direct", 48, 40, sc.extrinsics, sc.intrinsics, sc.near * torch.tensor([1.0, 1.2, 0.8]), sc.far, sc.means[None],
                cs._pack_covariances(sc.covariances)[None], sc.opacities[None], cp, sc.feature_sh[None, ..., 0].contiguous())


def perview_case(scale_invariant):
    """per-view inputs with SH colour (degree 2), 2 views, G = 300, 32 x 32: k_preprocess, then the separate SH payload pass"""
    sc = make_scene(300, image_size=32, views=2, seed=SEEDS["perview"], color_sh_degree=2, feature_channels=None)
    rep = lambda t: t[None].repeat(2, *([1] * t.dim()))
    return Case("sh", 32, 32, sc.extrinsics, sc.intrinsics, sc.near * torch.tensor([1.0, 1.3]), sc.far, rep(sc.means),
                rep(sc.covariances), rep(sc.opacities), rep(sc.color_sh), None, scale_invariant=scale_invariant)


def table64(case, mode, leaves=None, dtype=torch.float32):
    """The case's view table from the float64 statement of the camera math (``leaves``: ext, intr, near, far to use)."""
    ext, intr, near, far = leaves or (case.ext.to(F64), case.intr.to(F64), case.near.to(F64), case.far.to(F64))
    vt, full, cp, tx, ty, s = _chain64(ext, intr, near, far, case.scale_invariant)
    return R.make_view_table(vt, full, cp, tx, ty, torch.tensor(BG, dtype=F64), s, dtype=dtype, depth_mode=mode, near=near, far=far)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 expectation
# ---------------------------------------------------------------------------------------------------------------------
def _view_inputs64(case, rec, v, t):
    """What view v hands to the oracle, float64, differentiable in the tensors of ``t`` and in ``rec``: scaled means,
    packed scaled covariance, opacity, payload kwargs, with the depth payload d as the LAST feature channel."""
    si = v * case.S // case.V
    s = rec[40]
    m = t["means"][si]
    ms = m * s
    cov = t["cov"][si]
    c6 = (cs._pack_covariances(cov) if cov.shape[-2:] == (3, 3) else cov) * s * s
    d = du.payload(rec[None], 0, m)
    deg, kw, feats = 0, {}, None
    if case.kind == "sh":
        if t["color"] is not None:
            deg = int(round(t["color"].shape[-1] ** 0.5)) - 1
            kw["shs"] = t["color"][si].transpose(1, 2)
        if t["feat"] is not None:
            dirn = ms - rec[32:35][None]
            dirn = dirn / dirn.norm(dim=-1, keepdim=True)
            feats = 0.5 + eval_sh(int(round(t["feat"].shape[-1] ** 0.5)) - 1, t["feat"][si], dirn)
    else:
        kw["colors_precomp"] = t["color"][si]
        feats = t["feat"][si]
    feats = d[:, None] if feats is None else torch.cat([feats, d[:, None]], 1)
    return deg, ms, c6, t["opac"][si][:, None], kw, feats


def _expect(case, views32, w=None, leaves64=None, views64=None):
    """Per view: (colour, feature, mask, depth) of the float64 oracle and the C oracle's forward dict.  With cotangents
    ``w`` the loss is accumulated and returned (the caller differentiates)."""
    t = leaves64 or {k: (None if x is None else x.to(F64)) for k, x in case.leaves().items()}
    outs, fwds, loss = [], [], 0.0
    for v in range(case.V):
        rec = views32[v].detach().to(F64) if views64 is None else views64[v]
        deg, ms, c6, op, kw, feats = _view_inputs64(case, rec, v, t)
        col, feat, mask, _, _ = TO.rasterize(case.H, case.W, rec[35], rec[36], rec[37:40], rec[0:16], rec[16:32], rec[32:35],
                                             deg, ms, c6, op, features=feats, **kw)
        depth, feat = feat[-1:], (feat[:-1] if feat.shape[0] > 1 else None)
        outs.append((col, feat, mask, depth))
        if w is not None:
            loss = loss + _loss(col, feat, mask, depth, w[v])
        n = lambda x: None if x is None else x.detach().float().contiguous().numpy()
        r32 = views32[v].detach()
        view = orc.View(case.H, case.W, float(r32[35]), float(r32[36]), r32[37:40].numpy(), r32[0:16].reshape(4, 4).numpy(),
                        r32[16:32].reshape(4, 4).numpy(), r32[32:35].numpy(), deg)
        f = orc.forward(view, n(ms), n(c6), n(op), n(kw.get("shs")), n(kw.get("colors_precomp")), n(feats))
        assert len(f["fragile"]) == 0 and not f["fragile_overflow"], f"view {v}: pick another seed ({len(f['fragile'])} fragile)"
        fwds.append(f)
    return outs, fwds, loss


def _loss(col, feat, mask, depth, w):
    out = (mask * w["mask"]).sum() + (depth * w["depth"]).sum()
    if col is not None:
        out = out + (col * w["col"]).sum()
    if feat is not None:
        out = out + (feat * w["feat"][: feat.shape[0]]).sum()
    return out


def _weights(case, seed=0):
    g = torch.Generator().manual_seed(seed)
    H, W = case.H, case.W
    return [dict(col=torch.randn(3, H, W, generator=g, dtype=F64), feat=torch.randn(4, H, W, generator=g, dtype=F64),
                 mask=torch.randn(1, H, W, generator=g, dtype=F64), depth=torch.randn(1, H, W, generator=g, dtype=F64))
            for _ in range(case.V)]


# ---------------------------------------------------------------------------------------------------------------------
# the HIP side
# ---------------------------------------------------------------------------------------------------------------------
def _device_table(case, mode, dev, cams=None):
    ext, intr, near, far = cams or (case.ext.to(dev), case.intr.to(dev), case.near.to(dev), case.far.to(dev))   # (cams: a list)
    return cs._view_table(ext, intr, near, far, torch.tensor(BG, device=dev), case.scale_invariant, mode)


def _run(case, mode, dev, leaves=None, path=None, cams=None):
    """(colour, feature, mask, depth (V,H,W), radii | None) of the case through its public entry point."""
    t = leaves or {k: (None if x is None else x.to(dev)) for k, x in case.leaves().items()}
    shape = (case.H, case.W)
    is_table = torch.is_tensor(cams)          # a ready (V, 44) table (the `views` path) instead of the four camera tensors
    ext, intr, near, far = (case.ext.to(dev), case.intr.to(dev), case.near.to(dev), case.far.to(dev)) if (cams is None or is_table) else cams
    bg = torch.tensor(BG, device=dev)
    kw = {} if mode is None else dict(depth_mode=mode)
    if path == "scenes":        # (b, v, ...) cameras, (b, g, ...) Gaussians
        b = case.S
        u = lambda x: x.unflatten(0, (b, case.V // b))
        o = cs.render_scenes(u(ext), u(intr), u(near), u(far), shape, bg, t["means"], t["cov"], t["opac"], t["color"], t["feat"],
                             scale_invariant=case.scale_invariant, **kw)
        return o.color, o.feature, o.mask, o.depth, None
    if path == "cuda":          # per-view everything
        o = cs.render_cuda(ext, intr, near, far, shape, bg.expand(case.V, 3), t["means"], t["cov"], t["opac"], t["color"], t["feat"],
                           scale_invariant=case.scale_invariant, **kw)
        return o.color, o.feature, o.mask, o.depth, None
    views = cams if is_table else table64(case, mode).to(dev)
    sq = lambda x: x[0] if x.shape[0] == 1 else x
    return R.rasterize_views(views, case.H, case.W, 0, sq(t["means"]), sq(t["cov"]), sq(t["opac"])[..., None],
                             colors_precomp=sq(t["color"]), features=sq(t["feat"]))


def _table_of(case, mode, dev, path):
    """The float32 table the run of ``path`` renders with, on the host."""
    return (table64(case, mode) if path == "views" else _device_table(case, mode, dev).cpu())


CASES = {"fused": (fused_case, "scenes"), "plain": (plain_case, "views"),
         "perview": (functools.partial(perview_case, True), "cuda"), "perview_unscaled": (functools.partial(perview_case, False), "cuda")}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name][0]()


def _assert_depth(got, want, fwd, what):
    want = want.detach().numpy()
    dscale = max(1.0, float(np.abs(want).max()))
    util.assert_close_except_fragile(got.cpu().numpy(), want, fwd, IMG_TOL * dscale, what, flip_bound=2e-2 * dscale, scale=dscale)


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_oracle_and_leaves_the_rest_alone(hip_device, name, mode):
    dev = hip_device
    case, path = _case(name), CASES[name][1]
    with torch.no_grad():
        views32 = _table_of(case, mode, dev, path)
        assert bool((views32[:, 41] == R.DEPTH_MODES[mode]).all()) and torch.equal(views32[:, 42], case.near) and torch.equal(views32[:, 43], case.far)
        outs, fwds, _ = _expect(case, views32)
        col, feat, mask, depth, radii = _run(case, mode, dev, path=path)
        base = _run(case, None, dev, path=path)
    for v in range(case.V):
        _assert_depth(depth[v][None], outs[v][3], fwds[v], f"{name} {mode} depth[view {v}]")
    # colour, feature, mask and radii do not know about the mode: bit for bit the call without one
    for a, b in zip((col, feat, mask, radii), base[:3] + (base[4],)):
        assert (a is None and b is None) or torch.equal(a, b)
    assert not torch.equal(depth, base[3])


@pytest.mark.parametrize("name", ["fused", "plain"])
def test_native_mode_written_explicitly_is_no_mode(hip_device, name):
    dev = hip_device
    case, path = _case(name), CASES[name][1]
    with torch.no_grad():
        a = _run(case, None, dev, path=path)
        for explicit in ("native", 0):
            b = _run(case, explicit, dev, path=path)
            for x, y in zip(a, b):
                assert (x is None and y is None) or torch.equal(x, y)
        if path == "views":    # and a table without the keyword at all: slots 41..43 are 0.0
            t = table64(case, None)
            assert bool((t[:, 41:44] == 0).all())
            c = _run(case, None, dev, cams=t.to(dev))
            for x, y in zip(a, c):
                assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("mode", MODES)
def test_fused_against_two_pass(hip_device, mode):
    """render_scenes(depth_mode=m).depth against render_depth_scenes(mode=m): same inputs, same compositing decisions, the
    per-Gaussian value computed in the projection kernel instead of on the host."""
    dev = hip_device
    case = _case("fused")
    b = case.S
    u = lambda x: x.to(dev).unflatten(0, (b, case.V // b))
    with torch.no_grad():
        one = _run(case, mode, dev, path="scenes")[3]
        two = cs.render_depth_scenes(u(case.ext), u(case.intr), u(case.near), u(case.far), (case.H, case.W), case.means.to(dev),
                                     case.cov.to(dev), case.opac.to(dev), mode=mode).flatten(0, 1)
    scale = max(1.0, float(two.abs().max()))
    err = float((one - two).abs().max())
    print(f"{mode}: fused vs two-pass max abs err {err:.3e} (scale {scale:.3e})")
    assert err <= IMG_TOL * scale


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_grads(name, mode, dev_index):
    """float64 gradients of the case's loss w.r.t. its scene-level tensors (computed once per (case, mode))."""
    dev = torch.device("cuda", dev_index)
    case, path = _case(name), CASES[name][1]
    views32 = _table_of(case, mode, dev, path)
    w = _weights(case)
    leaves = {k: (None if x is None else x.to(F64).clone().requires_grad_(True)) for k, x in case.leaves().items()}
    _, fwds, loss = _expect(case, views32, w, leaves)
    loss.backward()
    frag = [util.fragile_gaussians(f, case.W) for f in fwds]
    return views32, w, {k: (None if x is None else x.grad) for k, x in leaves.items()}, frag


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["fused", "plain"])
def test_backward_matches_oracle(hip_device, name, mode, rev):
    from latentsplat_amd import _lib
    dev = hip_device
    case, path = _case(name), CASES[name][1]
    views32, w, want, frag = _reference_grads(name, mode, dev.index or 0)
    leaves = {k: (None if x is None else x.to(dev).clone().requires_grad_(True)) for k, x in case.leaves().items()}
    try:
        _lib.set_knob("LSR_BWD_REV", rev)
        col, feat, mask, depth, _ = _run(case, mode, dev, leaves=leaves, path=path)
        loss = 0.0
        for v in range(case.V):
            loss = loss + _loss(col[v].double(), feat[v].double(), mask[v][None].double(), depth[v][None].double(),
                                {k: x.to(dev) for k, x in w[v].items()})
        loss.backward()
    finally:
        _lib.set_knob("LSR_BWD_REV", 2)
    direct = np.unique(np.concatenate([f[0] for f in frag])).astype(np.int64)
    behind = np.unique(np.concatenate([f[1] for f in frag])).astype(np.int64)
    G = case.means.shape[1]
    for k, g in want.items():
        got = leaves[k].grad
        assert got is not None, k
        for s in range(case.S):
            a, b = got[s].detach().cpu().numpy().reshape(G, -1), g[s].numpy().reshape(G, -1)
            util.assert_grad_close_except_fragile(a, b, direct, behind, GRAD_TOL, f"{name} {mode} rev={rev} dL/d{k}[{s}]")


# ---------------------------------------------------------------------------------------------------------------------
# the colour clamp, and the "log" mode as the reference wrote it
# ---------------------------------------------------------------------------------------------------------------------
def _clamp_case():
    sc = make_scene(500, image_size=48, views=2, seed=SEEDS["clamp"], color_sh_degree=None, feature_channels=4)
    g = torch.Generator().manual_seed(2)
    return sc, Case("direct", 48, 48, sc.extrinsics, sc.intrinsics, sc.near, sc.far, sc.means[None],
                    cs._pack_covariances(sc.covariances)[None], sc.opacities[None], torch.rand(1, 500, 3, generator=g),
                    sc.feature_sh[None, ..., 0].contiguous())


def _depth_only_grads(case, mode, dev, views32):
    """d(sum w depth)/d(means, views) on the device and in float64"""
    w = _weights(case, seed=3)
    zero = lambda d: {k: (x if k == "depth" else torch.zeros_like(x)) for k, x in d.items()}
    leaves = {k: (None if x is None else x.to(dev).clone().requires_grad_(True)) for k, x in case.leaves().items()}
    views = views32.to(dev).clone().requires_grad_(True)
    out = _run(case, mode, dev, leaves=leaves, cams=views)
    sum((out[3][v][None].double() * w[v]["depth"].to(dev)).sum() for v in range(case.V)).backward()
    l64 = {k: (None if x is None else x.to(F64).clone().requires_grad_(True)) for k, x in case.leaves().items()}
    v64 = [views32[v].detach().to(F64).clone().requires_grad_(True) for v in range(case.V)]
    outs, fwds, loss = _expect(case, views32, [zero(x) for x in w], l64, v64)
    loss.backward()
    return out, outs, fwds, leaves["means"].grad[0].cpu().double(), views.grad.cpu().double(), l64["means"].grad[0], torch.stack([r.grad for r in v64])


def test_clamped_gaussians_contribute_nothing(hip_device):
    dev = hip_device
    sc, case = _clamp_case()
    # near such that C0 u + 0.5 < 0 (relative disparity: roughly z < 0.36 near) for the nearest ~quarter of the scene; the
    # near cull (view z of the scaled scene <= 0.2) removes what is closer than 0.2 near
    z0 = torch.einsum("bij,gj->bgi", torch.linalg.inv(sc.extrinsics), torch.nn.functional.pad(sc.means, (0, 1), value=1.0))[..., 2]
    case.near = z0.quantile(0.25, dim=1) / 0.34
    case.far = case.near * 40
    views32 = table64(case, "relative_disparity")
    z = torch.stack([du.camera_depth(views32, v, sc.means) for v in range(2)])
    u = R.depth_mode_value(z, case.near[:, None], case.far[:, None], "relative_disparity")
    visible = z > 0.2 * case.near[:, None] * (1 + 1e-6)
    clamped = visible & (R.SH_C0 * u + 0.5 < 0)
    frac = clamped.sum(1).float() / visible.sum(1).float()
    print("clamped share of the visible Gaussians per view:", frac.tolist())
    assert bool(((frac >= 0.05) & (frac <= 0.5)).all())
    zc = z[clamped] / case.near[:, None].expand_as(z)[clamped]
    assert float(zc.min()) >= 0.2 and float(zc.max()) <= 0.37
    assert bool((R.depth_mode_payload(z, case.near[:, None], case.far[:, None], "relative_disparity")[clamped] == 0).all())
    out, outs, fwds, gm, gv, wm, wv = _depth_only_grads(case, "relative_disparity", dev, views32)
    for v in range(2):
        _assert_depth(out[3][v][None].detach(), outs[v][3], fwds[v], f"clamp depth[view {v}]")
    # a Gaussian clamped in BOTH views gets no depth-path gradient at all... its mean still moves the weights of what it
    # occludes, so compare with the oracle (which clamps the same way) rather than with zero
    util.assert_grad_close_except_fragile(gm.numpy(), wm.numpy(), np.zeros(0, np.int64), np.zeros(0, np.int64), GRAD_TOL, "clamp dL/dmeans")
    # near / far receive the gradient of the unclamped Gaussians only.  (The scale slot is not compared here: d depends on
    # z / near alone and view 0 is the identity camera, for which scaling the scene is a symmetry of a depth-only loss — its
    # dL/dscale is the residue of terms that cancel, not a quantity with a relative bar; test_camera_gradients holds slot 40.)
    for v in range(2):
        for sl in (slice(42, 43), slice(43, 44)):
            err, norm = float((gv[v, sl] - wv[v, sl]).abs().max()), float(wv[v, sl].norm())
            print(f"view {v} slot {sl.start}: err {err:.3e} norm {norm:.3e}")
            assert err <= 1e-3 * max(norm, 1e-6), (v, sl, gv[v, sl], wv[v, sl])
    # the payload itself: a scene of ONLY clamped Gaussians renders an all-zero depth image and returns no depth-path gradient
    both = clamped.all(0)
    assert int(both.sum()) >= 8
    sub = Case("direct", 48, 48, case.ext, case.intr, case.near, case.far, case.means[:, both], case.cov[:, both], case.opac[:, both],
               case.color[:, both], case.feat[:, both])
    leaves = {k: x.to(dev).clone().requires_grad_(True) for k, x in sub.leaves().items()}
    views = views32.to(dev).clone().requires_grad_(True)
    o = _run(sub, "relative_disparity", dev, leaves=leaves, cams=views)
    assert float(o[2].max()) > 0.01 and float(o[3].abs().max()) == 0.0
    o[3].sum().backward()
    assert float(leaves["means"].grad.abs().max()) == 0.0 and float(views.grad.abs().max()) == 0.0


def test_log_mode_is_log_far(hip_device):
    """near < far: the reference's ``log(max(min(z, near), far))`` is log(far) for every Gaussian — reproduced, not fixed."""
    dev = hip_device
    sc, case = _clamp_case()
    views32 = table64(case, "log")
    z = torch.stack([du.camera_depth(views32, v, sc.means) for v in range(2)])
    d = R.depth_mode_payload(z, case.near[:, None], case.far[:, None], "log")
    want = torch.clamp_min(R.SH_C0 * case.far.log() + 0.5, 0.0)
    assert torch.allclose(d, want[:, None].expand_as(d), rtol=1e-6, atol=0)
    out, outs, fwds, gm, gv, wm, wv = _depth_only_grads(case, "log", dev, views32)
    for v in range(2):
        _assert_depth(out[3][v][None].detach(), outs[v][3], fwds[v], f"log depth[view {v}]")
        # depth = d(far) * mask, to float rounding
        assert torch.allclose(out[3][v].detach().cpu(), float(want[v]) * out[2][v].detach().cpu(), rtol=1e-5, atol=1e-6)
        assert float(gv[v, 43].abs()) > 0 and float(gv[v, 42]) == 0.0
        assert abs(float(gv[v, 43] - wv[v, 43])) <= 1e-3 * abs(float(wv[v, 43]))
    # the means still receive the gradient of the WEIGHTS (the payload is a constant): what the oracle says, at the bar
    util.assert_grad_close_except_fragile(gm.numpy(), wm.numpy(), np.zeros(0, np.int64), np.zeros(0, np.int64), GRAD_TOL, "log dL/dmeans")
    # and the depth PATH (dL/dd dd/dz) is zero: with a cotangent on the depth only, the table's scale slot gets exactly the
    # projection's gradient, i.e. what a native-depth run with the cotangent w * d(far) on the MASK gives
    leaves = {k: x.to(dev).clone().requires_grad_(True) for k, x in case.leaves().items()}
    views = table64(case, None).to(dev).clone().requires_grad_(True)
    o = _run(case, None, dev, leaves=leaves, cams=views)
    w = _weights(case, seed=3)
    sum((o[2][v][None].double() * float(want[v]) * w[v]["depth"].to(dev)).sum() for v in range(2)).backward()
    ref = leaves["means"].grad[0].cpu().double()
    assert float((gm - ref).abs().max()) <= GRAD_TOL * max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["disparity", "relative_disparity"])
def test_camera_gradients(hip_device, mode):
    dev = hip_device
    sc = make_scene(200, image_size=32, views=2, seed=SEEDS["camera"], color_sh_degree=1, feature_channels=4, feature_sh_degree=0)
    ext = sc.extrinsics.clone()
    ext[:, :3, 3] += torch.tensor([0.03, -0.02, 0.05])
    case = Case("sh", 32, 32, ext, sc.intrinsics, sc.near * 1.2, sc.far, sc.means[None], sc.covariances[None], sc.opacities[None],
                sc.color_sh[None], sc.feature_sh[None])
    w = _weights(case, seed=5)
    wd = lambda v: {k: x.to(dev) for k, x in w[v].items()}
    gpu_loss = lambda o: sum(_loss(o[0][v].double(), o[1][v].double(), o[2][v][None].double(), o[3][v][None].double(), wd(v)) for v in range(2))
    # (1) dL/d(view record) of the op itself: slots 40, 42, 43 (and the rest) against the float64 statement
    views32 = table64(case, mode)
    views = views32.to(dev).clone().requires_grad_(True)
    t = {k: x.to(dev) for k, x in case.leaves().items()}
    o = R.rasterize_views(views, 32, 32, 1, t["means"][0], t["cov"][0], t["opac"][0][:, None], shs=t["color"][0], shs_channel_major=True,
                          feature_sh=t["feat"][0])
    gpu_loss(o).backward()
    got = views.grad.cpu().double()
    v64 = [views32[v].detach().to(F64).clone().requires_grad_(True) for v in range(2)]
    _, _, loss = _expect(case, views32, w, None, v64)
    loss.backward()
    blocks = dict(vm=slice(0, 16), pm=slice(16, 32), campos=slice(32, 35), tanfov=slice(35, 37), bg=slice(37, 40), scale=slice(40, 41),
                  near=slice(42, 43), far=slice(43, 44))
    for v in range(2):
        want = v64[v].grad
        assert float(want[41]) == 0.0 and float(got[v, 41]) == 0.0
        for nm, sl in blocks.items():
            err, norm = float((got[v, sl] - want[sl]).abs().max()), float(want[sl].norm())
            print(f"view {v} {nm}: err {err:.3e} norm {norm:.3e}")
            assert err <= 1e-3 * max(norm, 1e-6), (v, nm, got[v, sl], want[sl])
        if mode == "disparity":
            assert float(got[v, 42]) == 0.0 and float(got[v, 43]) == 0.0
        else:
            assert float(got[v, 42].abs()) > 0 and float(got[v, 43].abs()) > 0
    # (2) chained into the leaves through render_cuda and render_scenes
    cams = [case.ext, case.intr, case.near, case.far]
    c64 = [c.to(F64).clone().requires_grad_(True) for c in cams]
    _, _, loss = _expect(case, table64(case, mode), w, None, table64(case, mode, c64, dtype=F64))
    loss.backward()
    for path in ("cuda", "scenes"):
        leaves = [c.to(dev).clone().requires_grad_(True) for c in cams]
        tt = t if path == "scenes" else {k: x.expand(2, *x.shape[1:]).contiguous() for k, x in t.items()}
        o = _run(case, mode, dev, leaves=tt, path=path, cams=leaves)
        gpu_loss(o).backward()
        _assert_grads_close([x.grad for x in leaves], [x.grad for x in c64], 2e-3, names=("extrinsics", "intrinsics", "near", "far"))
    # (3) without a mode the three slots receive exactly nothing
    views = table64(case, None).to(dev).clone().requires_grad_(True)
    o = R.rasterize_views(views, 32, 32, 1, t["means"][0], t["cov"][0], t["opac"][0][:, None], shs=t["color"][0], shs_channel_major=True,
                          feature_sh=t["feat"][0])
    gpu_loss(o).backward()
    assert bool((views.grad[:, 41:44] == 0).all()) and float(views.grad[:, 40].abs().min()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.asarray(a)).to(dev)


def _decoder_forward(g, dev, mode):
    from latentsplat_amd import decoder as dec
    gauss = dec.Gaussians(_t(g["in_means"], dev), _t(g["in_covariances"], dev), _t(g["in_opacities"], dev),
                          _t(g["in_color_harmonics"], dev), _t(g["in_feature_harmonics"], dev))
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), [float(x) for x in g["in_bg"]], False).to(dev)
    calls = []
    real = cs.rasterize_views
    cs.rasterize_views = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    dec.set_fused_depth_modes(True)
    try:
        out = d.forward(gauss, _t(g["in_extrinsics"], dev), _t(g["in_intrinsics"], dev), _t(g["in_near"], dev),
                        _t(g["in_far"], dev), tuple(int(x) for x in g["in_image_shape"]), depth_mode=mode)
    finally:
        dec.set_fused_depth_modes(False)
        cs.rasterize_views = real
    assert len(calls) == 1
    return out


def _assert_decoder(out, want):
    """the bars tests/test_surface_gpu.py holds the decoder fixtures to"""
    np.testing.assert_allclose(out.mask.cpu().numpy(), want["mask"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(out.depth.cpu().numpy(), want["depth"], atol=1e-4 * max(1.0, np.abs(want["depth"]).max()), rtol=0)
    np.testing.assert_allclose(out.color.cpu().numpy(), want["color"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(out.feature_posterior.mean.cpu().numpy(), want["posterior_mean"], atol=1e-4, rtol=0)
    lv, lw = out.feature_posterior.logvar.cpu().numpy(), want["posterior_logvar"]
    np.testing.assert_allclose(np.exp(np.minimum(lv, 20.0)), np.exp(np.minimum(lw, 20.0)),
                               atol=1e-4 * max(1.0, float(np.exp(np.minimum(lw, 20.0)).max())), rtol=0)
    sel = lw > -4
    np.testing.assert_allclose(lv[sel], lw[sel], atol=6e-3, rtol=0)


def test_decoder_disparity_fixture_with_the_switch_on(hip_device):
    g = np.load(os.path.join(GOLD, "boundary_disparity_depth.npz"))
    want = np.load(os.path.join(GOLD, "decoder_disparity_depth.npz"))
    with torch.no_grad():
        _assert_decoder(_decoder_forward(g, hip_device, "disparity"), want)


@pytest.mark.parametrize("mode", ["relative_disparity", "log"])
def test_decoder_new_fixtures_with_the_switch_on(hip_device, mode):
    g = du.load_fixture()
    want = dict(mask=g["decoder_mask"], depth=g[f"depth_{mode}"], color=g["decoder_color"],
                posterior_mean=g["decoder_posterior_mean"], posterior_logvar=g["decoder_posterior_logvar"])
    with torch.no_grad():
        _assert_decoder(_decoder_forward(g, hip_device, mode), want)
