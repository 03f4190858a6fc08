"""Absolute view-space gradients (AbsGS; ``means2D_abs``, ``lsr_backward_absgrad``) on the MI355X against the float64
restatement of tests/absgrad_ref.py: every instance of the compositing backward that carries the two magnitude sums (plain and
list-splitting, both walk orders, with and without the depth gradient, fixed-point flush), the view-parallel instances of the
projection backward, the modes, the output buffer, the ordinary gradients of the same call, and the autograd surfaces.

Every check:  err <= max(CLEAN_TOL x max |want|, 4 x stock error)  (tests/absgrad_ref.py ``hold``), printed with the kernel
error, the stock error and their ratio."""
from __future__ import annotations

import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd import rasterizer as R
from latentsplat_amd.density import DensityControl
from latentsplat_amd.scene_model import GaussianScene
from tests import absgrad_ref as A

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _run(c, absgrad=True, with_depth=True, poison=False):
    """One forward and backward of ``rasterize_views`` on the case under the loss of absgrad_ref: dict of host tensors —
    ``abs`` (V, G, 2) (None without ``absgrad``), ``m2d`` (V, G, 2), ``radii``, ``grads`` name -> gradient, ``raw`` the
    (V, G, 3) abs gradient as it came."""
    dev = torch.device("cuda:0")
    L = {k: t.to(dev).clone().requires_grad_(True) for k, t in A.tensors(c).items()}
    kw = {k: L[k] for k in L if k not in ("means", "cov", "opac")}
    if c.antialiasing:
        kw["antialiasing"] = True
    m2d = torch.zeros(c.V, c.G, 3, device=dev, requires_grad=True)
    mabs = torch.zeros(c.V, c.G, 3, device=dev, requires_grad=True) if absgrad else None
    if absgrad:
        kw["means2D_abs"] = mabs
    col, feat, mask, depth, radii = R.rasterize_views(c.views.to(dev), c.H, c.W, c.kw.get("sh_degree", 0), L["means"], L["cov"],
                                                      L["opac"], means2D=m2d, **kw)
    w = A.weights(c)
    loss = 0.0
    for v in range(c.V):
        loss = loss + A.loss(None if col is None else col[v].double(), None if feat is None else feat[v].double(),
                             mask[v][None].double(), depth[v][None].double(), {k: t.to(dev) for k, t in w[v].items()}, with_depth)
    if poison:
        # best effort against stale memory (as tests/test_camera_grads_gpu.py does for its workspace): blocks of the output's
        # size filled with NaN and freed are what the caching allocator most likely hands the backward's torch.empty
        for _ in range(3):
            torch.full((c.V, c.G, 3), NAN, device=dev)
    loss.backward()
    torch.cuda.synchronize()
    return dict(abs=None if mabs is None else mabs.grad[..., :2].cpu(), raw=None if mabs is None else mabs.grad.cpu(),
                m2d=m2d.grad[..., :2].cpu(), m2d_raw=m2d.grad.cpu(), radii=radii.cpu(), grads={k: t.grad.cpu() for k, t in L.items()})


def _hold_abs(c, got, with_depth=True, what=None):
    want, stock = A.references(c.name, with_depth)
    what = what or c.name
    assert torch.equal(got["radii"], want["radii"]), what
    A.hold(what, "abs", got["abs"], want["abs"], stock["abs"])
    A.hold(what, "means2D", got["m2d"], want["signed"], stock["signed"])
    assert float(got["raw"][..., 2].abs().max()) == 0.0


def _hold_ordinary(c, got, with_depth=True, what=None):
    want, stock = A.references(c.name, with_depth)
    for k, g in got["grads"].items():
        A.hold(what or c.name, k, g, want["grads"][k], stock["grads"][k])
    A.hold(what or c.name, "means2D", got["m2d"], want["signed"], stock["signed"])


class _Knobs:
    """Development knobs of the library for the duration of a block, restored to their defaults afterwards."""
    DEFAULTS = dict(LSR_BWD_PARTS=-1, LSR_BWD_REV=2, LSR_DETERMINISTIC=0)

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        for k, v in self.values.items():
            _lib.set_knob(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            _lib.set_knob(k, self.DEFAULTS[k])


# ---- 1. views: the PARTS instances of the projection backward -------------------------------------------------------------
@pytest.mark.parametrize("name", ["V1", "V3", "V5"])
def test_views(hip_device, name):
    c = A.case(name)
    _hold_abs(c, _run(c))


# ---- 2. the compositing instances ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("parts", [0, 3])
def test_compositing_instances(hip_device, parts, rev, with_depth, det):
    """LSR_BWD_PARTS 0: the plain instance (at 32 x 32 a launch always splits otherwise), 3: every list walked by 8 waves;
    LSR_BWD_REV 0 / 1: front to back / back to front; with / without g_depth: the DEPTH_GRAD instances (full / packed table
    row); LSR_DETERMINISTIC: the fixed-point flush."""
    c = A.case("V3")
    with _Knobs(LSR_BWD_PARTS=parts, LSR_BWD_REV=rev, LSR_DETERMINISTIC=det):
        got = _run(c, with_depth=with_depth)
    _hold_abs(c, got, with_depth, what=f"V3 parts {parts} rev {rev} depth {int(with_depth)} det {det}")


# ---- 3. modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aa", "perview", "feat"])
def test_modes(hip_device, name):
    """antialiasing=True with sub-pixel splats (u carries o' = o rho); per-view (V, G, .) inputs; 3 colours + 1 feature (the 4
    padded channels full, slots 14 / 15 right behind them)"""
    c = A.case(name)
    got = _run(c)
    _hold_abs(c, got)
    _hold_ordinary(c, got)


# ---- 4. buffer and equality -------------------------------------------------------------------------------------------
def test_every_row_is_written_and_culled_rows_are_zero(hip_device):
    c = A.case("V5")
    got = _run(c, poison=True)
    assert bool(torch.isfinite(got["raw"]).all())
    culled = got["radii"] == 0
    assert bool(culled.any()) and bool((~culled).any())
    assert float(got["raw"][culled].abs().max()) == 0.0
    want, _ = A.references("V5")
    reached = want["abs"].amax(-1) > 0
    assert bool((got["raw"][..., :2].amax(-1)[reached] > 0).all())       # and zero rows ONLY where nothing arrives
    _hold_abs(c, got)


def test_c_abi_writes_every_row_of_a_nan_buffer(hip_device):
    """``lsr_backward_absgrad`` itself (no camera gradient: grad_views / view_grad_ws NULL) on a ``means2D_abs`` buffer
    pre-filled with NaN: finite everywhere, zero rows exactly where radii == 0, the values at the bar."""
    import ctypes as C
    from tests.antialias_ref import Run
    dev = torch.device("cuda:0")
    c = A.case("V5")
    want, stock = A.references("V5")
    shs = c.kw["shs"].to(dev).contiguous()
    d = _lib.Dims(c.V, c.G, c.H, c.W, 0, _lib.COLOR_SH, c.kw["sh_degree"], shs.shape[-2], 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0, 0, 0)
    run = Run(c.views.to(dev).contiguous(), c.means.to(dev).contiguous(), c.cov.to(dev).contiguous(), c.opac.to(dev).contiguous(),
              shs, None, d)
    assert torch.equal(run.radii.cpu(), want["radii"])
    w = A.weights(c)
    g = lambda k: torch.stack([x[k] for x in w]).float().to(dev).contiguous()
    g_color, g_mask, g_depth = g("col"), g("mask")[:, 0].contiguous(), g("depth")[:, 0].contiguous()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f32 = dict(dtype=torch.float32, device=dev)
    d_means, d_cov, d_opac, d_shs = (torch.empty_like(t) for t in (run.means, run.cov6, run.opac, shs))
    d_m2d = torch.full((c.V, c.G, 3), NAN, **f32)
    d_abs = torch.full((c.V, c.G, 3), NAN, **f32)
    gradws = torch.empty(run.lib.lsr_grad_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
    fwd = _lib.Outputs(p(run.color_out), None, None, p(run.depth_out), None, None)
    gout = _lib.OutGrads(p(g_color), None, p(g_mask), p(g_depth))
    gin = _lib.InGrads(p(d_means), p(d_cov), p(d_opac), p(d_shs), None, p(d_m2d))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(run.lib.lsr_backward_absgrad(C.byref(d), C.byref(run.inp), p(run.geom), p(run.bin), p(run.img), run.P, p(run.radii),
                                            C.byref(fwd), C.byref(gout), p(gradws), C.byref(gin), None, None, p(d_abs), stream),
               "lsr_backward_absgrad")
    torch.cuda.synchronize()
    got = d_abs.cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(d_m2d).all())
    culled = want["radii"] == 0
    assert bool(culled.any()) and float(got[culled].abs().max()) == 0.0 and float(got[..., 2].abs().max()) == 0.0
    A.hold("C ABI, NaN buffer", "abs", got[..., :2], want["abs"], stock["abs"])
    A.hold("C ABI, NaN buffer", "means2D", d_m2d[..., :2].cpu(), want["signed"], stock["signed"])


def test_camera_gradient_in_the_same_call(hip_device):
    """views.requires_grad together with ``means2D_abs``: ``lsr_backward_absgrad`` with grad_views — the camera gradient is the
    one of the call without ``means2D_abs`` (bit for bit under LSR_DETERMINISTIC), the abs gradient the one without cameras"""
    dev = torch.device("cuda:0")
    c = A.case("V3")

    def run(absgrad):
        views = c.views.to(dev).requires_grad_(True)
        L = {k: t.to(dev).clone().requires_grad_(True) for k, t in A.tensors(c).items()}
        mabs = torch.zeros(c.V, c.G, 3, device=dev, requires_grad=True)
        col, _, mask, depth, _ = R.rasterize_views(views, c.H, c.W, c.kw["sh_degree"], L["means"], L["cov"], L["opac"], shs=L["shs"],
                                                   **(dict(means2D_abs=mabs) if absgrad else {}))
        w = A.weights(c)
        sum(A.loss(col[v].double(), None, mask[v][None].double(), depth[v][None].double(), {k: t.to(dev) for k, t in w[v].items()})
            for v in range(c.V)).backward()
        return views.grad.cpu(), mabs.grad, L["means"].grad.cpu()

    with _Knobs(LSR_DETERMINISTIC=1):
        (va, ga, ma), (vb, gb, mb) = run(True), run(False)
    assert gb is None and torch.equal(va, vb) and torch.equal(ma, mb) and float(va.abs().max()) > 0
    want, stock = A.references("V3")
    A.hold("V3 with camera gradient", "abs", ga[..., :2].cpu(), want["abs"], stock["abs"])


@pytest.mark.parametrize("name", ["V3", "aa", "feat"])
def test_abs_dominates_the_signed_gradient_of_the_same_call(hip_device, name):
    c = A.case(name)
    got = _run(c)
    want, stock = A.references(name)
    bar = A.bar(want["abs"], stock["abs"])[0] + A.bar(want["signed"], stock["signed"])[0]
    short = float((got["m2d"].abs().double() - got["abs"].double()).max())
    print(f"{name}: max(|means2D grad| - abs) = {short:.3e}, bar {bar:.3e}")
    assert short <= bar


def test_one_pixel_splats_have_equal_abs_and_signed_gradients(hip_device):
    c = A.case("onepix")
    got = _run(c)
    _hold_abs(c, got)
    want, stock = A.references("onepix")
    assert int((got["abs"].amax(-1) > 0).sum()) == A.ONEPIX
    bar = A.bar(want["abs"], stock["abs"])[0] + A.bar(want["signed"], stock["signed"])[0]     # each side at its own bar
    diff = float((got["abs"].double() - got["m2d"].abs().double()).abs().max())
    print(f"onepix: max |abs - |means2D grad|| = {diff:.3e}, bar {bar:.3e}")
    assert diff <= bar


# ---- 5. the ordinary gradients of a call that asks for the abs gradient -----------------------------------------------------
@pytest.mark.parametrize("with_depth", [True, False])
def test_ordinary_gradients_pass_the_oracle_check(hip_device, with_depth):
    c = A.case("V5")
    _hold_ordinary(c, _run(c, absgrad=True, with_depth=with_depth), with_depth, what="V5 with means2D_abs")
    _hold_ordinary(c, _run(c, absgrad=False, with_depth=with_depth), with_depth, what="V5 without")


@pytest.mark.parametrize("parts", [0, -1])
def test_ordinary_gradients_bitwise_in_deterministic_mode(hip_device, parts):
    """Under LSR_DETERMINISTIC the cross-tile sums are order independent, so the call with and the call without
    ``means2D_abs`` can be compared bit for bit: the ABS instances form every ordinary record slot with the operations of the
    plain ones."""
    c = A.case("V5")
    with _Knobs(LSR_DETERMINISTIC=1, LSR_BWD_PARTS=parts):
        a, b = _run(c, absgrad=True), _run(c, absgrad=False)
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert torch.equal(a["m2d_raw"], b["m2d_raw"])


# ---- 6. autograd surfaces ---------------------------------------------------------------------------------------------
def test_shared_leaf_sums_the_views(hip_device):
    """a (G, 3) ``means2D_abs`` receives the sum over the views, as a shared ``means2D`` does"""
    dev = torch.device("cuda:0")
    c = A.case("V3")
    L = {k: t.to(dev) for k, t in A.tensors(c).items()}
    mabs = torch.zeros(c.G, 3, device=dev, requires_grad=True)
    col, _, mask, depth, _ = R.rasterize_views(c.views.to(dev), c.H, c.W, c.kw["sh_degree"], L["means"].requires_grad_(True), L["cov"],
                                               L["opac"], shs=L["shs"], means2D_abs=mabs)
    w = A.weights(c)
    sum(A.loss(col[v].double(), None, mask[v][None].double(), depth[v][None].double(), {k: t.to(dev) for k, t in w[v].items()})
        for v in range(c.V)).backward()
    want, stock = A.references("V3")
    A.hold("V3 shared leaf", "abs", mabs.grad[:, :2].cpu(), want["abs"].sum(0), stock["abs"].sum(0))


def test_drop_in_rasterizer_delivers_the_gradient(hip_device):
    dev = torch.device("cuda:0")
    c = A.case("V1")
    rec = c.views[0]
    rs = R.GaussianRasterizationSettings(c.H, c.W, float(rec[35]), float(rec[36]), rec[37:40].to(dev), 1.0,
                                         rec[0:16].reshape(4, 4).to(dev), rec[16:32].reshape(4, 4).to(dev), c.kw["sh_degree"],
                                         rec[32:35].to(dev), False, False)
    s = float(rec[40])
    means = (c.means * s).to(dev).requires_grad_(True)
    mabs = torch.zeros(c.G, 3, device=dev, requires_grad=True)
    m2d = torch.zeros(c.G, 3, device=dev, requires_grad=True)
    col, _, mask, depth, radii = R.GaussianRasterizer(rs)(means3D=means, means2D=m2d, opacities=c.opac.to(dev), shs=c.kw["shs"].to(dev),
                                                          cov3D_precomp=(c.cov * s * s).to(dev), means2D_abs=mabs)
    w = {k: t.to(dev) for k, t in A.weights(c)[0].items()}
    A.loss(col.double(), None, mask.double(), depth.double(), w).backward()
    want, stock = A.references("V1")
    A.hold("GaussianRasterizer", "abs", mabs.grad[:, :2].cpu(), want["abs"][0], stock["abs"][0])
    A.hold("GaussianRasterizer", "means2D", m2d.grad[:, :2].cpu(), want["signed"][0], stock["signed"][0])


def test_more_than_four_channels_raises(hip_device):
    dev = torch.device("cuda:0")
    c = A.case("feat")
    L = {k: t.to(dev) for k, t in A.tensors(c).items()}
    mabs = torch.zeros(c.V, c.G, 3, device=dev, requires_grad=True)
    feats = torch.rand(c.G, 2, device=dev)
    with pytest.raises(_lib.LsrError, match="payload channels"):
        R.rasterize_views(c.views.to(dev), c.H, c.W, 0, L["means"].requires_grad_(True), L["cov"], L["opac"],
                          colors_precomp=L["colors_precomp"], features=feats, means2D_abs=mabs)
    with pytest.raises(_lib.LsrError, match="payload channels"):
        R.rasterize_views(c.views.to(dev), c.H, c.W, 0, L["means"], L["cov"], L["opac"], features=torch.rand(c.G, 5, device=dev),
                          means2D_abs=mabs)


def _scene_of(c, dev):
    """A GaussianScene whose activation reproduces nothing in particular: 160 Gaussians in front of the case's cameras."""
    g = torch.Generator().manual_seed(3)
    n = c.G
    return GaussianScene.from_tensors(c.means.to(dev), (0.5 * torch.randn(n, 1, 3, generator=g)).to(dev),
                                      (0.1 * torch.randn(n, 3, 3, generator=g)).to(dev), torch.randn(n, 1, generator=g).to(dev),
                                      (torch.randn(n, 3, generator=g) * 0.3 - 2.5).to(dev), torch.randn(n, 4, generator=g).to(dev))


def test_scene_render_and_density_control(hip_device):
    """``scene.render(means2D_abs=)`` delivers the gradient, and ``DensityControl.update`` accumulates its norm over the
    visible views: checked against the restatement on the scene's own activated tensors."""
    dev = torch.device("cuda:0")
    base = A.case("V3")
    scene = _scene_of(base, dev)
    a = scene.activated()
    c = A.cases.Case(base.views, 32, 32, a.means.detach().cpu(), a.covariances.detach().cpu(), a.opacities.detach().cpu().reshape(-1, 1),
                     dict(shs=a.shs.detach().cpu().contiguous(), sh_degree=int(a.sh_degree)), None, 0)
    c.name, c.antialiasing = "scene", False
    assert c.cov.shape[-1] == 6
    fragile = A.cases.fragile_counts(c.views, 32, 32, c.means, c.cov, c.opac, A.payload_of(c))
    assert fragile == [0] * c.V, fragile          # (a decision within rounding of a threshold has no gradient to compare)
    want, stock = A.reference(c), A.reference(c, torch.float32)
    control = DensityControl(scene)
    (col, _, mask, depth, radii), leaf = control.render(base.views.to(dev), 32, 32, absgrad=True)
    assert leaf.shape == (c.V, c.G, 3)
    w = A.weights(c)
    sum(A.loss(col[v].double(), None, mask[v][None].double(), depth[v][None].double(), {k: t.to(dev) for k, t in w[v].items()})
        for v in range(c.V)).backward()
    assert torch.equal(radii.cpu(), want["radii"])
    A.hold("scene.render", "abs", leaf.grad[..., :2].cpu(), want["abs"], stock["abs"])
    control.update(leaf.grad, radii)
    vis = (want["radii"] > 0).double()
    norm = lambda r: (r["abs"].norm(dim=-1) * vis).sum(0)
    A.hold("DensityControl.update", "accum", control.xyz_gradient_accum[:, 0].cpu(), norm(want), norm(stock))
    assert torch.equal(control.denom[:, 0].cpu().double(), vis.sum(0))
    # the classic leaf through the same convenience is the signed gradient
    (_, _, _, _, _), leaf2 = control.render(base.views.to(dev), 32, 32)
    assert leaf2.grad is None and leaf2.requires_grad


def test_fit_tool_with_absgrad(hip_device, tmp_path):
    """tools/fit_ply.py --absgrad: the densification runs on the absolute gradient, the threshold's default follows, and
    fit.json says so (the tool is what this test is about: 20 steps at 48 x 48)"""
    import json
    import os
    import sys
    from tests import scene_params_ref as sref
    from tests import util
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, 2000, 64, 2)
    common = [str(path), "--views", "3", "--size", "48", "--steps", "20", "--drop", "0.5", "--densify-interval", "5", "--densify-until", "6"]
    res = fit_ply.main(common + ["--out", str(tmp_path / "abs"), "--absgrad"])
    classic = fit_ply.main(common + ["--out", str(tmp_path / "classic")])
    assert json.load(open(tmp_path / "abs" / "fit.json")) == res
    assert res["absgrad"] is True and classic["absgrad"] is False
    ev, ev0 = res["densify_events"], classic["densify_events"]
    print("absgrad event:", ev, "\nclassic event:", ev0)
    assert [e["step"] for e in ev] == [5] and ev[0]["n_out"] > res["gaussians_first"] == classic["gaussians_first"]
    assert res["loss_last"] < res["loss_first"]


def test_worst_figures(hip_device):
    """(last: prints what the checks above measured, kernel error / bar per quantity)"""
    print("worst kernel / bar:", ", ".join(f"{k} {v:.3f}" for k, v in sorted(A.WORST.items())))
