"""The 3D smoothing filter on the MI355X: lsr_filter3d_compute against the float64 restatement of the published loop over
cameras (tests/filter3d_ref.py), lsr_scene_activate_filtered_forward / _backward against float64 autograd, and the filter
through GaussianScene: the filtered render against the fused scene, the gradients a render sends down, the saved file and
the fitting tool."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import filter3d_ref as fref
from tests import scene_params_ref as sref
from tests import util
from tests.test_scene_params_gpu import SHAPES

pytestmark = pytest.mark.gpu

WIDTH = 64
PAST_THE_GRID = 2048 * 256 + 3          # the pass caps its grid at 2048 workgroups of 256 lanes: lanes take a second row
H = W = 64
G, VIEWS = 2000, 2
UP = ("shs", "opacities", "cov3D")


def _np(d: dict) -> dict:
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


def _dev(p: dict, dev, keys=sref.PARAMS):
    return [torch.from_numpy(p[k]).to(dev) for k in keys]


def _pass(pts: np.ndarray, views: np.ndarray, dev, **kw):
    from latentsplat_amd import compute_filter_3d
    f, seen = compute_filter_3d(torch.from_numpy(pts).to(dev), torch.from_numpy(views).to(dev), WIDTH, return_seen=True, **kw)
    assert f.shape == (len(pts), 1) and f.dtype == torch.float32 and seen.shape == (len(pts),) and seen.dtype == torch.bool
    return f.cpu().numpy()[:, 0], seen.cpu().numpy()


def _check_pass(pts, views, dev, show, margin=0.15, variance=0.2):
    """Both modes against the restatement: `seen` exactly (the builders leave no pair at a threshold, and that is asserted,
    so no pair is left out), the filter within the derived rounding bound."""
    for per_view in (False, True):
        ref = fref.filter_ref(pts, views, WIDTH, margin, variance, per_view)
        assert ref["near"] == 0, "the inputs leave a pair at a threshold"
        got, seen = _pass(pts, views, dev, margin=margin, variance=variance, per_view=per_view)
        assert np.array_equal(seen, ref["seen"])
        err = np.abs(got.astype(np.float64) - ref["filter"])
        worst = np.max(err / np.maximum(ref["bound"], 1e-300), initial=0.0)
        print(f"{show} per_view={per_view}: seen {int(seen.sum())}/{len(pts)}, worst err / bound {worst:.3f} (bound = 8 u T / s sqrt(var) / F)")
        assert (err <= ref["bound"]).all()
        again, seen_again = _pass(pts, views, dev, margin=margin, variance=variance, per_view=per_view)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(seen_again, seen)
    return ref


# (n, V).  k_filter3d_cameras is one workgroup of 256 lanes, and compute_filter_3d is handed every training camera of a
# dataset: from camera 256 on a lane compacts a second record (V = 257: lane 0 alone) and a third (V = 600), and the
# largest focal length is taken over all of them.
CAMERA_LANES = 256                      # kFilterThreads
PASS_CASES = [(n, V) for V in (1, 2, 65) for n in (1, 63, 64, 65, 257, 1031)] + [(65, 257), (257, 257), (65, 600), (257, 600)]


@pytest.mark.parametrize("n,V", PASS_CASES)
def test_filter_pass_matches_the_published_loop(hip_device, n, V):
    views = fref.circle_views(V, seed=V)
    if V > CAMERA_LANES:
        # On a dense circle no single camera decides who is seen, so one lost record would not show.  The last camera, whose
        # record only a lane's last trip compacts, gets the narrowest field of view by a tenth: it alone sets the largest
        # focal length F, and F scales every filter of the published mode (the bound on a filter is a few 1e-7 of it).
        views[V - 1, 35] = np.float32(0.9) * views[:, 35].min()
        focal = WIDTH / (2.0 * views[:, 35].astype(np.float64))
        assert focal[V - 1] > 1.1 * focal[:V - 1].max()
    pts = fref.draw_points(n, views, seed=100 * V + n)
    ref = _check_pass(pts, views, hip_device, f"n={n} V={V}")
    if n >= 257:                                              # the draw covers every kind of pair
        pz = np.stack([fref.project(pts.astype(np.float64), r.astype(np.float64))[2] for r in views])
        assert (pz < fref.NEAR).any() and ref["seen"].any() and not ref["seen"].all()
        tight = fref.filter_ref(pts, views, WIDTH, margin=0.0)["seen"]
        assert (ref["seen"] & ~tight).any()                   # ... some seen only inside the margin


def test_filter_pass_past_the_grid_cap(hip_device):
    views = fref.circle_views(2, seed=7)
    pts = fref.draw_points(PAST_THE_GRID, views, seed=8)
    ref = _check_pass(pts, views, hip_device, f"n={PAST_THE_GRID} V=2")
    assert 0 < ref["seen"].sum() < PAST_THE_GRID


def test_filter_pass_with_a_scene_scale(hip_device):
    """A table of build_view_table(scale_invariant=True) with near = 2: view[40] = 0.5, translations halved."""
    from latentsplat_amd.rasterizer import build_view_table
    V, dev = 3, hip_device
    ext = torch.from_numpy(fref.circle_extrinsics(V, seed=5).astype(np.float32)).to(dev)
    intr = torch.tensor([[[1.1, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1.0]], [[0.8, 0, 0.5], [0, 1.3, 0.5], [0, 0, 1.0]],
                         [[1.6, 0, 0.5], [0, 1.6, 0.5], [0, 0, 1.0]]], device=dev)
    table = build_view_table(ext, intr, torch.full((V,), 2.0, device=dev), torch.full((V,), 50.0, device=dev),
                             torch.zeros(3, device=dev), scale_invariant=True)
    views = table.cpu().numpy()
    assert np.array_equal(views[:, 40], np.full(V, 0.5, np.float32))
    pts = fref.draw_points(777, views, seed=6)
    ref = _check_pass(pts, views, dev, "scale 0.5")
    assert 0 < ref["seen"].sum() < 777


def test_points_either_side_of_every_threshold(hip_device):
    """Explicit points 1 % inside and outside the near plane and the widened frustum of one camera, and inside the margin
    band, at the default and at another margin: `seen` is what the construction says."""
    for margin in (0.15, 0.3):
        views = fref.circle_views(3, seed=11)
        pts, valid = fref.threshold_points(views[0], margin)
        got, seen = _pass(pts, views[:1], hip_device, margin=margin)
        ref = fref.filter_ref(pts, views[:1], WIDTH, margin)
        assert ref["near"] == 0 and np.array_equal(ref["seen"], valid) and np.array_equal(seen, valid)
        assert (np.abs(got - ref["filter"]) <= ref["bound"]).all()
        assert np.allclose(got[~valid], got[valid].max(), rtol=0, atol=0)        # the unseen take the largest seen filter
        _check_pass(pts, views, hip_device, f"thresholds margin={margin}", margin=margin, variance=0.5)


def test_unseen_and_non_finite_points(hip_device):
    views = fref.circle_views(1, seed=3)
    behind = np.stack([fref.world_point(views[0], (x, 0.1, -1.0 - 0.01 * i)) for i, x in enumerate(np.linspace(-1, 1, 70))])
    got, seen = _pass(behind, views, hip_device)
    assert not seen.any() and not got.any()                                       # nothing seen: every filter is 0
    views = fref.circle_views(4, seed=3)
    pts = fref.draw_points(300, views, seed=9)
    clean, clean_seen = _pass(pts, views, hip_device)
    assert clean_seen[:64].any()
    bad = pts.copy()
    bad[5, 0], bad[64, 2], bad[130, 1], bad[299] = np.nan, np.nan, np.inf, np.nan
    got, seen = _pass(bad, views, hip_device)
    ref = fref.filter_ref(bad, views, WIDTH)
    rows = [5, 64, 130, 299]
    assert not seen[rows].any() and np.array_equal(seen, ref["seen"])
    assert (got[rows] == got[seen].max()).all() and np.isfinite(got).all()        # the fallback value
    keep = np.ones(300, bool)
    keep[rows] = False
    untouched = keep & clean_seen
    assert np.array_equal(got[untouched], clean[untouched])                       # no other row's own value changes
    # a camera that cannot be used (a NaN tanfov, a zero scale) sees nothing and does not enter the largest focal length
    broken = views.copy()
    broken[1, 35], broken[2, 40] = np.nan, 0.0
    got_b, seen_b = _pass(pts, broken, hip_device)
    ref_b = fref.filter_ref(pts, broken[[0, 3]], WIDTH)
    assert np.array_equal(seen_b, ref_b["seen"]) and (np.abs(got_b - ref_b["filter"]) <= ref_b["bound"]).all()


# ---- the filtered activation ----

CASES = [(n, K, m) for n, K in SHAPES for m in (1.0, 0.5)]


@pytest.mark.parametrize("n,K,m", CASES)
def test_filtered_forward_and_backward_match_the_restatement(hip_device, n, K, m):
    from latentsplat_amd import activate_scene_filtered
    from latentsplat_amd.scene_model import activate_backward, activate_forward
    p = sref.make_params(n, K, seed=1000 * K + n)
    up = sref.make_upstream(n, K, seed=n + K)
    filt = fref.make_filter(n, seed=7 * n + K)
    t = _dev(p, hip_device)
    f = torch.from_numpy(filt).to(hip_device)
    got = _np(activate_forward(*t, scale_modifier=m, filter_3d=f))
    assert set(got) == {"shs", "opacities", "cov3D", "scales", "rotations"}
    fref.assert_forward_matches(got, fref.expected(p, filt, m), show=f"n={n} K={K} m={m}")
    assert np.array_equal(got["shs"], np.concatenate([p["features_dc"], p["features_rest"]], 1))
    plain = _np(activate_forward(*t, scale_modifier=m))
    assert np.array_equal(got["rotations"], plain["rotations"]) and np.array_equal(got["shs"], plain["shs"])
    g = [torch.from_numpy(up[k]).to(hip_device) for k in UP]
    back = _np(activate_backward(*t, *g, scale_modifier=m, filter_3d=f))
    fref.assert_backward_matches(back, p, filt, up, m, show=f"n={n} K={K} m={m}")
    # the autograd op is the raw kernels, bit for bit, and the filter (n,) or (n, 1) is the same filter
    leaves = [x.clone().requires_grad_(True) for x in t]
    outs = activate_scene_filtered(*leaves, f[:, 0], scale_modifier=m)
    torch.autograd.backward(outs, g)
    for k, leaf in zip(sref.PARAMS, leaves):
        assert np.array_equal(leaf.grad.cpu().numpy(), back[k]), k
    for k, o in zip(UP, outs):
        assert np.array_equal(o.detach().cpu().numpy(), got[k]), k


def test_filtered_optional_pieces(hip_device):
    from latentsplat_amd import activate_scene_filtered
    from latentsplat_amd.scene_model import activate_backward, activate_forward
    n, K, m = 300, 9, 0.5
    p = sref.make_params(n, K, seed=21)
    up = sref.make_upstream(n, K, seed=22)
    filt = fref.make_filter(n, seed=23)
    t = _dev(p, hip_device)
    f = torch.from_numpy(filt).to(hip_device)
    g = {k: torch.from_numpy(v).to(hip_device) for k, v in up.items()}
    full = _np(activate_forward(*t, scale_modifier=m, filter_3d=f))
    for only in ("shs", "opacities", "cov3D", "scales", "rotations"):             # each output alone
        got = activate_forward(*t, scale_modifier=m, want=(only,), filter_3d=f)
        assert list(got) == [only] and np.array_equal(got[only].cpu().numpy(), full[only])
    all_back = _np(activate_backward(*t, g["shs"], g["opacities"], g["cov3D"], scale_modifier=m, filter_3d=f))
    for only in sref.PARAMS:                                                     # each gradient alone, in the kernel
        got = activate_backward(*t, g["shs"], g["opacities"], g["cov3D"], scale_modifier=m, want=(only,), filter_3d=f)
        assert list(got) == [only] and np.array_equal(got[only].cpu().numpy(), all_back[only])
    # each upstream gradient alone; the opacities now reach the scaling too (through the coefficient)
    reached = dict(shs=("features_dc", "features_rest"), opacities=("opacity", "scaling"), cov3D=("scaling", "rotation"))
    for i, name in enumerate(UP):
        leaves = [x.clone().requires_grad_(True) for x in t]
        outs = activate_scene_filtered(*leaves, f, scale_modifier=m)
        outs[i].backward(g[name])
        grads = {k: leaf.grad for k, leaf in zip(sref.PARAMS, leaves)}
        assert sorted(k for k, v in grads.items() if v is not None) == sorted(reached[name])
        fref.assert_backward_matches(_np({k: v for k, v in grads.items() if v is not None}), p, filt, {name: up[name]}, m)
        direct = _np(activate_backward(*t, *[g[k] if k == name else None for k in UP], scale_modifier=m, filter_3d=f))
        fref.assert_backward_matches(direct, p, filt, {name: up[name]}, m)
        for k in sref.PARAMS:
            if k in reached[name]:
                assert np.array_equal(grads[k].cpu().numpy(), direct[k]), k
            else:
                assert not direct[k].any(), k
    # a parameter that does not require grad gets none; the others are unchanged bit for bit; the filter never gets one
    for frozen in sref.PARAMS:
        leaves = [x.clone().requires_grad_(k != frozen) for k, x in zip(sref.PARAMS, t)]
        fl = f.clone().requires_grad_(True)
        torch.autograd.backward(activate_scene_filtered(*leaves, fl, scale_modifier=m), [g[k] for k in UP])
        assert fl.grad is None
        for k, leaf in zip(sref.PARAMS, leaves):
            assert (leaf.grad is None) if k == frozen else np.array_equal(leaf.grad.cpu().numpy(), all_back[k]), (frozen, k)
    # an empty scene
    empty = [x[:0] for x in t]
    assert activate_forward(*empty, filter_3d=f[:0])["shs"].shape == (0, K, 3)
    assert activate_backward(*empty, None, None, None, filter_3d=f[:0])["rotation"].shape == (0, 4)
    # a filter of another length is refused before any launch
    with pytest.raises(_lib.LsrError, match="stale"):
        activate_forward(*t, filter_3d=f[:-1])
    with pytest.raises(_lib.LsrError, match="stale"):
        activate_scene_filtered(*t, f[:-1])
    # a NaN filter entry is NaN for that Gaussian and for no other; a zero filter is the unfiltered map at its bars
    bad = f.clone()
    bad[7] = float("nan")
    out = _np(activate_forward(*t, scale_modifier=m, filter_3d=bad))
    assert np.isnan(out["cov3D"][7]).all() and np.isnan(out["opacities"][7]).all() and np.isnan(out["scales"][7]).all()
    keep = np.arange(n) != 7
    for k in full:
        assert np.array_equal(out[k][keep], full[k][keep]), k
    zero = _np(activate_forward(*t, scale_modifier=m, filter_3d=torch.zeros_like(f)))
    from tests import ply_import_ref as ref
    ref.assert_matches(zero, _np(activate_forward(*t, scale_modifier=m)))


def test_filtered_two_calls_give_identical_bits(hip_device):
    from latentsplat_amd.scene_model import activate_backward, activate_forward
    n, K = 5000, 16
    p = sref.make_params(n, K, seed=31)
    up = sref.make_upstream(n, K, seed=32)
    t = _dev(p, hip_device)
    f = torch.from_numpy(fref.make_filter(n, seed=33)).to(hip_device)
    g = [torch.from_numpy(up[k]).to(hip_device) for k in UP]
    a, b = (_np(activate_forward(*t, filter_3d=f)) for _ in range(2))
    c, d = (_np(activate_backward(*t, *g, filter_3d=f)) for _ in range(2))
    for x, y in ((a, b), (c, d)):
        for k in x:
            assert np.array_equal(x[k], y[k]), k


# ---- through the scene ----

@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("filter3d") / "point_cloud.ply"
    sc, table, names = sref.write_scene_file(path, G, W, VIEWS)
    return path, sc, table, names


def _views(sc, dev):
    from latentsplat_amd.rasterizer import build_view_table
    return build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                            torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False)


def _scene_and_filter(scene_file, dev):
    from latentsplat_amd import GaussianScene
    path, sc, table, names = scene_file
    scene = GaussianScene.from_ply(path, dev)
    views = _views(sc, dev)
    filt, seen = scene.compute_filter_3d(views, W, return_seen=True)
    assert filt.shape == (G, 1) and seen.sum() > G // 2 and (filt > 0).all()
    return scene, views, filt


def test_filtered_render_is_the_render_of_the_fused_scene(hip_device, scene_file):
    """scene.render(filter_3d=f) against a second scene built from fused_parameters, rendered through the EXISTING
    unfiltered path: the project's 1e-4 image bar, and equal radii (a covariance eigenvalue that lands on a ceil boundary
    could differ by one pixel: such Gaussians are counted, and this seeded input has none: on its first run 0 of the 4 000
    radii differed, 3 348 of them on screen, and the images agreed to 3e-7)."""
    from latentsplat_amd import GaussianScene, fused_parameters
    scene, views, filt = _scene_and_filter(scene_file, hip_device)
    # the filter matters here: it is of the size of the scales
    ratio = (filt / scene._scaling.detach().exp().amin(1, keepdim=True)).median()
    print(f"median filter / smallest scale {float(ratio):.3f}")
    assert 0.05 < float(ratio) < 50
    with torch.no_grad():
        color, _, mask, depth, radii = scene.render(views, H, W, filter_3d=filt)
        plain = scene.render(views, H, W)[0]
        opacity, scaling = fused_parameters(scene._opacity, scene._scaling, filt)
        fused = GaussianScene.from_tensors(scene._xyz, scene._features_dc, scene._features_rest, opacity, scaling, scene._rotation)
        color_f, _, mask_f, depth_f, radii_f = fused.render(views, H, W)
    assert (color - plain).abs().max() > 1e-2                                     # (not the unfiltered image)
    for a, b, what in ((color, color_f, "color"), (mask, mask_f, "mask"), (depth, depth_f, "depth")):
        err = float((a - b).abs().max())
        print(f"{what}: filtered render against the fused scene, worst difference {err:.3e} (bar 1e-4)")
        assert err <= 1e-4 * max(1.0, float(b.abs().max()) if what == "depth" else 1.0), what
    differing = int((radii != radii_f).sum())
    print(f"radii that differ: {differing} of {radii.numel()} ({int((radii > 0).sum())} on screen)")
    assert differing == 0 and (radii > 0).sum() > G // 2


def test_filtered_render_gradients_are_the_kernels_backward_of_what_the_rasterizer_sends_down(hip_device, scene_file, monkeypatch):
    import latentsplat_amd.rasterizer as rasterizer
    from latentsplat_amd.scene_model import activate_backward
    path, sc, table, names = scene_file
    scene, views, filt = _scene_and_filter(scene_file, hip_device)
    cot = torch.randn((VIEWS, 3, H, W), generator=torch.Generator().manual_seed(9)).to(hip_device)
    fed = {}
    real = rasterizer.rasterize_views

    def recording(views_, h, w, degree, means3D, cov3D, opacities, shs=None, **kw):
        for t in (cov3D, opacities, shs):
            t.retain_grad()
        fed.update(degree=degree, means=means3D, cov3D=cov3D, opacities=opacities, shs=shs)
        return real(views_, h, w, degree, means3D, cov3D, opacities, shs=shs, **kw)

    monkeypatch.setattr(rasterizer, "rasterize_views", recording)
    color = scene.render(views, H, W, filter_3d=filt)[0]
    (color * cot).sum().backward()
    assert fed["means"] is scene._xyz
    up = {k: fed[k].grad for k in UP}
    assert all(v is not None and v.abs().max() > 0 for v in up.values())
    got = {k: getattr(scene, "_" + k).grad.cpu().numpy() for k in sref.PARAMS}
    fref.assert_backward_matches(got, sref.split_table(table, names), filt.cpu().numpy(), _np(up), 1.0, show="filtered render gradients")
    params = [scene._features_dc, scene._features_rest, scene._opacity, scene._scaling, scene._rotation]
    kernel = _np(activate_backward(*params, up["shs"], up["opacities"], up["cov3D"], filter_3d=filt))
    for k in sref.PARAMS:
        assert np.array_equal(got[k], kernel[k]), k
    # the activated scene the rasterizer was fed is the filtered kernel's, at its bars
    want = fref.expected(sref.split_table(table, names), filt.cpu().numpy())
    fref.assert_forward_matches(_np({k: fed[k] for k in UP}), want, show="fed")


def test_fused_file_round_trip_and_the_unfiltered_path(hip_device, scene_file, tmp_path):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.scene_model import activate_forward
    path, sc, table, names = scene_file
    scene, views, filt = _scene_and_filter(scene_file, hip_device)
    p = sref.split_table(table, names)
    scene.save_ply(tmp_path / "fused.ply", filter_3d=filt)
    back = GaussianScene.from_ply(tmp_path / "fused.ply", hip_device)
    act = back.activated()
    got = dict(shs=act.shs, opacities=act.opacities, cov3D=act.covariances, scales=act.scales, rotations=act.rotations)
    fref.assert_forward_matches(_np(got), fref.expected(p, filt.cpu().numpy()), show="fused file")
    for k in ("xyz", "features_dc", "features_rest", "rotation"):               # the other columns go out as they are
        assert np.array_equal(getattr(back, "_" + k).detach().cpu().numpy(), p[k]), k
    # filter_3d=None is today's path, bit for bit: the raw file, the activation, the render
    scene.save_ply(tmp_path / "raw.ply", filter_3d=None)
    assert np.array_equal(GaussianScene.from_ply(tmp_path / "raw.ply", hip_device).rows().cpu().numpy(), table)
    params = [scene._features_dc, scene._features_rest, scene._opacity, scene._scaling, scene._rotation]
    direct = _np(activate_forward(*params))
    act = scene.activated(filter_3d=None)
    for k, v in dict(shs=act.shs, opacities=act.opacities, cov3D=act.covariances, scales=act.scales, rotations=act.rotations).items():
        assert np.array_equal(v.detach().cpu().numpy(), direct[k]), k
    with torch.no_grad():
        a, b = scene.render(views, H, W, filter_3d=None), scene.render(views, H, W)
    for x, y in zip(a, b):                                    # (no feature image here: None on both sides)
        assert (x is None and y is None) or torch.equal(x, y)
    assert [k for k, _ in scene.named_parameters()] == ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    # a filter of the scene before a pruning is refused
    keep = torch.arange(G, device=hip_device) % 3 != 0
    scene.replace_parameters_(**{k[1:]: v.detach()[keep] for k, v in scene.named_parameters()})
    with pytest.raises(_lib.LsrError, match="stale"):
        scene.render(views, H, W, filter_3d=filt)
    assert scene.render(views, H, W, filter_3d=scene.compute_filter_3d(views, W))[0].shape == (VIEWS, 3, H, W)


def test_fit_tool_with_the_3d_filter(hip_device, scene_file, tmp_path):
    from latentsplat_amd import GaussianScene
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    out = tmp_path / "fit"
    res = fit_ply.main([str(scene_file[0]), "--out", str(out), "--views", "3", "--size", "48", "--steps", "30", "--drop", "0.5",
                        "--filter-3d", "--filter-3d-interval", "15", "--densify-interval", "10"])
    print("fit:", {k: v for k, v in res.items() if k not in ("densify_events", "filter_3d_events")})
    assert json.load(open(out / "fit.json")) == res
    assert res["filter_3d"] is True and res["filter_3d_interval"] == 15 and res["fused_ply"] == "point_cloud_fused.ply"
    events, densify = res["filter_3d_events"], res["densify_events"]
    print("filter events:", events)
    assert [e["step"] for e in densify] == [10, 20, 30]
    # before the first step, after every densification (with the new row count), and every 15 steps
    assert [(e["step"], e["reason"]) for e in events] == [(0, "start"), (10, "densify"), (15, "interval"), (20, "densify"),
                                                          (30, "densify")]
    assert events[0]["gaussians"] == res["gaussians_first"]
    for e, d in zip([e for e in events if e["reason"] == "densify"], densify):
        assert e["gaussians"] == d["n_out"]
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
    raw = GaussianScene.from_ply(out / "point_cloud.ply", hip_device)
    fused = GaussianScene.from_ply(out / "point_cloud_fused.ply", hip_device)
    assert raw.num_gaussians == fused.num_gaussians == res["gaussians_last"]
    assert all(torch.isfinite(q).all() for q in fused.parameters())
    assert torch.equal(raw._xyz, fused._xyz) and torch.equal(raw._rotation, fused._rotation)
    # sqrt(s^2 + f^2) >= s and o c <= o, up to the rounding of one float32 exp / log round trip of values below 20
    assert (fused._scaling >= raw._scaling - 1e-5).all() and (fused._scaling > raw._scaling + 1e-3).any()
    assert (fused._opacity <= raw._opacity + 1e-5).all()
