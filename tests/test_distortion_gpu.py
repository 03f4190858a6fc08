"""The depth distortion regulariser on the MI355X: lsr_scene_depth_moments_* and lsr_distortion_loss_* against the float64
restatement (tests/distortion_ref.py) under the project's error rule (at most 4 x the stock float32 composition's own error,
per quantity), bit-reproducibility, written-not-accumulated outputs, batch independence, graph capture, the operators
through GaussianScene.render_with_distortion / render_surface against the float64 chain, the pivot measured, and the tools."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import distortion_ref as dref

pytestmark = pytest.mark.gpu

# one lane per Gaussian in at most LSR_DIST_MAX_BLOCKS workgroups of LSR_DIST_THREADS: from here on a lane owns a second one
PAST_ONE_TRIP = _lib.DIST_THREADS * _lib.DIST_MAX_BLOCKS + 65
# k_dist_cameras is ONE workgroup of LSR_DIST_THREADS = 256 lanes: from camera 256 on a lane compacts a second record
MANY_VIEWS = 2 * _lib.DIST_THREADS + 3
B_SHAPES = [(1, 1, 1), (1, 3, 5), (3, 31, 33), (2, 32, 32), (2, 65, 70)]
H, W = 48, 40
GRAD_TOL = 1e-3     # max |got - want| <= GRAD_TOL ||want||_2 per tensor: the bar of the parity tests against the oracle


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- A ----

def _run_A(case, upstream, dev):
    """(moments, grad_xyz) of the HIP operator, the gradient buffer pre-filled with NaN (written, never accumulated)."""
    from latentsplat_amd.distortion import depth_moments_backward, depth_moments_forward
    views, xyz, pivot = _t(case["views"], dev), _t(case["xyz"], dev), _t(case["pivot"], dev)
    out = depth_moments_forward(views, xyz, case["space"], pivot)
    grad = torch.full((xyz.shape[0], 3), float("nan"), device=dev)
    depth_moments_backward(views, xyz, _t(upstream, dev), case["space"], pivot, out=grad)
    return out, grad


def _check_A(case, dev, show):
    V, n = case["views"].shape[0], case["xyz"].shape[0]
    up = np.random.default_rng(n + V).standard_normal((V, n, 2)).astype(np.float32)
    out, grad = _run_A(case, up, dev)
    assert out.shape == (V, n, 2) and grad.shape == (n, 3)
    want, stock = dref.moments_and_grad(case, up, torch.float64), dref.moments_and_grad(case, up, torch.float32)
    dref.held("moments", out.cpu().numpy(), want["moments"], stock["moments"], show)
    dref.held("grad_xyz", grad.cpu().numpy(), want["grad_xyz"], stock["grad_xyz"], show)
    assert np.abs(want["moments"]).min() > 0 and np.abs(want["grad_xyz"]).max() > 0
    again, grad_again = _run_A(case, up, dev)
    assert np.array_equal(_bits(out), _bits(again)) and np.array_equal(_bits(grad), _bits(grad_again))
    return out, grad


@pytest.mark.parametrize("space", dref.SPACES)
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_depth_moments_against_float64(hip_device, n, V, space):
    """A non-zero pivot and a scene scale != 1 in slot 40 in every case."""
    scale = (0.5, 1.0, 2.5)[:V]
    _check_A(dref.scene_case(n, V, seed=10 * n + V, scale40=scale, space=space), hip_device, f"n={n} V={V} {space}")


@pytest.mark.parametrize("space", dref.SPACES)
def test_depth_moments_without_a_pivot(hip_device, space):
    case = dref.scene_case(130, 2, seed=3, with_pivot=False, space=space)
    out, _ = _check_A(case, hip_device, f"no pivot {space}")
    piv = dref.scene_case(130, 2, seed=3, space=space)
    zero = dict(piv, pivot=np.zeros(2, np.float32))
    assert np.array_equal(_bits(out), _bits(_run_A(zero, np.zeros((2, 130, 2), np.float32), hip_device)[0]))      # NULL is 0


def test_depth_moments_past_one_grid_stride_trip(hip_device):
    """The lanes 0..64 of the first workgroup take a second Gaussian; every row against float64."""
    assert PAST_ONE_TRIP > _lib.DIST_THREADS * _lib.DIST_MAX_BLOCKS
    _check_A(dref.scene_case(PAST_ONE_TRIP, 1, seed=5, scale40=0.5, space="ndc"), hip_device, f"n={PAST_ONE_TRIP}")


def test_depth_moments_with_more_cameras_than_compaction_lanes(hip_device):
    """V = 2 x 256 + 3: a compaction lane takes a second record and three lanes a third.  The cameras repeat 7 distinct ones
    cyclically (7 is coprime to 256: record v and record v - 256 are different cameras), each with its own pivot."""
    n, B = 65, 7
    base = dref.scene_case(n, B, seed=9, scale40=tuple(np.linspace(0.5, 2.0, B)), space="ndc")
    idx = np.arange(MANY_VIEWS) % B
    case = dict(base, views=np.ascontiguousarray(base["views"][idx]), pivot=np.ascontiguousarray(base["pivot"][idx]))
    assert not np.array_equal(case["views"][256], case["views"][0])
    out, grad = _check_A(case, hip_device, f"V={MANY_VIEWS} cyclic over {B}")
    assert np.array_equal(_bits(out), _bits(out[:B][torch.from_numpy(idx).to(hip_device)]))      # one camera, one answer
    assert float(grad.abs().max()) > 0


def test_rows_that_are_not_finite_or_behind_the_camera_give_zero(hip_device):
    from latentsplat_amd import gaussian_depth_moments
    for space in dref.SPACES:
        case = dref.scene_case(130, 2, seed=4, space=space)
        views, pivot = _t(case["views"], hip_device), _t(case["pivot"], hip_device)
        clean = gaussian_depth_moments(views, _t(case["xyz"], hip_device), space, pivot)
        case["xyz"][3, 2] = np.nan
        case["xyz"][64, 0] = np.inf
        case["xyz"][65, 1] = -np.inf
        behind = -2.0 * case["views"][0, 32:35] / case["views"][0, 40]        # twice as far out as camera 0, on its side
        case["xyz"][129] = -behind
        xyz = _t(case["xyz"], hip_device).requires_grad_(True)
        out = gaussian_depth_moments(views, xyz, space, pivot)
        bad = torch.zeros(130, dtype=torch.bool, device=hip_device)
        bad[[3, 64, 65]] = True
        assert not out[:, bad].any() and not out[0, 129].any() and bool(out[1, 129].all())
        good = ~bad
        good[129] = False
        assert np.array_equal(_bits(out[:, good]), _bits(clean[:, good]))
        out.sum().backward()
        assert bool(torch.isfinite(xyz.grad).all()) and not xyz.grad[bad].any() and bool(xyz.grad[good].any(-1).all())
        # row 129 has its gradient from view 1 alone
        only1 = torch.autograd.grad(gaussian_depth_moments(views[1:], xyz, space, pivot[1:]).sum(), xyz)[0]
        assert np.array_equal(_bits(xyz.grad[129]), _bits(only1[129]))


def test_only_the_positions_receive_a_gradient(hip_device):
    from latentsplat_amd import gaussian_depth_moments
    case = dref.scene_case(65, 2, seed=6)
    views, xyz, pivot = _t(case["views"], hip_device), _t(case["xyz"], hip_device).requires_grad_(True), _t(case["pivot"], hip_device)
    gaussian_depth_moments(views, xyz, "ndc", pivot).square().sum().backward()
    assert xyz.grad is not None and views.grad is None and pivot.grad is None
    with pytest.raises(_lib.LsrError, match="views requires grad"):
        gaussian_depth_moments(views.clone().requires_grad_(True), xyz, "ndc", pivot)
    with pytest.raises(_lib.LsrError, match="pivot requires grad"):
        gaussian_depth_moments(views, xyz, "ndc", pivot.clone().requires_grad_(True))
    native = views.clone()
    native[:, 42:44] = 0.0
    with pytest.raises(_lib.LsrError, match="near < far"):
        gaussian_depth_moments(native, xyz, "ndc", pivot)


# ---- B ----

@functools.lru_cache(maxsize=None)
def _image_refs(V, H, W, weighted):
    case = dref.image_case(V, H, W, seed=H + W + V, weighted=weighted)
    return case, dref.distortion_and_grads(case, torch.float64), dref.distortion_and_grads(case, torch.float32)


def _run_B(case, dev, want=("loss", "per_view", "distortion"), grads=("moment_map", "alpha"), views=slice(None)):
    from latentsplat_amd.distortion import distortion_loss_backward, distortion_loss_forward
    mm, alpha, weight = (_t(None if case[k] is None else case[k][views], dev) for k in ("moment_map", "alpha", "weight"))
    out = distortion_loss_forward(mm, alpha, weight, want=want)
    like = dict(moment_map=mm, alpha=alpha)
    buf = {k: torch.full_like(like[k], float("nan")) for k in grads}           # written, never accumulated
    g = distortion_loss_backward(mm, alpha, torch.tensor([dref.GRAD_LOSS], device=dev), weight, want=grads, out=buf)
    out.update({"grad_" + k: v for k, v in g.items()})
    return out


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("V,H,W", B_SHAPES)
def test_distortion_loss_against_float64(hip_device, V, H, W, weighted):
    case, want, stock = _image_refs(V, H, W, weighted)
    show = f"{V}x{H}x{W} weighted={weighted}"
    got = _run_B(case, hip_device)
    for k in ("loss", "per_view", "distortion", "grad_moment_map", "grad_alpha"):
        dref.held(k, got[k].cpu().numpy(), want[k], stock[k], show)
    if weighted and H * W > 100:
        assert (case["weight"] == 0).any() and not got["grad_alpha"][_t(case["weight"], hip_device) == 0].any()
    again = _run_B(case, hip_device)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (show, k)          # two calls, the same bits
    for k in range(V):                                                            # a view alone: the bits it has in the batch
        alone = _run_B(case, hip_device, want=("per_view",), grads=(), views=slice(k, k + 1))
        assert np.array_equal(_bits(alone["per_view"]), _bits(got["per_view"][k:k + 1])), (show, k)


def test_every_optional_output_in_turn(hip_device):
    case, _, _ = _image_refs(2, 65, 70, True)
    full = _run_B(case, hip_device)
    names, grads = ("loss", "per_view", "distortion"), ("moment_map", "alpha")
    for skip in names:
        got = _run_B(case, hip_device, want=tuple(k for k in names if k != skip))
        for k in names:
            assert (k not in got) if k == skip else np.array_equal(_bits(got[k]), _bits(full[k])), (skip, k)
    for skip in grads:
        got = _run_B(case, hip_device, grads=tuple(k for k in grads if k != skip))
        for k in grads:
            assert ("grad_" + k not in got) if k == skip else np.array_equal(_bits(got["grad_" + k]), _bits(full["grad_" + k])), (skip, k)
    only = _run_B(case, hip_device, want=("distortion",), grads=())
    assert np.array_equal(_bits(only["distortion"]), _bits(full["distortion"]))


def test_loss_function_and_distortion_map(hip_device):
    from latentsplat_amd import distortion_loss, distortion_map
    case, want, stock = _image_refs(3, 31, 33, True)
    mm, alpha = (_t(case[k], hip_device).requires_grad_(True) for k in ("moment_map", "alpha"))
    loss = distortion_loss(mm, alpha, _t(case["weight"], hip_device))
    assert loss.shape == ()
    (loss * dref.GRAD_LOSS).backward()
    dref.held("loss", loss.detach().cpu().numpy(), want["loss"], stock["loss"], "autograd")
    dref.held("grad_moment_map", mm.grad.cpu().numpy(), want["grad_moment_map"], stock["grad_moment_map"], "autograd")
    dref.held("grad_alpha", alpha.grad.cpu().numpy(), want["grad_alpha"], stock["grad_alpha"], "autograd")
    dref.held("distortion", distortion_map(mm.detach(), alpha.detach()).cpu().numpy(), want["distortion"], stock["distortion"], "map")


# ---- through the scene ----

@functools.lru_cache(maxsize=None)
def _layered():
    """About 200 Gaussians (sh_degree 1) over depths 2 to 6 in front of 2 views: D is of order one, no test of cancellation."""
    return dref.layered_params(200, 7, 2.0, 6.0), dref.forward_views(2)


def test_render_with_distortion_is_render_with_the_moments_as_features(hip_device):
    from latentsplat_amd import depth_pivot, gaussian_depth_moments
    dev = hip_device
    p, views = _layered()
    scene, tv = dref.scene_of(p, dev), _t(views, dev)
    for space in dref.SPACES:
        pivot = depth_pivot(tv, (0.0, 0.0, 4.0), space)
        with torch.no_grad():
            color, mm, mask, depth, radii = scene.render_with_distortion(tv, H, W, space=space, pivot=pivot)
            moments = gaussian_depth_moments(tv, scene._xyz, space, pivot)
            c2, f2, m2, d2, r2 = scene.render(tv, H, W, features=moments)
            for a, b in ((color, c2), (mm, f2), (mask, m2), (depth, d2)):
                assert np.array_equal(_bits(a), _bits(b))
            assert mm.shape == (2, 2, H, W) and torch.equal(radii, r2) and float(mask.max()) > 0.5
            # the 8-channel path against the 5- and 6-channel ones
            cs, ns, ms, ks, ds, rs = scene.render_surface(tv, H, W, space=space, pivot=pivot)
            _, nmap, _, _, _ = scene.render_with_normals(tv, H, W)
            assert ns.shape == (2, 3, H, W) and ms.shape == (2, 2, H, W)
            for a, b in ((cs, color), (ms, mm), (ks, mask), (ds, depth), (ns, nmap)):
                assert np.array_equal(_bits(a), _bits(b))
            assert torch.equal(rs, radii)


def test_linear_moments_are_the_rasterizers_depth(hip_device):
    """space="linear", pivot 0, slot 40 = 1, a NATIVE table: channel 0 of the moment map is the depth image of the same call,
    which pins z to the projection kernels' own.  The stock error is that of the rasterizer's own depth against float64."""
    dev = hip_device
    p, views = _layered()
    assert (views[:, 40] == 1).all() and (views[:, 41] == 0).all()
    scene, tv = dref.scene_of(p, dev), _t(views, dev)
    with torch.no_grad():
        _, mm, _, depth, _ = scene.render_with_distortion(tv, H, W, space="linear")
    _, _, want, _ = dref.float64_chain(p, views, H, W, "linear", grads=False)
    dref.held("M1 vs depth", mm[:, 0].cpu().numpy(), want[:, 0], depth.reshape(2, H, W).cpu().numpy().astype(np.float64), "linear")
    assert float(depth.max()) > 1.0


@pytest.mark.parametrize("space,surface", [("ndc", False), ("linear", True), ("disparity", False)])
def test_scene_gradients_against_the_float64_chain(hip_device, space, surface):
    from latentsplat_amd import depth_pivot, distortion_loss
    dev = hip_device
    p, views = _layered()
    scene, tv = dref.scene_of(p, dev), _t(views, dev)
    pivot = depth_pivot(tv, (0.0, 0.0, 4.0), space)
    weight = np.random.default_rng(1).uniform(0.0, 1.0, (2, H, W)).astype(np.float32)
    if surface:
        _, _, mm, mask, _, _ = scene.render_surface(tv, H, W, space=space, pivot=pivot)
    else:
        _, mm, mask, _, _ = scene.render_with_distortion(tv, H, W, space=space, pivot=pivot)
    loss = distortion_loss(mm, mask, _t(weight, dev))
    got = torch.autograd.grad(loss, [scene._xyz, scene._scaling, scene._rotation, scene._opacity])
    want_loss, _, _, want = dref.float64_chain(p, views, H, W, space, pivot.cpu().numpy(), weight)
    print(f"{space}: loss {float(loss.detach()):.7e} against {want_loss:.7e}")
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * abs(want_loss) and want_loss > 0
    for name, g in zip(("xyz", "scaling", "rotation", "opacity"), got):
        err, norm = float(np.abs(g.cpu().numpy().astype(np.float64) - want[name]).max()), float(np.linalg.norm(want[name]))
        print(f"  {name:9s} max error {err:.3e}  norm {norm:.3e}  ratio {err / norm:.2e}")
        assert norm > 0 and err <= GRAD_TOL * norm, name


def test_the_posed_path_renders_the_transformed_scene(hip_device):
    from latentsplat_amd import GaussianScene, similarity_matrix
    dev = hip_device
    p, views = _layered()
    scene, tv = dref.scene_of(p, dev), _t(views, dev)
    M = similarity_matrix(torch.tensor([0.99, 0.05, -0.08, 0.03]), torch.tensor([0.1, -0.2, 0.3]), 1.1).to(dev)
    with torch.no_grad():
        posed = scene.render_with_distortion(tv, H, W, transforms=M)
        plain = scene.render_with_distortion(tv, H, W)
        moved = GaussianScene.from_tensors(**{k[1:]: v.detach().clone() for k, v in scene.named_parameters()}).to(dev).transform_(M)
        direct = moved.render_with_distortion(tv, H, W)
    for a, b in zip(posed[:4], direct[:4]):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    assert float((posed[1] - plain[1]).abs().max()) > 1e-2                    # the moments moved with the scene


def test_means2d_abs_meets_the_payload_limit(hip_device):
    dev = hip_device
    p, views = _layered()
    scene, tv = dref.scene_of(p, dev), _t(views[:1], dev)
    for render in (scene.render_with_distortion, scene.render_surface):
        m2d_abs = torch.zeros(1, scene.num_gaussians, 3, device=dev, requires_grad=True)
        with pytest.raises(_lib.LsrError, match="payload channels"):
            render(tv, 32, 32, means2D_abs=m2d_abs)


def test_graph_capture_replays_the_eager_bits(hip_device):
    """Operator A, the render and operator B (both ways) captured in one torch.cuda.graph and replayed on new positions."""
    from latentsplat_amd.distortion import (depth_moments_backward, depth_moments_forward, distortion_loss_backward,
                                            distortion_loss_forward)
    from latentsplat_amd.rasterizer import last_forward_status, rasterize_views
    dev = hip_device
    p, views = _layered()
    scene, tv = dref.scene_of(p, dev), _t(views, dev)
    pivot = _t(dref.pivot_of(views, (0.0, 0.0, 4.0), "ndc"), dev)
    one = torch.ones(1, device=dev)
    with torch.no_grad():
        shs, opac, cov, _, _ = scene._activate(1.0, False)
        xyz = scene._xyz.detach().clone()
        rasterize_views(tv, H, W, 1, xyz, cov, opac, shs=shs, features=depth_moments_forward(tv, xyz, "ndc", pivot))
        kw = dict(pair_capacity=2 * last_forward_status()["num_pairs"] + 64, max_tile_hint=2048)

        def step():
            moments = depth_moments_forward(tv, xyz, "ndc", pivot, check=False)       # (no host read inside a capture)
            _, mm, mask, _, _ = rasterize_views(tv, H, W, 1, xyz, cov, opac, shs=shs, features=moments, **kw)
            out = distortion_loss_forward(mm, mask, None, want=("loss", "distortion"))
            g = distortion_loss_backward(mm, mask, one)
            gx = depth_moments_backward(tv, xyz, moments, "ndc", pivot)
            return moments, mm, mask, out["loss"], out["distortion"], g["moment_map"], g["alpha"], gx

        side = torch.cuda.Stream(dev)                # warm-up on a side stream, as torch.cuda.graph asks for
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        xyz.add_(torch.tensor([0.02, -0.01, 0.05], device=dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert not last_forward_status()["overflow"]
        replayed = [t.clone() for t in captured]
        eager = step()
    for a, b in zip(replayed, eager):
        assert np.array_equal(_bits(a), _bits(b))
    assert float(replayed[3]) > 0.0


# ---- the pivot ----

def test_the_pivot_takes_the_cancellation_out(hip_device):
    """Gaussians within +-0.01 of a plane at distance 4, space="linear", one view of 32 x 32: the distortion map of the float32
    pipeline against the float64 chain, with pivot 0 and with depth_pivot at the plane.  The pivoted error is strictly
    smaller; the figures are printed (tools/bench_distortion.py records them; DESIGN.md 2.28 says what to expect: with pivot 0
    the blended M2 is about 16 A and carries float32 roundings of about 16 x 6e-8 per blended entry, against a D of at most
    (0.02)^2 / 4 = 1e-4; pivoted, M2 is at most 1e-4 A and its roundings are below 1e-11: a ratio of about (4 / 0.01)^2 =
    1.6e5).  Seen on an MI355X: 6.40e-6 with pivot 0, 2.47e-11 pivoted, ratio 2.6e5, largest D 5.65e-5."""
    res = dref.pivot_errors(hip_device)
    print(f"pivot 0: {res['err_pivot_0']:.3e}   pivoted: {res['err_pivoted']:.3e}   ratio {res['ratio']:.3g}   "
          f"max D {res['max_distortion']:.3e}")
    assert res["max_distortion"] > 0 and res["err_pivoted"] < res["err_pivot_0"]


# ---- tools ----

def _tool(name):
    from tests import util
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_the_fitting_and_rendering_tools(hip_device, tmp_path):
    from latentsplat_amd import distortion_map
    from tests import scene_params_ref as sref
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, 2000, 64, 2)
    fit = _tool("fit_ply")
    argv = [str(path), "--views", "2", "--size", "48", "--steps", "20", "--noise", "0.2"]
    res = fit.main(argv + ["--out", str(tmp_path / "fit"), "--dist-reg", "1", "--normal-reg", "0.05", "--normal-alpha-min", "0.3"])
    assert json.load(open(tmp_path / "fit" / "fit.json")) == res
    assert res["dist_reg"] == 1.0 and res["dist_reg_from"] == 0 and res["dist_space"] == "ndc" and res["normal_reg"] == 0.05
    assert np.isfinite(res["loss_last"]) and np.isfinite(res["dist_loss_first"]) and np.isfinite(res["dist_loss_last"])
    assert np.isfinite(res["normal_loss_last"]) and res["dist_loss_first"] > 0
    alone = fit.main(argv + ["--out", str(tmp_path / "alone"), "--dist-reg", "0.5", "--dist-reg-from", "3", "--dist-space", "linear"])
    assert alone["dist_space"] == "linear" and np.isfinite(alone["dist_loss_last"]) and "normal_reg" not in alone
    plain = fit.main(argv + ["--out", str(tmp_path / "plain")])
    assert not any(k.startswith("dist_") for k in plain)
    with pytest.raises(SystemExit, match="absgrad"):
        fit.main(argv + ["--out", str(tmp_path / "refused"), "--dist-reg", "1", "--absgrad", "--densify-interval", "2"])
    out = tmp_path / "distortion.npy"
    render = _tool("render_ply")
    render.main([str(path), "--out", str(tmp_path / "renders"), "--views", "2", "--size", "48", "--distortion", str(out)])
    got = np.load(out)
    assert got.shape == (2, 48, 48) and got.dtype == np.float32 and np.isfinite(got).all() and got.max() > 0
    for k in range(2):
        assert got[k].shape == (48, 48)
    # ... equal to distortion_map of the same render: the tool's cameras, the moments about the centre as the payload
    from latentsplat_amd.distortion import depth_pivot, gaussian_depth_moments, with_near_far
    from latentsplat_amd.ply_import import load_ply
    from latentsplat_amd.rasterizer import build_view_table, rasterize_views
    with torch.no_grad():
        s = load_ply(str(path), hip_device)
        centre, extent = render.scene_extent(s.means)
        ext, intr, near, far = render.circle_cameras(centre, extent, 2, 2.5)
        views = build_view_table(ext, intr, near, far, torch.zeros(3, device=hip_device))
        dv = with_near_far(views, near, far)
        moments = gaussian_depth_moments(dv, s.means, "ndc", depth_pivot(dv, centre, "ndc"))
        _, mm, mask, _, _ = rasterize_views(views, 48, 48, s.sh_degree, s.means, s.covariances, s.opacities, shs=s.shs, features=moments)
    assert np.array_equal(got.view(np.uint32), _bits(distortion_map(mm, mask)))


def test_train_colmap_with_both_regularisers(hip_device, tmp_path):
    """A few steps on a capture written the way tests/test_capture_gpu.py writes its fixture: six circle cameras around a
    seeded scene, a PINHOLE model with photographs."""
    import math

    from latentsplat_amd import GaussianScene
    from latentsplat_amd.capture import cameras_extent
    from latentsplat_amd.rasterizer import build_view_table
    from tests import colmap_ref as cr
    dev = hip_device
    N, VIEWS, W0, H0, RADIUS = 2000, 6, 48, 40, 4.0
    rng = np.random.default_rng(11)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    scene = GaussianScene.from_tensors(xyz=f(rng.uniform(-1.0, 1.0, (N, 3))), features_dc=f(rng.uniform(-1.5, 1.5, (N, 1, 3))),
                                       features_rest=torch.zeros((N, 0, 3)), opacity=f(rng.uniform(-3.5, -1.8, (N, 1))),
                                       scaling=f(np.log(rng.uniform(0.6, 0.9, (N, 3)))), rotation=f(rng.standard_normal((N, 4)))).to(dev)
    c2w = np.zeros((VIEWS, 4, 4))
    for k in range(VIEWS):
        ang = 2 * math.pi * k / VIEWS + 0.1
        offset = np.array([math.cos(ang), 0.15 * math.sin(3 * ang), math.sin(ang)])
        forward = -offset / np.linalg.norm(offset)
        right = np.cross([0.0, 1.0, 0.0], forward)
        right /= np.linalg.norm(right)
        c2w[k, :3, 0], c2w[k, :3, 1], c2w[k, :3, 2], c2w[k, :3, 3] = right, np.cross(forward, right), forward, RADIUS * offset
        c2w[k, 3, 3] = 1.0
    _, extent = cameras_extent(c2w[:, :3, 3])
    FX, FY = 0.8 * W0, 0.8 * H0
    intr = torch.tensor([[FX / W0, 0, 0.5], [0, FY / H0, 0.5], [0, 0, 1.0]], device=dev).repeat(VIEWS, 1, 1)
    near, far = torch.full((VIEWS,), 0.01 * extent, device=dev), torch.full((VIEWS,), 100.0 * extent, device=dev)
    with torch.no_grad():
        table = build_view_table(torch.from_numpy(c2w.astype(np.float32)).to(dev), intr, near, far, torch.zeros(3, device=dev))
        render = scene.render(table, H0, W0)[0].clamp(0.0, 1.0)
    u8 = torch.round(render * 255.0).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    camera = dict(id=5, model=1, width=W0, height=H0, params=[FX, FY, W0 / 2.0, H0 / 2.0])
    xyz = scene._xyz.detach().cpu().numpy()
    rgb = np.clip(np.rint((0.5 + 0.28209479177387814 * scene._features_dc.detach().cpu().numpy()[:, 0]) * 255), 0, 255).astype(np.uint8)
    cr.write_capture(tmp_path / "bin", c2w, [camera], [5] * VIEWS, [np.ascontiguousarray(u8[k]) for k in range(VIEWS)],
                     [f"view_{k}.npy" for k in range(VIEWS)], xyz, rgb, fmt="bin")
    train = _tool("train_colmap")
    argv = [str(tmp_path / "bin"), "--steps", "6", "--hold", "3", "--batch", "2", "--seed", "1", "--densify-interval", "0"]
    res = train.main(argv + ["--out", str(tmp_path / "fit"), "--dist-reg", "1", "--normal-reg", "0.05", "--reg-from", "2",
                             "--normal-alpha-min", "0.3"])
    assert json.load(open(tmp_path / "fit" / "metrics.json")) == res
    assert res["dist_reg"] == 1.0 and res["normal_reg"] == 0.05 and res["reg_from"] == 2 and res["dist_space"] == "ndc"
    for k in ("loss_last", "dist_loss_first", "dist_loss_last", "normal_loss_first", "normal_loss_last"):
        assert np.isfinite(res[k]), k
    assert res["dist_loss_first"] > 0
    alone = train.main(argv + ["--out", str(tmp_path / "alone"), "--dist-reg", "1", "--dist-space", "disparity"])
    assert np.isfinite(alone["dist_loss_last"]) and "normal_loss_last" not in alone
    plain = train.main(argv + ["--out", str(tmp_path / "plain")])
    assert not any(k.startswith(("dist_", "normal_", "reg_")) for k in plain)


def test_worst_ratios(hip_device):
    """Last in the file: what the rule saw, for the README row."""
    print("WORST", json.dumps({k: round(v, 3) for k, v in sorted(dref.WORST.items())}))
    assert all(v <= dref.MARGIN for v in dref.WORST.values()), dref.WORST
