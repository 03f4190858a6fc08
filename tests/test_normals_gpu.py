"""The depth-normal consistency regulariser on the MI355X: lsr_scene_normals_* and lsr_normal_consistency_* against the
float64 restatement (tests/normals_ref.py) under its error rule (at most 4 x the stock float32 composition's own error,
per quantity), bit-reproducibility, written-not-accumulated outputs, graph capture, and the operators through
GaussianScene.render_with_normals."""
import functools

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import normals_ref as nref
from tests import scene_params_ref as sref

pytestmark = pytest.mark.gpu


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def _dev(case: dict, dev, keys):
    return [torch.from_numpy(case[k]).to(dev) for k in keys]


A_KEYS = ("views", "xyz", "scaling", "rotation")


def _run_A(case: dict, upstream: np.ndarray, dev):
    """(normals, grad_rotation) of the HIP operator, the gradient buffer pre-filled with NaN (written, never accumulated)."""
    from latentsplat_amd.normals import normals_backward, normals_forward
    views, xyz, scaling, rotation = _dev(case, dev, A_KEYS)
    out = normals_forward(views, xyz, scaling, rotation)
    grad = torch.full((xyz.shape[0], 4), float("nan"), device=dev)
    normals_backward(views, xyz, scaling, rotation, torch.from_numpy(upstream).to(dev), out=grad)
    return out, grad


def _check_A(case: dict, dev, show: str):
    nref.check_scene_case(case)
    V, n = case["views"].shape[0], case["xyz"].shape[0]
    up = np.random.default_rng(n + V).standard_normal((V, n, 3)).astype(np.float32)
    want, stock = nref.normals_and_grad(case, up, torch.float64), nref.normals_and_grad(case, up, torch.float32)
    out, grad = _run_A(case, up, dev)
    assert out.shape == (V, n, 3) and grad.shape == (n, 4)
    nref.held("normals", out.cpu().numpy(), want["normals"], stock["normals"], show)
    nref.held("grad_rotation", grad.cpu().numpy(), want["grad_rotation"], stock["grad_rotation"], show)
    again, grad_again = _run_A(case, up, dev)
    assert np.array_equal(_bits(out), _bits(again)) and np.array_equal(_bits(grad), _bits(grad_again))
    return out, grad


@pytest.mark.parametrize("V", [1, 3, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_scene_normals_against_float64(hip_device, n, V):
    out, _ = _check_A(nref.scene_case(n, V, seed=10 * n + V), hip_device, f"n={n} V={V}")
    assert float((out.norm(dim=-1) - 1).abs().max()) < 1e-6


@functools.lru_cache(maxsize=None)
def _cyclic_case(n, V, B):
    """V views that repeat B distinct cameras of make_views cyclically.  A full circle of hundreds of cameras cannot keep
    every axis 1e-2 off perpendicular to every view direction (some camera always comes that close, and the builder's redraw
    does not end), so the case is scene_case at B views, which meets check_scene_case as it stands, with
    views[v] = base[v % B].  B is coprime to 256: record v and record v - 256 are different cameras."""
    assert np.gcd(B, 256) == 1 and V > 256
    case = nref.scene_case(n, B, seed=10 * n + V)
    case["views"] = np.ascontiguousarray(case["views"][np.arange(V) % B])
    return case


@pytest.mark.parametrize("n,V,B", [(65, 257, 5), (63, 600, 7)])
def test_scene_normals_with_more_cameras_than_compaction_lanes(hip_device, n, V, B):
    """k_normals_cameras is one workgroup of 256 lanes: from camera 256 on a lane compacts a second record, and a third."""
    case = _cyclic_case(n, V, B)
    assert not np.array_equal(case["views"][256], case["views"][0]) and np.array_equal(case["views"][B], case["views"][0])
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    cos = nref.view_cosines(*(t64(case[k]) for k in A_KEYS)).numpy()
    flips = (cos > 0).any(0) & (cos < 0).any(0)
    assert flips.any() and not flips.all()                   # some Gaussians change sign between views, some do not
    out, grad = _check_A(case, hip_device, f"n={n} V={V} cyclic over {B}")
    assert float((out.norm(dim=-1) - 1).abs().max()) < 1e-6 and float(grad.abs().max()) > 0
    assert np.array_equal(_bits(out), _bits(out[:B][torch.arange(V, device=hip_device) % B]))      # one camera, one answer


@pytest.mark.parametrize("quat_scale", [1e-3, 1e3])
def test_scene_normals_of_raw_quaternions(hip_device, quat_scale):
    """The kernel normalises: quaternions a thousand times shorter and longer than unit, and a scene scale != 1 in slot 40."""
    case = nref.scene_case(257, 3, seed=7, quat_scale=quat_scale, scale40=(0.5, 1.0, 2.5))
    out, grad = _check_A(case, hip_device, f"|q| x {quat_scale:g}")
    unit = dict(case, rotation=(case["rotation"].astype(np.float64) / quat_scale).astype(np.float32))
    views, xyz, scaling, rotation = _dev(unit, hip_device, A_KEYS)
    from latentsplat_amd import gaussian_normals
    assert float((gaussian_normals(views, xyz, scaling, rotation) - out).abs().max()) < 1e-6
    assert float(grad.abs().max()) > 0


@pytest.mark.parametrize("ties", ["two", "three"])
def test_scale_ties_go_to_the_lowest_index(hip_device, ties):
    """Exact two-way ties at every pair of indices and three-way ties; log-scales and activated scales give the same bits."""
    from latentsplat_amd import gaussian_normals
    case = nref.scene_case(300, 3, seed=3, ties=ties)
    out, _ = _check_A(case, hip_device, f"ties={ties}")
    views, xyz, scaling, rotation = _dev(case, hip_device, A_KEYS)
    activated = torch.exp(scaling)
    tied = (scaling[:, 0] == scaling[:, 1]) | (scaling[:, 0] == scaling[:, 2]) | (scaling[:, 1] == scaling[:, 2])
    assert int(tied.sum()) == 100 and bool(((activated[:, 0] == activated[:, 1]) | (activated[:, 0] == activated[:, 2]) |
                                            (activated[:, 1] == activated[:, 2]))[tied].all())
    assert np.array_equal(_bits(gaussian_normals(views, xyz, activated, rotation)), _bits(out))


def test_rows_that_are_not_finite_give_zero(hip_device):
    from latentsplat_amd import gaussian_normals
    case = nref.scene_case(130, 2, seed=4)
    clean = gaussian_normals(*_dev(case, hip_device, A_KEYS))
    case["rotation"][3] = 0.0
    case["rotation"][64, 2] = np.nan
    case["xyz"][65, 0] = np.inf
    case["xyz"][129, 1] = np.nan
    views, xyz, scaling, rotation = _dev(case, hip_device, A_KEYS)
    rotation.requires_grad_(True)
    out = gaussian_normals(views, xyz, scaling, rotation)
    bad = torch.zeros(130, dtype=torch.bool, device=hip_device)
    bad[[3, 64, 65, 129]] = True
    assert not out[:, bad].any() and np.array_equal(_bits(out[:, ~bad]), _bits(clean[:, ~bad]))
    out.sum().backward()
    assert bool(torch.isfinite(rotation.grad).all()) and not rotation.grad[bad].any() and bool(rotation.grad[~bad].any(-1).all())


def test_only_the_rotation_receives_a_gradient(hip_device):
    from latentsplat_amd import gaussian_normals
    views, *leaves = _dev(nref.scene_case(65, 2, seed=6), hip_device, A_KEYS)
    leaves = [t.requires_grad_(True) for t in leaves]
    with pytest.raises(_lib.LsrError, match="views requires grad"):       # the normals turn with the view: no silent partial gradient
        gaussian_normals(views.clone().requires_grad_(True), *leaves)
    gaussian_normals(views, *leaves).square().sum().backward()
    assert leaves[0].grad is None and leaves[1].grad is None and leaves[2].grad is not None


# ---- B ----

B_KEYS = ("normal_map", "depth", "alpha", "views")
GRAD_LOSS = 0.75
SIZES = [(3, 3), (1, 5), (2, 7), (5, 4), (33, 31), (65, 34), (70, 97)]
# (V, H, W, offcentre) past the loops of k_image_mean_finish (csrc/lsr_image_sum.h), which no size above enters a second time: its 16 waves take the
# images w, w + 16, ... and a wave's 64 lanes the tiles l, l + 64, ... of an image (tests/test_normals_cpu.py asserts what
# each case reaches).  One row of valid pixels under 65 tiles, 66 tiles with a partial last one, and 9 x 8 tiles with
# interior ones.  At 3 x 2049 and 257 x 225 the tiles from the 65th on hold border pixels alone and their slots are 0: a
# finish kernel that left them out would not show there, so 258 x 225 goes with them, whose ninth row of tiles holds a
# row of valid pixels.
FINISH_WAVES, WAVE, TILE = 16, 64, 32
PAST_THE_FINISH = [(17, 3, 3, False), (33, 5, 4, True), (1, 3, 2049, False), (1, 3, 2081, True), (2, 257, 225, True),
                   (2, 258, 225, True)]


@functools.lru_cache(maxsize=None)
def _image_refs(V, H, W, offcentre):
    kw = dict(offcentre=True, scale40=tuple(np.linspace(0.5, 2.0, V)), zero_block=True) if offcentre else {}
    case = nref.image_case(V, H, W, seed=H + W + V, **kw)
    nref.check_image_case(case)
    return case, nref.consistency_and_grads(case, GRAD_LOSS, torch.float64), nref.consistency_and_grads(case, GRAD_LOSS, torch.float32)


def _run_B(case: dict, dev, want=("loss", "per_view", "depth_normals", "valid"), grads=("normal_map", "depth", "alpha")):
    from latentsplat_amd.normals import normal_consistency_backward, normal_consistency_forward
    N, depth, alpha, views = _dev(case, dev, B_KEYS)
    out = normal_consistency_forward(N, depth, alpha, views, case["alpha_min"], want=want)
    like = dict(normal_map=N, depth=depth, alpha=alpha)
    buf = {k: torch.full_like(like[k], float("nan")) for k in grads}           # written, never accumulated
    g = normal_consistency_backward(N, depth, alpha, views, torch.tensor([GRAD_LOSS], device=dev), case["alpha_min"],
                                    want=grads, out=buf)
    out.update({"grad_" + k: v for k, v in g.items()})
    return out


@pytest.mark.parametrize("offcentre", [False, True])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_normal_consistency_against_float64(hip_device, H, W, V, offcentre):
    _check_B(hip_device, V, H, W, offcentre)


@pytest.mark.parametrize("V,H,W,offcentre", PAST_THE_FINISH)
def test_normal_consistency_against_float64_past_the_finish_loops(hip_device, V, H, W, offcentre):
    """per_view is compared element by element: an image credited to the wrong wave, or a tile left out, shows."""
    _check_B(hip_device, V, H, W, offcentre)


def _check_B(hip_device, V, H, W, offcentre):
    case, want, stock = _image_refs(V, H, W, offcentre)
    show = f"{V}x{H}x{W} offcentre={offcentre}"
    got = _run_B(case, hip_device)
    assert np.array_equal(got["valid"].cpu().numpy().astype(bool), want["valid"]), show
    assert (int(want["valid"].sum()) > 0) == (H >= 3 and W >= 3)
    for k in ("loss", "per_view", "depth_normals", "grad_normal_map", "grad_depth", "grad_alpha"):
        nref.held(k, got[k].cpu().numpy(), want[k], stock[k], show)
    if H < 3 or W < 3:
        assert not got["loss"].any() and not got["grad_depth"].any() and not got["grad_alpha"].any() and not got["grad_normal_map"].any()
    again = _run_B(case, hip_device)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (show, k)


def test_every_optional_output_in_turn(hip_device):
    case, _, _ = _image_refs(3, 65, 34, True)
    full = _run_B(case, hip_device)
    names = ("loss", "per_view", "depth_normals", "valid")
    grads = ("normal_map", "depth", "alpha")
    for skip in names:
        got = _run_B(case, hip_device, want=tuple(k for k in names if k != skip))
        for k in names:
            assert (k not in got) if k == skip else np.array_equal(_bits(got[k]), _bits(full[k])), (skip, k)
    for skip in grads:
        got = _run_B(case, hip_device, grads=tuple(k for k in grads if k != skip))
        for k in grads:
            assert ("grad_" + k not in got) if k == skip else np.array_equal(_bits(got["grad_" + k]), _bits(full["grad_" + k])), (skip, k)
    only = _run_B(case, hip_device, want=("valid",), grads=("alpha",))
    assert np.array_equal(_bits(only["valid"]), _bits(full["valid"])) and np.array_equal(_bits(only["grad_alpha"]), _bits(full["grad_alpha"]))


def test_loss_function_and_depth_to_normals(hip_device):
    from latentsplat_amd import depth_to_normals, normal_consistency_loss
    case, want, stock = _image_refs(3, 70, 97, True)
    N, depth, alpha, views = _dev(case, hip_device, B_KEYS)
    for t in (N, depth, alpha):
        t.requires_grad_(True)
    with pytest.raises(_lib.LsrError, match="views requires grad"):       # the rays depend on the table: no silent partial gradient
        normal_consistency_loss(N, depth, alpha, views.clone().requires_grad_(True), case["alpha_min"])
    loss = normal_consistency_loss(N, depth, alpha, views, case["alpha_min"])
    assert loss.shape == ()
    (loss * GRAD_LOSS).backward()
    for k, t in (("grad_normal_map", N), ("grad_depth", depth), ("grad_alpha", alpha)):
        nref.held(k, t.grad.cpu().numpy(), want[k], stock[k], "autograd")
    normals, valid = depth_to_normals(depth.detach(), alpha.detach(), views.detach(), case["alpha_min"])
    assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), want["valid"])
    nref.held("depth_normals", normals.cpu().numpy(), want["depth_normals"], stock["depth_normals"], "depth_to_normals")
    # a depth map faces the camera everywhere: <n~, ray> < 0 at every valid pixel, the direction operator A gives a Gaussian
    H, W = depth.shape[1:]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    for v in range(3):
        rx, ry = nref.pixel_rays(torch.from_numpy(case["views"][v].astype(np.float64)), H, W, xs, ys)
        n = normals[v].double().cpu()
        assert bool(((n[0] * rx + n[1] * ry + n[2])[valid[v].cpu()] < 0).all())


# ---- through the scene ----

def _scene(n, dev, seed=0):
    from latentsplat_amd import GaussianScene
    p = sref.make_params(n, 4, seed=seed)
    rng = np.random.default_rng(seed)
    p["xyz"] = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    p["scaling"] = np.log(rng.uniform(0.03, 0.12, (n, 3))).astype(np.float32)
    p["opacity"] = rng.uniform(0.0, 3.0, (n, 1)).astype(np.float32)
    return GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in p.items()}).to(dev)


def test_render_with_normals_is_render_with_the_normals_as_features(hip_device):
    from latentsplat_amd import gaussian_normals, normal_consistency_loss
    dev = hip_device
    scene = _scene(2000, dev, seed=1)
    views = torch.from_numpy(nref.make_views(2, seed=5)).to(dev)
    H, W = 48, 40
    for kw in (dict(), dict(antialiasing=True), dict(filter_3d=scene.compute_filter_3d(views, W), antialiasing=True)):
        color, nmap, mask, depth, radii = scene.render_with_normals(views, H, W, **kw)
        normals = gaussian_normals(views, scene._xyz, scene._scaling, scene._rotation)
        c2, f2, m2, d2, r2 = scene.render(views, H, W, features=normals, **kw)
        for a, b in ((color, c2), (nmap, f2), (mask, m2), (depth, d2)):
            assert np.array_equal(_bits(a), _bits(b))
        assert nmap.shape == (2, 3, H, W) and torch.equal(radii, r2)
        loss = normal_consistency_loss(nmap, depth, mask, views, 0.3)
        grads = torch.autograd.grad(loss, [scene._xyz, scene._scaling, scene._rotation, scene._opacity])
        assert float(loss.detach()) > 0 and all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads)


GRAD_TOL = 1e-3     # max |got - want| <= GRAD_TOL ||want||_2 per tensor: the bar of the parity tests against the oracle
                    # (tests/test_camera_grads_gpu.py::_kernel_vs_oracle)


def _float64_chain(params: dict, filt: np.ndarray, views: np.ndarray, H: int, W: int, antialiasing: bool, alpha_min: float):
    """render_with_normals + normal_consistency_loss in float64 on the host, from the shared chain
    (tests/surface_chain_ref.py): the filtered activation restated (tests/filter3d_ref.py; a zero filter is the unfiltered
    map), operator A restated, the oracle's rasterizer per view, operator B restated.  (loss, gradients of xyz, scaling,
    rotation, opacity)."""
    from tests import surface_chain_ref as chain
    res = chain.chain(params, views, H, W, dict(normal=1.0), filt=filt, antialiasing=antialiasing, alpha_min=alpha_min)
    return res["terms"]["normal"], {k: res["grad"][k] for k in ("xyz", "scaling", "rotation", "opacity")}


@pytest.mark.parametrize("filtered,antialiasing", [(False, False), (True, True)])
def test_scene_gradients_against_the_float64_chain(hip_device, filtered, antialiasing):
    """About 2 000 Gaussians, 2 views at 48 x 40, through render_with_normals and normal_consistency_loss: the loss and the
    gradients that reach _xyz, _scaling, _rotation and _opacity against the same chain in float64."""
    from latentsplat_amd import normal_consistency_loss
    dev, H, W, alpha_min = hip_device, 48, 40, 0.3
    scene = _scene(2000, dev, seed=4)
    views = nref.make_views(2, seed=8)
    tv = torch.from_numpy(views).to(dev)
    filt = scene.compute_filter_3d(tv, W) if filtered else None
    kw = dict(filter_3d=filt, antialiasing=True) if filtered else {}
    _, nmap, mask, depth, _ = scene.render_with_normals(tv, H, W, **kw)
    loss = normal_consistency_loss(nmap, depth, mask, tv, alpha_min)
    got = torch.autograd.grad(loss, [scene._xyz, scene._scaling, scene._rotation, scene._opacity])
    params = {k[1:]: v.detach().cpu().numpy() for k, v in scene.named_parameters()}
    filt64 = filt.cpu().numpy() if filtered else np.zeros((2000, 1), np.float32)
    want_loss, want = _float64_chain(params, filt64, views, H, W, antialiasing, alpha_min)
    print(f"filtered={filtered}: loss {float(loss.detach()):.7f} against {want_loss:.7f}")
    assert abs(float(loss.detach()) - want_loss) <= 1e-5 * max(abs(want_loss), 1e-3) and want_loss > 1e-3
    for name, g in zip(("xyz", "scaling", "rotation", "opacity"), got):
        err, norm = float(np.abs(g.cpu().numpy().astype(np.float64) - want[name]).max()), float(np.linalg.norm(want[name]))
        print(f"  {name:9s} max error {err:.3e}  norm {norm:.3e}  ratio {err / norm:.2e}")
        assert norm > 0 and err <= GRAD_TOL * norm, name


def test_the_posed_path_renders_the_transformed_scene(hip_device):
    from latentsplat_amd import GaussianScene, similarity_matrix
    dev = hip_device
    scene = _scene(500, dev, seed=2)
    views = torch.from_numpy(nref.make_views(2, seed=6)).to(dev)
    M = similarity_matrix(torch.tensor([0.9, 0.1, -0.3, 0.2]), torch.tensor([0.1, -0.2, 0.15]), 1.1).to(dev)
    posed = [t.detach() for t in scene.render_with_normals(views, 48, 40, transforms=M)]
    moved = GaussianScene.from_tensors(**{k[1:]: v.detach().clone() for k, v in scene.named_parameters()}).to(dev).transform_(M)
    direct = [t.detach() for t in moved.render_with_normals(views, 48, 40)]
    for a, b in zip(posed[:4], direct[:4]):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    assert float(posed[1].abs().max()) > 0.1


def test_means2d_abs_meets_the_payload_limit(hip_device):
    dev = hip_device
    scene = _scene(64, dev, seed=3)
    views = torch.from_numpy(nref.make_views(1, seed=7)).to(dev)
    m2d_abs = torch.zeros(1, 64, 3, device=dev, requires_grad=True)
    with pytest.raises(_lib.LsrError, match="payload channels"):
        scene.render_with_normals(views, 32, 32, means2D_abs=m2d_abs)


def _tool(name):
    import os
    import sys

    from tests import util
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_the_fitting_and_rendering_tools(hip_device, tmp_path):
    """fit_ply --normal-reg / --flatten-reg runs the term from --normal-reg-from on and records it; render_ply --normals
    writes the rendered normal map next to the depth's normals."""
    import json
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, 2000, 64, 2)
    fit = _tool("fit_ply")
    argv = [str(path), "--views", "2", "--size", "48", "--steps", "6", "--noise", "0.2"]
    res = fit.main(argv + ["--out", str(tmp_path / "fit"), "--normal-reg", "0.05", "--normal-reg-from", "2", "--normal-alpha-min", "0.3",
                           "--flatten-reg", "1.0"])
    assert json.load(open(tmp_path / "fit" / "fit.json")) == res
    assert res["normal_reg"] == 0.05 and res["normal_reg_from"] == 2 and res["normal_alpha_min"] == 0.3 and res["flatten_reg"] == 1.0
    assert np.isfinite(res["loss_last"]) and np.isfinite(res["normal_loss_first"]) and np.isfinite(res["normal_loss_last"])
    plain = fit.main(argv + ["--out", str(tmp_path / "plain")])
    assert not any(k.startswith(("normal_", "flatten_")) for k in plain)
    with pytest.raises(SystemExit, match="absgrad"):
        fit.main(argv + ["--out", str(tmp_path / "refused"), "--normal-reg", "0.05", "--absgrad", "--densify-interval", "2"])
    out = tmp_path / "normals.npy"
    _tool("render_ply").main([str(path), "--out", str(tmp_path / "renders"), "--views", "2", "--size", "48", "--normals", str(out),
                              "--normal-alpha-min", "0.3"])
    both = np.load(out)
    assert both.shape == (2, 2, 3, 48, 48) and np.isfinite(both).all() and np.abs(both[0]).max() > 0.1 and np.abs(both[1]).max() > 0.1
    length = np.linalg.norm(both[1], axis=1)
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))


def test_graph_capture_replays_the_eager_bits(hip_device):
    """A and B, forward and backward, captured in one torch.cuda.graph and replayed on new inputs: the eager bits."""
    from latentsplat_amd import gaussian_normals, normal_consistency_loss
    dev = hip_device
    ca, cb = nref.scene_case(257, 3, seed=8), nref.scene_case(257, 3, seed=9)
    ia, _, _ = _image_refs(3, 65, 34, True)
    ib, _, _ = _image_refs(3, 65, 34, False)
    s_views, s_xyz, s_scaling = _dev(ca, dev, A_KEYS[:3])
    s_rot = torch.from_numpy(ca["rotation"]).to(dev).requires_grad_(True)
    s_N, s_depth, s_alpha = (t.requires_grad_(True) for t in _dev(ia, dev, B_KEYS[:3]))
    s_v2 = torch.from_numpy(ia["views"]).to(dev)
    up = torch.from_numpy(np.random.default_rng(0).standard_normal((3, 257, 3)).astype(np.float32)).to(dev)

    def step():
        out = gaussian_normals(s_views, s_xyz, s_scaling, s_rot)
        g_rot, = torch.autograd.grad(out, s_rot, up)
        loss = normal_consistency_loss(s_N, s_depth, s_alpha, s_v2, ia["alpha_min"])
        return (out, g_rot, loss) + torch.autograd.grad(loss, [s_N, s_depth, s_alpha])

    side = torch.cuda.Stream(dev)                # warm-up on a side stream, as torch.cuda.graph asks for
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for dst, src in ((s_views, cb["views"]), (s_xyz, cb["xyz"]), (s_scaling, cb["scaling"]), (s_rot, cb["rotation"]),
                         (s_N, ib["normal_map"]), (s_depth, ib["depth"]), (s_alpha, ib["alpha"]), (s_v2, ib["views"])):
            dst.copy_(torch.from_numpy(src).to(dev))
    graph.replay()
    torch.cuda.synchronize(dev)
    replayed = [t.clone() for t in captured]
    eager = step()
    for a, b in zip(replayed, eager):
        assert np.array_equal(_bits(a), _bits(b))
    assert float(replayed[2]) != 0.0
