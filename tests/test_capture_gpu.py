"""End to end: a seeded scene rendered from six circle cameras, quantised, cropped (which moves the principal point off the
centre by whole pixels), written as a COLMAP model with photographs, loaded back through latentsplat_amd.capture.Capture,
compared with what was rendered, and trained on with tools/train_colmap.py.

The scene is built so that the rasterizer's result does not depend on where the tile grid lies, because the original render
and the render through the capture's centred camera see the same rays on grids 2 x 1 pixels apart.  The rasterizer lists a
Gaussian for the tiles of the published rectangle, `(int)((p - r) / 16) .. (int)((p + r + 15) / 16)` with `r = ceil(3 sigma)`,
and blends it at every pixel of those tiles where its alpha reaches 1 / 255.  On the left / top a pixel outside the listed
tiles is more than `r` from the centre; on the right / bottom only more than `r - 1` (the published expression truncates a
float, it is no integer ceiling): the pixels `r - 1 < dx <= r` are blended when they share a tile with the rectangle and dropped
when they start the next tile.  Such a pixel has `alpha <= opacity exp(-(3 sigma - 1)^2 / (2 sigma^2))`, with `sigma^2` the
larger eigenvalue of the projected covariance.  Small Gaussians lose the most: at sigma = 1 px the factor is exp(-2) = 0.14,
and a scene of 0.6 .. 1.3 px Gaussians with opacities up to 0.33 differs between the two grids by up to 4.5e-3 in colour and
6.0e-3 in the mask (measured; with opacities up to 0.95 1.4e-2; by 5e-7 for a grid moved by a whole tile).  Here every scale
is at least 0.6 world units and every depth at most 4.05 + sqrt(2) = 5.46, so sigma >= 0.6 x 38.4 / 5.46 = 4.2 px, the factor is
at most exp(-(11.6)^2 / (2 x 17.6)) = 0.022, and with opacities up to sigmoid(-1.8) = 0.142 the dropped alpha stays below
0.0031 < 1 / 255: such a pixel fails the alpha test on either grid, and both renders blend the same Gaussians at every pixel."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import colmap_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, VIEWS, W0, H0 = 2000, 6, 48, 40
CROP_LEFT, CROP_TOP = 4, 2
FX, FY = 0.8 * W0, 0.8 * H0
RADIUS = 4.0


def _scene(dev):
    from latentsplat_amd import GaussianScene
    rng = np.random.default_rng(11)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    q = rng.standard_normal((N, 4))
    return GaussianScene.from_tensors(xyz=f(rng.uniform(-1.0, 1.0, (N, 3))), features_dc=f(rng.uniform(-1.5, 1.5, (N, 1, 3))),
                                      features_rest=torch.zeros((N, 0, 3)), opacity=f(rng.uniform(-3.5, -1.8, (N, 1))),
                                      scaling=f(np.log(rng.uniform(0.6, 0.9, (N, 3)))), rotation=f(q)).to(dev)


def _circle():
    """float64 camera-to-world matrices on a circle around the origin, looking at it (x right, y down, z forward)."""
    c2w = np.zeros((VIEWS, 4, 4))
    for k in range(VIEWS):
        ang = 2 * math.pi * k / VIEWS + 0.1
        offset = np.array([math.cos(ang), 0.15 * math.sin(3 * ang), math.sin(ang)])
        forward = -offset / np.linalg.norm(offset)
        right = np.cross([0.0, 1.0, 0.0], forward)
        right /= np.linalg.norm(right)
        c2w[k, :3, 0], c2w[k, :3, 1], c2w[k, :3, 2], c2w[k, :3, 3] = right, np.cross(forward, right), forward, RADIUS * offset
        c2w[k, 3, 3] = 1.0
    return c2w


@pytest.fixture(scope="module")
def world(hip_device, tmp_path_factory):
    from latentsplat_amd.capture import Capture, cameras_extent
    from latentsplat_amd.rasterizer import build_view_table
    dev = hip_device
    scene = _scene(dev)
    c2w = _circle()
    _, extent = cameras_extent(c2w[:, :3, 3])
    ext = torch.from_numpy(c2w.astype(np.float32)).to(dev)
    intr = torch.tensor([[FX / W0, 0, 0.5], [0, FY / H0, 0.5], [0, 0, 1.0]], device=dev).repeat(VIEWS, 1, 1)
    near, far = torch.full((VIEWS,), 0.01 * extent, device=dev), torch.full((VIEWS,), 100.0 * extent, device=dev)
    with torch.no_grad():
        render = scene.render(build_view_table(ext, intr, near, far, torch.zeros(3, device=dev)), H0, W0)[0].clamp(0.0, 1.0)
    u8 = torch.round(render * 255.0).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()           # (V, H0, W0, 3)
    cropped = [np.ascontiguousarray(u8[k, CROP_TOP:, CROP_LEFT:]) for k in range(VIEWS)]
    camera = dict(id=5, model=1, width=W0 - CROP_LEFT, height=H0 - CROP_TOP, params=[FX, FY, W0 / 2.0 - CROP_LEFT, H0 / 2.0 - CROP_TOP])
    names = [f"view_{(7 * k) % VIEWS}.npy" for k in range(VIEWS)]                               # file order is not name order
    xyz = scene._xyz.detach().cpu().numpy()
    rgb = np.clip(np.rint((0.5 + 0.28209479177387814 * scene._features_dc.detach().cpu().numpy()[:, 0]) * 255), 0, 255).astype(np.uint8)
    root = tmp_path_factory.mktemp("capture")
    cr.write_capture(root / "bin", c2w, [camera], [5] * VIEWS, cropped, names, xyz, rgb, fmt="bin")
    cr.write_capture(root / "txt", c2w, [camera], [5] * VIEWS, cropped, [n.replace(".npy", ".ppm") for n in names], xyz, rgb, fmt="txt")
    capture = Capture.load(root / "bin", device=dev)
    order = sorted(range(VIEWS), key=lambda k: names[k])
    return dict(dev=dev, scene=scene, c2w=c2w[order], render=render[order], u8=u8[order], capture=capture, root=root, extent=extent,
                xyz=xyz, rgb=rgb)


def test_capture_recovers_cameras_targets_and_coverage(world):
    cap, dev = world["capture"], world["dev"]
    Hs, Ws = H0 - CROP_TOP, W0 - CROP_LEFT
    assert len(cap) == VIEWS and cap.names == sorted(cap.names) and cap.sizes == [(Hs, Ws)] * VIEWS
    assert cap.model.format == "binary"
    assert np.abs(cap.extrinsics.double().cpu().numpy() - world["c2w"]).max() < 1e-6
    want_intr = np.array([[FX / Ws, 0, 0.5], [0, FY / Hs, 0.5], [0, 0, 1]], np.float32)
    assert np.array_equal(cap.intrinsics.cpu().numpy(), np.broadcast_to(want_intr, (VIEWS, 3, 3)))
    assert cap.cameras_extent == pytest.approx(world["extent"], rel=1e-12) and cap.cameras_extent == pytest.approx(1.1 * RADIUS, rel=0.05)
    assert torch.allclose(cap.near, torch.full((VIEWS,), 0.01 * world["extent"], device=dev)) and torch.allclose(cap.far, 1e4 * cap.near)
    idx = list(range(VIEWS))
    targets, coverage = cap.targets(idx), cap.coverage(idx)
    assert targets.shape == (VIEWS, 3, Hs, Ws) and coverage.shape == (VIEWS, Hs, Ws)
    # the principal point sits (2, 1) pixels left of / above the cropped image's centre: the target camera sees two columns
    # and one row the photograph does not have, and everything else is the photograph moved by whole pixels
    want_cov = np.ones((Hs, Ws), np.float32)
    want_cov[:, :CROP_LEFT // 2] = 0
    want_cov[:CROP_TOP // 2, :] = 0
    assert np.array_equal(coverage.cpu().numpy(), np.broadcast_to(want_cov, (VIEWS, Hs, Ws)))
    want = np.zeros((VIEWS, 3, Hs, Ws), np.float32)
    moved = world["u8"][:, CROP_TOP:, CROP_LEFT:].astype(np.float32) / np.float32(255.0)     # the photograph: target (i, j) = photograph (i - 1, j - 2)
    want[:, :, CROP_TOP // 2:, CROP_LEFT // 2:] = moved.transpose(0, 3, 1, 2)[:, :, :Hs - CROP_TOP // 2, :Ws - CROP_LEFT // 2]
    assert np.array_equal(targets.cpu().numpy().view(np.uint32), want.view(np.uint32))
    xyz, rgb = cap.points
    assert np.array_equal(xyz.cpu().numpy(), world["xyz"]) and np.array_equal(rgb.cpu().numpy(), world["rgb"].astype(np.float32) / np.float32(255))
    assert cap.split(4) == ([1, 2, 3, 5], [0, 4]) and cap.split(0) == (idx, [])
    assert torch.equal(cap.targets([4, 1]), targets[[4, 1]]) and torch.equal(cap.coverage([2]), coverage[[2]])
    with pytest.raises(Exception):
        cap.targets([VIEWS])


def test_text_model_and_ppm_photographs_load_to_the_same_capture(world):
    from latentsplat_amd.capture import Capture
    cap = world["capture"]
    other = Capture.load(world["root"] / "txt", device=world["dev"], batch=4)
    idx = list(range(VIEWS))
    assert other.model.format == "text" and [n[:-4] for n in other.names] == [n[:-4] for n in cap.names]
    assert torch.equal(other.targets(idx), cap.targets(idx)) and torch.equal(other.coverage(idx), cap.coverage(idx))
    assert torch.equal(other.extrinsics, cap.extrinsics) and torch.equal(other.intrinsics, cap.intrinsics)
    half = Capture.load(world["root"] / "bin", resolution=2, device=world["dev"], near=0.5, far=50.0)
    Hs, Ws = H0 - CROP_TOP, W0 - CROP_LEFT
    assert half.sizes == [(Hs // 2, Ws // 2)] * VIEWS and float(half.near[0]) == 0.5 and float(half.far[0]) == 50.0
    assert half.intrinsics[0, 0, 0].item() == pytest.approx(FX / 2 / (Ws // 2), rel=1e-6)
    src = np.stack([np.load(world["root"] / "bin" / "images" / n) for n in half.names])
    cam = cr.camera_numbers(1, [FX, FY, W0 / 2.0 - CROP_LEFT, H0 / 2.0 - CROP_TOP])
    image, coverage, _ = cr.prepare_ref(src, cam, Hs // 2, Ws // 2, FX / 2, FY / 2)
    assert np.abs(half.targets(idx).double().cpu().numpy() - image).max() < 1e-6             # (exact path: float32 rounding of the quotient)
    assert np.array_equal(half.coverage(idx).double().cpu().numpy(), coverage)
    with pytest.raises(Exception, match="missing"):
        Capture.load(world["root"] / "missing", device=world["dev"])


def test_rendering_through_the_capture_agrees_with_the_targets(world):
    """The render through the capture's camera table against the targets on the covered pixels: at most the quantisation
    step (the original render against its uint8 round trip) plus 1 / 255.

    The two renders see the same rays on tile grids 2 x 1 pixels apart; the scene is one for which the rasterizer blends the
    same Gaussians at every pixel on either grid (the module's docstring)."""
    cap, scene, dev = world["capture"], world["scene"], world["dev"]
    idx = list(range(VIEWS))
    (H, W), = set(cap.sizes)
    with torch.no_grad():
        render = scene.render(cap.views(idx, torch.zeros(3, device=dev)), H, W)[0].clamp(0.0, 1.0)
    covered = cap.coverage(idx)[:, None].expand(-1, 3, -1, -1) > 0
    quantisation = float((world["render"] - torch.from_numpy(world["u8"]).to(dev).permute(0, 3, 1, 2).float() / 255.0).abs().max())
    worst = float((render - cap.targets(idx)).abs()[covered].max())
    print(f"capture render vs targets: worst {worst:.3e}, quantisation {quantisation:.3e}, bound {quantisation + 1 / 255:.3e}")
    assert 0.0 < quantisation <= 0.5 / 255 + 1e-6
    assert worst <= quantisation + 1.0 / 255.0
    assert float(cap.targets(idx)[covered].max()) > 0.2                # (the comparison is not of black images)


def test_a_crop_by_whole_tiles_agrees_to_float_error(world, tmp_path):
    """The control of the test above: the same scene and poses rendered at (48 + 32) x (40 + 32) and cropped by 32 columns
    and 32 rows, so that the capture's centred 48 x 40 camera sits 16 x 16 pixels, one tile, inside the original grid.
    Whatever the scene, both renders then list the same Gaussians for every tile, and the capture's render agrees with the
    original to float error."""
    from latentsplat_amd.capture import Capture
    from latentsplat_amd.rasterizer import build_view_table
    dev, scene, extent = world["dev"], world["scene"], world["extent"]
    V, Wb, Hb, cut = 3, W0 + 32, H0 + 32, 32
    c2w = _circle()[:V]
    ext = torch.from_numpy(c2w.astype(np.float32)).to(dev)
    intr = torch.tensor([[FX / Wb, 0, 0.5], [0, FY / Hb, 0.5], [0, 0, 1.0]], device=dev).repeat(V, 1, 1)
    near, far = torch.full((V,), 0.01 * extent, device=dev), torch.full((V,), 100.0 * extent, device=dev)
    with torch.no_grad():
        big = scene.render(build_view_table(ext, intr, near, far, torch.zeros(3, device=dev)), Hb, Wb)[0].clamp(0.0, 1.0)
    u8 = torch.round(big * 255.0).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    camera = dict(id=1, model=1, width=Wb - cut, height=Hb - cut, params=[FX, FY, Wb / 2.0 - cut, Hb / 2.0 - cut])
    cr.write_capture(tmp_path, c2w, [camera], [1] * V, [u8[k, cut:, cut:] for k in range(V)], [f"{k}.npy" for k in range(V)],
                     world["xyz"], world["rgb"])
    cap = Capture.load(tmp_path, device=dev, near=0.01 * extent, far=100.0 * extent)
    idx = list(range(V))
    assert cap.sizes == [(H0, W0)] * V
    coverage = cap.coverage(idx)
    assert bool((coverage[:, :16] == 0).all()) and bool((coverage[:, :, :16] == 0).all()) and bool((coverage[:, 16:, 16:] == 1).all())
    inner = big[:, :, 16:16 + H0, 16:16 + W0]
    photo = (u8[:, cut:, cut:].astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)       # target (i, j) = photograph (i - 16, j - 16)
    assert np.array_equal(cap.targets(idx)[:, :, 16:, 16:].cpu().numpy(), photo[:, :, :H0 - 16, :W0 - 16])
    with torch.no_grad():
        render = scene.render(cap.views(idx, torch.zeros(3, device=dev)), H0, W0)[0].clamp(0.0, 1.0)
    assert float((render - inner).abs().max()) < 1e-5
    covered = (coverage > 0)[:, None].expand(-1, 3, -1, -1)
    assert float((render - cap.targets(idx)).abs()[covered].max()) <= 0.5 / 255 + 1e-5


def test_train_colmap_tool(world, tmp_path):
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_colmap
    res = train_colmap.main([str(world["root"] / "bin"), "--out", str(tmp_path / "fit"), "--steps", "30", "--hold", "3", "--batch", "2", "--seed", "1"])
    assert os.path.getsize(tmp_path / "fit" / "point_cloud.ply") > N * 14 * 4
    with open(tmp_path / "fit" / "metrics.json") as f:
        stored = json.load(f)
    assert stored["loss_first"] == res["loss_first"] and stored["loss_last"] == res["loss_last"]
    print(f"train_colmap: loss {res['loss_first']:.4f} -> {res['loss_last']:.4f}, psnr {res['psnr']:.2f}, ssim {res['ssim']:.4f}, "
          f"{res['ms_per_step']:.2f} ms / step")
    assert res["loss_last"] < res["loss_first"]
    assert res["gaussians"] == N and res["steps"] == 30 and res["train_views"] == 4 and res["test_views"] == 2
    assert res["ms_per_step"] > 0 and math.isfinite(res["psnr"]) and 0.0 < res["ssim"] <= 1.0
    from latentsplat_amd import GaussianScene
    assert GaussianScene.from_ply(tmp_path / "fit" / "point_cloud.ply", world["dev"]).num_gaussians == N
