"""3DGS scene import on the MI355X: lsr_ply_unpack against the float64 restatement (tests/ply_import_ref.py), the
round trip through this project's own export, and a loaded file rendered against the oracle."""
import json
import os

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import ply_import_ref as ref
from tests import util
from tests.test_ply_cpu import GOLDEN

pytestmark = pytest.mark.gpu

CASES = [(n, K, False) for n in (1, 63, 64, 65, 257, 1000) for K in (1, 4, 16)] + [(1000, 9, True)]


def _np(scene):
    f = lambda t: t.cpu().numpy()
    return dict(means=f(scene.means), shs=f(scene.shs), opacities=f(scene.opacities), scales=f(scene.scales),
                rotations=f(scene.rotations), cov3D=f(scene.covariances))


@pytest.mark.parametrize("n,K,shuffled", CASES)
def test_unpack_matches_the_restatement(hip_device, tmp_path, n, K, shuffled):
    from latentsplat_amd.ply_import import load_ply, unpack_vertices
    # the shuffled case: 3 extra properties and no normals -> K = 9 rows of 41 floats, an odd stride, so that rows
    # (and the workgroups' blocks of rows) start at every 16-byte phase
    names = ref.shuffled_names(K, extra=3, seed=7) if shuffled else ref.standard_names(K)
    assert not shuffled or (len(names) == 41 and names != ref.standard_names(K))
    table = ref.make_table(n, names, seed=1000 * K + n)
    want = ref.expected(table, names)
    ref.write_ply(tmp_path / "s.ply", names, table, comments=("a test scene",))
    scene = load_ply(tmp_path / "s.ply", hip_device)
    assert scene.sh_degree == {1: 0, 4: 1, 9: 2, 16: 3}[K] and scene.shs.shape == (n, K, 3)
    ref.assert_matches(_np(scene), want)
    # the same through the device-table entry point, from a table that does not start 16-byte aligned
    flat = torch.empty(table.size + 1, device=hip_device)
    flat[1:] = torch.from_numpy(table).reshape(-1).to(hip_device)
    raw = unpack_vertices(flat[1:].view(n, len(names)), names, opacity="raw")
    ref.assert_matches(_np(raw), ref.expected(table, names, opacity="raw"))
    assert np.array_equal(raw.opacities.cpu().numpy()[:, 0], table[:, names.index("opacity")])


@pytest.mark.parametrize("K,extra", [(25, 0), (4, 120), (4, 250)])
def test_unpack_degree_4_and_wide_rows(hip_device, K, extra):
    """Degree 4 (89-float rows), and rows wide enough that the LDS budget, not the workgroup size, sets the rows per
    workgroup: 143 floats (fewer than 128 rows fit) and 273 floats (fewer than 64)."""
    from latentsplat_amd.ply_import import unpack_vertices
    names = ref.shuffled_names(K, extra=extra, seed=9) if extra else ref.standard_names(K)
    assert len(names) == {0: 89, 120: 143, 250: 273}[extra]
    table = ref.make_table(300, names, seed=extra + K)
    got = unpack_vertices(torch.from_numpy(table).to(hip_device), names)
    assert got.sh_degree == {25: 4, 4: 1}[K]
    ref.assert_matches(_np(got), ref.expected(table, names))


def test_optional_outputs_and_empty_scene(hip_device, tmp_path):
    from latentsplat_amd.ply_import import layout_from_names, load_ply, unpack_table
    names = ref.standard_names(4)
    ref.write_ply(tmp_path / "e.ply", names, np.zeros((0, len(names)), np.float32))
    empty = load_ply(tmp_path / "e.ply", hip_device)
    assert empty.means.shape == (0, 3) and empty.shs.shape == (0, 4, 3) and empty.covariances.shape == (0, 6)
    assert empty.opacities.shape == (0, 1) and empty.sh_degree == 1
    table = ref.make_table(300, names, seed=3)
    want = ref.expected(table, names)
    rows = torch.from_numpy(table).to(hip_device)
    layout = layout_from_names(names, 300)
    for only in ("means", "shs", "opacities", "scales", "rotations", "cov3D"):
        got = unpack_table(rows, layout, want=(only,))
        assert list(got) == [only]
        ref.assert_matches({only: got[only].cpu().numpy()}, want)
    got = unpack_table(rows, layout, want=("means", "cov3D"))
    ref.assert_matches({k: v.cpu().numpy() for k, v in got.items()}, want)
    with pytest.raises(_lib.LsrError, match="unknown outputs"):
        unpack_table(rows, layout, want=("means", "cov3d"))


def test_own_export_round_trip(hip_device, tmp_path):
    from latentsplat_amd.ply_export import export_ply, pack_vertices
    from latentsplat_amd.ply_import import load_ply
    z = np.load(GOLDEN)
    args = [torch.tensor(z[k], device=hip_device) for k in ("extrinsics", "means", "scales", "rotations", "harmonics", "opacities")]
    table = pack_vertices(*args).cpu().numpy()
    export_ply(*args, tmp_path / "own.ply")
    scene = load_ply(tmp_path / "own.ply", hip_device, opacity="raw")
    f = lambda t: t.cpu().numpy()
    assert scene.sh_degree == 0
    assert np.array_equal(f(scene.means), table[:, 0:3]) and np.array_equal(f(scene.shs)[:, 0, :], table[:, 6:9])
    assert np.array_equal(f(scene.opacities)[:, 0], table[:, 9])
    np.testing.assert_allclose(f(scene.scales), np.exp(table[:, 10:13].astype(np.float64)), rtol=2e-5, atol=2e-5)
    q = table[:, 13:17].astype(np.float64)
    np.testing.assert_allclose(f(scene.rotations), q / np.linalg.norm(q, axis=1, keepdims=True), rtol=2e-5, atol=2e-5)


def test_unpack_at_size(hip_device, tmp_path):
    from latentsplat_amd.ply_import import load_ply
    n, K = 393_216, 16
    names = ref.standard_names(K)
    table = ref.make_table(n, names, seed=11)
    ref.write_ply(tmp_path / "big.ply", names, table)
    assert os.path.getsize(tmp_path / "big.ply") > 97_000_000
    ref.assert_matches(_np(load_ply(tmp_path / "big.ply", hip_device)), ref.expected(table, names))


# ---- a loaded file through the rasterizer ----

H = W = 64
G, VIEWS = 2000, 2


@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    """A degree-1 scene of 2 000 Gaussians in front of two cameras, as a standard scene file: positions, projected
    sizes and opacities of the synthetic test scenes, orientations and SH coefficients drawn here."""
    sc = util.make_scene(G, image_size=W, views=VIEWS, color_sh_degree=1, feature_channels=None)
    rng = np.random.default_rng(5)
    names = ref.standard_names(4)
    table = np.zeros((G, len(names)), np.float32)
    col = names.index
    z = sc.means[:, 2].numpy()
    major = np.exp(rng.uniform(np.log(0.3), np.log(3.0), G)) * z / (0.8 * W)
    table[:, col("x"):col("x") + 3] = sc.means.numpy()
    for k in range(3):
        table[:, col(f"scale_{k}")] = np.log(major * (1.0 if k == 0 else rng.uniform(0.3, 1.0, G)))
    table[:, col("rot_0"):col("rot_0") + 4] = rng.standard_normal((G, 4)) * rng.uniform(0.5, 2.0, (G, 1))
    p = sc.opacities.numpy().astype(np.float64).clip(1e-4, 1 - 1e-4)
    table[:, col("opacity")] = np.log(p / (1 - p))
    sh = sc.color_sh.numpy()                                           # (G, 3, K): channel-major, as the file stores it
    table[:, col("f_dc_0"):col("f_dc_0") + 3] = sh[:, :, 0]
    table[:, col("f_rest_0"):col("f_rest_0") + 9] = sh[:, :, 1:].reshape(G, 9)
    path = tmp_path_factory.mktemp("ply_scene") / "point_cloud.ply"
    ref.write_ply(path, names, table)
    return path, sc


def _oracle_forwards(views, scene):
    """Per view: the oracle's forward with its list of fragile evaluations (what oracle_rasterize_views drops)."""
    from oracle import oracle as orc
    c = lambda t: t.detach().cpu()
    n = lambda t: t.float().contiguous().numpy()
    outs = []
    for v in range(views.shape[0]):
        vw = c(views)[v]
        view = orc.View(H, W, float(vw[35]), float(vw[36]), vw[37:40].numpy(), vw[0:16].numpy().reshape(4, 4),
                        vw[16:32].numpy().reshape(4, 4), vw[32:35].numpy(), scene.sh_degree)
        m, c6, op, sh, _, _ = util.to_boundary(c(views), v, c(scene.means), c(scene.covariances), c(scene.opacities),
                                               c(scene.shs), None, None, None, False)
        outs.append(orc.forward(view, n(m), n(c6), n(op), n(sh), None, None))
    return outs


def test_loaded_scene_renders_what_the_oracle_renders(hip_device, scene_file):
    import diff_gaussian_rasterization as dgr
    from latentsplat_amd.decoder.cuda_splatting import _scaled_cameras
    from latentsplat_amd.ply_import import load_ply
    from latentsplat_amd.rasterizer import build_view_table, get_color_sh_convention, rasterize_views
    path, sc = scene_file
    dev = hip_device
    assert get_color_sh_convention() == "3dgs"
    s = load_ply(path, dev)
    assert s.sh_degree == 1 and s.means.shape == (G, 3)
    bg = torch.tensor([0.1, 0.2, 0.3])
    views = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev), bg.to(dev),
                             scale_invariant=False)
    with torch.no_grad():
        color, _, mask, depth, radii = rasterize_views(views, H, W, s.sh_degree, s.means, s.covariances, s.opacities, shs=s.shs)
    want = util.oracle_rasterize_views(views, H, W, s.sh_degree, s.means, s.covariances, s.opacities, shs=s.shs)
    fwd = _oracle_forwards(views, s)
    assert (radii.cpu().numpy() > 0).sum() > G // 2
    for v in range(VIEWS):
        assert np.array_equal(want[0][v].numpy(), fwd[v]["color"])
        assert np.array_equal(radii[v].cpu().numpy(), want[4][v].numpy())
        util.assert_close_except_fragile(color[v].cpu().numpy(), want[0][v].numpy(), fwd[v], 1e-4, f"loaded scene colour[view {v}]")
        util.assert_close_except_fragile(mask[v].cpu().numpy(), want[2][v].numpy(), fwd[v], 1e-4, f"loaded scene mask[view {v}]")
        dscale = max(1.0, float(np.abs(want[3][v].numpy()).max()))      # depth: 1e-4 of the largest rendered depth, as elsewhere
        util.assert_close_except_fragile(depth[v].cpu().numpy(), want[3][v].numpy(), fwd[v], 1e-4 * dscale, f"loaded scene depth[view {v}]",
                                         flip_bound=2e-2 * max(dscale, float(fwd[v]["gdepth"].max(initial=1.0))), scale=dscale)

    # the published single-view interface: cov3D_precomp, and scales / rotations in its place
    cams, _ = _scaled_cameras(sc.extrinsics, sc.intrinsics, sc.near, sc.far, False)
    for v in range(VIEWS):
        rs = dgr.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=float(cams.tan_fov_x[v]), tanfovy=float(cams.tan_fov_y[v]), bg=bg.to(dev),
            scale_modifier=1.0, viewmatrix=cams.view_matrix[v].to(dev), projmatrix=cams.full_projection[v].to(dev),
            sh_degree=s.sh_degree, campos=cams.campos[v].to(dev), prefiltered=False, debug=False)
        with torch.no_grad():
            a = dgr.GaussianRasterizer(rs)(means3D=s.means, means2D=None, opacities=s.opacities, shs=s.shs,
                                           cov3D_precomp=s.covariances)
            b = dgr.GaussianRasterizer(rs)(means3D=s.means, means2D=None, opacities=s.opacities, shs=s.shs,
                                           scales=s.scales, rotations=s.rotations)
        util.assert_close_except_fragile(a[0].cpu().numpy(), want[0][v].numpy(), fwd[v], 1e-4, f"GaussianRasterizer colour[view {v}]")
        util.assert_close_except_fragile(b[0].cpu().numpy(), a[0].cpu().numpy(), fwd[v], 1e-4, f"scales / rotations colour[view {v}]")
        util.assert_close_except_fragile(b[2][0].cpu().numpy(), a[2][0].cpu().numpy(), fwd[v], 1e-4, f"scales / rotations mask[view {v}]")


def test_render_tool(hip_device, scene_file, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import render_ply
    finally:
        sys.path.pop(0)
    path, _ = scene_file
    out = tmp_path / "renders"
    status = render_ply.main([str(path), "--out", str(out), "--views", "3", "--size", "48"])
    color, mask, depth = (np.load(out / f"{k}.npy") for k in ("color", "mask", "depth"))
    assert color.shape == (3, 3, 48, 48) and mask.shape == (3, 48, 48) and depth.shape == (3, 48, 48)
    assert np.isfinite(color).all() and np.isfinite(depth).all() and mask.max() > 0.01       # a non-empty mask
    saved = json.load(open(out / "status.json"))
    assert saved == status and saved["num_pairs"] > 0 and saved["gaussians"] == G and not saved["overflow"]
    assert min(saved["visible"]) > 0
