"""Mesh extraction on the MI355X: lsr_tsdf_integrate and lsr_mesh_count / lsr_mesh_emit against the numpy restatement
(tests/tsdf_ref.py): fusion under the project's error rule on every lattice point that is not fragile, with EQUAL weights;
faces EQUAL as integer arrays; bit-reproducibility, chunked calls, graph capture, the capacity contract of the C ABI, the
rasterizer's pixel convention, and the operators through GaussianScene.extract_mesh."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import normals_ref as nref
from tests import scene_params_ref as sref
from tests import tsdf_ref as tr

pytestmark = pytest.mark.gpu


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def _volume(case: dict, dev, state=None):
    """A TSDFVolume of the case's lattice, empty or holding ``state`` (numpy arrays of tests/tsdf_ref.py)."""
    from latentsplat_amd.mesh import TSDFVolume
    vol = TSDFVolume(case["origin"], case["voxel_size"], case["dims"], trunc=case.get("trunc"), color=case.get("has_color", True), device=dev)
    if state is not None:
        vol.tsdf.copy_(torch.from_numpy(state["tsdf"]))
        vol.weight.copy_(torch.from_numpy(state["weight"]))
        if vol.color is not None:
            vol.color.copy_(torch.from_numpy(state["color"]))
    return vol


def _fuse(vol, case: dict, dev, lo=0, hi=None):
    dev_ = lambda a: None if a is None else torch.from_numpy(a[lo:hi]).to(dev)
    vol.integrate(dev_(case["depth"]), dev_(case["alpha"]), dev_(case["views"]), color=dev_(case["image_color"]),
                  alpha_min=case["alpha_min"], depth_max=case["depth_max"], max_weight=case["max_weight"])
    return vol


def _state(vol) -> dict:
    return dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=None if vol.color is None else vol.color.cpu().numpy())


def _same(a, b) -> bool:
    return all(x is None and y is None or np.array_equal(_bits(x), _bits(y)) for x, y in ((a.tsdf, b.tsdf), (a.weight, b.weight), (a.color, b.color)))


# ---- fusion ----

@pytest.mark.parametrize("color", [True, False])
@pytest.mark.parametrize("V", tr.FUSION_V)
@pytest.mark.parametrize("nx", tr.FUSION_NX)
def test_fusion_against_float64(hip_device, nx, V, color):
    case, want, stock = tr.fusion_refs((nx, 5, 3), V, tr.fusion_seed(nx, V), color)
    vol = _fuse(_volume(case, hip_device), case, hip_device)
    tr.compare_fusion(_state(vol), want, stock, f"nx={nx} V={V} color={color}")
    assert (vol.color is None) == (not color)
    again = _fuse(_volume(case, hip_device), case, hip_device)                    # two identical runs: the same bits
    assert _same(vol, again)


def test_fusion_of_more_views_than_the_compaction_workgroup_has_lanes(hip_device):
    case, want, stock = tr.fusion_refs((65, 5, 3), 257, 77, True)
    vol = _fuse(_volume(case, hip_device), case, hip_device)
    tr.compare_fusion(_state(vol), want, stock, "V=257")
    assert float(vol.weight.max()) > 40


def test_one_call_over_five_views_is_three_plus_two(hip_device):
    for color in (True, False):
        case, _, _ = tr.fusion_refs((130, 5, 3), 5, tr.fusion_seed(130, 5), color)
        whole = _fuse(_volume(case, hip_device), case, hip_device)
        parts = _fuse(_fuse(_volume(case, hip_device), case, hip_device, 0, 3), case, hip_device, 3, 5)
        assert _same(whole, parts) and float(whole.weight.max()) >= 2


def test_cameras_that_see_nothing_leave_the_volume_alone(hip_device):
    case, want, _ = tr.fusion_refs((65, 5, 3), 3, 5, True, kind="away")
    assert (want["weight"] == 0).all()
    rng = np.random.default_rng(1)
    shape = want["tsdf"].shape
    state = dict(tsdf=rng.uniform(-1, 1, shape).astype(np.float32), weight=rng.integers(0, 5, shape).astype(np.float32),
                 color=rng.uniform(0, 1, (3,) + shape).astype(np.float32))
    vol = _fuse(_volume(case, hip_device, state), case, hip_device)
    got = _state(vol)
    for k in state:
        assert np.isfinite(got[k]).all() and np.array_equal(got[k].view(np.uint32), state[k].view(np.uint32)), k


def test_cameras_inside_the_volume(hip_device):
    """The brick rejection is conservative: with the cameras inside the volume, where bricks straddle every frustum plane
    and the camera plane itself, each lattice point still gets exactly the reference's observations."""
    case, want, stock = tr.fusion_refs((65, 9, 4), 3, 11, True, kind="inside")
    assert 0.05 < float((want["weight"] > 0).mean()) < 0.95           # some points behind a camera or outside its image
    vol = _fuse(_volume(case, hip_device), case, hip_device)
    tr.compare_fusion(_state(vol), want, stock, "inside")


@pytest.mark.parametrize("kw", tr.LIMIT_CASES, ids=str)
def test_depth_max_and_max_weight(hip_device, kw):
    free, _, _ = tr.fusion_refs((130, 5, 3), 5, tr.fusion_seed(130, 5), True)
    case, want, stock = tr.fusion_refs((130, 5, 3), 5, tr.fusion_seed(130, 5), True, **kw)
    unlimited = tr.integrate(tr.empty_volume(case["dims"]), free, np.float64)
    assert not np.array_equal(unlimited["weight"], want["weight"])    # the limit changes the result
    vol = _fuse(_volume(case, hip_device), case, hip_device)
    tr.compare_fusion(_state(vol), want, stock, str(kw))
    if "max_weight" in kw:
        assert float(vol.weight.max()) == kw["max_weight"]


def test_graph_replay_equals_the_eager_call(hip_device):
    dev = hip_device
    ca, _, _ = tr.fusion_refs((65, 5, 3), 3, tr.fusion_seed(65, 3), True)
    cb, _, _ = tr.fusion_refs((65, 5, 3), 3, 4242, True)
    vol = _volume(ca, dev)
    s_depth, s_alpha, s_views, s_color = (torch.from_numpy(ca[k]).to(dev) for k in ("depth", "alpha", "views", "image_color"))
    step = lambda: vol.integrate(s_depth, s_alpha, s_views, color=s_color)
    side = torch.cuda.Stream(dev)                # warm-up on a side stream, as torch.cuda.graph asks for
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for dst, k in ((s_depth, "depth"), (s_alpha, "alpha"), (s_views, "views"), (s_color, "image_color")):
        dst.copy_(torch.from_numpy(cb[k]).to(dev))
    vol.reset()
    graph.replay()
    torch.cuda.synchronize(dev)
    eager = _fuse(_volume(cb, dev), cb, dev)
    assert _same(vol, eager) and float(vol.weight.max()) >= 1


def test_the_rasterizer_puts_a_gaussian_on_the_pixel_fusion_reads(hip_device):
    """The render of one small opaque Gaussian has its mask maximum at the (ix, iy) the reference computes for its mean:
    fusion inverts the rasterizer's own ndc = (2 x + 1) / W - 1."""
    from latentsplat_amd.rasterizer import rasterize_views
    dev, H, W = hip_device, 20, 24
    views = nref.make_views(3, seed=3, offcentre=True)
    rng = np.random.default_rng(0)
    for _ in range(1000):                        # an off-centre mean that no camera sees within 0.25 of a pixel boundary
        mean = rng.uniform(-0.5, 0.5, 3)
        f = np.array([tr.pixel_of(v, mean, H, W) for v in views])
        if (np.abs(f - np.round(f)) < 0.25).all() and (np.abs(f - [(W - 1) / 2, (H - 1) / 2]) > 1.5).all() and \
                (f > 1).all() and (f < [W - 2, H - 2]).all():
            break
    else:
        raise AssertionError("no such mean")
    means = torch.tensor(mean[None], dtype=torch.float32, device=dev)
    cov = torch.tensor([[1e-4, 0, 0, 1e-4, 0, 1e-4]], dtype=torch.float32, device=dev)
    _, _, mask, depth, _ = rasterize_views(torch.from_numpy(views).to(dev), H, W, 0, means, cov, torch.ones((1, 1), device=dev),
                                           colors_precomp=torch.ones((1, 3), device=dev))
    for v in range(3):
        at = int(mask[v].argmax())
        assert float(mask[v].max()) > 0.1
        assert (at % W, at // W) == (int(np.floor(f[v, 0] + 0.5)), int(np.floor(f[v, 1] + 0.5))), (v, f[v])


# ---- extraction ----

GRIDS = {
    "random-5x4x3": lambda: tr.random_grid((5, 4, 3), 1),
    "nx2": lambda: tr.random_grid((2, 3, 3), 2, invalid=0.1),
    "nx64": lambda: tr.random_grid((64, 3, 3), 3, invalid=0.1),
    "nx65": lambda: tr.random_grid((65, 3, 3), 4, invalid=0.1),
    "nx129": lambda: tr.random_grid((129, 3, 3), 5, invalid=0.1),
    "zeros": lambda: tr.random_grid((5, 4, 3), 6, invalid=0.0, zeros=True),
    "sphere": lambda: tr.sphere_grid(),
}


def _extract(grid: dict, dev, color=True, min_weight=1.0):
    case = dict(origin=grid["origin"], voxel_size=grid["voxel_size"], dims=grid["dims"], has_color=color)
    vol = _volume(case, dev, dict(tsdf=grid["tsdf"], weight=grid["weight"], color=grid["color"]))
    return vol, vol.extract_mesh(min_weight)


@pytest.mark.parametrize("name", list(GRIDS))
def test_extraction_against_the_reference(hip_device, name):
    grid = GRIDS[name]()
    want_v, want_f, want_c = tr.grid_mesh(grid)
    stock_v, _, stock_c = tr.grid_mesh(grid, dt=np.float32)
    vol, (vertices, faces, colors) = _extract(grid, hip_device)
    assert faces.dtype == torch.int32 and vertices.shape == (len(want_v), 3) and colors.shape == (len(want_v), 3)
    assert len(want_f) > 0 and np.array_equal(faces.cpu().numpy(), want_f)
    nref.held("vertices", vertices.cpu().numpy(), want_v, stock_v.astype(np.float64), name)
    nref.held("vertex_colors", colors.cpu().numpy(), want_c, stock_c.astype(np.float64), name)
    v2, f2, c2 = vol.extract_mesh()                                   # two runs: the same bits
    assert np.array_equal(_bits(vertices), _bits(v2)) and torch.equal(faces, f2) and np.array_equal(_bits(colors), _bits(c2))
    _, (v3, f3, c3) = _extract(grid, hip_device, color=False)
    assert c3 is None and np.array_equal(_bits(vertices), _bits(v3)) and torch.equal(faces, f3)
    if name == "sphere":                                              # the manifold checks, on the KERNEL's output
        st, ref = tr.mesh_stats(vertices.cpu().numpy(), faces.cpu().numpy()), tr.mesh_stats(want_v, want_f)
        assert st["directed_once"] and st["paired"] and st["euler"] == 2 and st["outward"] > 0
        assert abs(st["area"] / ref["area"] - 1) <= 1e-5
    if name == "zeros":                                               # degenerate triangles are kept, wound like the rest
        p = want_v[want_f]
        assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any()


def test_a_higher_min_weight_drops_lattice_points(hip_device):
    grid = tr.random_grid((9, 4, 3), 8, invalid=0.2)
    want_v, want_f, _ = tr.grid_mesh(grid, min_weight=2.0)
    _, (vertices, faces, _) = _extract(grid, hip_device, min_weight=2.0)
    assert 0 < len(want_f) < len(tr.grid_mesh(grid)[1])
    assert vertices.shape[0] == len(want_v) and np.array_equal(faces.cpu().numpy(), want_f)


def test_an_all_positive_grid_gives_empty_tensors(hip_device):
    grid = tr.random_grid((5, 4, 3), 7)
    grid["tsdf"] = np.abs(grid["tsdf"]) + 0.1
    _, (vertices, faces, colors) = _extract(grid, hip_device)
    assert vertices.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3) and faces.dtype == torch.int32


def test_a_capacity_below_the_count_writes_nothing_beyond_it(hip_device):
    """Through the C ABI: vertices and faces at or beyond the capacity are not written, the call returns LSR_OK."""
    dev = hip_device
    grid = tr.sphere_grid(12, seed=1)
    want_v, want_f, want_c = tr.grid_mesh(grid)
    case = dict(origin=grid["origin"], voxel_size=grid["voxel_size"], dims=grid["dims"])
    vol = _volume(case, dev, grid)
    lib = _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ws = torch.empty(lib.lsr_mesh_workspace_bytes(C.byref(vol._dims)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.call("lsr_mesh_count", C.byref(vol._dims), ptr(vol.tsdf), ptr(vol.weight), 1.0, ptr(ws), ptr(counts), stream)
    nv, nf = counts.tolist()
    assert (nv, nf) == (len(want_v), len(want_f))
    cap_v, cap_f = nv // 2, nf // 3
    vertices = torch.full((nv, 3), -7.0, device=dev)
    colors = torch.full((nv, 3), -7.0, device=dev)
    faces = torch.full((nf, 3), -7, dtype=torch.int32, device=dev)
    _lib.call("lsr_mesh_emit", C.byref(vol._dims), ptr(vol.tsdf), ptr(vol.weight), ptr(vol.color), 1.0, ptr(ws), ptr(counts), cap_v, cap_f,
              ptr(vertices), ptr(colors), ptr(faces), stream)
    torch.cuda.synchronize(dev)
    assert bool((vertices[cap_v:] == -7).all()) and bool((colors[cap_v:] == -7).all()) and bool((faces[cap_f:] == -7).all())
    assert np.array_equal(faces[:cap_f].cpu().numpy(), want_f[:cap_f])
    assert np.abs(vertices[:cap_v].cpu().numpy() - want_v[:cap_v]).max() < 1e-6


# ---- through the scene ----

def _scene(n, dev, seed=0):
    from latentsplat_amd import GaussianScene
    p = sref.make_params(n, 4, seed=seed)
    rng = np.random.default_rng(seed)
    p["xyz"] = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    p["scaling"] = np.log(rng.uniform(0.03, 0.12, (n, 3))).astype(np.float32)
    p["opacity"] = rng.uniform(0.0, 3.0, (n, 1)).astype(np.float32)
    return GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in p.items()}).to(dev)


def test_scene_extract_mesh_is_render_integrate_extract(hip_device, tmp_path):
    from latentsplat_amd.mesh import TSDFVolume, load_mesh_ply, save_mesh_ply
    dev = hip_device
    scene = _scene(2000, dev, seed=1)
    views = torch.from_numpy(nref.make_views(4, seed=5)).to(dev)
    H = W = 64
    voxel, trunc = 0.1, 0.4
    vertices, faces, colors = scene.extract_mesh(views, H, W, voxel, batch=3)
    with torch.no_grad():
        solid = scene._xyz[torch.sigmoid(scene._opacity).reshape(-1) > 0.5]
        lo, hi = (solid.min(dim=0).values - trunc).tolist(), (solid.max(dim=0).values + trunc).tolist()
        vol = TSDFVolume.from_bounds(lo, hi, voxel, device=dev)
        assert vol.trunc == pytest.approx(trunc)
        for at in (0, 3):
            color, _, mask, depth, _ = scene.render(views[at:at + 3], H, W)
            vol.integrate(depth, mask, views[at:at + 3], color=color)
        v2, f2, c2 = vol.extract_mesh()
    assert faces.shape[0] >= 1 and vertices.shape[0] >= 3
    assert np.array_equal(_bits(vertices), _bits(v2)) and torch.equal(faces, f2) and np.array_equal(_bits(colors), _bits(c2))
    path = tmp_path / "mesh.ply"
    save_mesh_ply(path, vertices, faces, colors)
    lv, lf, lc = load_mesh_ply(path)
    assert np.array_equal(lv.view(np.uint32), _bits(vertices)) and np.array_equal(lf, faces.cpu().numpy())
    assert np.array_equal(lc, np.clip(np.rint(colors.double().cpu().numpy() * 255), 0, 255).astype(np.uint8))
