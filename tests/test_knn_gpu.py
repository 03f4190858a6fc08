"""The exact three-nearest-neighbour search on the MI355X (lsr_knn3, csrc/knn.hip) against the float64 brute force of
tests/knn_ref.py (run on the card), GaussianScene.from_point_cloud (also from a points file read onto the card), and the
fitting tool started from points.

The bar for every element of dist2 and mean_dist2 is |got - want| <= 16 * 2^-24 * want (tests/knn_ref.py BAR): each
float32 difference is rounded once, squaring doubles that, three non-negative terms are added, the mean adds two
additions and a division — at most about 8 * 2^-24 — and the bar is twice that.  Exact zeros must be exact.  Nothing
is exempt.

Sizes: the constants of csrc/knn.hip are kQueries = 64 queries per search workgroup (one wavefront), kChunk = 128 sorted
points per chunk (one box, one LDS stage) and kGroup = 64 chunks per second-level box (= lanes of one ballot); groups are
tested in blocks of 64.  4 and 5 are the smallest legal clouds (a wave with fewer valid lanes than neighbours to find);
63 / 64 / 65 straddle a wavefront, 127 / 128 / 129 a chunk and 255 / 256 / 257 two (129 and 257: a last chunk of one
point, which finds all its neighbours elsewhere); 1000 is eight chunks in one group; 70 001 is 547 chunks in nine
groups: more than one level of the box table, and more chunks than a ballot has lanes.  Only beyond kChunk * kGroup * 64
= 524 288 points is there a second block of groups: 90^3 = 729 000 (an integer lattice, whose exact answer costs O(n))
and 600 001 clustered points (a seeded sample of queries against the brute force) walk it."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import knn_ref as ref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu

QUERIES, CHUNK, GROUP = 64, 128, 64
BIG = 70_001
SIZES = [4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, BIG]
LATTICE_SIDE, SAMPLED = 90, 600_001                          # beyond one block of 64 groups
assert BIG > 4 * CHUNK * GROUP and BIG > CHUNK * 256 and 1000 > 3 * CHUNK and BIG % CHUNK != 0 and BIG % QUERIES != 0
assert min(LATTICE_SIDE ** 3, SAMPLED) > CHUNK * GROUP * 64
assert all(s in SIZES for s in (QUERIES - 1, QUERIES, QUERIES + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1))
FLOOR = 2.0 ** -20
MARGIN = 4.0


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _points(name, n, dev):
    return torch.from_numpy(ref.cloud(name, n).copy()).to(dev)


@functools.lru_cache(maxsize=None)
def _kernel(name, n):
    """(dist2, index, mean) of the kernel as numpy arrays, once per case."""
    from latentsplat_amd import knn3, mean_knn_dist2
    p = _points(name, n, torch.device("cuda:0"))
    dist2, index = knn3(p)
    mean = mean_knn_dist2(p)
    return dist2.cpu().numpy(), index.cpu().numpy(), mean.cpu().numpy()


def _worst(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want > 0, np.abs(got.astype(np.float64) - want) / want, np.where(got == want, 0.0, np.inf))
    return float(rel.max()) / 2.0 ** -24


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ref.NAMES)
def test_distances(hip_device, name, n):
    want_d, _, want_mean = ref.reference(name, n, hip_device)
    dist2, _, mean = _kernel(name, n)
    assert dist2.shape == (n, 3) and dist2.dtype == np.float32 and mean.shape == (n,) and mean.dtype == np.float32
    print(f"{name} n={n}: worst dist2 {_worst(dist2, want_d):.2f} x 2^-24, worst mean {_worst(mean, want_mean):.2f} x 2^-24 (bar 16)")
    assert (np.diff(dist2, axis=1) >= 0).all()
    assert ref.within_bar(dist2, want_d).all()
    assert ref.within_bar(mean, want_mean).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ref.NAMES)
def test_indices(hip_device, name, n):
    _, want_i, _ = ref.reference(name, n, hip_device)
    dist2, index, _ = _kernel(name, n)
    assert index.shape == (n, 3) and index.dtype == np.int32
    assert (index >= 0).all() and (index < n).all()
    assert (index != np.arange(n)[:, None]).all()
    assert (index[:, 0] != index[:, 1]).all() and (index[:, 0] != index[:, 2]).all() and (index[:, 1] != index[:, 2]).all()
    assert ref.within_bar(dist2, ref.pair_dist2(ref.cloud(name, n), index)).all()
    if name in ref.EXACT_INDEX_NAMES:
        assert np.array_equal(index, want_i)


def test_lattice_beyond_one_block_of_groups(hip_device):
    """729 000 sites of an integer lattice, shuffled: every distance is 1 and the indices are the three lowest-indexed
    axis neighbours (tests/knn_ref.py lattice_neighbours)."""
    from latentsplat_amd import knn3, mean_knn_dist2
    n = LATTICE_SIDE ** 3
    i = np.arange(n)
    sites = np.stack([i % LATTICE_SIDE, (i // LATTICE_SIDE) % LATTICE_SIDE, i // LATTICE_SIDE ** 2], 1)
    cloud = sites[np.random.default_rng(n).permutation(n)].astype(np.float32)
    p = torch.from_numpy(cloud).to(hip_device)
    dist2, index = knn3(p)
    assert (dist2 == 1.0).all() and (mean_knn_dist2(p) == 1.0).all()
    assert np.array_equal(index.cpu().numpy(), ref.lattice_neighbours(cloud))


def test_sampled_queries_beyond_one_block_of_groups(hip_device):
    """600 001 clustered points; 2048 seeded queries (the first and the last wave's among them) against the brute force."""
    from latentsplat_amd import knn3, mean_knn_dist2
    n = SAMPLED
    cloud = ref.cloud("clusters", n)
    p = torch.from_numpy(cloud.copy()).to(hip_device)
    dist2, index = (t.cpu().numpy() for t in knn3(p))
    mean = mean_knn_dist2(p).cpu().numpy()
    who = np.unique(np.concatenate([np.random.default_rng(7).integers(0, n, 2048), [0, n - 1]]))
    want_d, _, want_mean = ref.knn3_ref(cloud, hip_device, chunk=256, queries=who)
    print(f"clusters n={n}, {who.size} queries: worst dist2 {_worst(dist2[who], want_d):.2f} x 2^-24, worst mean {_worst(mean[who], want_mean):.2f} x 2^-24")
    assert ref.within_bar(dist2[who], want_d).all() and ref.within_bar(mean[who], want_mean).all()
    # every row: ordered, in range, not itself, distinct, and the distances are those of the indices
    assert (np.diff(dist2, axis=1) >= 0).all() and (index >= 0).all() and (index < n).all() and (index != np.arange(n)[:, None]).all()
    assert (index[:, 0] != index[:, 1]).all() and (index[:, 0] != index[:, 2]).all() and (index[:, 1] != index[:, 2]).all()
    assert ref.within_bar(dist2, ref.pair_dist2(cloud, index)).all()


def _all_three(p):
    from latentsplat_amd import knn
    return knn._run(p, True, True, True)


@pytest.mark.parametrize("name, n", [("clusters", BIG), ("lattice", BIG), ("dup", 1000), ("normal", 5)])
def test_two_calls_give_the_same_bits(hip_device, name, n):
    p = _points(name, n, hip_device)
    first, second = _all_three(p), _all_three(p)
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name, n", [("clusters", BIG), ("lattice", 1000), ("outlier", 257)])
def test_each_output_alone(hip_device, name, n):
    from latentsplat_amd import knn
    p = _points(name, n, hip_device)
    full = _all_three(p)
    for k in range(3):
        want = [False] * 3
        want[k] = True
        alone = knn._run(p, *want)
        assert [t is not None for t in alone] == want
        assert np.array_equal(_bits(alone[k]), _bits(full[k]))


def test_side_stream(hip_device):
    dev = hip_device
    p = _points("clusters", BIG, dev)
    main = _all_three(p)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        other = _all_three(p)
    side.synchronize()
    for a, b in zip(main, other):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n", [1000, BIG])
def test_non_contiguous_input(hip_device, n):
    from latentsplat_amd import knn3, mean_knn_dist2
    wide = torch.zeros((n, 4), device=hip_device)
    wide[:, 1:] = _points("clusters", n, hip_device)
    view = wide[:, 1:]
    assert not view.is_contiguous()
    got, want = knn3(view), knn3(view.contiguous())
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
    assert np.array_equal(_bits(mean_knn_dist2(view)), _bits(mean_knn_dist2(view.contiguous())))


def test_wrappers_refuse_what_they_cannot_take(hip_device):
    from latentsplat_amd import knn3
    for bad in (torch.zeros((10, 2), device=hip_device), torch.zeros((3, 3), device=hip_device),
                torch.zeros((10, 3), device=hip_device, dtype=torch.float64)):
        with pytest.raises(_lib.LsrError):
            knn3(bad)
    d, i = knn3(torch.zeros((0, 3), device=hip_device))
    assert tuple(d.shape) == (0, 3) and tuple(i.shape) == (0, 3)


# ---- GaussianScene.from_point_cloud ----

C0 = 0.28209479177387814


def _held(name, got, want, stock, show):
    """The bar of tests/test_density_gpu.py: within 4 x the float32 torch-CPU composition's error against float64, with a
    floor of 2^-20 of the quantity's scale."""
    got, want, stock = (np.asarray(a, np.float64) for a in (got, want, stock))
    scale = float(np.abs(want).max())
    err, err_stock = float(np.abs(got - want).max()), float(np.abs(stock - want).max())
    bar = max(MARGIN * err_stock, FLOOR * scale)
    print(f"{show} {name:10s} kernel {err:.3e}  composition {err_stock:.3e}  bar {bar:.3e}  ({want.size} elements)")
    assert err <= bar, (show, name, err, err_stock, bar)


@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("n", [1000, BIG])
def test_from_point_cloud(hip_device, n, degree):
    from latentsplat_amd import GaussianScene
    dev = hip_device
    cloud = ref.cloud("clusters", n)
    colors = np.random.default_rng(n + degree).uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    p = torch.from_numpy(cloud.copy()).to(dev)
    scene = GaussianScene.from_point_cloud(p, torch.from_numpy(colors).to(dev), sh_degree=degree)
    K = (degree + 1) ** 2
    assert scene.num_gaussians == n and scene.max_sh_degree == degree and scene.active_sh_degree == 0
    shapes = dict(_xyz=(n, 3), _features_dc=(n, 1, 3), _features_rest=(n, K - 1, 3), _opacity=(n, 1), _scaling=(n, 3), _rotation=(n, 4))
    for k, s in shapes.items():
        t = getattr(scene, k)
        assert tuple(t.shape) == s and t.dtype == torch.float32 and t.device == p.device and t.requires_grad, k
    assert np.array_equal(_bits(scene._xyz), _bits(cloud))
    rot = scene._rotation.detach().cpu().numpy()
    assert (rot[:, 0] == 1.0).all() and not rot[:, 1:].any() and not scene._features_rest.detach().any()
    assert (scene._opacity.detach().cpu().numpy() == np.float32(math.log(0.1 / 0.9))).all()
    # the float64 formula and the float32 torch-CPU composition of the published lines, both from the reference's distances
    _, _, mean64 = ref.reference("clusters", n, dev)
    want_scaling = np.repeat(np.log(np.sqrt(np.maximum(mean64, 1e-7)))[:, None], 3, 1)
    mean32 = torch.from_numpy(mean64.astype(np.float32))
    stock_scaling = torch.log(torch.sqrt(torch.clamp_min(mean32, 0.0000001)))[..., None].repeat(1, 3).numpy()
    _held("_scaling", scene._scaling.detach().cpu().numpy(), want_scaling, stock_scaling, f"n={n} degree={degree}:")
    want_dc = (colors.astype(np.float64) - 0.5) / C0
    stock_dc = ((torch.from_numpy(colors) - 0.5) / C0).numpy()
    _held("_features_dc", scene._features_dc.detach().cpu().numpy()[:, 0, :], want_dc, stock_dc, f"n={n} degree={degree}:")
    grey = GaussianScene.from_point_cloud(p, None, sh_degree=degree)
    assert not grey._features_dc.detach().any() and np.array_equal(_bits(grey._scaling), _bits(scene._scaling))


def test_from_point_cloud_edge_cases(hip_device):
    from latentsplat_amd import GaussianScene
    dev = hip_device
    same = GaussianScene.from_point_cloud(_points("same", 1000, dev))
    got = same._scaling.detach().cpu().numpy()
    stock = torch.log(torch.sqrt(torch.clamp_min(torch.zeros(1000), 0.0000001)))[..., None].repeat(1, 3).numpy()
    _held("_scaling", got, np.full((1000, 3), 0.5 * math.log(1e-7)), stock, "same:")
    assert (_bits(got) == _bits(got)[0, 0]).all()
    assert same.max_sh_degree == 3
    bad = _points("normal", 1000, dev)
    bad[517, 1] = float("nan")
    with pytest.raises(_lib.LsrError, match="non-finite"):
        GaussianScene.from_point_cloud(bad)
    bad[517, 1] = float("inf")
    with pytest.raises(_lib.LsrError, match="non-finite"):
        GaussianScene.from_point_cloud(bad)
    for kw in (dict(sh_degree=5), dict(sh_degree=-1), dict(initial_opacity=1.0), dict(min_dist2=0.0)):
        with pytest.raises(_lib.LsrError):
            GaussianScene.from_point_cloud(_points("normal", 64, dev), **kw)
    with pytest.raises(_lib.LsrError):
        GaussianScene.from_point_cloud(_points("normal", 64, dev), torch.zeros((63, 3), device=dev))


def test_points_file_to_scene(hip_device, tmp_path):
    """A storePly-layout file (x y z nx ny nz red green blue) read straight onto the card and into a scene."""
    from latentsplat_amd import GaussianScene, load_points_ply
    n = 3001
    cloud = ref.cloud("clusters", n)
    rows = np.zeros(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                              ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rgb = np.random.default_rng(1).integers(0, 256, (n, 3))
    for k, name in enumerate("xyz"):
        rows[name] = cloud[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rows[name] = rgb[:, k]
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    head += "".join(f"property {'uchar' if t == 'u1' else 'float'} {name}\n" for name, t in (("x", "f4"), ("y", "f4"), ("z", "f4"),
                    ("nx", "f4"), ("ny", "f4"), ("nz", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")))
    path = tmp_path / "points3D.ply"
    path.write_bytes((head + "end_header\n").encode() + rows.tobytes())
    points, colors = load_points_ply(path, hip_device)
    assert points.device == colors.device == torch.zeros(1, device=hip_device).device
    assert np.array_equal(_bits(points), _bits(cloud))
    assert np.array_equal(colors.cpu().numpy(), rgb.astype(np.float32) / np.float32(255.0))
    scene = GaussianScene.from_point_cloud(points, colors, sh_degree=1)
    direct = GaussianScene.from_point_cloud(torch.from_numpy(cloud.copy()).to(hip_device), colors, sh_degree=1)
    assert scene.num_gaussians == n and np.array_equal(_bits(scene.rows()), _bits(direct.rows()))
    path.write_bytes((head.replace("vertex %d" % n, "vertex 0") + "end_header\n").encode())
    points, colors = load_points_ply(path, hip_device)
    assert tuple(points.shape) == (0, 3) and tuple(colors.shape) == (0, 3) and points.is_cuda


G, W, VIEWS = 2000, 64, 2


def test_scene_from_points_renders_and_trains(hip_device):
    """The points of a synthetic scene in front of its cameras: the scene renders finite images and the optimizer and the
    density control take it as they take a loaded one."""
    from latentsplat_amd import DensityControl, GaussianScene, SceneAdam
    from latentsplat_amd.rasterizer import build_view_table
    dev = hip_device
    sc = util.make_scene(G, image_size=W, views=VIEWS, color_sh_degree=1, feature_channels=None)
    views = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                             torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False).detach()
    colors = torch.rand((G, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    scene = GaussianScene.from_point_cloud(sc.means.to(dev).float(), colors, sh_degree=2)
    with torch.no_grad():
        target = scene.render(views, W, W)[0]
    assert tuple(target.shape) == (VIEWS, 3, W, W) and torch.isfinite(target).all() and float(target.std()) > 0
    opt = SceneAdam.for_scene(scene, extent=1.0)
    control = DensityControl(scene)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((VIEWS, scene.num_gaussians, 3), device=dev, requires_grad=True)
        color, _, _, _, radii = scene.render(views, W, W, means2D=means2D)
        loss = (color - 0.5).abs().mean()
        loss.backward()
        opt.step()
        control.update(means2D.grad, radii)
        losses.append(float(loss.detach()))
    counts = control.densify_and_prune(opt, 1e-7, 0.005, 1.0, 0)
    assert counts["n_in"] == G and counts["n_out"] == scene.num_gaussians > 0
    assert np.isfinite(losses).all() and all(torch.isfinite(p).all() for p in scene.parameters())
    with torch.no_grad():
        assert torch.isfinite(scene.render(views, W, W)[0]).all()


def test_fit_tool_from_points(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, G, W, VIEWS)
    out = tmp_path / "fit"
    res = fit_ply.main([str(path), "--out", str(out), "--views", "3", "--size", "48", "--steps", "20", "--drop", "0.5",
                        "--from-points", "--sh-degree-interval", "5", "--densify-interval", "5", "--densify-until", "6"])
    print("fit:", {k: v for k, v in res.items() if k != "densify_events"})
    assert json.load(open(out / "fit.json")) == res
    assert res["from_points"] is True and res["active_sh_degree_last"] == 1 and res["sh_degree"] == 1
    assert res["gaussians_first"] == G                       # --drop is ignored
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
    fitted = GaussianScene.from_ply(out / "point_cloud.ply", hip_device)
    assert fitted.num_gaussians == res["gaussians_last"]
    assert all(torch.isfinite(p).all() for p in fitted.parameters())
