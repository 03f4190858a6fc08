"""Mesh evaluation and cleanup on the MI355X: cloud_metrics against the float64 restatement of tests/mesh_eval_ref.py from
the bit-exact distances of tests/nn_ref.py, the area-weighted mesh sampler, connected components (csrc/mesh_components.hip)
against the numpy union-find, clean_mesh against its numpy restatement, and the whole chain on an analytic volume: a unit
sphere with a floater, extracted, sampled, scored, cleaned and scored again, directly and through tools/eval_mesh.py.

Bars.  Counts (precision, recall) are integers: equal.  Means: within 2^-40 relative (float64 sums of at most 10^5
non-negative terms in whatever order).  Labels: equal.  A sampled point: within 8 * 2^-24 of its face's largest coordinate
magnitude of the face's triangle (one rounding of a float64 convex combination to float32 is 2^-24 of the coordinate).
The share of a face of a quarter of the area among 100 000 draws: 0.25 +- 0.007, five sigma of the binomial.
End to end: tau = 0.1 is two voxels; the floater is at least 0.41 from the unit sphere; the largest nearest-neighbour
distance between two independent 20 000-point uniform samples of the unit sphere is 0.042 - 0.050, and marching
tetrahedra on an exact distance field misses the sphere by O(h^2 / R), about 10^-3: a factor of two below tau."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import mesh_eval_ref as ref
from tests import nn_ref
from tests import util

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, dev=DEV):
    return torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


# ---- cloud_metrics ----

PRED_N, GT_N = 5000, 70_001
TAUS = (0.05, 0.1, 0.3)


@functools.lru_cache(maxsize=None)
def _clouds():
    pred, gt = nn_ref.cloud("normal", PRED_N), nn_ref.cloud("normal", GT_N)
    to_gt = nn_ref.nn_ref_torch(pred, gt, DEV)[0]
    to_pred = nn_ref.nn_ref_torch(gt, pred, DEV, chunk=8192)[0]
    return pred, gt, to_gt, to_pred


def _check_metrics(got, want, show):
    for k in ref.COUNT_KEYS:
        assert got[k] == want[k], (show, k, got[k], want[k])
    for k in ref.MEAN_KEYS:
        rel = abs(got[k] - want[k]) / want[k]
        print(f"{show} {k:16s} {got[k]:.17g}  reference {want[k]:.17g}  relative {rel / ref.MEAN_BAR:.3f} x 2^-40")
        assert rel <= ref.MEAN_BAR, (show, k)


@pytest.mark.parametrize("max_dist", [None, 0.2])
def test_cloud_metrics_against_the_reference(hip_device, max_dist):
    from latentsplat_amd import cloud_metrics
    pred, gt, to_gt, to_pred = _clouds()
    got = cloud_metrics(_dev(pred), _dev(gt), thresholds=TAUS, max_dist=max_dist)
    want = ref.metrics_ref(to_gt, to_pred, TAUS, max_dist)
    _check_metrics(got, want, f"max_dist={max_dist}:")
    assert all(0 < c < PRED_N for c in got["precision_count"]) and all(0 < c < GT_N for c in got["recall_count"])
    assert got["max_dist"] == max_dist
    json.dumps(got)                                                 # plain numbers and lists


def test_max_dist_clips_the_means_only(hip_device):
    from latentsplat_amd import cloud_metrics
    pred, gt, to_gt, to_pred = _clouds()
    free = cloud_metrics(_dev(pred), _dev(gt), thresholds=TAUS)
    clipped = cloud_metrics(_dev(pred), _dev(gt), thresholds=TAUS, max_dist=0.2)
    assert float(np.sqrt(to_gt.max())) > 0.2 and float(np.sqrt(to_pred.max())) > 0.2
    for k in ("accuracy", "completeness", "chamfer", "accuracy_sq", "completeness_sq"):
        assert clipped[k] < free[k]
    for k in ref.COUNT_KEYS:
        assert clipped[k] == free[k]
    assert clipped["accuracy"] <= 0.2 and clipped["completeness"] <= 0.2


def test_gt_index_gives_the_same_numbers(hip_device):
    from latentsplat_amd import NearestIndex, cloud_metrics
    pred, gt, _, _ = _clouds()
    gt_dev = _dev(gt)
    index = NearestIndex(gt_dev)
    plain = cloud_metrics(_dev(pred), gt_dev, thresholds=TAUS, max_dist=0.5)
    for cloud in (pred, np.array(pred[:1000]) * np.float32(1.5)):   # one index, two meshes' worth of samples
        with_index = cloud_metrics(_dev(cloud), gt_dev, thresholds=TAUS, max_dist=0.5, gt_index=index)
        assert with_index == cloud_metrics(_dev(cloud), gt_dev, thresholds=TAUS, max_dist=0.5)
    assert cloud_metrics(_dev(pred), gt_dev, thresholds=TAUS, max_dist=0.5, gt_index=index) == plain
    with pytest.raises(_lib.LsrError, match="gt_index"):
        cloud_metrics(_dev(pred), gt_dev[:100], gt_index=index)


def test_fscore_is_zero_when_nothing_is_within_tau(hip_device):
    from latentsplat_amd import cloud_metrics
    pred, gt, _, _ = _clouds()
    far = cloud_metrics(_dev(pred + np.float32(100.0)), _dev(gt[:5000]), thresholds=(1.0,))
    assert far["precision"] == [0.0] and far["recall"] == [0.0] and far["fscore"] == [0.0] and far["accuracy"] > 100.0
    same = cloud_metrics(_dev(pred), _dev(pred), thresholds=(1e-6,))
    assert same["precision"] == [1.0] and same["recall"] == [1.0] and same["fscore"] == [1.0] and same["chamfer"] == 0.0
    for bad in (torch.zeros((0, 3), device=hip_device), torch.zeros((5, 2), device=hip_device)):
        with pytest.raises(_lib.LsrError):
            cloud_metrics(bad, _dev(gt[:10]))
        with pytest.raises(_lib.LsrError):
            cloud_metrics(_dev(gt[:10]), bad)


# ---- sample_mesh ----

def _random_mesh(nv, nf, seed, degenerate_every=0):
    rng = np.random.default_rng(seed)
    vertices = (rng.standard_normal((nv, 3)) * 3.0 + 10.0).astype(np.float32)
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    if degenerate_every:
        faces[::degenerate_every, 2] = faces[::degenerate_every, 1]      # a repeated corner: zero area
    return vertices, faces


def _triangle_residual(points, vertices, faces, face):
    """Distance (max norm) from every point to a point of its face's triangle, relative to the face's largest coordinate
    magnitude: least-squares barycentrics in float64, clamped into the triangle."""
    p = points.astype(np.float64)
    a, b, c = (vertices.astype(np.float64)[faces[face, k]] for k in range(3))
    e0, e1, r = b - a, c - a, p - a
    d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    r0, r1 = (r * e0).sum(1), (r * e1).sum(1)
    det = d00 * d11 - d01 * d01
    s, t = np.clip((d11 * r0 - d01 * r1) / det, 0.0, 1.0), np.clip((d00 * r1 - d01 * r0) / det, 0.0, 1.0)
    over = np.maximum(s + t, 1.0)
    s, t = s / over, t / over
    inside = a + s[:, None] * e0 + t[:, None] * e1
    scale = np.abs(np.stack([a, b, c], 1)).max(axis=(1, 2))
    return np.abs(p - inside).max(axis=1) / scale


def test_sampled_points_lie_in_their_faces(hip_device):
    from latentsplat_amd import sample_mesh
    vertices, faces = _random_mesh(300, 500, 1)
    m = 50_000
    points, face = sample_mesh(_dev(vertices), _dev(faces), m, torch.Generator().manual_seed(3))
    assert points.dtype == torch.float32 and tuple(points.shape) == (m, 3) and face.dtype == torch.int32 and tuple(face.shape) == (m,)
    face_np = face.cpu().numpy()
    assert face_np.min() >= 0 and face_np.max() < 500
    res = _triangle_residual(points.cpu().numpy(), vertices, faces, face_np)
    print(f"worst residual {res.max() / 2.0 ** -24:.2f} x 2^-24 of the face's largest coordinate (bar 8)")
    assert res.max() <= 8.0 * 2.0 ** -24
    # in proportion to area: the drawn share of every face against its share of the area, five sigma of the binomial
    tri = vertices.astype(np.float64)[faces]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    share = area / area.sum()
    drawn = np.bincount(face_np, minlength=500) / m
    assert (np.abs(drawn - share) <= 5.0 * np.sqrt(share * (1.0 - share) / m) + 1.0 / m).all()


def test_the_same_generator_state_gives_the_same_bits(hip_device):
    from latentsplat_amd import sample_mesh
    vertices, faces = (_dev(a) for a in _random_mesh(300, 500, 1))
    first = sample_mesh(vertices, faces, 10_001, torch.Generator().manual_seed(7))
    second = sample_mesh(vertices, faces, 10_001, torch.Generator().manual_seed(7))
    other = sample_mesh(vertices, faces, 10_001, torch.Generator().manual_seed(8))
    assert np.array_equal(_bits(first[0]), _bits(second[0])) and torch.equal(first[1], second[1])
    assert not np.array_equal(_bits(first[0]), _bits(other[0]))
    on_device = torch.Generator(device=hip_device).manual_seed(7)
    a = sample_mesh(vertices, faces, 1000, on_device)
    b = sample_mesh(vertices, faces, 1000, torch.Generator(device=hip_device).manual_seed(7))
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    empty = sample_mesh(vertices, faces, 0)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0,)


def test_a_zero_area_face_is_never_drawn(hip_device):
    from latentsplat_amd import sample_mesh
    vertices, faces = _random_mesh(300, 501, 2, degenerate_every=3)
    _, face = sample_mesh(_dev(vertices), _dev(faces), 30_000, torch.Generator().manual_seed(1))
    face = face.cpu().numpy()
    assert (face % 3 != 0).all() and len(np.unique(face)) > 300
    flat = np.zeros((4, 3), np.float32)
    flat[:, 0] = [0, 1, 2, 3]                                       # four vertices on a line: no area at all
    with pytest.raises(_lib.LsrError, match="area"):
        sample_mesh(_dev(flat), _dev(np.array([[0, 1, 2], [1, 2, 3]], np.int32)), 10)
    with pytest.raises(_lib.LsrError):
        sample_mesh(_dev(vertices), _dev(np.array([[0, 1, 300]], np.int32)), 10)


def test_two_triangles_of_areas_one_to_three(hip_device):
    from latentsplat_amd import sample_mesh
    vertices = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 0, 1], [8, 0, 1], [5, 2, 1]], np.float32)      # areas 1 and 3
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    m = 100_000
    points, face = sample_mesh(_dev(vertices), _dev(faces), m, torch.Generator().manual_seed(11))
    share = float((face == 0).sum()) / m
    print(f"first-face share {share:.5f} (0.25 +- 0.007)")
    assert abs(share - 0.25) <= 0.007
    p = points.cpu().numpy()
    assert (p[face.cpu().numpy() == 0, 2] == 0).all() and (p[face.cpu().numpy() == 1, 2] == 1).all()


# ---- connected components ----

def _labels(faces, nv):
    from latentsplat_amd import mesh_components
    labels, rounds = mesh_components(_dev(np.asarray(faces, np.int32).reshape(-1, 3)), nv, return_rounds=True)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (nv,)
    return labels.cpu().numpy(), rounds


def test_two_tetrahedra_with_interleaved_numbers(hip_device):
    _, faces = ref.two_tetrahedra()
    labels, _ = _labels(faces, 8)
    assert labels.tolist() == [0, 1, 0, 1, 0, 1, 0, 1] and np.array_equal(labels, ref.components_ref(faces, 8))


def test_a_permuted_strip_converges_far_below_the_cap(hip_device):
    nv = 70_001
    _, faces = ref.strip(nv, 4)
    labels, rounds = _labels(faces, nv)
    print(f"strip of {nv} vertices, permuted: {rounds} rounds (cap {_lib.MESH_COMPONENT_ROUNDS})")
    assert not labels.any() and np.array_equal(labels, ref.components_ref(faces, nv))
    assert rounds <= 40
    again, _ = _labels(faces, nv)
    assert np.array_equal(labels, again)


def test_a_grid_and_isolated_vertices(hip_device):
    vertices, faces = ref.grid_mesh(64, isolated=100)
    nv = len(vertices)
    labels, _ = _labels(faces, nv)
    assert np.array_equal(labels, ref.components_ref(faces, nv))
    assert not labels[:4096].any() and np.array_equal(labels[4096:], np.arange(4096, nv))


def test_repeated_corners_and_no_faces(hip_device):
    faces = np.array([[2, 2, 5], [3, 3, 3], [7, 4, 7], [4, 4, 1]], np.int32)
    labels, _ = _labels(faces, 9)
    assert labels.tolist() == [0, 1, 2, 3, 1, 2, 6, 1, 8] and np.array_equal(labels, ref.components_ref(faces, 9))
    labels, rounds = _labels(np.zeros((0, 3), np.int32), 300)
    assert np.array_equal(labels, np.arange(300)) and rounds == 0
    labels, _ = _labels(np.zeros((0, 3), np.int32), 0)
    assert labels.shape == (0,)


@pytest.mark.parametrize("nv", [63, 64, 65, 255, 256, 257])
def test_vertex_counts_around_a_wavefront_and_a_workgroup(hip_device, nv):
    """Several strips and fans over shuffled numbers, with some vertices left out."""
    rng = np.random.default_rng(nv)
    perm = rng.permutation(nv)
    cut = sorted(rng.choice(np.arange(3, nv - 3), 4, replace=False).tolist())
    faces = []
    for lo, hi in zip([0] + cut, cut + [nv - 2]):
        ids = perm[lo:hi]
        faces += [[ids[i], ids[i + 1], ids[i + 2]] for i in range(len(ids) - 2)]
    faces = np.array(faces, np.int32)[rng.permutation(len(faces))]
    labels, _ = _labels(faces, nv)
    want = ref.components_ref(faces, nv)
    assert np.array_equal(labels, want) and len(set(want.tolist())) >= 5


def test_a_corner_out_of_range_is_refused(hip_device):
    from latentsplat_amd import clean_mesh, mesh_components
    _, faces = ref.two_tetrahedra()
    for bad in (8, -1, 2 ** 31 - 1):
        f = faces.copy()
        f[5, 1] = bad
        with pytest.raises(_lib.LsrError, match="outside"):
            mesh_components(_dev(f), 8)
        with pytest.raises(_lib.LsrError, match="outside"):
            clean_mesh(torch.zeros((8, 3), device=hip_device), _dev(f), keep_largest=1)
    for bad in (torch.zeros((4, 2), dtype=torch.int32, device=hip_device), torch.zeros((4, 3), dtype=torch.int64, device=hip_device)):
        with pytest.raises(_lib.LsrError):
            mesh_components(bad, 8)


# ---- clean_mesh ----

SIZES = [5, 1, 9, 5, 2, 9, 1]


@pytest.mark.parametrize("kw", [dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=3), dict(keep_largest=4), dict(min_faces=5),
                                dict(min_faces=2), dict(keep_largest=3, min_faces=6), dict(keep_largest=100), dict(keep_largest=0),
                                dict(min_faces=10), dict()], ids=str)
def test_clean_mesh_against_the_reference(hip_device, kw):
    from latentsplat_amd import clean_mesh
    vertices, faces, fan_labels = ref.blobs(SIZES, 6)
    vertices = np.concatenate([vertices, np.full((3, 3), -7.0, np.float32)])      # and three vertices no face names
    colors = np.random.default_rng(1).uniform(0, 1, vertices.shape).astype(np.float32)
    v, f, c, info = clean_mesh(_dev(vertices), _dev(faces), _dev(colors), **kw)
    want_v, want_f, keep_v, want_info = ref.clean_ref(vertices, faces, ref.components_ref(faces, len(vertices)), **kw)
    assert info == want_info and sum(SIZES) == info["faces_kept"] + info["faces_dropped"]
    assert info["vertices_kept"] + info["vertices_dropped"] == len(vertices) and info["components"] == len(SIZES)
    assert f.dtype == torch.int32 and v.dtype == torch.float32
    assert np.array_equal(_bits(v), _bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)      # order preserved
    assert np.array_equal(_bits(c), _bits(colors[keep_v]))
    # the remapped faces index the same coordinates as before
    kept_faces = faces[keep_v[faces[:, 0]]]
    assert np.array_equal(_bits(v.cpu().numpy()[f.cpu().numpy()]), _bits(vertices[kept_faces]))
    if kw == dict(keep_largest=1):                                  # two components of 9 faces: the lower label wins
        assert set(ref.components_ref(faces, len(vertices))[keep_v].tolist()) == {min(fan_labels[2], fan_labels[5])}
    if kw == dict(keep_largest=3):                                  # both of 9, then two of 5 tie: the lower label
        assert min(fan_labels[0], fan_labels[3]) in ref.components_ref(faces, len(vertices))[keep_v]
    without = clean_mesh(_dev(vertices), _dev(faces), None, **kw)
    assert without[2] is None and torch.equal(without[1], f)


# ---- end to end: a unit sphere and a floater ----

SAMPLES, TAU = 20_000, 0.1


@functools.lru_cache(maxsize=None)
def _sphere_case():
    from latentsplat_amd import TSDFVolume, clean_mesh, cloud_metrics, sample_mesh
    vol = TSDFVolume(ref.SPHERE_ORIGIN, ref.SPHERE_VOXEL, ref.SPHERE_DIMS, device=DEV)
    vol.tsdf.copy_(_dev(ref.two_sphere_tsdf(vol.trunc)))
    vol.weight.fill_(1.0)
    vol.color.fill_(0.5)
    vertices, faces, colors = vol.extract_mesh()
    gt = _dev(ref.unit_sphere_samples(SAMPLES, 2))
    raw = cloud_metrics(sample_mesh(vertices, faces, SAMPLES, torch.Generator().manual_seed(0))[0], gt, thresholds=(TAU,))
    cv, cf, cc, info = clean_mesh(vertices, faces, colors, keep_largest=1)
    cleaned = cloud_metrics(sample_mesh(cv, cf, SAMPLES, torch.Generator().manual_seed(0))[0], gt, thresholds=(TAU,))
    return dict(mesh=(vertices, faces, colors), gt=gt, raw=raw, clean_mesh=(cv, cf, cc), info=info, cleaned=cleaned)


def test_a_floater_costs_precision_and_cleanup_restores_it(hip_device):
    from latentsplat_amd import mesh_components
    case = _sphere_case()
    vertices, faces, _ = case["mesh"]
    raw, cleaned, info = case["raw"], case["cleaned"], case["info"]
    labels = mesh_components(faces, vertices.shape[0]).cpu().numpy()
    print(f"mesh: {vertices.shape[0]} vertices, {faces.shape[0]} faces, {len(np.unique(labels))} components; cleanup {info}")
    print(f"before: precision {raw['precision'][0]:.5f} recall {raw['recall'][0]:.5f} accuracy {raw['accuracy']:.5f}")
    print(f"after:  precision {cleaned['precision'][0]:.5f} recall {cleaned['recall'][0]:.5f} accuracy {cleaned['accuracy']:.5f}")
    assert info["components"] == 2 and info["components_kept"] == 1 and 0 < info["faces_dropped"] < info["faces_kept"]
    assert raw["precision"][0] < 1.0 and raw["precision"][0] > 0.9          # the floater draws about 2 % of the samples
    assert cleaned["precision"][0] == 1.0 and cleaned["recall"][0] == 1.0 and cleaned["fscore"][0] == 1.0
    assert cleaned["accuracy"] < 0.05
    cv = case["clean_mesh"][0].double().norm(dim=1)
    assert float((cv - 1.0).abs().max()) < 0.01                             # what is left is the unit sphere


def _write_points(path, points):
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(points)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
    path.write_bytes(head.encode() + np.ascontiguousarray(points, "<f4").tobytes())


def test_eval_tool(hip_device, tmp_path):
    from latentsplat_amd import save_mesh_ply
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import eval_mesh
    finally:
        sys.path.pop(0)
    case = _sphere_case()
    mesh, gt = tmp_path / "mesh.ply", tmp_path / "gt.ply"
    save_mesh_ply(mesh, *case["mesh"])
    _write_points(gt, case["gt"].cpu().numpy())
    common = [str(mesh), "--gt", str(gt), "--samples", str(SAMPLES), "--thresholds", str(TAU), "--seed", "0"]
    raw = eval_mesh.main(common + ["--out", str(tmp_path / "raw.json")])
    assert json.load(open(tmp_path / "raw.json")) == raw and raw["gt_kind"] == "points" and "cleanup" not in raw
    cleaned = eval_mesh.main(common + ["--keep-largest", "1", "--out", str(tmp_path / "out" / "cleaned.json")])
    assert json.load(open(tmp_path / "out" / "cleaned.json")) == cleaned
    for got, want in ((raw, case["raw"]), (cleaned, case["cleaned"])):
        for k, v in want.items():
            assert got[k] == v, k
    assert cleaned["cleanup"] == dict(keep_largest=1, min_faces=None, **case["info"])
    assert cleaned["faces"] == case["info"]["faces_kept"] and raw["faces"] == raw["faces_in"] == cleaned["faces_in"]
    # a mesh as the ground truth is sampled too: the cleaned mesh against itself
    save_mesh_ply(gt, case["clean_mesh"][0], case["clean_mesh"][1])
    itself = eval_mesh.main([str(mesh), "--gt", str(gt), "--samples", str(SAMPLES), "--thresholds", str(TAU), "--keep-largest", "1",
                             "--out", str(tmp_path / "itself.json")])
    assert itself["gt_kind"] == "mesh" and itself["num_gt"] == SAMPLES and itself["precision"] == [1.0] and itself["recall"] == [1.0]


def test_mesh_tool_cleanup_flags(hip_device, tmp_path):
    """tools/mesh_ply.py with --keep-largest / --min-faces writes clean_mesh of what it writes without them."""
    from latentsplat_amd import clean_mesh, load_mesh_ply
    from tests import scene_params_ref as sref
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import mesh_ply
    finally:
        sys.path.pop(0)
    from latentsplat_amd import GaussianScene
    scene = tmp_path / "point_cloud.ply"
    p = sref.make_params(2000, 4, seed=1)                           # the solid blob of tests/test_mesh_gpu.py
    rng = np.random.default_rng(1)
    p["xyz"] = rng.uniform(-1.2, 1.2, (2000, 3)).astype(np.float32)
    p["scaling"] = np.log(rng.uniform(0.03, 0.12, (2000, 3))).astype(np.float32)
    p["opacity"] = rng.uniform(0.0, 3.0, (2000, 1)).astype(np.float32)
    GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in p.items()}).to(hip_device).save_ply(scene)
    common = [str(scene), "--views", "6", "--size", "64", "--voxel-size", "0.06"]
    plain = mesh_ply.main(common + ["--out", str(tmp_path / "plain.ply")])
    kept = mesh_ply.main(common + ["--out", str(tmp_path / "kept.ply"), "--keep-largest", "1", "--min-faces", "2"])
    assert "cleanup" not in plain and plain["faces"] > 0
    v, f, c = load_mesh_ply(tmp_path / "plain.ply")
    want = clean_mesh(_dev(v), _dev(f), None, keep_largest=1, min_faces=2)
    got_v, got_f, got_c = load_mesh_ply(tmp_path / "kept.ply")
    assert np.array_equal(_bits(got_v), _bits(want[0])) and np.array_equal(got_f, want[1].cpu().numpy())
    assert np.array_equal(got_c, c[_kept_rows(v, f, want)])
    assert kept["cleanup"] == dict(keep_largest=1, min_faces=2, **want[3]) and kept["faces"] == want[3]["faces_kept"] <= plain["faces"]


def _kept_rows(v, f, cleaned):
    """The rows of the input's vertices that clean_mesh kept (labels again, from the reference)."""
    labels = ref.components_ref(f, len(v))
    _, _, keep_v, _ = ref.clean_ref(v, f, labels, keep_largest=1, min_faces=2)
    assert int(keep_v.sum()) == cleaned[0].shape[0]
    return keep_v
