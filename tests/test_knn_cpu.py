"""The point-cloud initialisation without a GPU: the reference of tests/knn_ref.py against a k-d tree, the host side of
lsr_knn3 (sizing, every argument check: all of them return before any GPU work), the refusal of CPU tensors, and the
host reader of point cloud files (lsr_ply_read_points_header / lsr_ply_read_points) through load_points_ply."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import knn_ref as ref

SIZES = [4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 70_001]      # those of tests/test_knn_gpu.py


@pytest.mark.parametrize("name", ["normal", "clusters"])
def test_reference_matches_a_kd_tree(name):
    spatial = pytest.importorskip("scipy.spatial")
    n = 5001
    p = ref.cloud(name, n)
    dist2, index, mean = ref.reference(name, n)
    d4, _ = spatial.cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=4)
    tree = np.sort(d4, axis=1)[:, 1:] ** 2            # the query point itself is one of the zeros: drop one
    assert np.allclose(dist2, tree, rtol=1e-9, atol=0.0)
    assert (np.diff(dist2, axis=1) >= 0).all()
    assert (index != np.arange(n)[:, None]).all() and (index >= 0).all() and (index < n).all()
    assert np.array_equal(ref.pair_dist2(p, index), dist2)
    assert np.allclose(mean, tree.sum(1) / 3.0, rtol=1e-9, atol=0.0)


def test_reference_breaks_ties_toward_the_lower_index():
    p = np.zeros((6, 3), np.float32)
    p[5] = 1.0
    dist2, index, _ = ref.knn3_ref(p)
    assert index[:5].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]] and not dist2[:5].any()
    assert index[5].tolist() == [0, 1, 2] and (dist2[5] == 3.0).all()


def test_lattice_reference_matches_the_brute_force():
    i = np.arange(216)
    cloud = np.stack([i % 6, (i // 6) % 6, i // 36], 1)[np.random.default_rng(0).permutation(216)].astype(np.float32)
    dist2, index, _ = ref.knn3_ref(cloud)
    assert (dist2 == 1.0).all() and np.array_equal(index, ref.lattice_neighbours(cloud))
    sub = ref.knn3_ref(cloud, queries=[5, 100, 215])
    assert np.array_equal(sub[1], index[[5, 100, 215]]) and np.array_equal(sub[0], dist2[[5, 100, 215]])


def test_workspace_bytes():
    lib = _lib.load()
    assert [lib.lsr_knn3_workspace_bytes(n) for n in (-5, -1, 0)] == [0, 0, 0]
    sizes = [lib.lsr_knn3_workspace_bytes(n) for n in SIZES + [3_000_000]]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= 3_000_000 * (8 + 8 + 4 + 16)     # two key buffers, the order and the sorted records


@pytest.mark.parametrize("n, points, outs, ws, code", [
    (-1, 1, (1, 1, 1), 1, -1),
    (1, 1, (1, 1, 1), 1, -1), (2, 1, (1, 1, 1), 1, -1), (3, 1, (1, 1, 1), 1, -1),     # there are no three neighbours
    (_lib.KNN_MAX_POINTS + 1, 1, (1, 1, 1), 1, -1),
    (4, 0, (1, 1, 1), 1, -2),                          # points NULL
    (4, 1, (0, 0, 0), 1, -2),                          # all three outputs NULL
    (4, 1, (1, 0, 0), 0, -2), (1000, 1, (0, 1, 1), 0, -2),     # workspace NULL
    (0, 0, (0, 0, 0), 0, 0),                           # n == 0: nothing to do, nothing needed
])
def test_arguments_are_checked_before_any_gpu_work(n, points, outs, ws, code):
    """Dummy pointers: a call that got past the checks would have to touch them (and a device this machine lacks)."""
    lib = _lib.load()
    ptr = lambda on: C.c_void_p(0x1000 if on else None)
    assert lib.lsr_knn3(n, ptr(points), *(ptr(o) for o in outs), ptr(ws), None) == code


def test_cpu_tensors_are_refused():
    from latentsplat_amd import GaussianScene, knn3, mean_knn_dist2
    p = torch.from_numpy(ref.cloud("normal", 64).copy())
    for f in (knn3, mean_knn_dist2, GaussianScene.from_point_cloud):
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            f(p)


# ---- point cloud files ----

def _write(path, dtype, rows, fmt="binary_little_endian", element="vertex", count=None, extra="", type_names=None, cut=0, rename=None):
    """A PLY whose vertex rows are the numpy structured array ``rows`` of ``dtype``."""
    spell = {"f4": "float", "f8": "double", "u1": "uchar", "i1": "char", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint"}
    spell.update(type_names or {})
    head = f"ply\nformat {fmt} 1.0\ncomment written by numpy\nelement {element} {len(rows) if count is None else count}\n"
    for name, t in dtype:
        head += f"property {spell[t.lstrip('<')]} {(rename or {}).get(name, name)}\n"
    body = np.asarray(rows, dtype=np.dtype([(k, "<" + t.lstrip("<")) for k, t in dtype])).tobytes()
    with open(path, "wb") as f:
        f.write((head + extra + "end_header\n").encode() + (body[:len(body) - cut] if cut else body))


def _cloud_rows(dtype, n, seed=0):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=np.dtype(dtype))
    for name, t in dtype:
        rows[name] = rng.integers(0, 256, n) if t[-2] in "ui" else rng.standard_normal(n) * 3.0
    return rows


XYZ = [("x", "f4"), ("y", "f4"), ("z", "f4")]
NORMALS = [("nx", "f4"), ("ny", "f4"), ("nz", "f4")]
RGB = [("red", "u1"), ("green", "u1"), ("blue", "u1")]
STORE_PLY = XYZ + NORMALS + RGB                        # what the published trainer's storePly writes

LAYOUTS = {
    "store_ply": STORE_PLY,
    "no_colours": XYZ + NORMALS,
    "no_normals": XYZ + RGB,
    "bare": XYZ,
    "double": [("x", "f8"), ("y", "f8"), ("z", "f8")] + RGB,
    "mixed_width": [("x", "f8"), ("y", "f4"), ("z", "f8")],
    "shuffled": [("blue", "u1"), ("z", "f4"), ("nx", "f4"), ("red", "u1"), ("x", "f4"), ("ny", "f4"), ("green", "u1"), ("y", "f4"), ("nz", "f4")],
    "alpha": XYZ + RGB + [("alpha", "u1")],
    "other_types": [("id", "i4"), ("x", "f4"), ("flag", "i1"), ("y", "f4"), ("err", "f8"), ("z", "f4"), ("track", "u2"), ("w", "i2"), ("u", "u4")] + RGB,
}


@pytest.mark.parametrize("n", [0, 1, 777, 20_000])      # 20 000 rows of the widest layout: more than one read batch
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_load_points_ply_round_trips(tmp_path, layout, n):
    from latentsplat_amd import load_points_ply
    dtype = LAYOUTS[layout]
    rows = _cloud_rows(dtype, n)
    path = tmp_path / "points3D.ply"
    _write(path, dtype, rows, type_names={"f4": "float32", "u1": "uint8"} if layout == "alpha" else None)
    points, colors = load_points_ply(path, "cpu")
    assert points.dtype == torch.float32 and tuple(points.shape) == (n, 3)
    want = np.stack([rows[k].astype(np.float32) for k in "xyz"], 1)
    assert np.array_equal(points.numpy().view(np.uint32), want.view(np.uint32))
    if any(k == "red" for k, _ in dtype):
        rgb = np.stack([rows[k] for k in ("red", "green", "blue")], 1).astype(np.float32) / np.float32(255.0)
        assert colors.dtype == torch.float32 and np.array_equal(colors.numpy(), rgb)
        assert n == 0 or (0.0 <= colors.min() and colors.max() <= 1.0)
    else:
        assert colors is None


def _code(path):
    lib = _lib.load()
    n, has = C.c_int64(-7), C.c_int32(-7)
    rc = lib.lsr_ply_read_points_header(str(path).encode(), C.byref(n), C.byref(has))
    xyz, rgb = np.full((64, 3), 7.0, np.float32), np.full((64, 3), 7.0, np.float32)
    rc2 = lib.lsr_ply_read_points(str(path).encode(), xyz.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), 64)
    assert rc2 == rc
    if rc != 0:                                         # the outputs are written only when every check has passed
        assert n.value == -7 and has.value == -7 and (xyz == 7.0).all() and (rgb == 7.0).all()
    return rc


@pytest.mark.parametrize("what, kw, code", [
    ("ascii", dict(fmt="ascii"), -5),
    ("big_endian", dict(fmt="binary_big_endian"), -5),
    ("list_property", dict(extra="property list uchar int vertex_indices\n"), -5),
    ("second_element", dict(extra="element face 0\n"), -5),
    ("colours_of_another_type", dict(dtype=XYZ + [("red", "f4"), ("green", "f4"), ("blue", "f4")]), -5),
    ("only_some_colours", dict(dtype=XYZ + [("red", "u1"), ("green", "u1")]), -5),
    ("integer_coordinates", dict(dtype=[("x", "i4"), ("y", "i4"), ("z", "i4")]), -5),
    ("malformed_header", dict(extra="property float\n"), -1),
    ("unknown_type", dict(type_names={"u1": "byte"}), -1),
    ("missing_z", dict(dtype=[("x", "f4"), ("y", "f4")] + RGB), -1),
    ("x_twice", dict(dtype=XYZ + [("again", "f4")], rename=dict(again="x")), -1),
    ("negative_count", dict(count=-1), -1),
    ("overflowing_count", dict(count=2 ** 63), -1),
    ("count_beyond_the_file", dict(count=2 ** 40), -1),
    ("short_by_one_byte", dict(cut=1), -1),
])
def test_load_points_ply_rejections(tmp_path, what, kw, code):
    from latentsplat_amd import load_points_ply
    kw = dict(kw)
    dtype = kw.pop("dtype", STORE_PLY)
    path = tmp_path / f"{what}.ply"
    _write(path, dtype, _cloud_rows(dtype, 5), **kw)
    assert _code(path) == code
    with pytest.raises(_lib.LsrError, match="unsupported" if code == -5 else "invalid"):
        load_points_ply(path, "cpu")


def test_load_points_ply_no_such_file_and_short_buffer(tmp_path):
    lib = _lib.load()
    assert _code(tmp_path / "nope.ply") == -1
    path = tmp_path / "p.ply"
    _write(path, STORE_PLY, _cloud_rows(STORE_PLY, 65))
    xyz = np.full((64, 3), 7.0, np.float32)
    assert lib.lsr_ply_read_points(str(path).encode(), xyz.ctypes.data_as(C.c_void_p), None, 64) == -1 and (xyz == 7.0).all()
    assert lib.lsr_ply_read_points(str(path).encode(), None, None, 65) == -2
