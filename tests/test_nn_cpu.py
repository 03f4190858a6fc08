"""The cross-cloud nearest-neighbour query without a GPU: the float32 reference of tests/nn_ref.py (its numpy and eager
torch forms agree bit for bit, it stays within the derived bound of the float64 form, it matches a k-d tree), the host
side of lsr_nn_build / lsr_nn_query (sizing, every argument check: all of them return before any GPU work) and the
refusal of CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import nn_ref as ref

CASES = [("normal", 300, 257), ("clusters", 129, 1000), ("offset", 64, 500), ("aniso", 100, 333), ("dup", 200, 200),
         ("same", 10, 70), ("outlier", 65, 129), ("lattice", 100, 343), ("plane", 77, 128), ("line", 5, 2), ("normal", 1, 1)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name, m, n", CASES)
def test_numpy_and_torch_forms_agree_bit_for_bit(name, m, n):
    q, r = ref.cloud(name, m), ref.cloud(name, n)
    d_np, i_np = ref.nn_ref_numpy(q, r, chunk=64)
    d_t, i_t = ref.nn_ref_torch(q, r, "cpu", chunk=100)
    assert d_np.dtype == d_t.dtype == np.float32 and np.array_equal(_bits(d_np), _bits(d_t)) and np.array_equal(i_np, i_t)
    assert np.array_equal(_bits(ref.pair_dist2_f32(q, r, i_np)), _bits(d_np))
    assert (i_np >= 0).all() and (i_np < n).all()


@pytest.mark.parametrize("name, m, n", CASES)
def test_float32_form_is_within_the_bound_of_the_float64_form(name, m, n):
    q, r = ref.cloud(name, m), ref.cloud(name, n)
    d32, i32 = ref.nn_ref_numpy(q, r)
    d64, _ = ref.nn_ref_f64(q, r)
    # the pair the float32 search chose, in float64: its float32 distance is within the bound of it
    picked = ((q.astype(np.float64) - r[i32].astype(np.float64)) ** 2).sum(-1)
    assert (np.abs(d32.astype(np.float64) - picked) <= ref.BOUND * picked).all()
    assert ((picked == 0) == (d32 == 0)).all()                      # exact zeros are exact
    # and the minimum itself: rounding is monotonic in each operation, so the minima differ by no more than the bound
    assert (np.abs(d32.astype(np.float64) - d64) <= ref.BOUND * d64).all()
    assert ((d64 == 0) == (d32 == 0)).all()


def test_reference_breaks_ties_toward_the_lower_index():
    r = np.array([[1, 1, 1], [0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]], np.float32)
    q = np.array([[0, 0, 0], [0.5, 0.5, 0.0], [0.5, 0.5, 0.5], [9, 9, 9]], np.float32)
    for d, i in (ref.nn_ref_numpy(q, r), ref.nn_ref_torch(q, r), ref.nn_ref_f64(q, r)):
        assert i.tolist() == [1, 1, 0, 0] and d.tolist() == [0.0, 0.5, 0.75, 192.0]


@pytest.mark.parametrize("name", ["normal", "clusters"])
def test_reference_matches_a_kd_tree(name):
    spatial = pytest.importorskip("scipy.spatial")
    q, r = ref.cloud(name, 3001), ref.cloud(name, 5001)
    d64, i64 = ref.nn_ref_f64(q, r)
    dist, at = spatial.cKDTree(r.astype(np.float64)).query(q.astype(np.float64), k=1)
    assert np.allclose(d64, dist ** 2, rtol=1e-9, atol=0.0)
    assert np.array_equal(i64, at)                                 # (continuous clouds: no ties)
    d32, i32 = ref.nn_ref_numpy(q, r)
    assert (np.abs(d32.astype(np.float64) - dist ** 2) <= ref.BOUND * dist ** 2).all()


def test_lattice_cell_centres():
    cloud = ref.lattice(6, 1)
    q, want = ref.lattice_cell_centres(cloud, (1, 0, 2), 3)
    d, i = ref.nn_ref_numpy(q, cloud)
    assert q.shape == (27, 3) and (d == 0.75).all() and np.array_equal(i, want)


def test_sizes():
    lib = _lib.load()
    sizes = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 70_001, 600_001, 3_000_000]
    for f, per_point in ((lib.lsr_nn_index_bytes, 16), (lib.lsr_nn_build_workspace_bytes, 12), (lib.lsr_nn_query_workspace_bytes, 20)):
        assert [f(n) for n in (-5, -1, 0)] == [0, 0, 0]
        got = [f(n) for n in sizes]
        assert all(s > 0 for s in got) and got == sorted(got)
        assert all(s >= per_point * n for s, n in zip(got, sizes))
        assert f(_lib.KNN_MAX_POINTS + 5) == f(_lib.KNN_MAX_POINTS)
    # the index: the sorted 16-byte records, the sorted keys and the two levels of boxes
    assert lib.lsr_nn_index_bytes(3_000_000) >= 3_000_000 * (16 + 8) + (3_000_000 // 128) * 32


@pytest.mark.parametrize("n, points, mem, ws, code", [
    (0, 1, 1, 1, -1), (-1, 1, 1, 1, -1), (_lib.KNN_MAX_POINTS + 1, 1, 1, 1, -1),
    (1, 0, 1, 1, -2), (5, 1, 0, 1, -2), (1000, 1, 1, 0, -2),
])
def test_build_arguments_are_checked_before_any_gpu_work(n, points, mem, ws, code):
    """Dummy pointers: a call that got past the checks would have to touch them (and a device this machine lacks)."""
    lib = _lib.load()
    ptr = lambda on: C.c_void_p(0x1000 if on else None)
    assert lib.lsr_nn_build(n, ptr(points), ptr(mem), ptr(ws), None) == code


@pytest.mark.parametrize("n, mem, m, queries, outs, ws, code", [
    (0, 1, 5, 1, (1, 1), 1, -1), (-3, 1, 5, 1, (1, 1), 1, -1), (_lib.KNN_MAX_POINTS + 1, 1, 5, 1, (1, 1), 1, -1),
    (10, 1, -1, 1, (1, 1), 1, -1), (10, 1, _lib.KNN_MAX_POINTS + 1, 1, (1, 1), 1, -1),
    (0, 1, 0, 1, (1, 1), 1, -1),                        # an empty reference is invalid even for no queries
    (10, 0, 5, 1, (1, 1), 1, -2), (10, 1, 5, 0, (1, 1), 1, -2), (10, 1, 5, 1, (0, 0), 1, -2), (10, 1, 5, 1, (1, 0), 0, -2),
    (10, 1, 1000, 1, (0, 1), 0, -2),
    (10, 0, 0, 0, (0, 0), 0, 0),                        # m == 0: nothing to do, nothing needed
])
def test_query_arguments_are_checked_before_any_gpu_work(n, mem, m, queries, outs, ws, code):
    lib = _lib.load()
    ptr = lambda on: C.c_void_p(0x1000 if on else None)
    assert lib.lsr_nn_query(n, ptr(mem), m, ptr(queries), *(ptr(o) for o in outs), ptr(ws), None) == code


def test_exports_and_lazy_names():
    import latentsplat_amd
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsr_nn.h")).read()
    for name in ("lsr_nn_index_bytes", "lsr_nn_build_workspace_bytes", "lsr_nn_build", "lsr_nn_query_workspace_bytes", "lsr_nn_query"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in header, name
    assert lib.lsr_abi_version() == 10
    for name in ("NearestIndex", "nearest"):
        assert latentsplat_amd._LAZY[name] == "nn" and callable(getattr(latentsplat_amd, name))


def test_cpu_tensors_are_refused():
    from latentsplat_amd import NearestIndex, nearest
    p = torch.from_numpy(ref.cloud("normal", 64).copy())
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        NearestIndex(p)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        nearest(p, p)
