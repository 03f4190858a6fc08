"""Mesh evaluation and cleanup without a GPU: the references of tests/mesh_eval_ref.py (the union-find against
scipy.sparse.csgraph, the metrics against a hand-computed case, the cleanup's ordering and ties), the host side of the
component calls (every argument check returns before any GPU work), the exports, and the refusal of CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import mesh_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meshes():
    yield "two_tetrahedra", ref.two_tetrahedra()
    yield "strip", ref.strip(5001, 1)
    yield "grid", ref.grid_mesh(16, isolated=10)
    v, f, _ = ref.blobs([5, 1, 9, 5, 2], 3)
    yield "blobs", (v, f)


@pytest.mark.parametrize("name, mesh", list(_meshes()), ids=[n for n, _ in _meshes()])
def test_union_find_matches_csgraph(name, mesh):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse import csgraph
    vertices, faces = mesh
    nv = len(vertices)
    labels = ref.components_ref(faces, nv)
    rows = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
    cols = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
    graph = sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv))
    count, comp = csgraph.connected_components(graph, directed=False)
    lowest = np.full(count, nv, np.int64)
    np.minimum.at(lowest, comp, np.arange(nv))
    assert np.array_equal(labels, lowest[comp]) and labels.dtype == np.int32
    assert (labels <= np.arange(nv)).all() and np.array_equal(labels[labels], labels)


def test_union_find_on_the_named_meshes():
    _, faces = ref.two_tetrahedra()
    assert ref.components_ref(faces, 8).tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    v, faces = ref.strip(1001, 2)
    assert not ref.components_ref(faces, 1001).any()
    v, faces = ref.grid_mesh(8, isolated=5)
    assert ref.components_ref(faces, 69).tolist() == [0] * 64 + [64, 65, 66, 67, 68]
    assert ref.components_ref(np.zeros((0, 3), np.int32), 4).tolist() == [0, 1, 2, 3]
    assert ref.components_ref(np.array([[2, 2, 5], [3, 3, 3]]), 6).tolist() == [0, 1, 2, 3, 4, 2]      # repeated corners


def test_metrics_reference_on_a_hand_computed_case():
    to_gt, to_pred = np.array([0.0, 0.25, 4.0, 1.0], np.float32), np.array([0.0, 9.0], np.float32)
    m = ref.metrics_ref(to_gt, to_pred, thresholds=(0.5, 1.0, 1e-9), max_dist=None)
    assert m["accuracy"] == (0.0 + 0.5 + 2.0 + 1.0) / 4 and m["completeness"] == 1.5 and m["chamfer"] == (0.875 + 1.5) / 2
    assert m["accuracy_sq"] == 5.25 / 4 and m["completeness_sq"] == 4.5
    assert m["precision_count"] == [1, 2, 1] and m["recall_count"] == [1, 1, 1]       # d < tau is strict: 0.5 and 1.0 are not inside
    assert m["precision"] == [0.25, 0.5, 0.25] and m["recall"] == [0.5, 0.5, 0.5]
    assert m["fscore"][0] == 2 * 0.25 * 0.5 / 0.75
    clipped = ref.metrics_ref(to_gt, to_pred, thresholds=(0.5,), max_dist=1.5)
    assert clipped["accuracy"] == (0.0 + 0.5 + 1.5 + 1.0) / 4 and clipped["completeness"] == 0.75 and clipped["completeness_sq"] == 1.125
    assert clipped["precision_count"] == [1] and clipped["recall_count"] == [1]        # the counts see the unclipped distances
    assert ref.metrics_ref([4.0], [4.0], thresholds=(1.0,))["fscore"] == [0.0]          # nothing within tau: 0, not 0 / 0


def test_cleanup_reference_order_and_ties():
    sizes = [5, 1, 9, 5, 2]
    vertices, faces, fan_labels = ref.blobs(sizes, 3)
    labels = ref.components_ref(faces, len(vertices))
    assert sorted(set(labels.tolist())) == sorted(fan_labels)
    v, f, keep_v, info = ref.clean_ref(vertices, faces, labels, keep_largest=2)
    tie = min(fan_labels[0], fan_labels[3])                         # two fans of 5 faces: the lower label wins
    assert set(labels[keep_v].tolist()) == {fan_labels[2], tie}
    assert info == dict(components=5, components_kept=2, faces_kept=14, faces_dropped=8, vertices_kept=18, vertices_dropped=14)
    assert np.array_equal(v, vertices[keep_v]) and np.array_equal(v[f], vertices[faces[keep_v[faces[:, 0]]]])
    _, _, _, info = ref.clean_ref(vertices, faces, labels, min_faces=5)
    assert info["components_kept"] == 3 and info["faces_kept"] == 19
    _, _, _, info = ref.clean_ref(vertices, faces, labels, keep_largest=3, min_faces=6)
    assert info["components_kept"] == 1 and info["faces_kept"] == 9
    v, f, keep_v, info = ref.clean_ref(vertices, faces, labels)
    assert keep_v.all() and np.array_equal(f, faces) and info["faces_dropped"] == 0


def test_two_sphere_volume_and_samples():
    tsdf = ref.two_sphere_tsdf(0.2)
    assert tsdf.shape == (49, 49, 49) and tsdf.dtype == np.float32 and tsdf.min() == -1.0 and tsdf.max() == 1.0
    assert tsdf[24, 24, 24] == -1.0 and tsdf[42, 42, 42] < 0 and tsdf[38, 38, 38] > 0.9      # centre, floater, between them
    s = ref.unit_sphere_samples(1000, 0)
    assert s.dtype == np.float32 and np.abs(np.linalg.norm(s.astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.parametrize("nv, labels, code", [(-1, 1, -1), (_lib.MESH_MAX_ELEMENTS + 1, 1, -1), (5, 0, -2), (0, 0, 0)])
def test_components_init_arguments_are_checked_before_any_gpu_work(nv, labels, code):
    lib = _lib.load()
    assert lib.lsr_mesh_components_init(nv, C.c_void_p(0x1000 if labels else None), None) == code


@pytest.mark.parametrize("nv, nf, faces, labels, changed, code", [
    (-1, 5, 1, 1, 1, -1), (5, -1, 1, 1, 1, -1), (_lib.MESH_MAX_ELEMENTS + 1, 5, 1, 1, 1, -1), (5, _lib.MESH_MAX_ELEMENTS + 1, 1, 1, 1, -1),
    (5, 5, 1, 1, 0, -2), (5, 5, 0, 1, 1, -2), (5, 5, 1, 0, 1, -2), (0, 0, 0, 0, 0, -2),
])
def test_components_round_arguments_are_checked_before_any_gpu_work(nv, nf, faces, labels, changed, code):
    lib = _lib.load()
    ptr = lambda on: C.c_void_p(0x1000 if on else None)
    assert lib.lsr_mesh_components_round(nv, nf, ptr(faces), ptr(labels), ptr(changed), None) == code


def test_exports_and_lazy_names():
    import latentsplat_amd
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsr_mesh.h")).read()
    for name in ("lsr_mesh_components_init", "lsr_mesh_components_round"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in header, name
    assert lib.lsr_abi_version() == 10 and _lib.MESH_COMPONENT_ROUNDS == 64
    for name, module in (("mesh_components", "mesh"), ("clean_mesh", "mesh"), ("cloud_metrics", "mesh_eval"), ("sample_mesh", "mesh_eval")):
        assert latentsplat_amd._LAZY[name] == module and callable(getattr(latentsplat_amd, name))


def test_cpu_tensors_are_refused():
    from latentsplat_amd import clean_mesh, cloud_metrics, mesh_components, sample_mesh
    vertices, faces = (torch.from_numpy(a) for a in ref.two_tetrahedra())
    for call in (lambda: cloud_metrics(vertices, vertices), lambda: sample_mesh(vertices, faces, 10),
                 lambda: mesh_components(faces, 8), lambda: clean_mesh(vertices, faces, keep_largest=1)):
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            call()


def test_eval_tool_parses_its_arguments_and_needs_a_device(tmp_path, monkeypatch):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_mesh
    finally:
        sys.path.pop(0)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no CPU fallback"):
        eval_mesh.main(["mesh.ply", "--gt", "gt.ply", "--out", str(tmp_path / "m.json"), "--thresholds", "0.1", "0.2", "--keep-largest", "1"])
    with pytest.raises(SystemExit):
        eval_mesh.main(["mesh.ply"])                                # --gt and --out are required
