"""References of the mesh evaluation and cleanup (latentsplat_amd/mesh_eval.py, mesh_components / clean_mesh of
latentsplat_amd/mesh.py) and the meshes and clouds their tests use.

:func:`metrics_ref` restates ``cloud_metrics`` in float64 numpy from the two arrays of squared distances;
:func:`components_ref` is a numpy union-find whose labels are the lowest vertex index of every component;
:func:`clean_ref` is the cleanup in plain numpy."""
import numpy as np


def metrics_ref(to_gt, to_pred, thresholds=(), max_dist=None) -> dict:
    """``to_gt``: dist2 of every pred point to the ground truth; ``to_pred``: of every ground-truth point to pred."""
    d_p, d_g = np.sqrt(np.asarray(to_gt, np.float64)), np.sqrt(np.asarray(to_pred, np.float64))
    s_p, s_g = np.asarray(to_gt, np.float64), np.asarray(to_pred, np.float64)
    c_p, c_g = (d_p, d_g) if max_dist is None else (np.minimum(d_p, max_dist), np.minimum(d_g, max_dist))
    if max_dist is not None:
        s_p, s_g = np.minimum(s_p, float(max_dist) ** 2), np.minimum(s_g, float(max_dist) ** 2)
    out = dict(accuracy=float(c_p.mean()), completeness=float(c_g.mean()), accuracy_sq=float(s_p.mean()),
               completeness_sq=float(s_g.mean()), num_pred=int(d_p.size), num_gt=int(d_g.size), thresholds=[float(t) for t in thresholds],
               precision=[], recall=[], fscore=[], precision_count=[], recall_count=[])
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    for tau in thresholds:
        cp, cg = int((d_p < tau).sum()), int((d_g < tau).sum())
        p, r = cp / d_p.size, cg / d_g.size
        out["precision_count"].append(cp)
        out["recall_count"].append(cg)
        out["precision"].append(p)
        out["recall"].append(r)
        out["fscore"].append(2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


MEAN_KEYS = ("accuracy", "completeness", "chamfer", "accuracy_sq", "completeness_sq")
COUNT_KEYS = ("num_pred", "num_gt", "thresholds", "precision_count", "recall_count", "precision", "recall", "fscore")
MEAN_BAR = 2.0 ** -40           # relative: float64 sums of at most 10^5 non-negative terms, in whatever order


def components_ref(faces, num_vertices: int) -> np.ndarray:
    """``labels (nv,) int32``: union-find with path halving over the faces' edges, then the lowest vertex of every set."""
    parent = list(range(num_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        ra, rb, rc = find(a), find(b), find(c)
        r = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = r
    roots = np.array([find(v) for v in range(num_vertices)], np.int64)
    lowest = np.full(num_vertices, num_vertices, np.int64)
    np.minimum.at(lowest, roots, np.arange(num_vertices))
    return lowest[roots].astype(np.int32)


def clean_ref(vertices, faces, labels, keep_largest=None, min_faces=None):
    """``(vertices, faces, kept_vertex_mask, info)``: sizes are face counts, ties toward the lower label, order kept."""
    vertices, faces, labels = np.asarray(vertices), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(labels, np.int64)
    nv = vertices.shape[0]
    size = np.bincount(labels[faces[:, 0]], minlength=nv) if len(faces) else np.zeros(nv, np.int64)
    with_faces = [int(l) for l in np.flatnonzero(size > 0)]
    kept = list(with_faces)
    if min_faces is not None:
        kept = [l for l in kept if size[l] >= min_faces]
    if keep_largest is not None:
        ranked = sorted(with_faces, key=lambda l: (-size[l], l))[:keep_largest]
        kept = [l for l in kept if l in set(ranked)]
    if keep_largest is None and min_faces is None:
        keep_v = np.ones(nv, bool)
    else:
        keep_v = np.isin(labels, kept)
    keep_f = keep_v[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    remap = np.cumsum(keep_v) - 1
    info = dict(components=len(with_faces), components_kept=len(kept), faces_kept=int(keep_f.sum()), faces_dropped=int((~keep_f).sum()),
                vertices_kept=int(keep_v.sum()), vertices_dropped=int((~keep_v).sum()))
    return vertices[keep_v], remap[faces[keep_f]].astype(np.int32), keep_v, info


# ---- meshes ----

def two_tetrahedra():
    """Two disjoint tetrahedra with interleaved vertex numbers: even vertices one, odd vertices the other."""
    tet = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    faces = np.concatenate([2 * tet, 2 * tet + 1]).astype(np.int32)
    corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    vertices = np.empty((8, 3), np.float32)
    vertices[0::2], vertices[1::2] = corners, corners + np.float32(5.0)
    return vertices, faces


def strip(nv: int, seed: int):
    """A triangle strip of ``nv`` vertices (faces (i, i+1, i+2)) whose numbering is randomly permuted: one component of the
    longest possible diameter."""
    perm = np.random.default_rng(seed).permutation(nv)
    i = np.arange(nv - 2)
    faces = perm[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)
    vertices = np.zeros((nv, 3), np.float32)
    vertices[perm, 0] = np.arange(nv) // 2
    vertices[perm, 1] = np.arange(nv) % 2
    return vertices, faces


def grid_mesh(side: int, isolated: int = 0):
    """A ``side x side`` grid of vertices, two triangles per cell, and ``isolated`` vertices that no face names."""
    j, i = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    vertices = np.concatenate([np.stack([i.ravel(), j.ravel(), np.zeros(side * side)], 1),
                               np.stack([np.arange(isolated), np.full(isolated, -3.0), np.ones(isolated)], 1)]).astype(np.float32)
    v = (j[:-1, :-1] * side + i[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([v, v + 1, v + side], 1), np.stack([v + 1, v + side + 1, v + side], 1)]).astype(np.int32)
    return vertices, faces


def blobs(sizes, seed: int):
    """Disjoint fans of ``sizes[k]`` faces each (a fan of f faces has f + 2 vertices), vertex numbers shuffled across the
    fans and faces shuffled: components of chosen face counts.  Returns ``(vertices, faces, lowest label of each fan)``."""
    rng = np.random.default_rng(seed)
    nv = sum(s + 2 for s in sizes)
    perm = rng.permutation(nv)
    faces, labels, at = [], [], 0
    vertices = np.zeros((nv, 3), np.float32)
    for k, s in enumerate(sizes):
        ids = perm[at:at + s + 2]
        at += s + 2
        faces += [[ids[0], ids[t + 1], ids[t + 2]] for t in range(s)]
        labels.append(int(ids.min()))
        ang = np.linspace(0.0, 1.5, s + 1)
        vertices[ids[0]] = (10.0 * k, 0.0, 0.0)
        vertices[ids[1:]] = np.stack([10.0 * k + np.cos(ang), np.sin(ang), np.zeros(s + 1)], 1)
    faces = np.array(faces, np.int32)[rng.permutation(len(faces))]
    return vertices, faces, labels


# ---- the end-to-end scene: a unit sphere and a floater ----

SPHERE_DIMS, SPHERE_VOXEL, SPHERE_ORIGIN = (49, 49, 49), 0.05, (-1.2, -1.2, -1.2)
FLOATER_CENTRE, FLOATER_RADIUS = (0.9, 0.9, 0.9), 0.15


def two_sphere_tsdf(trunc: float) -> np.ndarray:
    """``tsdf (49, 49, 49)`` float32, x-fastest: the signed distance (positive outside, the convention of
    tests/tsdf_ref.py) to the union of the unit sphere at the origin and the floater, in units of ``trunc``, clamped."""
    axis = [SPHERE_ORIGIN[k] + SPHERE_VOXEL * np.arange(SPHERE_DIMS[k]) for k in range(3)]
    z, y, x = np.meshgrid(axis[2], axis[1], axis[0], indexing="ij")
    unit = np.sqrt(x * x + y * y + z * z) - 1.0
    cx, cy, cz = FLOATER_CENTRE
    floater = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - FLOATER_RADIUS
    return np.clip(np.minimum(unit, floater) / trunc, -1.0, 1.0).astype(np.float32)


def unit_sphere_samples(n: int, seed: int) -> np.ndarray:
    """``n`` uniform samples of the unit sphere, float32."""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
