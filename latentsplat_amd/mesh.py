"""Mesh extraction for a trainable 3DGS scene, in HIP (csrc/tsdf.hip; C ABI include/lsr_mesh.h).

Every surface method built on Gaussians (2DGS, Gaussian Surfels, GOF, RaDe-GS, PGSR) ends the same way: it renders depth
from the training cameras, fuses it into a truncated signed distance volume and takes a triangle mesh from the zero level
set.  This module is that step:

1. :class:`TSDFVolume` holds a dense volume on the device; :meth:`TSDFVolume.integrate` fuses a batch of rendered views
   (depth of depth mode NATIVE, the mask, optionally colour, and the view table they were rendered with) in ONE pass over
   the volume: a lattice point's state stays in registers across the views of a call, so the volume traffic does not grow
   with the number of views.
2. :meth:`TSDFVolume.extract_mesh` runs marching tetrahedra on the Kuhn subdivision of the lattice (six tetrahedra per
   cube: no case table, unambiguous, watertight): ``(vertices, faces, colors)``.  It reads the two counts once, which is
   its only synchronisation, and allocates exactly.
3. :func:`save_mesh_ply` / :func:`load_mesh_ply` write and read a binary little-endian triangle-mesh ``.ply`` with numpy.
4. :func:`mesh_components` labels the connected components of a mesh (csrc/mesh_components.hip: hook and compress rounds
   with integer ``atomicMin``) and :func:`clean_mesh` keeps the largest of them: the ``post_process_mesh`` step that
   removes the floaters every TSDF of rendered depth contains.

:meth:`latentsplat_amd.scene_model.GaussianScene.extract_mesh` composes render, fusion and extraction.

Values only: fusion is post-training and nothing here has a gradient.  No atomics: the same bits every call.  float32 ROCm
tensors only; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_WHO = "mesh extraction"


class TSDFVolume:
    """A dense truncated signed distance volume on a ROCm device.  The sample of lattice point ``(i, j, k)`` sits at
    ``origin + voxel_size * (i, j, k)`` in world units (the scene's own space).  ``dims = (nx, ny, nz)``, each 2..2048 with
    at most 2^30 points; tensors are x-fastest: ``tsdf (nz, ny, nx)`` (the mean clamped distance in units of ``trunc``,
    in [-1, 1]), ``weight (nz, ny, nx)`` (observations), ``color (3, nz, ny, nx)`` or ``None``.

    ``trunc`` defaults to 4 voxel sizes: a default, not a measurement."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], trunc: Optional[float] = None,
                 color: bool = True, device="cuda"):
        nx, ny, nz = (int(d) for d in dims)
        self.origin = tuple(float(o) for o in origin)
        self.voxel_size = float(voxel_size)
        self.dims = (nx, ny, nz)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LsrError(f"{_WHO} needs a ROCm device (no CPU fallback), got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if len(self.origin) != 3:
            raise _lib.LsrError("origin must have 3 entries")
        self._dims = _lib.TsdfDims(nx=nx, ny=ny, nz=nz, origin=(C.c_float * 3)(*self.origin), voxel_size=self.voxel_size,
                                   trunc=self.trunc, has_color=1 if color else 0)
        if _lib.load().lsr_mesh_workspace_bytes(C.byref(self._dims)) == 0:
            raise _lib.LsrError(f"a TSDF volume has extents {_lib.TSDF_MIN_EXTENT}..{_lib.TSDF_MAX_EXTENT}, at most 2^30 lattice "
                                f"points and a finite positive voxel_size and trunc; got dims {self.dims}, voxel_size "
                                f"{self.voxel_size}, trunc {self.trunc}")
        self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.empty((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None
        self.reset()

    @classmethod
    def from_bounds(cls, lo: Sequence[float], hi: Sequence[float], voxel_size: float, **kw) -> "TSDFVolume":
        """The smallest volume with origin ``lo`` whose lattice reaches ``hi``."""
        dims = [max(_lib.TSDF_MIN_EXTENT, int(np.ceil((float(h) - float(l)) / float(voxel_size))) + 1) for l, h in zip(lo, hi)]
        return cls(lo, voxel_size, dims, **kw)

    def reset(self) -> None:
        """No observation anywhere: distance 1 (free space), weight 0, colour 0."""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def integrate(self, depth: Tensor, alpha: Tensor, views: Tensor, color: Optional[Tensor] = None, alpha_min: float = 0.5,
                  depth_max: Optional[float] = None, max_weight: Optional[float] = None) -> None:
        """Fuse ``V`` rendered views, in order: ``depth (V, H, W)`` is the rendered depth of depth mode NATIVE (sum of
        alpha T z), ``alpha (V, H, W)`` the mask, ``views (V, 44)`` the table they were rendered with, ``color
        (V, 3, H, W)`` the rendered colour (required exactly when the volume has colour).  Per lattice point and view: the
        point is projected with the record's own matrices to its NEAREST pixel (depth is never interpolated across an
        edge); the view is skipped unless ``alpha > alpha_min`` there, ``D = depth / alpha`` is finite and positive,
        ``D / s <= depth_max`` (world units; ``None``: no limit) and the projective distance ``sdf = (D - z) / s`` is at
        least ``-trunc``; then ``tsdf <- (tsdf w + min(1, sdf / trunc)) / (w + 1)``, colour likewise, ``w <- w + 1`` capped
        at ``max_weight`` (``None``: no cap).  Lists longer than 1024 views are fused in chunks: the recurrence is float32
        and the state between views is float32, so chunking does not change a bit.

        ``alpha_min = 0.5`` is a default, not a measurement."""
        depth = _args.f32(_WHO, "depth", depth)
        if depth.dim() != 3:
            raise _lib.LsrError(f"depth must be (V, H, W), got {tuple(depth.shape)}")
        V, H, W = depth.shape
        dev = self.device
        depth = _args.f32(_WHO, "depth", depth, None, dev).detach().contiguous()
        alpha = _args.f32(_WHO, "alpha", alpha, (V, H, W), dev).detach().contiguous()
        views = _args.f32(_WHO, "views", views, (V, _lib.VIEW_FLOATS), dev).detach().contiguous()
        if (color is not None) != (self.color is not None):
            raise _lib.LsrError("integrate takes color exactly when the volume has colour")
        if color is not None:
            color = _args.f32(_WHO, "color", color, (V, 3, H, W), dev).detach().contiguous()
        lib = _lib.load()
        step = _lib.TSDF_MAX_VIEWS
        if H * W > 0:
            step = max(1, min(step, ((1 << 31) - 1) // (H * W)))
        with torch.cuda.device(dev):
            for lo in range(0, V, step):
                n = min(step, V - lo)
                ws = _args.workspace(lib.lsr_tsdf_workspace_bytes(n), dev)
                _lib.call("lsr_tsdf_integrate", C.byref(self._dims), ptr(self.tsdf), ptr(self.weight), ptr(self.color), n, H, W,
                          ptr(depth[lo:lo + n]), ptr(alpha[lo:lo + n]), ptr(None if color is None else color[lo:lo + n]),
                          ptr(views[lo:lo + n]), float(alpha_min), float(depth_max or 0.0), float(max_weight or 0.0), ptr(ws),
                          _args.stream(dev))

    def extract_mesh(self, min_weight: float = 1.0):
        """``(vertices (Nv, 3) float32, faces (Nf, 3) int32, colors (Nv, 3) float32 or None)`` of the zero level set, by
        marching tetrahedra on the Kuhn subdivision (include/lsr_mesh.h states the numbering, the order and the winding:
        every face is wound so that its normal points toward positive distance, toward the cameras).  A lattice point
        takes part when ``weight >= min_weight``; it is inside when ``tsdf < 0``.  A vertex that no face uses may remain at
        the grid border or next to unobserved space.  An all-positive volume gives empty tensors.  One host read (the two
        counts)."""
        lib = _lib.load()
        dev = self.device
        ws = _args.workspace(lib.lsr_mesh_workspace_bytes(C.byref(self._dims)), dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.call("lsr_mesh_count", C.byref(self._dims), ptr(self.tsdf), ptr(self.weight), float(min_weight), ptr(ws),
                      ptr(counts), _args.stream(dev))
            nv, nf = (int(c) for c in counts.tolist())
            if nv >= 1 << 31 or nf >= 1 << 31:
                raise _lib.LsrError(f"the mesh has {nv} vertices and {nf} faces; both must stay below 2^31 (use a coarser volume)")
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
            colors = torch.empty((nv, 3), dtype=torch.float32, device=dev) if self.color is not None else None
            _lib.call("lsr_mesh_emit", C.byref(self._dims), ptr(self.tsdf), ptr(self.weight), ptr(self.color), float(min_weight),
                      ptr(ws), ptr(counts), nv, nf, ptr(vertices), ptr(colors), ptr(faces), _args.stream(dev))
        return vertices, faces, colors


def _faces(faces, num_vertices=None) -> Tensor:
    faces = _args.i32(_WHO, "faces", faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.LsrError(f"faces must be (nf, 3), got {tuple(faces.shape)}")
    if faces.shape[0] > _lib.MESH_MAX_ELEMENTS or (num_vertices is not None and not 0 <= num_vertices <= _lib.MESH_MAX_ELEMENTS):
        raise _lib.LsrError(f"a mesh has at most {_lib.MESH_MAX_ELEMENTS} vertices and faces")
    return faces.detach().contiguous()


def mesh_components(faces: Tensor, num_vertices: int, return_rounds: bool = False):
    """``labels (num_vertices,) int32``: the lowest vertex index of every vertex's connected component.  Two vertices are
    connected when a face of ``faces (nf, 3) int32`` names both BY INDEX (:meth:`TSDFVolume.extract_mesh` numbers a vertex
    once per lattice edge, so its meshes qualify; a soup with duplicated coordinates does not).  A vertex in no face
    labels itself.  A corner outside ``[0, num_vertices)`` is refused before anything is launched (one reduction, one
    host read).  The rounds of hooking and compression (include/lsr_mesh.h, part C) are driven from here: the changed
    flag is read after every round, and more than 64 rounds raise instead of looping (O(log nv) are needed).
    ``return_rounds``: also the number of rounds run, the confirming one included."""
    num_vertices = int(num_vertices)
    f = _faces(faces, num_vertices)
    dev, nf = f.device, f.shape[0]
    if nf > 0:
        lo, hi = (int(x) for x in torch.stack([f.min(), f.max()]).tolist())
        if lo < 0 or hi >= num_vertices:
            raise _lib.LsrError(f"faces name vertices {lo}..{hi}, outside 0..{num_vertices - 1}")
    labels = torch.empty((num_vertices,), dtype=torch.int32, device=dev)
    changed = torch.zeros((1,), dtype=torch.int32, device=dev)
    rounds = 0
    with torch.cuda.device(dev):
        _lib.call("lsr_mesh_components_init", num_vertices, ptr(labels), _args.stream(dev))
        if nf > 0 and num_vertices > 0:
            while True:
                if rounds == _lib.MESH_COMPONENT_ROUNDS:
                    raise _lib.LsrError(f"mesh_components did not converge in {rounds} rounds")
                _lib.call("lsr_mesh_components_round", num_vertices, nf, ptr(f), ptr(labels), ptr(changed), _args.stream(dev))
                rounds += 1
                if int(changed.item()) == 0:
                    break
    return (labels, rounds) if return_rounds else labels


def clean_mesh(vertices: Tensor, faces: Tensor, colors: Optional[Tensor] = None, keep_largest: Optional[int] = None,
               min_faces: Optional[int] = None):
    """``(vertices, faces, colors, info)`` without the small connected components (the published ``post_process_mesh``).
    A component's size is its FACE count.  ``keep_largest=K`` keeps the K largest (ties toward the lower label, the
    component's lowest vertex index); ``min_faces=F`` keeps those of at least F faces; with both a component has to pass
    both; with neither the mesh is returned as it is.  Vertices in no face form components of size 0: any filter drops
    them.  Kept faces and vertices stay in their original order, indices remapped.  The labels are HIP
    (:func:`mesh_components`); the compaction is plain torch (``bincount``, ``cumsum``) with one host read.
    ``info``: ``components`` (those with at least one face), ``components_kept``, ``faces_kept``, ``faces_dropped``,
    ``vertices_kept``, ``vertices_dropped``."""
    vertices = _args.f32(_WHO, "vertices", vertices)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise _lib.LsrError(f"vertices must be (nv, 3), got {tuple(vertices.shape)}")
    nv, dev = vertices.shape[0], vertices.device
    f = _faces(_args.i32(_WHO, "faces", faces, None, dev), nv)
    if colors is not None:
        colors = _args.f32(_WHO, "colors", colors, (nv, 3), dev)
    for name, value in (("keep_largest", keep_largest), ("min_faces", min_faces)):
        if value is not None and int(value) < 0:
            raise _lib.LsrError(f"{name} must not be negative")
    nf = f.shape[0]
    labels = mesh_components(f, nv).long()
    size = torch.bincount(labels[f[:, 0].long()], minlength=nv) if nf > 0 else torch.zeros((nv,), dtype=torch.int64, device=dev)
    keep = size > 0                                        # per label: a component with faces
    components = keep.sum()
    if min_faces is not None:
        keep = keep & (size >= int(min_faces))
    if keep_largest is not None:
        # the K largest, ties toward the lower label: a stable descending sort of the sizes keeps equal sizes in label order
        order = torch.sort(size, descending=True, stable=True).indices[:int(keep_largest)]
        top = torch.zeros_like(keep)
        top[order] = True
        keep = keep & top
    if keep_largest is None and min_faces is None:
        keep_vertex = torch.ones((nv,), dtype=torch.bool, device=dev)
        keep_face = torch.ones((nf,), dtype=torch.bool, device=dev)
    else:
        keep_vertex = keep[labels]
        keep_face = keep_vertex[f[:, 0].long()] if nf > 0 else torch.zeros((0,), dtype=torch.bool, device=dev)
    remap = torch.cumsum(keep_vertex.long(), 0) - 1
    counts = torch.stack([components, (keep & (size > 0)).sum(), keep_face.sum(), keep_vertex.sum()]).tolist()      # the one host read
    out_faces = remap[f[keep_face].long()].to(torch.int32)
    info = dict(components=int(counts[0]), components_kept=int(counts[1]), faces_kept=int(counts[2]), faces_dropped=nf - int(counts[2]),
                vertices_kept=int(counts[3]), vertices_dropped=nv - int(counts[3]))
    return vertices[keep_vertex], out_faces, None if colors is None else colors[keep_vertex], info


def _numpy(a, dtype):
    return np.ascontiguousarray((a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(dtype, copy=False))


def save_mesh_ply(path, vertices, faces, colors=None) -> None:
    """A binary little-endian triangle-mesh ``.ply``: ``x y z`` float vertices, with ``colors`` (floats, 0..1) also uchar
    ``red green blue`` (rounded to nearest, clamped), and ``list uchar int vertex_indices`` faces.  Plain numpy."""
    v = _numpy(vertices, "<f4").reshape(-1, 3)
    f = _numpy(faces, "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", "property float x", "property float y",
              "property float z"]
    if colors is not None:
        c = _numpy(colors, "<f4").reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"colors must be ({v.shape[0]}, 3)")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(v.shape[0], dtype=fields)
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        rgb = np.clip(np.rint(np.nan_to_num(c.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
        rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    tris = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    tris["n"], tris["v"] = 3, f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(rows.tobytes())
        out.write(tris.tobytes())


def load_mesh_ply(path):
    """``(vertices (Nv, 3) float32, faces (Nf, 3) int32, colors (Nv, 3) uint8 or None)`` of a file :func:`save_mesh_ply`
    wrote (binary little-endian, float ``x y z``, optional uchar ``red green blue``, triangles as ``list uchar int``)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a .ply file")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary little-endian files are read")
    counts, props, element = {}, {}, None
    for line in lines:
        word = line.split()
        if word[:1] == ["element"]:
            element = word[1]
            counts[element] = int(word[2])
            props[element] = []
        elif word[:1] == ["property"] and element is not None:
            props[element].append(" ".join(word[1:]))
    has_color = props.get("vertex") == ["float x", "float y", "float z", "uchar red", "uchar green", "uchar blue"]
    if not (has_color or props.get("vertex") == ["float x", "float y", "float z"]) or \
            props.get("face") != ["list uchar int vertex_indices"] or list(counts) != ["vertex", "face"]:
        raise ValueError(f"{path}: not a mesh this module wrote")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else [])
    at = end + len(b"end_header\n")
    rows = np.frombuffer(data, dtype=fields, count=counts["vertex"], offset=at)
    at += rows.nbytes
    tris = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=counts["face"], offset=at)
    if at + tris.nbytes != len(data) or (tris["n"] != 3).any():
        raise ValueError(f"{path}: not a triangle mesh of the announced size")
    vertices = np.stack([rows["x"], rows["y"], rows["z"]], -1).astype(np.float32)
    colors = np.stack([rows["red"], rows["green"], rows["blue"]], -1) if has_color else None
    return vertices, np.ascontiguousarray(tris["v"]).astype(np.int32), colors
