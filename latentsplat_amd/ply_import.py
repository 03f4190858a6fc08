"""3DGS ``.ply`` import: a scene file in the published ``point_cloud.ply`` layout to the tensors the rasterizer takes.

The library's host reader (csrc/ply_reader.cpp) parses the header into a layout and copies the rows into a pinned
buffer; one HIP kernel (``lsr_ply_unpack``, csrc/ply.hip) turns the row table into means, colour SH in the
rasterizer's ``(n, K, 3)`` layout, opacities, scales, unit quaternions and packed covariances.  C ABI:
include/lsr_ply.h.  ROCm float32 tensors only; no CPU fallback.

Files of the published 3DGS trainer store the opacity as a logit (``opacity="logit"``, the default) and their colour
SH in the ``"3dgs"`` basis (:func:`latentsplat_amd.rasterizer.set_color_sh_convention`, the default).  Files written
by :func:`latentsplat_amd.ply_export.export_ply` store the opacity as it is: load them with ``opacity="raw"``."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from math import isqrt
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr
from ._lib import PlyLayout, PlyOutputs

_OPACITY_FLAGS = {"logit": 0, "raw": _lib.PLY_OPACITY_RAW}


@dataclass
class Scene3DGS:
    means: Tensor          # (n, 3)
    covariances: Tensor    # (n, 6) xx,xy,xz,yy,yz,zz
    opacities: Tensor      # (n, 1)
    shs: Tensor            # (n, K, 3)
    scales: Tensor         # (n, 3)
    rotations: Tensor      # (n, 4) w,x,y,z, unit norm
    sh_degree: int


def layout_from_names(names: Sequence[str], n: int) -> PlyLayout:
    """The layout of a row table whose columns are ``names`` (the rules of ``lsr_ply_read_header``: any order,
    other names skipped, each required name exactly once, ``f_rest_0..3(K-1)-1`` for K in 1, 4, 9, 16, 25)."""
    names = list(names)
    if not 0 < len(names) <= _lib.PLY_MAX_STRIDE:
        raise _lib.LsrError(f"a row of {len(names)} properties is not supported (1..{_lib.PLY_MAX_STRIDE})")
    at: dict = {}
    for i, name in enumerate(names):
        at.setdefault(name, []).append(i)

    def one(name: str) -> int:
        where = at.get(name, [])
        if len(where) != 1:
            raise _lib.LsrError(f"property {name!r} is {'missing' if not where else 'given twice'}")
        return where[0]

    rest = [k for k in at if k.startswith("f_rest_")]
    K = isqrt(len(rest) // 3 + 1)
    if len(rest) != 3 * (K * K - 1) or K * K > _lib.PLY_MAX_SH_COEFFS:
        raise _lib.LsrError(f"{len(rest)} f_rest properties: expected 3 (K - 1) for K in 1, 4, 9, 16, 25")
    L = PlyLayout(n=n, data_offset=0, stride=len(names), sh_coeffs=K * K)
    L.xyz[:] = [one(k) for k in "xyz"]
    L.f_dc[:] = [one(f"f_dc_{i}") for i in range(3)]
    L.opacity = one("opacity")
    L.scale[:] = [one(f"scale_{i}") for i in range(3)]
    L.rot[:] = [one(f"rot_{i}") for i in range(4)]
    for i in range(len(rest)):
        L.f_rest[i] = one(f"f_rest_{i}")
    return L


def unpack_table(rows: Tensor, layout: PlyLayout, opacity: str = "logit", want: Optional[Sequence[str]] = None) -> dict:
    """``lsr_ply_unpack`` as it is: the outputs named in ``want`` (default: all of ``means, shs, opacities, scales,
    rotations, cov3D``) as a dict; the others are not computed."""
    if opacity not in _OPACITY_FLAGS:
        raise _lib.LsrError(f"opacity must be 'logit' or 'raw', got {opacity!r}")
    if not rows.is_cuda or rows.dtype != torch.float32:
        raise _lib.LsrError("ply import needs a float32 ROCm row table (no CPU fallback)")
    rows = rows.detach().contiguous()
    n, K, dev = layout.n, layout.sh_coeffs, rows.device
    if rows.dim() != 2 or tuple(rows.shape) != (n, layout.stride):
        raise _lib.LsrError(f"rows must be ({n}, {layout.stride}), got {tuple(rows.shape)}")
    shapes = dict(means=(n, 3), shs=(n, K, 3), opacities=(n, 1), scales=(n, 3), rotations=(n, 4), cov3D=(n, 6))
    unknown = [k for k in (want or ()) if k not in shapes]
    if unknown:
        raise _lib.LsrError(f"unknown outputs {unknown}; expected some of {list(shapes)}")
    out = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items() if want is None or k in want}
    ptrs = PlyOutputs(**{k: C.c_void_p(t.data_ptr()) for k, t in out.items()})
    with torch.cuda.device(dev):
        _lib.call("lsr_ply_unpack", C.byref(layout), C.c_void_p(rows.data_ptr()), _OPACITY_FLAGS[opacity], C.byref(ptrs),
                  _args.stream(dev))
    return out


def _scene(out: dict, K: int) -> Scene3DGS:
    return Scene3DGS(means=out["means"], covariances=out["cov3D"], opacities=out["opacities"], shs=out["shs"],
                     scales=out["scales"], rotations=out["rotations"], sh_degree=isqrt(K) - 1)


def unpack_vertices(rows: Tensor, names: Sequence[str], *, opacity: str = "logit") -> Scene3DGS:
    """``rows (n, len(names))`` on the device, one column per property name, to a :class:`Scene3DGS`."""
    layout = layout_from_names(names, rows.shape[0])
    return _scene(unpack_table(rows, layout, opacity), layout.sh_coeffs)


def read_header(path) -> PlyLayout:
    """The layout ``lsr_ply_read_header`` parses from the file (host only)."""
    layout = PlyLayout()
    _lib.call("lsr_ply_read_header", os.fsencode(str(path)), C.byref(layout))
    return layout


def load_ply(path, device, *, opacity: str = "logit") -> Scene3DGS:
    """Read a binary little-endian 3DGS scene file and unpack it on ``device``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.LsrError("load_ply unpacks on the MI355X: the device must be a ROCm ('cuda') device; "
                            "there is no CPU fallback")
    if opacity not in _OPACITY_FLAGS:
        raise _lib.LsrError(f"opacity must be 'logit' or 'raw', got {opacity!r}")
    layout = read_header(path)
    host = torch.empty((layout.n, layout.stride), dtype=torch.float32, pin_memory=True)
    _lib.call("lsr_ply_read_rows", os.fsencode(str(path)), C.c_void_p(host.data_ptr()), host.numel())
    return _scene(unpack_table(host.to(device, non_blocking=True), layout, opacity), layout.sh_coeffs)


def load_points_ply(path, device):
    """A point cloud file (the published trainer's ``points3D.ply``: binary little-endian ``x y z`` as float or double,
    optional uchar ``red green blue``, anything else skipped) as ``(points (n, 3), colors (n, 3) in [0, 1] or None)``,
    float32 on ``device``.  The library's host reader (``lsr_ply_read_points``); what
    :meth:`latentsplat_amd.scene_model.GaussianScene.from_point_cloud` starts from."""
    device = torch.device(device)
    n, has_colors = C.c_int64(0), C.c_int32(0)
    name = os.fsencode(str(path))
    _lib.call("lsr_ply_read_points_header", name, C.byref(n), C.byref(has_colors))
    pin = device.type == "cuda"
    xyz = torch.empty((n.value, 3), dtype=torch.float32, pin_memory=pin)
    rgb = torch.empty((n.value, 3), dtype=torch.float32, pin_memory=pin) if has_colors.value else None
    _lib.call("lsr_ply_read_points", name, ptr(xyz), ptr(rgb), n.value)
    return xyz.to(device), None if rgb is None else rgb.to(device)
