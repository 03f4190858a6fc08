"""3DGS ``.ply`` export.  Two writers: ``export_ply``, the mirror of the reference's (a viewer's copy: recentred, rescaled,
rotated, DC band only), and ``save_ply`` / ``save_gaussians`` / ``pack_scene`` further down, which keep the scene (every SH
band, logit opacities, scales and rotations taken from the covariances) in the published layout that ``load_ply`` reads.

``export_ply`` — mirror of /root/reference/src/model/ply_export.py (``export_ply`` :26-92,
``construct_list_of_attributes`` :13-23) on the MI355X: the per-Gaussian transform and the 17-float
vertex packing run as one HIP kernel (csrc/ply.hip, C ABI include/lsr_ply.h), the file is written
by the library's host writer.  ROCm float32 tensors only; no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr
from ._lib import PLY_VERTEX_FLOATS, PlyInputs


def construct_list_of_attributes(num_rest: int) -> list[str]:
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
    names += [f"f_rest_{i}" for i in range(num_rest)] + ["opacity"]
    return names + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]


def pack_vertices(extrinsics: Tensor, means: Tensor, scales: Tensor, rotations: Tensor, harmonics: Tensor,
                  opacities: Tensor) -> Tensor:
    """(gaussian, 17) float32 vertex records on the device, in the order of
    ``construct_list_of_attributes(0)``."""
    tensors = [extrinsics, means, scales, rotations, harmonics, opacities]
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError("export_ply needs float32 ROCm tensors (no CPU fallback)")
    extrinsics, means, scales, rotations, harmonics, opacities = (t.detach().contiguous() for t in tensors)
    n = means.shape[0]
    if harmonics.dim() != 3 or harmonics.shape[1] != 3:
        raise _lib.LsrError("harmonics must be (gaussian, 3, d_sh)")
    # the two global statistics of ply_export.py:35-41 (torch reductions on the device)
    center = means.median(dim=0).values.contiguous()
    scale_factor = (means - center).abs().quantile(0.95, dim=0).max().reshape(1).contiguous()
    out = torch.empty((n, PLY_VERTEX_FLOATS), device=means.device)
    inp = PlyInputs(ptr(extrinsics), ptr(means), ptr(scales), ptr(rotations), ptr(harmonics), ptr(opacities), ptr(center),
                    ptr(scale_factor))
    _lib.call("lsr_ply_pack", n, harmonics.shape[2], C.byref(inp), ptr(out), _args.stream(means))
    return out


def export_ply(extrinsics: Tensor, means: Tensor, scales: Tensor, rotations: Tensor, harmonics: Tensor,
               opacities: Tensor, path: Path) -> None:
    vertices = pack_vertices(extrinsics, means, scales, rotations, harmonics, opacities).cpu().contiguous()
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    _lib.call("lsr_ply_write_host", os.fsencode(str(path)), C.c_void_p(vertices.data_ptr()), vertices.shape[0])


# ---- scene export: a standard 3DGS scene file that keeps the scene (every SH band, logit opacities, geometry taken from
# the covariances), the inverse of latentsplat_amd.ply_import.  C ABI: include/lsr_ply.h, "scene export". ----

_CONVENTIONS = {"3dgs": _lib.SH_AXES_3DGS, "reference": _lib.SH_AXES_REFERENCE}


def pack_scene(means: Tensor, opacities: Tensor, shs: Tensor, *, covariances: Optional[Tensor] = None,
               scales: Optional[Tensor] = None, rotations: Optional[Tensor] = None, convention: Optional[str] = None,
               channel_major: Optional[bool] = None, max_sh_degree: Optional[int] = None) -> Tensor:
    """``(n, 14 + 3 K_out)`` float32 rows on the device in the order of ``construct_list_of_attributes(3 (K_out - 1))``
    (``lsr_ply_pack_scene``: one HIP kernel).

    Geometry is exactly one of ``covariances`` (``(n, 6)`` xx,xy,xz,yy,yz,zz or ``(n, 3, 3)``: decomposed on the device
    into log-scales and a quaternion) or ``scales (n, 3)`` with ``rotations (n, 4)`` w,x,y,z.  ``shs`` is ``(n, K, 3)`` or,
    channel-major, ``(n, 3, K)``; ``channel_major=None`` reads the layout off the shape.  ``convention`` is the basis the
    coefficients are in (``None``: the one this process renders with, ``get_color_sh_convention()``); ``"reference"``
    coefficients are changed to the ``"3dgs"`` basis the file format means.  ``max_sh_degree`` keeps the lower bands."""
    if (covariances is None) == (scales is None and rotations is None) or (scales is None) != (rotations is None):
        raise _lib.LsrError("pack_scene takes exactly one of covariances=, or scales= with rotations=")
    if shs.dim() != 3:
        raise _lib.LsrError(f"shs must be (n, K, 3) or (n, 3, K), got {tuple(shs.shape)}")
    if channel_major is None:
        if shs.shape[1] == 3 and shs.shape[2] == 3:
            raise _lib.LsrError("shs of shape (n, 3, 3) is ambiguous: say channel_major=True for (n, 3, K) or False for (n, K, 3)")
        if shs.shape[1] != 3 and shs.shape[2] != 3:
            raise _lib.LsrError(f"shs must be (n, K, 3) or (n, 3, K), got {tuple(shs.shape)}")
        channel_major = shs.shape[2] != 3
    if shs.shape[1 if channel_major else 2] != 3:
        raise _lib.LsrError(f"shs must be {'(n, 3, K)' if channel_major else '(n, K, 3)'}, got {tuple(shs.shape)}")
    K_in = shs.shape[2 if channel_major else 1]
    if K_in not in (1, 4, 9, 16, 25):
        raise _lib.LsrError(f"{K_in} SH coefficients per channel: expected 1, 4, 9, 16 or 25")
    K_out = K_in if max_sh_degree is None else min(K_in, (int(max_sh_degree) + 1) ** 2)
    if max_sh_degree is not None and max_sh_degree < 0:
        raise _lib.LsrError("max_sh_degree must be >= 0")
    if convention is None:
        from .rasterizer import get_color_sh_convention
        convention = get_color_sh_convention()
    if convention not in _CONVENTIONS:
        raise _lib.LsrError(f"convention must be '3dgs' or 'reference', got {convention!r}")
    given = [t for t in (means, opacities, shs, covariances, scales, rotations) if t is not None]
    for t in given:
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError("pack_scene needs float32 ROCm tensors (no CPU fallback)")
    n, dev = means.shape[0], means.device
    c = lambda t: None if t is None else t.detach().contiguous()
    means, opacities, shs, scales, rotations = c(means), c(opacities).reshape(-1), c(shs), c(scales), c(rotations)
    cov_elems = 0
    if covariances is not None:
        if tuple(covariances.shape) not in ((n, 6), (n, 3, 3)):
            raise _lib.LsrError(f"covariances must be (n, 6) or (n, 3, 3), got {tuple(covariances.shape)}")
        covariances = c(covariances)
        cov_elems = 6 if covariances.dim() == 2 else 9
    elif tuple(scales.shape) != (n, 3) or tuple(rotations.shape) != (n, 4):
        raise _lib.LsrError("scales must be (n, 3) and rotations (n, 4)")
    if tuple(means.shape) != (n, 3) or opacities.shape[0] != n or shs.shape[0] != n:
        raise _lib.LsrError("means must be (n, 3), opacities (n,) or (n, 1), shs n Gaussians")
    rows = torch.empty((n, _lib.ply_scene_row_floats(K_out)), dtype=torch.float32, device=dev)
    inp = _lib.PlySceneInputs(ptr(means), ptr(opacities), ptr(shs), ptr(covariances), ptr(scales), ptr(rotations), K_in,
                              int(bool(channel_major)), cov_elems, 0)
    opts = _lib.PlySceneOpts(_CONVENTIONS[convention], K_out, 0, 0)
    with torch.cuda.device(dev):
        _lib.call("lsr_ply_pack_scene", n, C.byref(inp), C.byref(opts), ptr(rows), _args.stream(dev))
    return rows


def save_ply(path, means: Tensor, opacities: Tensor, shs: Tensor, **opts) -> None:
    """Write a standard 3DGS scene file (binary little-endian, the published ``point_cloud.ply`` layout) that
    :func:`latentsplat_amd.ply_import.load_ply` and standard viewers read.  Arguments as :func:`pack_scene`."""
    rows = pack_scene(means, opacities, shs, **opts)
    host = torch.empty(rows.shape, dtype=torch.float32, pin_memory=True)
    host.copy_(rows)                                    # (device to pinned host: synchronises with the packing stream)
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    K = (rows.shape[1] - 14) // 3
    _lib.call("lsr_ply_write_scene_host", os.fsencode(str(path)), C.c_void_p(host.data_ptr()), rows.shape[0], K)


def save_gaussians(path, gaussians, scene: int = 0, **opts) -> None:
    """One scene of the decoder's ``Gaussians`` / ``VariationalGaussians`` (``means (b, g, 3)``, ``covariances
    (b, g, 3, 3)``, ``opacities (b, g)``, ``color_harmonics (b, g, 3, K)``) as a scene file."""
    if gaussians.color_harmonics is None:
        raise _lib.LsrError("save_gaussians needs color_harmonics: a scene file stores colour SH (feature harmonics have no "
                            "standard representation)")
    opts.setdefault("channel_major", True)
    save_ply(path, gaussians.means[scene], gaussians.opacities[scene], gaussians.color_harmonics[scene],
             covariances=gaussians.covariances[scene], **opts)
