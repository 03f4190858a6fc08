"""SH coefficient rotation on the MI355X (csrc/sh_rotate.hip, C ABI include/lsr_sh_rotate.h).

``rotate_sh`` has the signature and broadcasting of the reference's
(/root/reference/src/misc/sh_utils.py:100-120) and computes the same matrices — e3nn's
``wigner_D(l, *matrix_to_angles(R))`` — directly from the 3x3 rotation, so e3nn is not needed.
``rotate_harmonics`` is the fused form ``GaussianAdapter`` uses: degree masks, both tensors and
the broadcast over the depth samples in one launch each way
(gaussian_adapter.py:90-93,107-108).  ROCm float32 tensors only — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from math import isqrt, prod
from typing import Optional

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_COEFFS = (1, 4, 9, 16, 25)


def _need_rocm(*tensors: Optional[Tensor]):
    for t in tensors:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise _lib.LsrError("rotate_sh needs float32 ROCm tensors (no CPU fallback)")


def _degree(coeffs: int) -> int:
    if coeffs not in _COEFFS:
        raise _lib.LsrError(f"rotate_sh: {coeffs} coefficients; supported are {_COEFFS} (degree <= 4)")
    return isqrt(coeffs) - 1


def sh_rotation_matrices(rotations: Tensor, degree: int) -> Tensor:
    """(num, 3, 3) rotations, or a (num, 4, 4) camera-to-world table whose rotation corner is read in
    place -> (num, sum_{l <= degree} (2l+1)^2) packed per-band rotation matrices, row-major."""
    _need_rocm(rotations)
    if rotations.dim() != 3 or tuple(rotations.shape[1:]) not in ((3, 3), (4, 4)):
        raise _lib.LsrError("sh_rotation_matrices: rotations must be (num, 3, 3) or (num, 4, 4)")
    rotations = rotations.detach().contiguous()
    num, side = rotations.shape[0], rotations.shape[1]
    tables = torch.empty((num, _lib.sh_rotate_table_floats(degree)), device=rotations.device)
    _lib.call("lsr_sh_rotation_matrices", num, ptr(rotations), side, side * side, degree, ptr(tables), _args.stream(rotations))
    return tables


def _rows_view(t: Tensor) -> tuple[Tensor, int]:
    """(cams, rays, W) -> a tensor the kernel can walk as rows with one stride, and that stride."""
    cams, rays, width = t.shape
    if t.stride(2) == 1 or width == 1:
        if rays > 1:
            st, ok = t.stride(1), cams == 1 or t.stride(0) == t.stride(1) * rays
        else:
            st, ok = (t.stride(0) if cams > 1 else width), True
        if ok and st >= width:
            return t, st
    return t.contiguous(), width


class _ShRotate(torch.autograd.Function):
    """rows (cams, rays, 3 Kc + C Kf) [colour | feature] -> colour (cams, rays, S, 3, Kc) and feature
    (cams, rays, S, C, Kf) (None for an absent tensor).  `tables` are data: no gradient to the rotation."""

    @staticmethod
    def forward(ctx, rows, tables, color_mask, feature_mask, samples, color_coeffs, feat_channels, feat_coeffs):
        _need_rocm(rows, tables, color_mask, feature_mask)
        cams, rays, width = rows.shape
        if width != 3 * color_coeffs + feat_channels * feat_coeffs:
            raise _lib.LsrError("rotate_sh: row width does not match the coefficient counts")
        rows, stride = _rows_view(rows)
        tables = tables.contiguous()
        color_mask = None if color_mask is None else color_mask.contiguous()
        feature_mask = None if feature_mask is None else feature_mask.contiguous()
        dims = _lib.ShRotateDims(cams, rays, samples, color_coeffs, feat_channels if feat_coeffs else 0, feat_coeffs,
                                 tables.shape[1], 0, stride)
        dev = rows.device
        color = torch.empty((cams, rays, samples, 3, color_coeffs), device=dev) if color_coeffs else None
        feature = torch.empty((cams, rays, samples, feat_channels, feat_coeffs), device=dev) if feat_coeffs else None
        _lib.call("lsr_sh_rotate_forward", C.byref(dims), ptr(tables), ptr(rows), ptr(color_mask), ptr(feature_mask),
                  ptr(color), ptr(feature), _args.stream(rows))
        ctx.save_for_backward(tables, color_mask, feature_mask)
        ctx.dims = dims
        ctx.set_materialize_grads(False)
        return color, feature

    @staticmethod
    def backward(ctx, g_color, g_feature):
        tables, color_mask, feature_mask = ctx.saved_tensors
        dims = ctx.dims
        width = 3 * dims.color_coeffs + dims.feat_channels * dims.feat_coeffs
        if g_color is None and g_feature is None:
            return (None,) * 8
        g_color = None if g_color is None else g_color.contiguous()
        g_feature = None if g_feature is None else g_feature.contiguous()
        d_rows = torch.empty((dims.num_cameras, dims.rays, width), device=tables.device)
        _lib.call("lsr_sh_rotate_backward", C.byref(dims), ptr(tables), ptr(g_color), ptr(g_feature), ptr(color_mask),
                  ptr(feature_mask), ptr(d_rows), _args.stream(tables))
        return d_rows, None, None, None, None, None, None, None


def rotate_harmonics(rows: Tensor, rotations: Tensor, samples: int, color_coeffs: int, feat_channels: int,
                     feat_coeffs: int, color_mask: Optional[Tensor] = None, feature_mask: Optional[Tensor] = None):
    """Fused adapter path.  rows (cams, rays, 3 Kc + C Kf): per row the colour coefficients, then the
    feature coefficients (may be a strided view of a wider matrix); rotations (cams, 3, 3) or a
    (cams, 4, 4) camera-to-world table.  Returns (colour (cams, rays, S, 3, Kc) or None,
    feature (cams, rays, S, C, Kf) or None): out = D(R) (mask * in), written for each of the S samples."""
    degree = max(_degree(k) for k in (color_coeffs, feat_coeffs) if k)
    tables = sh_rotation_matrices(rotations, degree)
    return _ShRotate.apply(rows, tables, color_mask, feature_mask, int(samples), int(color_coeffs),
                           int(feat_channels), int(feat_coeffs))


def rotate_sh(sh_coefficients: Tensor, rotations: Tensor) -> Tensor:
    """sh_coefficients (*#batch, n), rotations (*#batch, 3, 3) -> (*batch, n); n a perfect square
    <= 25.  Per band l:  out_l = D_l(R) in_l  with  Y_l(R x) = D_l(R) Y_l(x)  in e3nn's real basis
    (the reference's rotate_sh, sh_utils.py:100-120).  Differentiable in the coefficients; the
    rotations are data."""
    _need_rocm(sh_coefficients, rotations)
    n = sh_coefficients.shape[-1]
    degree = _degree(n)
    if tuple(rotations.shape[-2:]) != (3, 3):
        raise _lib.LsrError("rotate_sh: rotations must be (..., 3, 3)")
    batch = tuple(torch.broadcast_shapes(sh_coefficients.shape[:-1], rotations.shape[:-2]))
    nb = len(batch)
    rb = (1,) * (nb - (rotations.dim() - 2)) + tuple(rotations.shape[:-2])
    # rotations that vary over a leading prefix of the batch only map straight onto [cam][rows]; any
    # other broadcast is made correct by expanding them (p = nb: one rotation per row)
    p = nb
    while p > 0 and rb[p - 1] == 1:
        p -= 1
    cams = prod(batch[:p])
    rot = rotations.detach().reshape(rb + (3, 3))[(slice(None),) * p + (0,) * (nb - p)]
    rot = rot.expand(batch[:p] + (3, 3)).reshape(cams, 3, 3)
    # a trailing batch dim the rotation does not vary over becomes the channel dim of a row
    channels = batch[-1] if p < nb and batch[-1] <= _lib.MAX_FEAT_CHANNELS else 1
    rays = prod(batch[p:]) // channels
    rows = sh_coefficients.expand(batch + (n,)).reshape(cams, rays, channels * n)
    if cams == 0 or rays == 0:
        return rows.reshape(batch + (n,)) * 1.0
    tables = sh_rotation_matrices(rot, degree)
    _, out = _ShRotate.apply(rows, tables, None, None, 1, 0, channels, n)
    return out.reshape(batch + (n,))
