"""Bilateral-grid appearance compensation for a trainable 3DGS scene, in HIP (csrc/bilagrid.hip, C ABI
include/lsr_bilagrid.h).

Photographs of one capture do not agree with each other: auto-exposure, white balance and vignetting change from one to
the next, and a scene fitted to them bakes the disagreement into floaters and view-dependent colour.  The remedy sits
between ``scene.render(...)`` and ``photometric_loss(...)``: one small learnable colour transform per training image.

* The published 3DGS trainer learns one 3 x 4 colour affine per image.
* "Bilateral Guided Radiance Field Processing" (Wang et al., SIGGRAPH 2024; gsplat's ``use_bilateral_grid``) learns one
  bilateral grid per image: a 16 x 16 x 8 table of 3 x 4 affines that every pixel slices by position and luminance, kept
  smooth by a total-variation term of weight 10.

A grid of size 1 x 1 x 1 is exactly the per-image affine, so one operator covers both.

:func:`bilagrid_slice` slices and applies (autograd in the grids and in the image), :func:`bilagrid_tv` is the total
variation, :class:`BilateralGrid` holds the parameter.  Definitions: include/lsr_bilagrid.h.  The grid gradient is summed
with float atomics: reproducible to summation order, not bit for bit; everything else gives the same bits every call.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor, nn

from . import _args, _lib
from ._args import ptr


def _check_grids(what: str, grids: Tensor) -> None:
    if not torch.is_tensor(grids) or not grids.is_cuda or grids.dtype != torch.float32:
        raise _lib.LsrError(f"{what} needs float32 ROCm tensors (no CPU fallback): grids is not one")
    if grids.dim() != 5 or grids.shape[1] != 12 or grids.numel() == 0:
        raise _lib.LsrError(f"grids must be (N, 12, L, Y, X), got {tuple(grids.shape)}")


def _dims(grids: Tensor, image_shape=(1, 3, 1, 1)) -> _lib.BilagridDims:
    N, _, L, Y, X = grids.shape
    V, _, H, W = image_shape
    return _lib.BilagridDims(num_views=V, height=H, width=W, num_grids=N, grid_l=L, grid_y=Y, grid_x=X, reserved0=0)


def _check_slice(grids: Tensor, image: Tensor, grid_idx: Tensor) -> None:
    _check_grids("bilagrid_slice", grids)
    if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.float32:
        raise _lib.LsrError("bilagrid_slice needs float32 ROCm tensors (no CPU fallback): image is not one")
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0:
        raise _lib.LsrError(f"image must be (V, 3, H, W), got {tuple(image.shape)}")
    if not torch.is_tensor(grid_idx) or grid_idx.dtype != torch.int32 or grid_idx.shape != (image.shape[0],):
        raise _lib.LsrError(f"grid_idx must be an int32 tensor of shape ({image.shape[0]},), one grid index per view")
    if image.device != grids.device or grid_idx.device != grids.device:
        raise _lib.LsrError(f"grids, image and grid_idx must be on one device ({grids.device})")


def slice_path(grids: Tensor, image: Tensor) -> int:
    """``lsr_bilagrid_slice_path``: the kernel path of these shapes, 32 or 16 (the edge of the pixel tile whose grid
    footprint is staged in LDS) or 0 (no tile's footprint fits: the parameter is read directly)."""
    rc = _lib.load().lsr_bilagrid_slice_path(C.byref(_dims(grids, image.shape)))
    if rc < 0:
        _lib.check(rc, "lsr_bilagrid_slice_path")
    return rc


def slice_forward(grids: Tensor, image: Tensor, grid_idx: Tensor) -> Tensor:
    """``lsr_bilagrid_slice_forward`` as it is (no autograd): the compensated images ``(V, 3, H, W)``."""
    _check_slice(grids, image, grid_idx)
    g, x, idx = grids.detach().contiguous(), image.detach().contiguous(), grid_idx.contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        stream = _args.stream(x)
        _lib.call("lsr_bilagrid_slice_forward", C.byref(_dims(g, x.shape)), ptr(g), ptr(x), ptr(idx), ptr(out), stream)
    return out


def slice_backward(grids: Tensor, image: Tensor, grid_idx: Tensor, grad_out: Tensor, grad_grids: Tensor = None, *,
                   want_grids: bool = True):
    """``lsr_bilagrid_slice_backward`` as it is: ``(grad_image, grad_grids)`` for the upstream gradient ``grad_out`` of the
    compensated images.  ``grad_grids``, when given, is a contiguous float32 tensor of the grids' shape that the call
    overwrites (it may be a view into a larger buffer).  ``want_grids=False`` (frozen grids): the grid gradient is neither
    allocated nor computed and comes back as ``None``; ``grad_image`` has the same bits."""
    _check_slice(grids, image, grid_idx)
    if not torch.is_tensor(grad_out) or grad_out.device != image.device or grad_out.dtype != torch.float32 or grad_out.shape != image.shape:
        raise _lib.LsrError("grad_out must be a float32 tensor of the image's shape on its device")
    g, x, idx, up = grids.detach().contiguous(), image.detach().contiguous(), grid_idx.contiguous(), grad_out.detach().contiguous()
    if not want_grids:
        if grad_grids is not None:
            raise _lib.LsrError("grad_grids was given but want_grids is False")
    elif grad_grids is None:
        grad_grids = torch.empty_like(g)
    elif (grad_grids.shape != g.shape or grad_grids.dtype != torch.float32 or grad_grids.device != g.device
          or not grad_grids.is_contiguous()):
        raise _lib.LsrError("grad_grids must be a contiguous float32 tensor of the grids' shape on their device")
    grad_image = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call("lsr_bilagrid_slice_backward", C.byref(_dims(g, x.shape)), ptr(g), ptr(x), ptr(idx), ptr(up),
                  ptr(grad_image), ptr(grad_grids) if want_grids else None, _args.stream(x))
    return grad_image, grad_grids


def tv_forward(grids: Tensor) -> Tensor:
    """``lsr_bilagrid_tv_forward`` as it is (no autograd): the total variation as a one-element tensor."""
    _check_grids("bilagrid_tv", grids)
    g = grids.detach().contiguous()
    lib = _lib.load()
    dims = _dims(g)
    tv = torch.empty(1, dtype=torch.float32, device=g.device)
    workspace = _args.loss_workspace(lib.lsr_bilagrid_tv_workspace_bytes(C.byref(dims)), g.device)
    with torch.cuda.device(g.device):
        _lib.call("lsr_bilagrid_tv_forward", C.byref(dims), ptr(g), ptr(workspace), ptr(tv), _args.stream(g))
    return tv


def tv_backward(grids: Tensor, grad_tv: Tensor) -> Tensor:
    """``lsr_bilagrid_tv_backward`` as it is: ``grad_tv * d tv / d grids``; ``grad_tv`` is a one-element float32 tensor on
    the device."""
    _check_grids("bilagrid_tv", grids)
    g, up = grids.detach().contiguous(), _args.upstream("grad_tv", grad_tv, grids.device, "one element on the grids' device")
    grad = torch.empty_like(g)
    with torch.cuda.device(g.device):
        _lib.call("lsr_bilagrid_tv_backward", C.byref(_dims(g)), ptr(g), ptr(up), ptr(grad), _args.stream(g))
    return grad


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, image, grid_idx):
        ctx.save_for_backward(grids, image, grid_idx)
        return slice_forward(grids, image, grid_idx)

    @staticmethod
    def backward(ctx, grad_out):
        grids, image, grid_idx = ctx.saved_tensors
        grad_image, grad_grids = slice_backward(grids, image, grid_idx, grad_out, want_grids=ctx.needs_input_grad[0])
        return grad_grids, (grad_image if ctx.needs_input_grad[1] else None), None


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        ctx.save_for_backward(grids)
        return tv_forward(grids).reshape(())

    @staticmethod
    def backward(ctx, grad_tv):
        grids, = ctx.saved_tensors
        # the upstream gradient stays on the device: the kernel reads it there
        return tv_backward(grids, grad_tv)


def bilagrid_slice(grids: Tensor, image: Tensor, grid_idx: Tensor) -> Tensor:
    """Slice the bilateral grids ``grids (N, 12, L, Y, X)`` by pixel position and luminance and apply the interpolated 3 x 4
    affine to every pixel of ``image (V, 3, H, W)``; view ``v`` uses grid ``grid_idx[v]`` (``int32 (V,)`` on the device; an
    index outside ``[0, N)`` passes the view through untouched, bit for bit, both ways).  Channel ``4 r + k`` of a grid is
    entry ``(r, k)`` of the matrix.  The same function as ``F.grid_sample(grids[idx], 2 (x, y, luma) - 1, "bilinear",
    "border", align_corners=True)`` followed by the affine, with ``(x, y) = ((col + 0.5) / W, (row + 0.5) / H)`` and
    ``luma = 0.299 r + 0.587 g + 0.114 b``.  Differentiable in ``grids`` and ``image``: one HIP launch forward, two backward."""
    _check_slice(grids, image, grid_idx)
    return _Slice.apply(grids, image, grid_idx)


def bilagrid_tv(grids: Tensor) -> Tensor:
    """Total variation of ``grids (N, 12, L, Y, X)`` as a scalar: over the three grid axes of size >= 2, the sum of
    ``mean((g[i + 1] - g[i]) ** 2)``.  Differentiable; deterministic both ways."""
    _check_grids("bilagrid_tv", grids)
    return _TotalVariation.apply(grids)


class BilateralGrid(nn.Module):
    """``num`` bilateral grids of ``grid_l x grid_y x grid_x`` colour affines, one per training image, initialised to the
    identity: the parameter ``grids (num, 12, grid_l, grid_y, grid_x)`` in the published layout.  The defaults, 16 x 16 x 8,
    are the published ones; ``BilateralGrid(num, 1, 1, 1)`` is one 3 x 4 affine per image, the published 3DGS trainer's
    exposure compensation."""

    def __init__(self, num: int, grid_x: int = 16, grid_y: int = 16, grid_l: int = 8):
        super().__init__()
        if num < 1 or not 1 <= grid_x <= _lib.BILAGRID_MAX_XY or not 1 <= grid_y <= _lib.BILAGRID_MAX_XY or not 1 <= grid_l <= _lib.BILAGRID_MAX_L:
            raise _lib.LsrError(f"BilateralGrid takes num >= 1, 1..{_lib.BILAGRID_MAX_XY} nodes in x and y and 1..{_lib.BILAGRID_MAX_L} "
                                f"in luminance, got {num}, {grid_x}, {grid_y}, {grid_l}")
        identity = torch.eye(3, 4, dtype=torch.float32).reshape(1, 12, 1, 1, 1)
        self.grids = nn.Parameter(identity.repeat(num, 1, grid_l, grid_y, grid_x))

    def forward(self, image: Tensor, grid_idx: Tensor) -> Tensor:
        """:func:`bilagrid_slice` of ``image (V, 3, H, W)`` with grid ``grid_idx[v]`` for view ``v``."""
        return bilagrid_slice(self.grids, image, grid_idx)

    def tv_loss(self) -> Tensor:
        """:func:`bilagrid_tv` of the parameter."""
        return bilagrid_tv(self.grids)

    def affine(self) -> Tensor:
        """The ``(num, 3, 4)`` colour affines of 1 x 1 x 1 grids (refused for any other size)."""
        if tuple(self.grids.shape[2:]) != (1, 1, 1):
            raise _lib.LsrError(f"affine() is defined for 1 x 1 x 1 grids only, these are {tuple(self.grids.shape[2:])}")
        return self.grids.reshape(-1, 3, 4)
