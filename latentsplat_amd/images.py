"""Photographs onto the rasterizer's camera, in HIP (csrc/image_prepare.hip; C ABI include/lsr_image.h).

The camera table of this package (:func:`latentsplat_amd.rasterizer.build_view_table`) is a symmetric frustum from the focal
lengths alone: a centred principal point and no lens distortion, as in the published trainer.  A photograph whose camera
was calibrated with an off-centre principal point, or with one of COLMAP's distortion models, disagrees with what the
rasterizer can render.  :func:`prepare_images` resamples a batch of photographs of ONE source camera onto the centred,
distortion-free pinhole camera at the training resolution, in one launch, and reports per output pixel how much of it the
photograph covers, so that a loss can leave the rest out.

uint8 ROCm tensors in, float32 ROCm tensors out; there is no CPU fallback.  Values only: targets need no gradient."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_DIST_USED = {0: 0, 1: 0, 2: 1, 3: 2, 4: 4}     # distortion numbers per model


@dataclass(frozen=True)
class SourceCamera:
    """The camera that took the photographs, in source pixels.  ``model`` is COLMAP's id: 0 ``SIMPLE_PINHOLE``, 1
    ``PINHOLE``, 2 ``SIMPLE_RADIAL`` (``dist = (k,)``), 3 ``RADIAL`` (``(k1, k2)``), 4 ``OPENCV`` (``(k1, k2, p1, p2)``)."""
    model: int
    fx: float
    fy: float
    cx: float
    cy: float
    dist: Sequence[float] = ()

    @classmethod
    def from_colmap(cls, model: int, params: Sequence[float]) -> "SourceCamera":
        """From a COLMAP model id and its parameters in COLMAP's order (``f cx cy``, ``fx fy cx cy``, ``f cx cy k``,
        ``f cx cy k1 k2``, ``fx fy cx cy k1 k2 p1 p2``; a longer list's tail is ignored)."""
        model = int(model)
        if model not in _lib.COLMAP_MODELS:
            raise _lib.LsrError(f"camera model {model} is not one of {sorted(n for n, _ in _lib.COLMAP_MODELS.values())}")
        p = [float(x) for x in params][: _lib.COLMAP_MODELS[model][1]]
        if len(p) != _lib.COLMAP_MODELS[model][1]:
            raise _lib.LsrError(f"{_lib.COLMAP_MODELS[model][0]} takes {_lib.COLMAP_MODELS[model][1]} parameters, got {len(p)}")
        if model in (0, 2, 3):       # one focal length
            return cls(model, p[0], p[0], p[1], p[2], tuple(p[3:]))
        return cls(model, p[0], p[1], p[2], p[3], tuple(p[4:]))

    def struct(self) -> _lib.ImageCamera:
        if self.model not in _DIST_USED or len(self.dist) != _DIST_USED[self.model]:
            raise _lib.LsrError(f"camera model {self.model} takes {_DIST_USED.get(self.model, '?')} distortion numbers, got {len(self.dist)}")
        dist = (C.c_float * 4)(*[float(x) for x in self.dist])
        return _lib.ImageCamera(model=int(self.model), reserved=0, fx=float(self.fx), fy=float(self.fy), cx=float(self.cx),
                                cy=float(self.cy), dist=dist)


def _dims(images_u8: Tensor, height: int, width: int, fx: float, fy: float) -> _lib.ImageDims:
    B, Hs, Ws, Cn = images_u8.shape
    return _lib.ImageDims(batch=B, src_height=Hs, src_width=Ws, channels=Cn, height=int(height), width=int(width),
                          fx=float(fx), fy=float(fy))


def subsamples(camera: SourceCamera, fx: float, fy: float) -> int:
    """``lsr_image_subsamples``: ``S = ceil(max(camera.fx / fx, camera.fy / fy, 1))`` in float32, the sub-samples per axis
    that :func:`prepare_images` averages per output pixel; more than 16 is refused."""
    d = _lib.ImageDims(batch=0, src_height=1, src_width=1, channels=3, height=1, width=1, fx=float(fx), fy=float(fy))
    cam = camera.struct()
    S = _lib.load().lsr_image_subsamples(C.byref(d), C.byref(cam))
    _lib.check(min(S, 0), "lsr_image_subsamples")
    return S


def prepare_images(images_u8: Tensor, camera: SourceCamera, height: int, width: int, fx: float, fy: float,
                   background: Optional[Tensor] = None):
    """``lsr_image_prepare``: ``(image (B, 3, height, width), coverage (B, height, width))``, float32, from the photographs
    ``images_u8 (B, Hs, Ws, C)`` (uint8, ``C`` 3 or 4, a ROCm tensor) of the source ``camera``.

    The target camera is a centred pinhole with the focal lengths ``fx, fy`` in output pixels.  Every output pixel averages
    ``S x S`` sub-samples (:func:`subsamples`), each mapped into the photograph through the source camera's principal point
    and distortion and read with bilinear interpolation; ``image`` is the mean over the sub-samples that land inside the
    photograph, divided by 255, and ``coverage`` their share (0 where the photograph has nothing to say: mask the loss with
    it).  RGBA photographs are composited over ``background`` (``(3,)``, default black).  For a power-of-two reduction of a
    pinhole photograph with a half-integer principal-point shift every operation is exact: the result is the block mean.

    One launch, no atomics, the same bits every call, graph-capturable; nothing is read back."""
    if not torch.is_tensor(images_u8) or not images_u8.is_cuda or images_u8.dtype != torch.uint8:
        raise _lib.LsrError("prepare_images needs a uint8 ROCm tensor of images (no CPU fallback): images_u8 is not one")
    if images_u8.dim() != 4 or images_u8.shape[3] not in (3, 4):
        raise _lib.LsrError(f"images_u8 must be (B, Hs, Ws, 3 or 4), got {tuple(images_u8.shape)}")
    dev = images_u8.device
    if background is None:
        background = torch.zeros(3, dtype=torch.float32, device=dev)
    background = _args.f32("prepare_images", "background", background, (3,), dev)
    d, cam = _dims(images_u8, height, width, fx, fy), camera.struct()
    src = images_u8.contiguous()
    B = src.shape[0]
    # (the library's checks come before the allocation: a refused call allocates nothing)
    _lib.call("lsr_image_prepare", C.byref(_lib.ImageDims(batch=0, src_height=d.src_height, src_width=d.src_width, channels=d.channels,
                                                          height=d.height, width=d.width, fx=d.fx, fy=d.fy)),
              C.byref(cam), None, None, None, None, None)
    image = torch.empty((B, 3, int(height), int(width)), dtype=torch.float32, device=dev)
    coverage = torch.empty((B, int(height), int(width)), dtype=torch.float32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call("lsr_image_prepare", C.byref(d), C.byref(cam), ptr(src), ptr(background.contiguous()), ptr(image), ptr(coverage),
                      _args.stream(dev))
    return image, coverage
