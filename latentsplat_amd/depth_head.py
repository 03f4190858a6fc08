"""Fused depth head on the MI355X (csrc/depth_head.hip, C ABI include/lsr_depth_head.h): the encoder's
depth logits to the sampled ``depths`` and ``opacities`` that ``GaussianAdapter.forward`` takes.

``depth_head`` is the op: softmax / sigmoid of the interleaved logits, sampling (or top-k), relative
disparity to depth, the optional transmittance quotient and the encoder's opacity map, one launch
forward and one backward.  ``DepthPredictorMonocular`` mirrors the reference's module
(src/model/encoder/epipolar/depth_predictor_monocular.py:10-81): same constructor, parameters,
``forward`` signature, shapes and random-generator consumption.  ``opacity_exponent`` is the warm-up
rule of the reference's ``map_pdf_to_opacity`` (src/model/encoder/encoder_epipolar.py:113-126).
ROCm float32 tensors only — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from math import prod
from typing import Optional

import torch
from torch import Tensor, nn

from . import _args, _lib
from ._args import ptr
from .gaussian_adapter import _row_stride


def opacity_exponent(initial: float, final: float, warm_up: int, global_step: int) -> float:
    """``2 ** (initial + min(global_step / warm_up, 1) * (final - initial))``: the exponent
    ``map_pdf_to_opacity`` uses at ``global_step`` (cfg.opacity_mapping)."""
    return 2 ** (initial + min(global_step / warm_up, 1) * (final - initial))


class _DepthHead(torch.autograd.Function):
    """logits (cams, rays, 2 S F) (may be a strided view), near / far (cams,), uniforms (cams, rays, F, k)
    or None -> depth, opacity (float32) and index (int32), each (cams, rays, F, k)."""

    @staticmethod
    def forward(ctx, logits, near, far, uniforms, surfaces, samples, flags, exponent, scale):
        for t in (logits, near, far, uniforms):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32):
                raise _lib.LsrError("depth_head needs float32 ROCm tensors (no CPU fallback)")
        cams, rays, width = logits.shape
        buckets = width // (2 * surfaces)
        stride = _row_stride(logits)
        if stride is None or stride < width:
            logits = logits.contiguous()
            stride = width
        near, far = near.contiguous(), far.contiguous()
        uniforms = None if uniforms is None else uniforms.contiguous()
        dims = _lib.DepthHeadDims(cams, rays, buckets, surfaces, samples, flags, exponent, scale, stride, width)
        dev = logits.device
        shape = (cams, rays, surfaces, samples)
        depth, opacity = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
        index = torch.empty(shape, device=dev, dtype=torch.int32)
        _lib.call("lsr_depth_head_forward", C.byref(dims), ptr(logits), ptr(near), ptr(far), ptr(uniforms), ptr(depth),
                  ptr(opacity), ptr(index), _args.stream(logits))
        ctx.save_for_backward(logits, near, far, index)
        ctx.dims = dims
        ctx.mark_non_differentiable(index)
        ctx.set_materialize_grads(False)
        return depth, opacity, index

    @staticmethod
    def backward(ctx, g_depth, g_opacity, _g_index):
        logits, near, far, index = ctx.saved_tensors
        dims = ctx.dims
        if g_depth is None and g_opacity is None:
            return (None,) * 9
        g_depth = None if g_depth is None else g_depth.contiguous()
        g_opacity = None if g_opacity is None else g_opacity.contiguous()
        # dense rows; for a strided view autograd's own view backward supplies the zeros around them
        d_logits = torch.empty((dims.num_cameras, dims.rays, 2 * dims.buckets * dims.surfaces), device=logits.device)
        _lib.call("lsr_depth_head_backward", C.byref(dims), ptr(logits), ptr(near), ptr(far), ptr(index), ptr(g_depth),
                  ptr(g_opacity), ptr(d_logits), _args.stream(logits))
        return d_logits, None, None, None, None, None, None, None, None


def depth_head(logits: Tensor, near: Tensor, far: Tensor, *, num_surfaces: int, uniforms: Optional[Tensor] = None,
               deterministic: bool = False, num_samples: Optional[int] = None, use_transmittance: bool = False,
               opacity_exponent: float = 1.0, opacity_scale: float = 1.0) -> tuple[Tensor, Tensor, Tensor]:
    """logits (*cams, rays, 2 S F): the depth head's Linear output, channel (bucket F + surface) 2 + c with
    c = 0 the pdf logit and c = 1 the offset logit (may be a strided view of a wider matrix); near, far
    (*cams).  Returns depth, opacity (float32) and index (int32), each (*cams, rays, F, k).

    Stochastic (default): ``uniforms`` (*cams, rays, F, k) in [0, 1] pick the buckets; when None they are
    drawn here with ``torch.rand`` (then ``num_samples`` = k is required).  ``deterministic``: the
    ``num_samples`` most probable buckets in descending order (ties to the lowest index).
    ``opacity = opacity_scale * 0.5 * (1 - (1 - x)**e + x**(1 / e))`` with e = ``opacity_exponent``
    (see :func:`opacity_exponent`) and x the normalised pdf at the index, or the transmittance quotient
    with ``use_transmittance``; e = 1 and scale 1 return x itself.

    Differentiable in ``logits`` only: near / far are constants, nothing flows through the indices or the
    uniforms.  The backward is bitwise reproducible."""
    for name, t in (("near", near), ("far", far)):
        if t.requires_grad:
            raise _lib.LsrError(f"depth_head: {name} requires grad, but the fused head treats near / far as constants")
    surfaces = int(num_surfaces)
    width = logits.shape[-1]
    if logits.dim() < 2 or surfaces < 1 or width % (2 * surfaces) != 0 or width == 0:
        raise _lib.LsrError(f"depth_head: logits (..., rays, {width}) is not 2 * buckets * {surfaces} wide")
    batch = tuple(logits.shape[:-2])
    if tuple(near.shape) != batch or tuple(far.shape) != batch:
        raise _lib.LsrError("depth_head: near / far must have the logits' leading (camera) shape")
    cams, rays = prod(batch), logits.shape[-2]
    if cams == 0:
        raise _lib.LsrError("depth_head: no cameras")
    if uniforms is not None and not deterministic:
        if tuple(uniforms.shape[:-1]) != batch + (rays, surfaces):
            raise _lib.LsrError("depth_head: uniforms must be (*cams, rays, num_surfaces, k)")
        if num_samples is not None and int(num_samples) != uniforms.shape[-1]:
            raise _lib.LsrError("depth_head: num_samples does not match the uniforms")
        samples = uniforms.shape[-1]
    else:
        if num_samples is None:
            raise _lib.LsrError("depth_head: num_samples is required without uniforms")
        samples = int(num_samples)
        uniforms = None
        if not deterministic:
            if not logits.is_cuda:
                raise _lib.LsrError("depth_head needs float32 ROCm tensors (no CPU fallback)")
            uniforms = torch.rand(batch + (rays, surfaces, samples), device=logits.device)
    flags = ((_lib.DEPTH_HEAD_DETERMINISTIC if deterministic else 0)
             | (_lib.DEPTH_HEAD_TRANSMITTANCE if use_transmittance else 0))
    out = _DepthHead.apply(logits.reshape(cams, rays, width), near.detach().reshape(cams), far.detach().reshape(cams),
                           None if uniforms is None else uniforms.detach().reshape(cams, rays, surfaces, samples),
                           surfaces, samples, flags, float(opacity_exponent), float(opacity_scale))
    return tuple(t.reshape(batch + (rays, surfaces, samples)) for t in out)


class DepthPredictorMonocular(nn.Module):
    """Mirror of the reference's ``DepthPredictorMonocular``: ``projection = Sequential(ReLU, Linear)``, so
    a reference checkpoint's ``projection.1.{weight,bias}`` loads unchanged; everything behind the
    projection is the fused HIP head.  ``to_pdf`` / ``to_offset`` are kept as attributes because the
    reference has them ("for hooks to latch onto"; nothing in the reference hooks them) — the fused path
    does NOT call them, so a hook registered on them never fires."""

    def __init__(self, d_in: int, num_samples: int, num_surfaces: int, use_transmittance: bool) -> None:
        super().__init__()
        self.projection = nn.Sequential(nn.ReLU(), nn.Linear(d_in, 2 * num_samples * num_surfaces))
        self.num_samples = num_samples          # the reference's name for the number of depth buckets
        self.num_surfaces = num_surfaces
        self.use_transmittance = use_transmittance
        self.to_pdf = nn.Softmax(dim=-1)
        self.to_offset = nn.Sigmoid()

    def forward(self, features: Tensor, near: Tensor, far: Tensor, deterministic: bool, gaussians_per_pixel: int, *,
                uniforms: Optional[Tensor] = None, opacity_exponent: float = 1.0, opacity_scale: float = 1.0
                ) -> tuple[Tensor, Tensor]:
        """features (b, v, r, d_in), near / far (b, v) -> depth, opacity (b, v, r, srf, gaussians_per_pixel).
        Stochastic without ``uniforms``: one ``torch.rand((b, v, r, srf, spp), device=...)`` is drawn,
        the reference's own call, so the generator is consumed identically.  With the defaults the
        second output is the reference's (the sampled pdf); the keyword-only extras fold the
        encoder's ``map_pdf_to_opacity(...) / gaussians_per_pixel`` into the same launch."""
        logits = self.projection(features)
        depth, opacity, _ = depth_head(logits, near, far, num_surfaces=self.num_surfaces, uniforms=uniforms,
                                       deterministic=deterministic, num_samples=gaussians_per_pixel,
                                       use_transmittance=self.use_transmittance,
                                       opacity_exponent=opacity_exponent, opacity_scale=opacity_scale)
        return depth, opacity
