"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024) for a trainable 3DGS scene, in HIP (csrc/filter3d.hip and
csrc/scene_params.hip; C ABI include/lsr_filter3d.h and include/lsr_scene.h).

A scene fitted at one distance erodes and grows needles when it is viewed from closer than the training cameras were:
nothing bounds how small a Gaussian may become relative to the cameras that supervised it.  The remedy: for each Gaussian
take the highest sampling rate (focal length over depth) among the training cameras that see it, convolve the Gaussian with
an isotropic low-pass of that size inside the activation, and correct the opacity by the determinant ratio.

:func:`compute_filter_3d` is the (Gaussians x cameras) pass, one HIP kernel that reads each position once;
:func:`activate_scene_filtered` is :func:`latentsplat_amd.scene_model.activate_scene` with the filter inside the same single
launch each way; :func:`fused_parameters` bakes the filter into opacity logits and log-scales for a scene file that any
viewer shows filtered.  :class:`latentsplat_amd.scene_model.GaussianScene` takes the filter in ``activated``, ``render``
and ``save_ply``.

The other half of Mip-Splatting, the screen-space 2D box filter that replaces the rasterizer's +0.3 dilation, is NOT
built: it lives inside the projection kernel, behind the rasterizer's ABI.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr
from .scene_model import _ActivateSceneFiltered, _filter, activate_forward


def compute_filter_3d(xyz: Tensor, views: Tensor, width: int, *, margin: float = 0.15, variance: float = 0.2,
                      per_view: bool = False, return_seen: bool = False):
    """``lsr_filter3d_compute``: the 3D filter ``(n, 1)`` of the positions ``xyz (n, 3)`` for the training cameras ``views
    (V, 44)`` (a table of ``build_view_table`` / ``make_view_table``) at image width ``width`` in pixels.

    A Gaussian is seen by a camera when it lies beyond the rasterizer's near plane and inside the frustum widened by
    ``margin`` of the image on each side (0.15: the published test).  Its filter is ``sqrt(variance)`` (0.2 published)
    times the smallest depth among the cameras that see it over the largest focal length of all cameras — the published
    rule — or, with ``per_view``, over the largest ``focal / depth`` among the cameras that see it, which is the same
    when all focal lengths agree and the exact bound when they do not.  A Gaussian no camera sees takes the largest
    filter among the seen ones; when none is seen, every filter is 0.  ``return_seen``: also the ``(n,)`` bool mask.

    Three launches whatever the number of cameras, nothing read back, two calls give the same bits."""
    for name, t in (("xyz", xyz), ("views", views)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError(f"compute_filter_3d needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.LsrError(f"xyz must be (n, 3), got {tuple(xyz.shape)}")
    if views.dim() != 2 or views.shape[1] != _lib.VIEW_FLOATS:
        raise _lib.LsrError(f"views must be (V, {_lib.VIEW_FLOATS}), got {tuple(views.shape)}")
    n, V, dev = xyz.shape[0], views.shape[0], xyz.device
    if views.device != dev:
        raise _lib.LsrError(f"views must be on {dev}")
    if n >= _lib.FILTER3D_MAX_ROWS or not 1 <= V <= _lib.FILTER3D_MAX_VIEWS:
        raise _lib.LsrError(f"compute_filter_3d takes fewer than 2^28 Gaussians and 1..{_lib.FILTER3D_MAX_VIEWS} cameras, got {n} and {V}")
    lib = _lib.load()
    filt = torch.empty((n, 1), dtype=torch.float32, device=dev)
    seen = torch.empty(n, dtype=torch.uint8, device=dev) if return_seen else None
    if n > 0:
        pts, table = xyz.detach().contiguous(), views.detach().contiguous()
        ws = _args.workspace(lib.lsr_filter3d_workspace_bytes(n, V), dev)
        mode = _lib.FILTER3D_PER_VIEW if per_view else _lib.FILTER3D_PUBLISHED
        with torch.cuda.device(dev):
            _lib.call("lsr_filter3d_compute", n, ptr(pts), V, ptr(table), int(width), float(margin), float(variance), mode,
                      ptr(filt), ptr(seen), ptr(ws), _args.stream(dev))
    else:      # the argument checks of the library, which launches nothing
        _lib.call("lsr_filter3d_compute", 0, None, V, None, int(width), float(margin), float(variance),
                  _lib.FILTER3D_PER_VIEW if per_view else _lib.FILTER3D_PUBLISHED, None, None, None, None)
    return (filt, seen.bool()) if return_seen else filt


def activate_scene_filtered(features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor, rotation: Tensor,
                            filter_3d: Tensor, scale_modifier: float = 1.0):
    """:func:`latentsplat_amd.scene_model.activate_scene` with the 3D filter ``filter_3d`` (``(n, 1)`` or ``(n,)``) inside
    it, differentiable in the five parameters: ``(shs, opacities, cov3D)``.  With ``s = exp(scaling)``, ``f`` the filter
    and ``v = s^2 + f^2``: ``cov3D = R diag(m^2 v) R^T`` and ``opacities = sigmoid(opacity) prod_k s_k / sqrt(v_k)``; the
    SH tensor as in the unfiltered map.  The filter is a constant of the map (no gradient).  One HIP launch forward, one
    backward; float32 ROCm tensors only."""
    for t in (features_dc, features_rest, opacity, scaling, rotation, filter_3d):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError("activate_scene_filtered needs float32 ROCm tensors (no CPU fallback)")
    filt = _filter(filter_3d, opacity.shape[0], opacity.device)
    return _ActivateSceneFiltered.apply(features_dc, features_rest, opacity, scaling, rotation, filt, float(scale_modifier),
                                        False)[:3]


def fused_parameters(opacity: Tensor, scaling: Tensor, filter_3d: Tensor):
    """``(opacity', scaling')``: opacity logits ``(n, 1)`` and log-scales ``(n, 3)`` with the 3D filter baked in, so that
    the UNFILTERED activation of them is the filtered activation of ``opacity`` and ``scaling``: ``logit(o c)`` and
    ``log(sqrt(v_k))`` from the filtered kernel's own forward outputs (``opacities`` and ``scales`` at modifier 1) and
    plain torch logarithms.  Once per save, not per step; no gradient."""
    for name, t in (("opacity", opacity), ("scaling", scaling), ("filter_3d", filter_3d)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError(f"fused_parameters needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    n, dev = opacity.shape[0], opacity.device
    with torch.no_grad():
        dc = torch.zeros((n, 1, 3), dtype=torch.float32, device=dev)       # the kernel's map takes all five parameters
        rotation = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        rotation[:, 0] = 1.0
        out = activate_forward(dc, dc[:, :0], opacity, scaling, rotation, 1.0, want=("opacities", "scales"), filter_3d=filter_3d)
        p = out["opacities"]
        return torch.log(p) - torch.log1p(-p), torch.log(out["scales"])
