"""The depth-normal consistency regulariser of a trainable 3DGS scene, in HIP (csrc/normals.hip; C ABI include/lsr_normals.h).

A scene fitted to colour alone renders well and has poor geometry: floaters, thick shells, depth maps no one can mesh.
The term 2DGS, Gaussian Surfels, GOF, RaDe-GS and PGSR share ties the orientation of the Gaussians to the surface that the
rendered depth describes:

1. :func:`gaussian_normals` gives every Gaussian, per view, a normal: its shortest axis, turned toward the camera, in camera
   space.
2. The UNCHANGED rasterizer blends those normals as a 3-channel ``features`` payload (background 0) into a normal map,
   next to the depth (sum of alpha T z, depth mode NATIVE) and the mask (sum of alpha T) it already returns:
   :meth:`latentsplat_amd.scene_model.GaussianScene.render_with_normals`.
3. :func:`normal_consistency_loss` penalises the angle between that map and the normals obtained by differentiating the
   rendered depth map (:func:`depth_to_normals`), in one fused pass each way.

What receives no gradient, and why: the shortest axis is chosen by an argmin and turned by a sign, both piecewise constant
in the positions and the scales, so :func:`gaussian_normals` hands a gradient to ``rotation`` alone (positions and scales
get theirs through the rasterizer: the blending weights and the depth).  In the loss the leading ``alpha`` of
``e = alpha - <N, n~>`` is a constant weight, as the published regulariser detaches it; ``alpha`` receives a gradient only
as the denominator of the expected depth.

The view table is NOT a constant of these operators: the normals are ``n_cam = R_view n_world``, smooth in the view
rotation, and the loss builds its pixel rays from the view and projection matrices.  Neither operator has a table
gradient, so both refuse a table that requires grad instead of returning a silent partial one (on a 200-Gaussian scene
the omitted part was 27 % of the full table gradient's norm).  Pass ``views.detach()`` to them and the
leaf to the render: the rasterizer hands the table its own gradient, which is then the partial one by the caller's choice.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_WHO = "the normal regulariser"


def _scene_inputs(views, xyz, scaling, rotation):
    views = _args.f32(_WHO, "views", views)
    if views.dim() != 2 or views.shape[1] != _lib.VIEW_FLOATS:
        raise _lib.LsrError(f"views must be (V, {_lib.VIEW_FLOATS}), got {tuple(views.shape)}")
    xyz = _args.f32(_WHO, "xyz", xyz)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.LsrError(f"xyz must be (n, 3), got {tuple(xyz.shape)}")
    n, dev = xyz.shape[0], xyz.device
    scaling = _args.f32(_WHO, "scaling", scaling, (n, 3), dev)
    rotation = _args.f32(_WHO, "rotation", rotation, (n, 4), dev)
    if views.device != dev:
        raise _lib.LsrError(f"views must be on {dev}")
    V = views.shape[0]
    if n >= _lib.NORMALS_MAX_ROWS or not 1 <= V <= _lib.NORMALS_MAX_VIEWS:
        raise _lib.LsrError(f"gaussian_normals takes fewer than 2^28 Gaussians and 1..{_lib.NORMALS_MAX_VIEWS} views, got {n} and {V}")
    return (views.detach().contiguous(), xyz.detach().contiguous(), scaling.detach().contiguous(),
            _args.quad(rotation.detach().contiguous()))


def _refuse_table_grad(who: str, views) -> None:
    if torch.is_tensor(views) and views.requires_grad:
        raise _lib.LsrError(f"{who}: views requires grad, and this operator has no pose gradient (pass views.detach(); the "
                            "rasterizer hands the table its own)")


def normals_forward(views: Tensor, xyz: Tensor, scaling: Tensor, rotation: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``lsr_scene_normals_forward`` as it is: ``(V, n, 3)`` values (into ``out`` when given)."""
    views, xyz, scaling, rotation = _scene_inputs(views, xyz, scaling, rotation)
    V, n, dev = views.shape[0], xyz.shape[0], xyz.device
    if out is None:
        out = torch.empty((V, n, 3), dtype=torch.float32, device=dev)
    else:
        _args.f32(_WHO, "out", out, (V, n, 3), dev, contiguous=True)
    if n > 0:
        ws = _args.workspace(_lib.load().lsr_scene_normals_workspace_bytes(n, V), dev)
        with torch.cuda.device(dev):
            _lib.call("lsr_scene_normals_forward", n, ptr(xyz), ptr(scaling), ptr(rotation), V, ptr(views), ptr(out), ptr(ws),
                      _args.stream(dev))
    return out


def normals_backward(views: Tensor, xyz: Tensor, scaling: Tensor, rotation: Tensor, grad_normals: Tensor,
                     out: Optional[Tensor] = None) -> Tensor:
    """``lsr_scene_normals_backward`` as it is: ``grad_rotation (n, 4)``, written (into ``out`` when given)."""
    views, xyz, scaling, rotation = _scene_inputs(views, xyz, scaling, rotation)
    V, n, dev = views.shape[0], xyz.shape[0], xyz.device
    grad_normals = _args.f32(_WHO, "grad_normals", grad_normals, (V, n, 3), dev).detach().contiguous()
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    else:
        _args.f32(_WHO, "out", out, (n, 4), dev, contiguous=True)
    if n > 0:
        ws = _args.workspace(_lib.load().lsr_scene_normals_workspace_bytes(n, V), dev)
        with torch.cuda.device(dev):
            _lib.call("lsr_scene_normals_backward", n, ptr(xyz), ptr(scaling), ptr(rotation), V, ptr(views), ptr(grad_normals),
                      ptr(out), ptr(ws), _args.stream(dev))
    return out


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, views, xyz, scaling, rotation):
        ctx.save_for_backward(views, xyz, scaling, rotation)
        return normals_forward(views, xyz, scaling, rotation)

    @staticmethod
    def backward(ctx, grad_normals):
        views, xyz, scaling, rotation = ctx.saved_tensors
        grad = normals_backward(views, xyz, scaling, rotation, grad_normals) if ctx.needs_input_grad[3] else None
        return None, None, None, grad


def gaussian_normals(views: Tensor, xyz: Tensor, scaling: Tensor, rotation: Tensor) -> Tensor:
    """The normal of every Gaussian in every view, ``(V, n, 3)``, unit length, camera space: the column of
    ``R(rotation / |rotation|)`` that belongs to the smallest entry of ``scaling`` (ties: the lowest index), negated when
    it points away from the camera, rotated by the view matrix.  ``views (V, 44)`` is a table of ``build_view_table`` /
    ``make_view_table``; ``scaling (n, 3)`` may be the raw log-scales or the activated scales (only the argmin is used:
    the same bits); ``rotation (n, 4)`` any non-zero quaternion, raw or unit, in the scene's ``(w, x, y, z)`` order.  A row
    that is not finite gives 0.

    Differentiable in ``rotation`` ONLY: the argmin and the sign are piecewise constant, so ``xyz`` and ``scaling``
    receive no gradient from this operator.  The normals do depend on the view rotation (``n_cam = R_view n_world``) and
    the operator has no gradient for it: a ``views`` that requires grad is refused, since a silent partial pose gradient is
    worse than a refusal.  Two HIP launches each way whatever the number of views; no atomics: the same bits every call."""
    _refuse_table_grad("gaussian_normals", views)
    return _GaussianNormals.apply(views, xyz, scaling, rotation)


def _image_inputs(normal_map, depth, alpha, views, alpha_min):
    depth = _args.f32(_WHO, "depth", depth)
    if depth.dim() != 3:
        raise _lib.LsrError(f"depth must be (V, H, W), got {tuple(depth.shape)}")
    V, H, W = depth.shape
    dev = depth.device
    alpha = _args.f32(_WHO, "alpha", alpha, (V, H, W), dev)
    if normal_map is not None:
        normal_map = _args.f32(_WHO, "normal_map", normal_map, (V, 3, H, W), dev).detach().contiguous()
    views = _args.f32(_WHO, "views", views, (V, _lib.VIEW_FLOATS), dev)
    dims = _lib.NormalDims(num_images=V, height=H, width=W, alpha_min=float(alpha_min), reserved0=0, reserved1=0)
    return normal_map, depth.detach().contiguous(), alpha.detach().contiguous(), views.detach().contiguous(), dims


def normal_consistency_forward(normal_map: Tensor, depth: Tensor, alpha: Tensor, views: Tensor, alpha_min: float = 0.5,
                               want=("loss",), out: Optional[dict] = None) -> dict:
    """``lsr_normal_consistency_forward`` as it is: the outputs named in ``want`` (``loss (1,)``, ``per_view (V,)``,
    ``depth_normals (V, 3, H, W)``, ``valid (V, H, W)`` uint8), written into the tensors of ``out`` where given
    (``out["workspace"]``: a uint8 tensor of ``lsr_normal_consistency_workspace_bytes`` to use instead of a fresh one).
    ``normal_map`` may be ``None`` when neither ``loss`` nor ``per_view`` is wanted."""
    normal_map, depth, alpha, views, dims = _image_inputs(normal_map, depth, alpha, views, alpha_min)
    V, H, W = depth.shape
    dev = depth.device
    shapes = {"loss": (1,), "per_view": (V,), "depth_normals": (V, 3, H, W), "valid": (V, H, W)}
    res = _args.results(want, shapes, dev, out)
    ws = (out or {}).get("workspace")
    if ws is None:
        ws = _args.loss_workspace(_lib.load().lsr_normal_consistency_workspace_bytes(C.byref(dims)), dev)
    with torch.cuda.device(dev):
        _lib.call("lsr_normal_consistency_forward", C.byref(dims), ptr(normal_map), ptr(depth), ptr(alpha), ptr(views), ptr(ws),
                  *(ptr(res.get(k)) for k in shapes), _args.stream(dev))
    return res


def normal_consistency_backward(normal_map: Tensor, depth: Tensor, alpha: Tensor, views: Tensor, grad_loss: Tensor,
                                alpha_min: float = 0.5, want=("normal_map", "depth", "alpha"), out: Optional[dict] = None) -> dict:
    """``lsr_normal_consistency_backward`` as it is: the gradients named in ``want``, written (into the tensors of ``out``
    where given).  ``grad_loss`` is a one-element float32 tensor on the device."""
    normal_map, depth, alpha, views, dims = _image_inputs(normal_map, depth, alpha, views, alpha_min)
    grad_loss = _args.upstream("grad_loss", grad_loss, depth.device)
    like = {"normal_map": normal_map, "depth": depth, "alpha": alpha}
    res = {k: (out[k] if out is not None and k in out else torch.empty_like(like[k])) for k in want}
    with torch.cuda.device(depth.device):
        _lib.call("lsr_normal_consistency_backward", C.byref(dims), ptr(normal_map), ptr(depth), ptr(alpha), ptr(views),
                  ptr(grad_loss), *(ptr(res.get(k)) for k in like), _args.stream(depth.device))
    return res


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal_map, depth, alpha, views, alpha_min):
        ctx.save_for_backward(normal_map, depth, alpha, views)
        ctx.alpha_min = alpha_min
        return normal_consistency_forward(normal_map, depth, alpha, views, alpha_min)["loss"].reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        normal_map, depth, alpha, views = ctx.saved_tensors
        names = ("normal_map", "depth", "alpha")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad) if need)
        # the upstream gradient stays on the device: the kernel reads it there
        g = normal_consistency_backward(normal_map, depth, alpha, views, grad_loss.reshape(1), ctx.alpha_min, want) if want else {}
        shape = {"normal_map": normal_map.shape, "depth": depth.shape, "alpha": alpha.shape}
        return tuple(g[k].reshape(shape[k]) if k in g else None for k in names) + (None, None)


def normal_consistency_loss(normal_map: Tensor, depth: Tensor, alpha: Tensor, views: Tensor, alpha_min: float = 0.5) -> Tensor:
    """The depth-normal consistency loss, a scalar: ``mean over views and pixels of e``, ``e = alpha - <N, n~>`` at valid
    pixels and 0 elsewhere.  ``normal_map (V, 3, H, W)`` is the rendered, NOT renormalised normal map of
    :func:`gaussian_normals`; ``depth (V, H, W)`` the rendered depth of depth mode NATIVE; ``alpha (V, H, W)`` the mask;
    ``views`` the table they were rendered with.  ``n~`` is the unit normal of the surface ``P = (depth / alpha) ray``,
    from the central differences of ``P`` over the four neighbours, signed to face the camera; the ray comes from the view
    record's own projection and view matrices, so an off-centre principal point and unequal fields of view are honoured.
    A pixel is valid when it is at least one pixel from every border, ``alpha > alpha_min`` at it and at its four
    neighbours, the five expected depths are finite and the cross product is not degenerate.  Images with fewer than 3
    rows or columns have no valid pixel: the loss is 0.  The scene scale of the view table cancels.

    ``alpha_min = 0.5`` is a default, not a measurement: pixels the scene covers less than half carry an expected depth
    that mixes surface and background.

    Gradients go to ``normal_map``, ``depth`` and ``alpha``; the leading ``alpha`` of ``e`` is a constant weight in the
    backward, as the published regulariser detaches it, so ``alpha`` receives its gradient through ``depth / alpha`` alone.
    The pixel rays depend on ``views`` and the loss has no gradient for it: a ``views`` that requires grad is refused (pass
    ``views.detach()``).  Two HIP launches forward and one backward; no atomics: the same bits every call."""
    _refuse_table_grad("normal_consistency_loss", views)
    return _NormalConsistency.apply(normal_map, depth, alpha, views, float(alpha_min))


def depth_to_normals(depth: Tensor, alpha: Tensor, views: Tensor, alpha_min: float = 0.5):
    """``(normals (V, 3, H, W), valid (V, H, W) bool)``: the camera-space unit normals ``n~`` of
    :func:`normal_consistency_loss` (0 where invalid) and its valid mask.  Values only."""
    _, d, a, _, _ = _image_inputs(None, depth, alpha, views, alpha_min)
    out = normal_consistency_forward(None, d, a, views, alpha_min, want=("depth_normals", "valid"))
    return out["depth_normals"], out["valid"].bool()


def flatten_loss(scaling: Tensor) -> Tensor:
    """``mean(min_k exp(scaling))``: the mean shortest extent of the Gaussians (raw log-scales in), the companion of the
    consistency term that makes the shortest axis a normal worth the name.  Plain torch."""
    return torch.exp(scaling).min(dim=-1).values.mean()
