"""The depth distortion regulariser of a trainable 3DGS scene, in HIP (csrc/distortion.hip; C ABI include/lsr_distortion.h).

The second geometric regulariser of 2DGS, Gaussian Surfels, GOF, RaDe-GS and PGSR, next to the depth-normal consistency of
:mod:`latentsplat_amd.normals`: the distortion term of Mip-NeRF 360 in the squared form of 2DGS, which pulls the Gaussians
along a ray onto one surface.  For one pixel with blending weights ``w_i = alpha_i T_i`` and per-Gaussian depths ``m_i``::

    D = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2 = A * M2 - M1^2,   A = sum w_i,  M1 = sum w_i m_i,  M2 = sum w_i m_i^2

1. :func:`gaussian_depth_moments` gives every Gaussian, per view, the pair ``(m', m'^2)``, ``m' = m - pivot``.
2. The UNCHANGED rasterizer blends the pairs as a 2-channel ``features`` payload (background 0) into a moment map, next to
   the mask ``A`` it already returns: :meth:`latentsplat_amd.scene_model.GaussianScene.render_with_distortion`, and with
   the normals :meth:`~latentsplat_amd.scene_model.GaussianScene.render_surface`.
3. :func:`distortion_loss` forms ``A * M2 - M1^2`` per pixel in double and averages it, in one fused pass each way.

``D`` does not change when one constant is subtracted from every ``m`` along a ray, and ``A * M2 - M1^2`` cancels in float32
when the layers are close compared with their distance: the regime the term exists for.  So the moments are taken about a
per-view ``pivot`` (:func:`depth_pivot` of the scene's centre, or of the centroid of a capture's sparse points).

``space="ndc"`` reads near and far from slots 42 / 43 of the view table.  ``build_view_table`` writes them only under a depth
mode other than NATIVE; a NATIVE table (what :meth:`render_surface` needs) gets them from :func:`with_near_far`, which the
rasterizer does not read under NATIVE.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_WHO = "the distortion regulariser"
SPACES = {"linear": _lib.DIST_LINEAR, "ndc": _lib.DIST_NDC, "disparity": _lib.DIST_DISPARITY}


def _space(space) -> int:
    if space not in SPACES:
        raise _lib.LsrError(f"space must be one of {', '.join(SPACES)}, got {space!r}")
    return SPACES[space]


def with_near_far(views: Tensor, near, far) -> Tensor:
    """A copy of the view table with ``near`` / ``far`` (numbers or ``(V,)``, the caller's UNSCALED ones) in slots 42 / 43,
    where ``space="ndc"`` reads them.  The rasterizer reads the two slots only under a depth mode other than NATIVE, so a
    NATIVE table renders the same bits with them."""
    out = views.detach().clone()
    out[:, 42] = torch.as_tensor(near, dtype=out.dtype, device=out.device)
    out[:, 43] = torch.as_tensor(far, dtype=out.dtype, device=out.device)
    return out


def _check_near_far(views: Tensor) -> None:
    # (the table lives on the device: one host read per call, of 2 V floats; include/lsr_distortion.h names this check)
    nf = views[:, 42:44].detach().double().cpu()
    if not bool(torch.isfinite(nf).all()) or bool((nf[:, 0] >= nf[:, 1]).any()):
        raise _lib.LsrError("space='ndc' needs finite near < far in slots 42 / 43 of every view (invalid argument): a table "
                            "of depth mode NATIVE carries 0 there; fill them with distortion.with_near_far")


def _scene_inputs(views, xyz, pivot, space, check: bool):
    views = _args.f32(_WHO, "views", views)
    if views.dim() != 2 or views.shape[1] != _lib.VIEW_FLOATS:
        raise _lib.LsrError(f"views must be (V, {_lib.VIEW_FLOATS}), got {tuple(views.shape)}")
    xyz = _args.f32(_WHO, "xyz", xyz)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.LsrError(f"xyz must be (n, 3), got {tuple(xyz.shape)}")
    n, dev, V = xyz.shape[0], xyz.device, views.shape[0]
    if views.device != dev:
        raise _lib.LsrError(f"views must be on {dev}")
    if pivot is not None:
        pivot = _args.f32(_WHO, "pivot", pivot, (V,), dev).detach().contiguous()
    if n >= _lib.DIST_MAX_ROWS or not 1 <= V <= _lib.DIST_MAX_VIEWS:
        raise _lib.LsrError(f"gaussian_depth_moments takes fewer than 2^28 Gaussians and 1..{_lib.DIST_MAX_VIEWS} views, got {n} and {V}")
    code = _space(space)
    if check and code == _lib.DIST_NDC:
        _check_near_far(views)
    return views.detach().contiguous(), xyz.detach().contiguous(), pivot, code


def depth_moments_forward(views: Tensor, xyz: Tensor, space: str = "ndc", pivot: Optional[Tensor] = None,
                          out: Optional[Tensor] = None, check: bool = True) -> Tensor:
    """``lsr_scene_depth_moments_forward`` as it is: ``(V, n, 2)`` values (into ``out`` when given).  ``check=False`` skips
    the host read of near / far under ``space="ndc"`` (a training loop, a graph capture)."""
    views, xyz, pivot, code = _scene_inputs(views, xyz, pivot, space, check)
    V, n, dev = views.shape[0], xyz.shape[0], xyz.device
    if out is None:
        out = torch.empty((V, n, 2), dtype=torch.float32, device=dev)
    else:
        _args.f32(_WHO, "out", out, (V, n, 2), dev, contiguous=True)
    if n > 0:
        ws = _args.workspace(_lib.load().lsr_scene_depth_moments_workspace_bytes(n, V), dev)
        with torch.cuda.device(dev):
            _lib.call("lsr_scene_depth_moments_forward", n, ptr(xyz), V, ptr(views), ptr(pivot), code, ptr(out), ptr(ws),
                      _args.stream(dev))
    return out


def depth_moments_backward(views: Tensor, xyz: Tensor, grad_moments: Tensor, space: str = "ndc", pivot: Optional[Tensor] = None,
                           out: Optional[Tensor] = None) -> Tensor:
    """``lsr_scene_depth_moments_backward`` as it is: ``grad_xyz (n, 3)``, written (into ``out`` when given)."""
    views, xyz, pivot, code = _scene_inputs(views, xyz, pivot, space, False)
    V, n, dev = views.shape[0], xyz.shape[0], xyz.device
    grad_moments = _args.f32(_WHO, "grad_moments", grad_moments, (V, n, 2), dev).detach().contiguous()
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    else:
        _args.f32(_WHO, "out", out, (n, 3), dev, contiguous=True)
    if n > 0:
        ws = _args.workspace(_lib.load().lsr_scene_depth_moments_workspace_bytes(n, V), dev)
        with torch.cuda.device(dev):
            _lib.call("lsr_scene_depth_moments_backward", n, ptr(xyz), V, ptr(views), ptr(pivot), code, ptr(grad_moments),
                      ptr(out), ptr(ws), _args.stream(dev))
    return out


class _DepthMoments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, views, xyz, pivot, space, check):
        ctx.save_for_backward(views, xyz, pivot)
        ctx.space = space
        return depth_moments_forward(views, xyz, space, pivot, check=check)

    @staticmethod
    def backward(ctx, grad_moments):
        views, xyz, pivot = ctx.saved_tensors
        grad = depth_moments_backward(views, xyz, grad_moments, ctx.space, pivot) if ctx.needs_input_grad[1] else None
        return None, grad, None, None, None


def gaussian_depth_moments(views: Tensor, xyz: Tensor, space: str = "ndc", pivot: Optional[Tensor] = None,
                           check: bool = True) -> Tensor:
    """The depth moments of every Gaussian in every view, ``(V, n, 2) = (m', m'^2)`` with ``m' = m - pivot[v]``.  ``z`` is the
    camera-space depth of the unscaled scene, the view-space z the rasterizer projects divided by slot 40 of the view;
    ``space``: ``"linear"`` ``m = z``; ``"ndc"`` ``m = f / (f - n) (1 - n / z)`` with near / far from slots 42 / 43 (the
    mapping of 2DGS; :func:`with_near_far`); ``"disparity"`` ``m = 1 / z``.  ``pivot (V,)``: :func:`depth_pivot`; ``None``
    is 0.  A pair that is not finite or has ``z <= 0`` gives ``(0, 0)``.

    Differentiable in ``xyz`` ONLY.  A ``views`` or ``pivot`` that requires grad is refused: a silent partial pose gradient
    is worse than a refusal.  ``space="ndc"`` costs one host read of near / far per call unless ``check=False``.  Two HIP
    launches each way whatever the number of views; no atomics: the same bits every call."""
    _space(space)
    if torch.is_tensor(views) and views.requires_grad:
        raise _lib.LsrError("gaussian_depth_moments: views requires grad, and this operator has no pose gradient (pass "
                            "views.detach(); the rasterizer hands the table its own)")
    if torch.is_tensor(pivot) and pivot.requires_grad:
        raise _lib.LsrError("gaussian_depth_moments: pivot requires grad; it is a constant of this operator")
    return _DepthMoments.apply(views, xyz, pivot, space, check)


def depth_pivot(views: Tensor, point, space: str = "ndc") -> Tensor:
    """``(V,)`` float32: the ``m`` of :func:`gaussian_depth_moments` for ONE world point ``(3,)`` in every view, in plain
    torch in float64, on the device of ``views`` (any device).  A caller passes the scene's centre, or for a capture the
    centroid of its sparse points."""
    code = _space(space)
    v = views.detach().double()
    p = torch.as_tensor(point, dtype=torch.float64, device=v.device).reshape(3)
    s = v[:, 40]
    z = (v[:, 2] * p[0] + v[:, 6] * p[1] + v[:, 10] * p[2]) + v[:, 14] / s
    if code == _lib.DIST_LINEAR:
        m = z
    elif code == _lib.DIST_DISPARITY:
        m = 1.0 / z
    else:
        _check_near_far(views)
        n, f = v[:, 42], v[:, 43]
        m = f / (f - n) * (1.0 - n / z)
    return m.float()


def _image_inputs(moment_map, alpha, weight):
    alpha = _args.f32(_WHO, "alpha", alpha)
    if alpha.dim() != 3:
        raise _lib.LsrError(f"alpha must be (V, H, W), got {tuple(alpha.shape)}")
    V, H, W = alpha.shape
    dev = alpha.device
    moment_map = _args.f32(_WHO, "moment_map", moment_map, (V, 2, H, W), dev).detach().contiguous()
    if weight is not None:
        weight = _args.f32(_WHO, "weight", weight, (V, H, W), dev).detach().contiguous()
    dims = _lib.DistortionDims(num_images=V, height=H, width=W, reserved0=0, reserved1=0, reserved2=0)
    return moment_map, alpha.detach().contiguous(), weight, dims


def distortion_loss_forward(moment_map: Tensor, alpha: Tensor, weight: Optional[Tensor] = None, want=("loss",),
                            out: Optional[dict] = None) -> dict:
    """``lsr_distortion_loss_forward`` as it is: the outputs named in ``want`` (``loss (1,)``, ``per_view (V,)``,
    ``distortion (V, H, W)``), written into the tensors of ``out`` where given (``out["workspace"]``: a uint8 tensor of
    ``lsr_distortion_loss_workspace_bytes`` to use instead of a fresh one)."""
    moment_map, alpha, weight, dims = _image_inputs(moment_map, alpha, weight)
    V, H, W = alpha.shape
    dev = alpha.device
    shapes = {"loss": (1,), "per_view": (V,), "distortion": (V, H, W)}
    res = _args.results(want, shapes, dev, out)
    ws = (out or {}).get("workspace")
    if ws is None:
        ws = _args.loss_workspace(_lib.load().lsr_distortion_loss_workspace_bytes(C.byref(dims)), dev)
    with torch.cuda.device(dev):
        _lib.call("lsr_distortion_loss_forward", C.byref(dims), ptr(moment_map), ptr(alpha), ptr(weight), ptr(ws),
                  *(ptr(res.get(k)) for k in shapes), _args.stream(dev))
    return res


def distortion_loss_backward(moment_map: Tensor, alpha: Tensor, grad_loss: Tensor, weight: Optional[Tensor] = None,
                             want=("moment_map", "alpha"), out: Optional[dict] = None) -> dict:
    """``lsr_distortion_loss_backward`` as it is: the gradients named in ``want``, written (into the tensors of ``out``
    where given).  ``grad_loss`` is a one-element float32 tensor on the device."""
    moment_map, alpha, weight, dims = _image_inputs(moment_map, alpha, weight)
    grad_loss = _args.upstream("grad_loss", grad_loss, alpha.device)
    like = {"moment_map": moment_map, "alpha": alpha}
    res = {k: (out[k] if out is not None and k in out else torch.empty_like(like[k])) for k in want}
    with torch.cuda.device(alpha.device):
        _lib.call("lsr_distortion_loss_backward", C.byref(dims), ptr(moment_map), ptr(alpha), ptr(weight), ptr(grad_loss),
                  *(ptr(res.get(k)) for k in like), _args.stream(alpha.device))
    return res


class _DistortionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, moment_map, alpha, weight):
        ctx.save_for_backward(moment_map, alpha, weight)
        return distortion_loss_forward(moment_map, alpha, weight)["loss"].reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        moment_map, alpha, weight = ctx.saved_tensors
        names = ("moment_map", "alpha")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad) if need)
        # the upstream gradient stays on the device: the kernel reads it there
        g = distortion_loss_backward(moment_map, alpha, grad_loss.reshape(1), weight, want) if want else {}
        shape = {"moment_map": moment_map.shape, "alpha": alpha.shape}
        return tuple(g[k].reshape(shape[k]) if k in g else None for k in names) + (None,)


def distortion_loss(moment_map: Tensor, alpha: Tensor, weight: Optional[Tensor] = None) -> Tensor:
    """The depth distortion loss, a scalar: ``mean over views and pixels of weight * (alpha * M2 - M1^2)``.
    ``moment_map (V, 2, H, W)`` is the rendered moment map of :func:`gaussian_depth_moments`, ``alpha (V, H, W)`` the mask
    of the same render, ``weight (V, H, W)`` an optional per-pixel weight (a capture's coverage map), which receives no
    gradient.  The difference is formed in double from the float32 maps and is NOT clamped: a negative value is rounding and
    keeps its gradient.  Gradients go to ``moment_map`` and ``alpha``.  Two HIP launches forward and one backward; no
    atomics: the same bits every call, and a view gives the same bits alone and in a batch."""
    if torch.is_tensor(weight) and weight.requires_grad:
        raise _lib.LsrError("distortion_loss: weight requires grad, and it receives none")
    return _DistortionLoss.apply(moment_map, alpha, weight)


def distortion_map(moment_map: Tensor, alpha: Tensor) -> Tensor:
    """``(V, H, W)``: ``alpha * M2 - M1^2`` per pixel, formed in double and rounded to float32 once.  Values only."""
    return distortion_loss_forward(moment_map, alpha, None, want=("distortion",))["distortion"]
