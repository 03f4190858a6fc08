"""A trainable 3DGS scene: the raw parameters a 3DGS trainer holds, activated for the rasterizer by one HIP kernel.

A scene file, and every 3DGS trainer, holds log-scales, unnormalised quaternions, opacity logits and the colour SH as
``f_dc`` / ``f_rest``; the rasterizer takes packed covariances, probabilities and one ``(n, K, 3)`` SH tensor.
:func:`activate_scene` is that map as a ``torch.autograd.Function`` over ``lsr_scene_activate_forward`` /
``lsr_scene_activate_backward`` (csrc/scene_params.hip, C ABI include/lsr_scene.h): one launch each way.
:class:`GaussianScene` holds a scene under the published trainer's parameter names, reads and writes scene files without
touching the values, and renders through :func:`latentsplat_amd.rasterizer.rasterize_views`.

The kernels take float32 ROCm tensors only; there is no CPU fallback.  Scene files mean the ``"3dgs"`` colour SH basis
(:func:`latentsplat_amd.rasterizer.set_color_sh_convention`, the default); nothing here changes that process-wide
setting."""
from __future__ import annotations

import ctypes as C
import math
import os
from math import isqrt
from pathlib import Path
from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from . import _args, _lib
from ._args import ptr
from .ply_import import Scene3DGS, read_header

_FORWARD_OUTPUTS = ("shs", "opacities", "cov3D", "scales", "rotations")
_PARAMS = ("features_dc", "features_rest", "opacity", "scaling", "rotation")


def _prepare(features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor, rotation: Tensor):
    """Checked, detached, contiguous parameters and ``(n, K)``."""
    given = (features_dc, features_rest, opacity, scaling, rotation)
    for name, t in zip(_PARAMS, given):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError(f"activate_scene needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    n = features_dc.shape[0]
    if tuple(features_dc.shape) != (n, 1, 3) or features_rest.dim() != 3 or features_rest.shape[0] != n or features_rest.shape[2] != 3:
        raise _lib.LsrError(f"features_dc must be (n, 1, 3) and features_rest (n, K - 1, 3), got {tuple(features_dc.shape)} "
                            f"and {tuple(features_rest.shape)}")
    K = features_rest.shape[1] + 1
    if K not in (1, 4, 9, 16, 25):
        raise _lib.LsrError(f"{K} SH coefficients per channel: expected 1, 4, 9, 16 or 25")
    if tuple(opacity.shape) != (n, 1) or tuple(scaling.shape) != (n, 3) or tuple(rotation.shape) != (n, 4):
        raise _lib.LsrError("opacity must be (n, 1), scaling (n, 3) and rotation (n, 4)")
    if len({t.device for t in given}) != 1:
        raise _lib.LsrError("the scene's tensors must be on one device")
    dc, rest, op, sc, rot = (t.detach().contiguous() for t in given)
    return (dc, rest, op, sc, _args.quad(rot)), n, K


def _filter(filter_3d, n: int, dev) -> Optional[Tensor]:
    """A checked, detached, contiguous 3D filter of ``n`` entries on ``dev`` (``None`` stays ``None``).  A filter of another
    length belongs to another scene, or to this one before a densification or a growth: refused before any launch."""
    if filter_3d is None:
        return None
    if torch.is_tensor(filter_3d) and tuple(filter_3d.shape) not in ((n,), (n, 1)):
        raise _lib.LsrError(f"filter_3d has shape {tuple(filter_3d.shape)} but the scene has {n} Gaussians: a 3D filter is computed "
                            "for one set of Gaussians and is stale after a densification, a growth or a pruning; compute it again")
    if not torch.is_tensor(filter_3d) or not filter_3d.is_cuda or filter_3d.dtype != torch.float32:
        raise _lib.LsrError("the filtered activation needs float32 ROCm tensors (no CPU fallback): filter_3d is not one")
    if filter_3d.device != dev:
        raise _lib.LsrError(f"filter_3d must be on {dev}")
    return filter_3d.detach().contiguous()


def _dims(n: int, K: int, scale_modifier: float) -> _lib.SceneDims:
    return _lib.SceneDims(n=n, sh_coeffs=K, scale_modifier=float(scale_modifier), reserved0=0, reserved1=0)


def activate_forward(features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor, rotation: Tensor,
                     scale_modifier: float = 1.0, want: Optional[Sequence[str]] = None, filter_3d: Optional[Tensor] = None) -> dict:
    """``lsr_scene_activate_forward`` as it is (no autograd): the outputs named in ``want`` (default: all of ``shs,
    opacities, cov3D, scales, rotations``) as a dict; the others are not computed.  With ``filter_3d`` (``(n,)`` or
    ``(n, 1)``, :func:`latentsplat_amd.filter3d.compute_filter_3d`): ``lsr_scene_activate_filtered_forward``."""
    params, n, K = _prepare(features_dc, features_rest, opacity, scaling, rotation)
    filt = _filter(filter_3d, n, params[0].device)
    shapes = dict(shs=(n, K, 3), opacities=(n, 1), cov3D=(n, 6), scales=(n, 3), rotations=(n, 4))
    unknown = [k for k in (want or ()) if k not in shapes]
    if unknown:
        raise _lib.LsrError(f"unknown outputs {unknown}; expected some of {list(shapes)}")
    dev = params[0].device
    out = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items() if want is None or k in want}
    if n == 0:
        return out
    ptrs = _lib.SceneOutputs(**{k: ptr(t) for k, t in out.items()})
    with torch.cuda.device(dev):
        stream = _args.stream(dev)
        if filt is None:
            _lib.call("lsr_scene_activate_forward", C.byref(_dims(n, K, scale_modifier)),
                      C.byref(_lib.SceneParams(*map(ptr, params))), C.byref(ptrs), stream)
        else:
            _lib.call("lsr_scene_activate_filtered_forward", C.byref(_dims(n, K, scale_modifier)),
                      C.byref(_lib.SceneParams(*map(ptr, params))), ptr(filt), C.byref(ptrs), stream)
    return out


def activate_backward(features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor, rotation: Tensor,
                      grad_shs: Optional[Tensor], grad_opacities: Optional[Tensor], grad_cov3D: Optional[Tensor],
                      scale_modifier: float = 1.0, want: Optional[Sequence[str]] = None,
                      filter_3d: Optional[Tensor] = None) -> dict:
    """``lsr_scene_activate_backward`` as it is: the gradients of the parameters named in ``want`` (default: all five)
    for the given upstream gradients (``None`` = zero).  With ``filter_3d``: ``lsr_scene_activate_filtered_backward`` (the
    filter is a constant and gets no gradient)."""
    params, n, K = _prepare(features_dc, features_rest, opacity, scaling, rotation)
    filt = _filter(filter_3d, n, params[0].device)
    unknown = [k for k in (want or ()) if k not in _PARAMS]
    if unknown:
        raise _lib.LsrError(f"unknown gradients {unknown}; expected some of {list(_PARAMS)}")
    dev = params[0].device
    ups = []
    for name, g, shape in (("shs", grad_shs, (n, K, 3)), ("opacities", grad_opacities, (n, 1)), ("cov3D", grad_cov3D, (n, 6))):
        if g is not None:
            if not g.is_cuda or g.dtype != torch.float32 or tuple(g.shape) != shape or g.device != dev:
                raise _lib.LsrError(f"the gradient of {name} must be a float32 ROCm tensor of shape {shape} on the scene's device")
            g = g.detach().contiguous()
        ups.append(g)
    out = {k: torch.empty_like(t) for k, t in zip(_PARAMS, params) if want is None or k in want}
    if n == 0:
        return out
    grads = _lib.SceneInGrads(**{k: ptr(t) for k, t in out.items()})
    with torch.cuda.device(dev):
        stream = _args.stream(dev)
        if filt is None:
            _lib.call("lsr_scene_activate_backward", C.byref(_dims(n, K, scale_modifier)),
                      C.byref(_lib.SceneParams(*map(ptr, params))), C.byref(_lib.SceneOutGrads(*map(ptr, ups))),
                      C.byref(grads), stream)
        else:
            _lib.call("lsr_scene_activate_filtered_backward", C.byref(_dims(n, K, scale_modifier)),
                      C.byref(_lib.SceneParams(*map(ptr, params))), ptr(filt),
                      C.byref(_lib.SceneOutGrads(*map(ptr, ups))), C.byref(grads), stream)
    return out


class _ActivateScene(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features_dc, features_rest, opacity, scaling, rotation, scale_modifier, geometry):
        ctx.set_materialize_grads(False)
        want = _FORWARD_OUTPUTS if geometry else _FORWARD_OUTPUTS[:3]
        out = activate_forward(features_dc, features_rest, opacity, scaling, rotation, scale_modifier, want)
        ctx.save_for_backward(features_dc, features_rest, opacity, scaling, rotation)
        ctx.scale_modifier = scale_modifier
        scales, rotations = out.get("scales"), out.get("rotations")
        if geometry:
            ctx.mark_non_differentiable(scales, rotations)
        return out["shs"], out["opacities"], out["cov3D"], scales, rotations

    @staticmethod
    def backward(ctx, g_shs, g_opacities, g_cov3D, _g_scales, _g_rotations):
        # a parameter gets a gradient (and a buffer) only where it is asked for and something reaches it
        reach = (g_shs, g_shs, g_opacities, g_cov3D, g_cov3D)
        want = [k for k, need, g in zip(_PARAMS, ctx.needs_input_grad, reach) if need and g is not None]
        if not want:
            return (None,) * 7
        got = activate_backward(*ctx.saved_tensors, g_shs, g_opacities, g_cov3D, ctx.scale_modifier, want)
        return tuple(got.get(k) for k in _PARAMS) + (None, None)


class _ActivateSceneFiltered(torch.autograd.Function):
    """:class:`_ActivateScene` with the 3D filter inside the map (a constant: no gradient).  The opacity coefficient
    depends on the scales, so the upstream gradient of the opacities reaches ``scaling`` too."""

    @staticmethod
    def forward(ctx, features_dc, features_rest, opacity, scaling, rotation, filter_3d, scale_modifier, geometry):
        ctx.set_materialize_grads(False)
        want = _FORWARD_OUTPUTS if geometry else _FORWARD_OUTPUTS[:3]
        out = activate_forward(features_dc, features_rest, opacity, scaling, rotation, scale_modifier, want, filter_3d=filter_3d)
        ctx.save_for_backward(features_dc, features_rest, opacity, scaling, rotation, filter_3d)
        ctx.scale_modifier = scale_modifier
        scales, rotations = out.get("scales"), out.get("rotations")
        if geometry:
            ctx.mark_non_differentiable(scales, rotations)
        return out["shs"], out["opacities"], out["cov3D"], scales, rotations

    @staticmethod
    def backward(ctx, g_shs, g_opacities, g_cov3D, _g_scales, _g_rotations):
        either = g_cov3D if g_cov3D is not None else g_opacities
        reach = (g_shs, g_shs, g_opacities, either, g_cov3D)
        want = [k for k, need, g in zip(_PARAMS, ctx.needs_input_grad, reach) if need and g is not None]
        if not want:
            return (None,) * 8
        *params, filter_3d = ctx.saved_tensors
        got = activate_backward(*params, g_shs, g_opacities, g_cov3D, ctx.scale_modifier, want, filter_3d=filter_3d)
        return tuple(got.get(k) for k in _PARAMS) + (None, None, None)


def activate_scene(features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor, rotation: Tensor,
                   scale_modifier: float = 1.0):
    """Raw 3DGS parameters to the rasterizer's inputs, differentiable: ``(shs (n, K, 3), opacities (n, 1), cov3D (n, 6))``.

    ``features_dc (n, 1, 3)`` and ``features_rest (n, K - 1, 3)`` are concatenated; ``opacity (n, 1)`` holds logits;
    ``cov3D = R diag((m s)^2) R^T`` packed as xx,xy,xz,yy,yz,zz with ``s = exp(scaling (n, 3))``, ``m =
    scale_modifier`` and ``R`` the rotation of ``rotation (n, 4)`` (w,x,y,z, any non-zero norm).  One HIP launch
    forward, one backward; float32 ROCm tensors only."""
    return _ActivateScene.apply(features_dc, features_rest, opacity, scaling, rotation, float(scale_modifier), False)[:3]


# ---- rows of a scene file <-> raw parameters: plain torch column gathers, once per load / save (any device) ----

def rows_to_parameters(rows: Tensor, layout: _lib.PlyLayout) -> dict:
    """The columns of a scene file's row table ``(n, stride)`` as the raw parameter tensors, bit for bit.  ``f_rest`` is
    channel-major in the file (``f_rest_{c (K - 1) + k}``) and ``(n, K - 1, 3)`` here."""
    n, K = rows.shape[0], layout.sh_coeffs
    col = lambda offsets: rows[:, torch.tensor(list(offsets), dtype=torch.long, device=rows.device)].contiguous()
    rest = col(layout.f_rest[:3 * (K - 1)]).reshape(n, 3, K - 1).transpose(1, 2).contiguous()
    return dict(xyz=col(layout.xyz), features_dc=col(layout.f_dc).reshape(n, 1, 3), features_rest=rest,
                opacity=col([layout.opacity]), scaling=col(layout.scale), rotation=col(layout.rot))


def parameters_to_rows(xyz: Tensor, features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor,
                       rotation: Tensor) -> Tensor:
    """``(n, 14 + 3 K)`` rows in the published property order: xyz, three zero normals, f_dc, channel-major f_rest,
    opacity, scale, rot; the values as they are."""
    n = xyz.shape[0]
    rest = features_rest.detach().transpose(1, 2).reshape(n, -1)
    cols = [xyz.detach(), torch.zeros_like(xyz), features_dc.detach().reshape(n, 3), rest, opacity.detach(),
            scaling.detach(), rotation.detach()]
    return torch.cat(cols, dim=1).contiguous()


class GaussianScene(nn.Module):
    """A 3DGS scene as trainers hold it: raw parameters under the published trainer's names (``_xyz (n, 3)``,
    ``_features_dc (n, 1, 3)``, ``_features_rest (n, K - 1, 3)``, ``_opacity (n, 1)`` logits, ``_scaling (n, 3)`` logs,
    ``_rotation (n, 4)`` w,x,y,z), so that state dicts and per-tensor optimiser recipes carry over.  ``max_sh_degree`` is
    the degree the stored bands reach, ``active_sh_degree`` the one rendered (:meth:`oneup_sh_degree`).

    The colour SH coefficients are in the ``"3dgs"`` basis, as scene files hold them; :meth:`render` renders with the
    process's colour SH convention as it finds it (``"3dgs"`` is the default) and does not change it."""

    def __init__(self, xyz: Tensor, features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor,
                 rotation: Tensor, active_sh_degree: Optional[int] = None):
        super().__init__()
        n = xyz.shape[0]
        K = features_rest.shape[1] + 1 if features_rest.dim() == 3 else 0
        shapes = ((xyz, (n, 3)), (features_dc, (n, 1, 3)), (features_rest, (n, K - 1, 3)), (opacity, (n, 1)),
                  (scaling, (n, 3)), (rotation, (n, 4)))
        if K not in (1, 4, 9, 16, 25) or any(tuple(t.shape) != s for t, s in shapes):
            raise _lib.LsrError("GaussianScene takes xyz (n, 3), features_dc (n, 1, 3), features_rest (n, K - 1, 3) with K in "
                                "1, 4, 9, 16, 25, opacity (n, 1), scaling (n, 3) and rotation (n, 4)")
        if any(t.dtype != torch.float32 for t, _ in shapes):
            raise _lib.LsrError("GaussianScene takes float32 tensors")
        p = lambda t: nn.Parameter(t.detach().clone().contiguous())
        self._xyz, self._features_dc, self._features_rest = p(xyz), p(features_dc), p(features_rest)
        self._opacity, self._scaling, self._rotation = p(opacity), p(scaling), p(rotation)
        self.max_sh_degree = isqrt(K) - 1
        self.active_sh_degree = self.max_sh_degree if active_sh_degree is None else int(active_sh_degree)
        if not 0 <= self.active_sh_degree <= self.max_sh_degree:
            raise _lib.LsrError(f"active_sh_degree must be in 0..{self.max_sh_degree}")

    @classmethod
    def from_tensors(cls, xyz: Tensor, features_dc: Tensor, features_rest: Tensor, opacity: Tensor, scaling: Tensor,
                     rotation: Tensor, active_sh_degree: Optional[int] = None) -> "GaussianScene":
        """From raw tensors (copied): log-scales, opacity logits, unnormalised quaternions."""
        return cls(xyz, features_dc, features_rest, opacity, scaling, rotation, active_sh_degree)

    @classmethod
    def from_ply(cls, path, device, *, check_opacity: bool = True) -> "GaussianScene":
        """The raw parameters of a binary little-endian 3DGS scene file, bit for bit (the library's host reader, then
        column gathers; nothing is activated and inverted again).  Logit-opacity files only: a file whose opacities all
        lie in [0, 1] stores probabilities, as this project's viewer export ``export_ply`` writes them, and is refused
        (``check_opacity=False`` takes the values as logits regardless)."""
        device = torch.device(device)
        layout = read_header(path)
        host = torch.empty((layout.n, layout.stride), dtype=torch.float32, pin_memory=device.type == "cuda")
        _lib.call("lsr_ply_read_rows", os.fsencode(str(path)), C.c_void_p(host.data_ptr()), host.numel())
        if check_opacity and layout.n > 0:
            o = host[:, layout.opacity]
            if float(o.min()) >= 0.0 and float(o.max()) <= 1.0:
                raise _lib.LsrError(f"{path}: every opacity lies in [0, 1]: the file stores probabilities, not logits (a viewer "
                                    "export of export_ply). Such a file holds no trainable scene; read it with "
                                    "load_ply(path, device, opacity=\"raw\")")
        return cls(**rows_to_parameters(host.to(device), layout))

    @classmethod
    def from_point_cloud(cls, points: Tensor, colors: Optional[Tensor] = None, sh_degree: int = 3, *,
                         initial_opacity: float = 0.1, min_dist2: float = 1e-7) -> "GaussianScene":
        """The published trainer's ``create_from_pcd``: a scene that starts from a sparse point cloud.  ``_xyz`` are the
        points ``(n, 3)`` (a float32 ROCm tensor, n >= 4), ``_features_dc`` is ``(colors - 0.5) / 0.28209479177387814``
        with ``colors (n, 3)`` in [0, 1] (``None``: grey, zeros), ``_features_rest`` zeros up to ``sh_degree`` (0..4),
        ``_opacity`` the logit of ``initial_opacity``, ``_rotation`` the identity, and every ``_scaling`` row
        ``log(sqrt(max(d, min_dist2)))`` three times over, ``d`` the mean squared distance of the point to its three
        nearest neighbours (:func:`latentsplat_amd.knn.mean_knn_dist2`: the search is the HIP kernel, the elementwise
        tail plain torch).  ``active_sh_degree`` starts at 0.  Non-finite coordinates are refused (one host read)."""
        from .knn import mean_knn_dist2
        if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.float32:
            raise _lib.LsrError("from_point_cloud needs a float32 ROCm tensor of points (no CPU fallback)")
        if points.dim() != 2 or points.shape[1] != 3:
            raise _lib.LsrError(f"points must be (n, 3), got {tuple(points.shape)}")
        if not 0 <= int(sh_degree) <= 4:
            raise _lib.LsrError("sh_degree must be in 0..4")
        if not 0.0 < initial_opacity < 1.0 or not min_dist2 > 0.0:
            raise _lib.LsrError("initial_opacity must lie in (0, 1) and min_dist2 must be positive")
        n, dev = points.shape[0], points.device
        points = points.detach().contiguous()
        if colors is not None and (not torch.is_tensor(colors) or colors.dtype != torch.float32 or colors.device != dev
                                   or tuple(colors.shape) != (n, 3)):
            raise _lib.LsrError(f"colors must be a float32 tensor of shape {(n, 3)} on {dev}")
        if not bool(torch.isfinite(points).all()):
            raise _lib.LsrError("from_point_cloud: the points hold a non-finite coordinate")
        dist2 = mean_knn_dist2(points)
        scaling = torch.log(torch.sqrt(torch.clamp_min(dist2, min_dist2)))[:, None].repeat(1, 3)
        K = (int(sh_degree) + 1) ** 2
        dc = torch.zeros((n, 1, 3), dtype=torch.float32, device=dev)
        if colors is not None:
            dc[:, 0, :] = (colors.detach() - 0.5) / 0.28209479177387814
        rotation = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        rotation[:, 0] = 1.0
        opacity = torch.full((n, 1), math.log(initial_opacity / (1.0 - initial_opacity)), dtype=torch.float32, device=dev)
        return cls(points, dc, torch.zeros((n, K - 1, 3), dtype=torch.float32, device=dev), opacity, scaling, rotation,
                   active_sh_degree=0)

    @property
    def num_gaussians(self) -> int:
        return self._xyz.shape[0]

    def replace_parameters_(self, **tensors: Tensor) -> None:
        """Install fresh ``nn.Parameter``s of a new row count (what densification and pruning produce): all six of
        ``xyz, features_dc, features_rest, opacity, scaling, rotation``, float32, on the scene's device, with the
        scene's SH width.  The tensors are taken as they are (detached, not copied); ``active_sh_degree`` and
        ``max_sh_degree`` stay.  An optimizer that held the old parameters has to be re-keyed by the caller
        (:meth:`latentsplat_amd.density.DensityControl.densify_and_prune` does)."""
        names = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
        if set(tensors) != set(names):
            raise _lib.LsrError(f"replace_parameters_ takes exactly {', '.join(names)}")
        n = tensors["xyz"].shape[0]
        rest = self._features_rest.shape[1]
        shapes = dict(xyz=(n, 3), features_dc=(n, 1, 3), features_rest=(n, rest, 3), opacity=(n, 1), scaling=(n, 3),
                      rotation=(n, 4))
        for k in names:
            t = tensors[k]
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shapes[k] or t.device != self._xyz.device:
                raise _lib.LsrError(f"replace_parameters_: {k} must be a float32 tensor of shape {shapes[k]} on {self._xyz.device}")
        for k in names:
            old = getattr(self, "_" + k)
            setattr(self, "_" + k, nn.Parameter(tensors[k].detach().contiguous(), requires_grad=old.requires_grad))

    def oneup_sh_degree(self) -> None:
        """Render one more SH band, up to the stored ones."""
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def _activate(self, scale_modifier: float, geometry: bool, filter_3d: Optional[Tensor] = None):
        if filter_3d is not None and torch.is_tensor(filter_3d) and filter_3d.numel() != self.num_gaussians:
            _filter(filter_3d, self.num_gaussians, self._xyz.device)          # stale: refused whatever the device
        if not self._xyz.is_cuda:
            raise _lib.LsrError("a GaussianScene is activated and rendered on the MI355X: move it to a ROCm ('cuda') device; "
                                "there is no CPU fallback")
        if filter_3d is not None:
            filt = _filter(filter_3d, self.num_gaussians, self._xyz.device)
            return _ActivateSceneFiltered.apply(self._features_dc, self._features_rest, self._opacity, self._scaling,
                                                self._rotation, filt, float(scale_modifier), geometry)
        return _ActivateScene.apply(self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation,
                                    float(scale_modifier), geometry)

    def compute_filter_3d(self, views: Tensor, width: int, **kw) -> Tensor:
        """The 3D smoothing filter of this scene's positions for the training cameras ``views`` (a table of
        ``build_view_table`` / ``make_view_table``) at image width ``width``: ``(n, 1)``, one HIP pass
        (:func:`latentsplat_amd.filter3d.compute_filter_3d`, which ``kw`` goes to).  The scene does not keep it: it is
        neither a parameter nor a buffer.  The caller holds the tensor, passes it to :meth:`activated`, :meth:`render` and
        :meth:`save_ply`, and computes it again when the Gaussians were densified, grown, pruned or have moved."""
        from .filter3d import compute_filter_3d
        return compute_filter_3d(self._xyz, views, width, **kw)

    def _posed(self, transforms: Optional[Tensor], transform_idx: Optional[Tensor], filter_3d, scale_modifier: float,
               geometry: bool, check: bool = True, poses=None):
        """The means and the activation of the scene moved by ``transforms``: the canonical parameters through
        :func:`latentsplat_amd.transform.transform_scene`, then through the unchanged activation.  With ``poses`` (a
        :class:`latentsplat_amd.pose.PartPoses`) instead: through :func:`latentsplat_amd.pose.pose_scene`, which also hands
        the poses their gradient."""
        xyz, rest, scaling, rotation = self._posed_parameters(transforms, transform_idx, filter_3d, check, poses)
        return xyz, _ActivateScene.apply(self._features_dc, rest, self._opacity, scaling, rotation, float(scale_modifier), geometry)

    def _posed_parameters(self, transforms: Optional[Tensor], transform_idx: Optional[Tensor], filter_3d, check: bool = True,
                          poses=None):
        """The raw parameters of the posed scene, ``(xyz, features_rest, scaling, rotation)``: what :meth:`_posed` activates."""
        from .transform import transform_scene
        if poses is not None and transforms is not None:
            raise _lib.LsrError("poses together with transforms: a scene is posed by one or the other (poses are the "
                                "differentiable form of the same similarities)")
        if filter_3d is not None:
            raise _lib.LsrError("transforms together with filter_3d: the 3D filter of a posed scene depends on where its parts "
                                "stand in front of the cameras and is the caller's to compute; pose the parameters with "
                                "transform_scene and pass the filter of the posed means to activate_scene_filtered")
        if not self._xyz.is_cuda:
            raise _lib.LsrError("a GaussianScene is activated and rendered on the MI355X: move it to a ROCm ('cuda') device; "
                                "there is no CPU fallback")
        if poses is not None:
            return poses(self._xyz, self._features_rest, self._scaling, self._rotation, transform_idx)
        return transform_scene(self._xyz, self._features_rest, self._scaling, self._rotation, transforms, transform_idx, check=check)

    def activated(self, scale_modifier: float = 1.0, filter_3d: Optional[Tensor] = None, transforms: Optional[Tensor] = None,
                  transform_idx: Optional[Tensor] = None, check_transforms: bool = True, poses=None) -> Scene3DGS:
        """The scene as the rasterizer takes it (differentiable in the parameters; ``scales`` and ``rotations`` are
        values only).  ``means`` is ``_xyz`` itself; ``sh_degree`` the active degree, ``shs`` all stored bands.  With
        ``filter_3d`` (:meth:`compute_filter_3d`) the 3D smoothing filter is inside the activation; ``None`` is the
        unfiltered map.  ``transforms`` / ``transform_idx``: the posed scene, as in :meth:`render` (``means`` is then the
        posed positions); ``poses``: the same with differentiable poses, as in :meth:`render`."""
        if transforms is not None or poses is not None:
            xyz, (shs, opacities, cov, scales, rotations) = self._posed(transforms, transform_idx, filter_3d, scale_modifier, True,
                                                                        check_transforms, poses)
            return Scene3DGS(means=xyz, covariances=cov, opacities=opacities, shs=shs, scales=scales, rotations=rotations,
                             sh_degree=self.active_sh_degree)
        shs, opacities, cov, scales, rotations = self._activate(scale_modifier, True, filter_3d)
        return Scene3DGS(means=self._xyz, covariances=cov, opacities=opacities, shs=shs, scales=scales,
                         rotations=rotations, sh_degree=self.active_sh_degree)

    def render(self, views: Tensor, height: int, width: int, scale_modifier: float = 1.0, filter_3d: Optional[Tensor] = None,
               transforms: Optional[Tensor] = None, transform_idx: Optional[Tensor] = None, check_transforms: bool = True,
               poses=None, antialiasing: bool = False, **kw):
        """``rasterize_views`` of the activated scene: ``(color, feature, mask, depth, radii)``.  ``views`` is a table
        of ``build_view_table`` / ``make_view_table`` (one that requires grad receives the camera gradient); ``kw``
        goes to ``rasterize_views``.  All stored SH coefficients are passed with ``sh_degree=active_sh_degree``.
        ``filter_3d`` (:meth:`compute_filter_3d`): render the scene with the 3D smoothing filter inside the activation.
        ``antialiasing=True``: the rasterizer compensates every splat's opacity for its 0.3 screen-space low-pass
        (``rasterize_views``); with ``filter_3d`` the two halves of Mip-Splatting, and independent of it.

        ``transforms`` (``(4, 4)`` or ``(T, 4, 4)`` similarities on the scene's device) with ``transform_idx`` (integer
        ``(n,)``: the transform of each Gaussian; ``None``: transform 0 for all; out of range: not moved) render the POSED
        scene: the canonical parameters go through :func:`latentsplat_amd.transform.transform_scene` (one more HIP launch;
        view-dependent colour rotated with the part) and then through the unchanged activation and rasterizer, so the
        gradients arrive at the canonical parameters; the transforms receive none.  ``check_transforms=True`` refuses what is
        not a similarity with one host read (a device sync) per call; a training loop that poses parts every step passes
        ``check_transforms=False``, which reads nothing back.  ``transforms=None`` is the code path
        without it.  Together with ``filter_3d`` it is refused: the filter of a posed scene is the caller's to compute.

        ``poses`` (a :class:`latentsplat_amd.pose.PartPoses`, with the same ``transform_idx``) poses the parts by learnable
        quaternions, translations and log-scales instead: the same posed scene, through
        :func:`latentsplat_amd.pose.pose_scene`, and the poses receive their gradient too.  It excludes ``transforms`` and,
        like it, ``filter_3d``; ``poses=None`` leaves every other path as it is."""
        from .rasterizer import rasterize_views
        if antialiasing:   # (only when asked for: the call without it is the call it always was)
            kw["antialiasing"] = True
        if transforms is not None or poses is not None:
            xyz, (shs, opacities, cov, _, _) = self._posed(transforms, transform_idx, filter_3d, scale_modifier, False,
                                                           check_transforms, poses)
            return rasterize_views(views, height, width, self.active_sh_degree, xyz, cov, opacities, shs=shs, **kw)
        shs, opacities, cov, _, _ = self._activate(scale_modifier, False, filter_3d)
        return rasterize_views(views, height, width, self.active_sh_degree, self._xyz, cov, opacities, shs=shs, **kw)

    def render_with_normals(self, views: Tensor, height: int, width: int, scale_modifier: float = 1.0,
                            filter_3d: Optional[Tensor] = None, transforms: Optional[Tensor] = None,
                            transform_idx: Optional[Tensor] = None, check_transforms: bool = True, poses=None,
                            antialiasing: bool = False, **kw):
        """:meth:`render` with the normals of the Gaussians (:func:`latentsplat_amd.normals.gaussian_normals`: the shortest
        axis of each, turned toward the camera, in camera space) as the ``features`` payload:
        ``(color, normal_map, mask, depth, radii)``.  ``normal_map (V, 3, H, W)`` is the blended sum of alpha T n (background
        0, not renormalised), which with ``depth`` and ``mask`` is what
        :func:`latentsplat_amd.normals.normal_consistency_loss` takes.  Every keyword is :meth:`render`'s.

        With ``transforms`` / ``poses`` the normals are those of the POSED raw scaling and rotation.  The payload is taken,
        so a caller's own ``features`` / ``feature_sh`` is refused.  Colour and normals are six payload channels: with
        ``means2D_abs`` the rasterizer's refusal of more than 4 payload channels applies unchanged (take the absolute
        gradient from a plain :meth:`render`).  The view table must carry depth mode NATIVE (what ``build_view_table`` /
        ``make_view_table`` write by default): the loss reads ``depth`` as the blended view-space z; nothing is read back to
        check it.  The normals hand a gradient to ``_rotation`` alone (the argmin and the sign are piecewise constant in
        the positions and scales); every other gradient is the rasterizer's.  The normals are NOT constant in the view
        rotation and have no gradient for it: a ``views`` that requires grad is refused, as by
        :meth:`render_with_distortion` (for a camera gradient that leaves the normals' part out, call
        ``gaussian_normals(views.detach(), ...)`` and :meth:`render` with ``features=``)."""
        from .normals import gaussian_normals
        from .rasterizer import rasterize_views
        if kw.get("features") is not None or kw.get("feature_sh") is not None:
            raise _lib.LsrError("render_with_normals: the features payload carries the normals; features / feature_sh of the "
                                "caller's own are refused (render them with render)")
        kw.pop("features", None)
        kw.pop("feature_sh", None)
        if antialiasing:
            kw["antialiasing"] = True
        if transforms is not None or poses is not None:
            xyz, rest, scaling, rotation = self._posed_parameters(transforms, transform_idx, filter_3d, check_transforms, poses)
            shs, opacities, cov, _, _ = _ActivateScene.apply(self._features_dc, rest, self._opacity, scaling, rotation,
                                                             float(scale_modifier), False)
        else:
            xyz, scaling, rotation = self._xyz, self._scaling, self._rotation
            shs, opacities, cov, _, _ = self._activate(scale_modifier, False, filter_3d)
        normals = gaussian_normals(views, xyz, scaling, rotation)
        return rasterize_views(views, height, width, self.active_sh_degree, xyz, cov, opacities, shs=shs, features=normals, **kw)

    def _surface_inputs(self, who: str, scale_modifier, filter_3d, transforms, transform_idx, check_transforms, poses,
                        antialiasing, kw):
        """What :meth:`render_with_distortion` and :meth:`render_surface` share: the refusal of a caller's payload and the
        (posed) raw parameters with their activation, ``(xyz, scaling, rotation, shs, opacities, cov)``."""
        if kw.get("features") is not None or kw.get("feature_sh") is not None:
            raise _lib.LsrError(f"{who}: the features payload is taken; features / feature_sh of the caller's own are refused "
                                "(render them with render)")
        kw.pop("features", None)
        kw.pop("feature_sh", None)
        if antialiasing:
            kw["antialiasing"] = True
        if transforms is not None or poses is not None:
            xyz, rest, scaling, rotation = self._posed_parameters(transforms, transform_idx, filter_3d, check_transforms, poses)
            shs, opacities, cov, _, _ = _ActivateScene.apply(self._features_dc, rest, self._opacity, scaling, rotation,
                                                             float(scale_modifier), False)
        else:
            xyz, scaling, rotation = self._xyz, self._scaling, self._rotation
            shs, opacities, cov, _, _ = self._activate(scale_modifier, False, filter_3d)
        return xyz, scaling, rotation, shs, opacities, cov

    def render_with_distortion(self, views: Tensor, height: int, width: int, space: str = "ndc", pivot: Optional[Tensor] = None,
                               scale_modifier: float = 1.0, filter_3d: Optional[Tensor] = None,
                               transforms: Optional[Tensor] = None, transform_idx: Optional[Tensor] = None,
                               check_transforms: bool = True, poses=None, antialiasing: bool = False,
                               check_near_far: bool = True, **kw):
        """:meth:`render` with the depth moments of the Gaussians
        (:func:`latentsplat_amd.distortion.gaussian_depth_moments`: ``(m', m'^2)``, ``m' = m - pivot``, ``m`` the depth in
        ``space``) as the ``features`` payload: ``(color, moment_map, mask, depth, radii)``.  ``moment_map (V, 2, H, W)`` is
        the blended ``(M1, M2)``, which with ``mask`` is what :func:`latentsplat_amd.distortion.distortion_loss` takes.
        Every other keyword is :meth:`render`'s.

        With ``transforms`` / ``poses`` the moments are those of the POSED positions.  The payload is taken, so a caller's
        own ``features`` / ``feature_sh`` is refused.  Colour and moments are five payload channels: with ``means2D_abs``
        the rasterizer's refusal of more than 4 payload channels applies unchanged.  Any depth mode may be in the view
        table: nothing here reads ``depth``.  ``space="ndc"`` reads near / far from slots 42 / 43
        (:func:`latentsplat_amd.distortion.with_near_far` for a NATIVE table) and checks them with one host read per call
        unless ``check_near_far=False``.  The moments hand their gradient to the positions alone: a ``views`` that requires
        grad is refused (the moments have no pose gradient, and a partial one would be silent)."""
        from .distortion import gaussian_depth_moments
        from .rasterizer import rasterize_views
        xyz, _, _, shs, opacities, cov = self._surface_inputs("render_with_distortion", scale_modifier, filter_3d, transforms,
                                                              transform_idx, check_transforms, poses, antialiasing, kw)
        moments = gaussian_depth_moments(views, xyz, space, pivot, check_near_far)
        return rasterize_views(views, height, width, self.active_sh_degree, xyz, cov, opacities, shs=shs, features=moments, **kw)

    def render_surface(self, views: Tensor, height: int, width: int, space: str = "ndc", pivot: Optional[Tensor] = None,
                       scale_modifier: float = 1.0, filter_3d: Optional[Tensor] = None, transforms: Optional[Tensor] = None,
                       transform_idx: Optional[Tensor] = None, check_transforms: bool = True, poses=None,
                       antialiasing: bool = False, check_near_far: bool = True, **kw):
        """Both geometric regularisers from one render: ``(color, normal_map, moment_map, mask, depth, radii)``, the
        ``normal_map (V, 3, H, W)`` of :meth:`render_with_normals` and the ``moment_map (V, 2, H, W)`` of
        :meth:`render_with_distortion`.  The payload is normals and moments: five feature channels, eight with colour, which
        is still inside the compositing kernels' 8-channel instances.  The two operator outputs are joined by one
        ``torch.cat`` (a copy of 20 bytes per (view, Gaussian) each way; tools/bench_distortion.py times it).  The view table
        must carry depth mode NATIVE, as for :meth:`render_with_normals`; ``means2D_abs`` is refused by the rasterizer, as
        there.  Neither payload has a gradient for the view table, which both depend on: a ``views`` that requires grad is
        refused, as by the two renders this one joins."""
        from .distortion import gaussian_depth_moments
        from .normals import gaussian_normals
        from .rasterizer import rasterize_views
        xyz, scaling, rotation, shs, opacities, cov = self._surface_inputs("render_surface", scale_modifier, filter_3d,
                                                                           transforms, transform_idx, check_transforms, poses,
                                                                           antialiasing, kw)
        normals = gaussian_normals(views, xyz, scaling, rotation)
        moments = gaussian_depth_moments(views, xyz, space, pivot, check_near_far)
        payload = torch.cat((normals, moments), dim=-1)
        color, feature, mask, depth, radii = rasterize_views(views, height, width, self.active_sh_degree, xyz, cov, opacities,
                                                             shs=shs, features=payload, **kw)
        return color, feature[:, :3], feature[:, 3:], mask, depth, radii

    @torch.no_grad()
    def extract_mesh(self, views: Tensor, height: int, width: int, voxel_size: float, bounds=None, trunc: Optional[float] = None,
                     batch: int = 8, min_weight: float = 1.0, **render_kw):
        """A triangle mesh of the scene's surface, ``(vertices (Nv, 3), faces (Nf, 3) int32, colors (Nv, 3))``: the views
        are rendered ``batch`` at a time (colour, depth of depth mode NATIVE, mask: :meth:`render`, which ``render_kw``
        goes to), fused into a :class:`latentsplat_amd.mesh.TSDFVolume` of ``voxel_size`` (world units) and the zero level
        set is extracted by marching tetrahedra.  ``bounds = (lo, hi)`` defaults to the box of the positions of the
        Gaussians with opacity above 0.5, padded by ``trunc`` (default: 4 voxel sizes; a default, not a measurement).
        ``views`` must carry depth mode NATIVE, as for :meth:`render_with_normals`.  Values only; one host read for the
        default bounds and one for the mesh's size."""
        from .mesh import TSDFVolume
        trunc = 4.0 * float(voxel_size) if trunc is None else float(trunc)
        if bounds is None:
            solid = self._xyz[torch.sigmoid(self._opacity).reshape(-1) > 0.5]
            if solid.shape[0] == 0:
                raise _lib.LsrError("extract_mesh: no Gaussian has opacity above 0.5; pass bounds")
            lo, hi = (solid.min(dim=0).values - trunc).tolist(), (solid.max(dim=0).values + trunc).tolist()
        else:
            lo, hi = bounds
        volume = TSDFVolume.from_bounds(lo, hi, voxel_size, trunc=trunc, color=True, device=self._xyz.device)
        for at in range(0, views.shape[0], max(1, int(batch))):
            v = views[at:at + max(1, int(batch))]
            color, _, mask, depth, _ = self.render(v, height, width, **render_kw)
            volume.integrate(depth, mask, v, color=color)
        return volume.extract_mesh(min_weight)

    def transform_(self, M: Tensor, idx: Optional[Tensor] = None) -> "GaussianScene":
        """Move the scene in place by the similarity ``M (4, 4)`` (or ``(T, 4, 4)`` with ``idx (n,)`` naming the transform
        of each Gaussian; out of range: not moved), under ``no_grad``: ``_xyz``, ``_features_rest`` (every SH band rotated
        with the scene), ``_scaling`` and ``_rotation`` are overwritten by one HIP launch
        (:func:`latentsplat_amd.transform.transform_scene_`); ``_features_dc`` and ``_opacity`` stay.  ``M`` may live on
        any device; anything that is not a similarity is refused.  Returns ``self``.

        What does not survive: the optimizer moments of ``_xyz``, ``_features_rest``, ``_scaling`` and ``_rotation`` (the
        first moment would have to be rotated with the parameters and ``exp_avg_sq`` is not covariant under a rotation at
        all), so the caller resets their optimizer state; and a ``filter_3d`` computed before, which must be multiplied by
        ``s`` (with cameras moved by :func:`latentsplat_amd.transform.transform_cameras`) or computed again."""
        from .transform import transform_scene_
        if not self._xyz.is_cuda:
            raise _lib.LsrError("a GaussianScene is transformed on the MI355X: move it to a ROCm ('cuda') device; there is no "
                                "CPU fallback")
        if not torch.is_tensor(M):
            raise _lib.LsrError("transform_ takes a (4, 4) or (T, 4, 4) tensor")
        with torch.no_grad():
            if M.device != self._xyz.device:
                from .transform import _matrices
                M = _matrices(M, True).to(self._xyz.device)
                transform_scene_(self._xyz, self._features_rest, self._scaling, self._rotation, M, idx, check=False)
            else:
                transform_scene_(self._xyz, self._features_rest, self._scaling, self._rotation, M, idx)
        return self

    @classmethod
    def merge(cls, scenes: Sequence["GaussianScene"], transforms: Optional[Tensor] = None) -> "GaussianScene":
        """One scene from several: the rows concatenated in order, ``_features_rest`` zero-padded to the highest stored
        degree, ``active_sh_degree`` the maximum.  With ``transforms (len(scenes), 4, 4)`` scene ``i`` is moved by
        transform ``i`` first, in ONE launch over the merged tensors with the scene number as the per-Gaussian index
        (two captures brought into one coordinate system).  The scenes must be on one device."""
        scenes = list(scenes)
        if not scenes or any(not isinstance(sc, GaussianScene) for sc in scenes):
            raise _lib.LsrError("merge takes a non-empty sequence of GaussianScene")
        dev = scenes[0]._xyz.device
        if any(sc._xyz.device != dev for sc in scenes):
            raise _lib.LsrError("merge: the scenes must be on one device")
        if transforms is not None and (not torch.is_tensor(transforms) or tuple(transforms.shape) != (len(scenes), 4, 4)):
            raise _lib.LsrError(f"merge: transforms must be ({len(scenes)}, 4, 4), one per scene")
        rest_rows = max(sc._features_rest.shape[1] for sc in scenes)
        with torch.no_grad():
            cat = lambda name: torch.cat([getattr(sc, name).detach() for sc in scenes], dim=0)
            rest = torch.cat([torch.nn.functional.pad(sc._features_rest.detach(), (0, 0, 0, rest_rows - sc._features_rest.shape[1]))
                              for sc in scenes], dim=0)
            merged = cls(cat("_xyz"), cat("_features_dc"), rest, cat("_opacity"), cat("_scaling"), cat("_rotation"),
                         active_sh_degree=max(sc.active_sh_degree for sc in scenes))
            if transforms is not None:
                counts = torch.tensor([sc.num_gaussians for sc in scenes], device=dev)
                merged.transform_(transforms, torch.repeat_interleave(torch.arange(len(scenes), device=dev), counts))
        return merged

    def quantize(self, **kw):
        """The scene with its view-dependent colour and its shape replaced by codebook indices
        (:func:`latentsplat_amd.vq.quantize_scene`, which ``kw`` goes to): a
        :class:`latentsplat_amd.vq.QuantizedScene`."""
        from .vq import quantize_scene
        return quantize_scene(self, **kw)

    def rows(self) -> Tensor:
        """The scene as rows of a scene file (:func:`parameters_to_rows`), on the parameters' device."""
        return parameters_to_rows(self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling,
                                  self._rotation)

    def save_ply(self, path, filter_3d: Optional[Tensor] = None) -> None:
        """Write the raw parameters as a standard 3DGS scene file.  The values go out as they are: a scene that was
        loaded and is saved untouched has bit-identical rows.  With ``filter_3d`` the FUSED scene is written instead:
        opacity logits and log-scales with the 3D smoothing filter baked in
        (:func:`latentsplat_amd.filter3d.fused_parameters`), so that any viewer shows the filtered scene; the other
        columns as they are."""
        if filter_3d is None:
            rows = self.rows().cpu()
        else:
            from .filter3d import fused_parameters
            _filter(filter_3d, self.num_gaussians, self._xyz.device)
            opacity, scaling = fused_parameters(self._opacity, self._scaling, filter_3d)
            rows = parameters_to_rows(self._xyz, self._features_dc, self._features_rest, opacity, scaling, self._rotation).cpu()
        path = Path(path)
        path.parent.mkdir(exist_ok=True, parents=True)
        _lib.call("lsr_ply_write_scene_host", os.fsencode(str(path)), C.c_void_p(rows.data_ptr()), rows.shape[0],
                  (self.max_sh_degree + 1) ** 2)
