"""Pose gradients for the rigid parts of a 3DGS scene: the similarity transform of :mod:`latentsplat_amd.transform`,
differentiable in the transforms themselves, in HIP.

A pose is a raw quaternion ``p`` (w,x,y,z, any non-zero norm), a translation ``t`` and, optionally, a log-scale ``l``:
``R = R(p / |p|)``, ``s = exp(l)``, ``x' = s R x + t``.  A 4x4 matrix is not a chart of the similarity group (which is why
``transform_scene`` gives its matrices no gradient); these seven numbers are.

:func:`pose_matrices` builds the ``(T, 4, 4)`` similarities (``lsr_pose_matrices``, evaluated in double).
:func:`pose_scene` is ``transform_scene`` on those matrices, bit for bit, as a ``torch.autograd.Function`` that is
differentiable in the four scene tensors (the existing adjoint launch, the same bits as ``transform_scene``'s) and in the
three pose tensors (``lsr_scene_pose_grad``, csrc/scene_pose.hip, C ABI include/lsr_pose.h: one streaming pass that forms 7
numbers per Gaussian from the saved input positions, the saved output quaternions and coefficients and the upstream
gradients, reduced per transform without atomics in a fixed order, plus one small finishing launch).  The pose launches
run only when a pose tensor needs a gradient.  Nothing is read back to the host, so the op can be captured in a graph; the
workspace comes from torch's caching allocator.  :class:`PartPoses` holds the poses of ``num`` parts as parameters.

At most ``LSR_POSE_MAX_TRANSFORMS`` (256) transforms per call; covariance-form scenes are not covered; float32 ROCm tensors
only, there is no CPU fallback.  Re-parametrising a pose (``from_matrices``) does not carry optimizer moments over."""
from __future__ import annotations

import ctypes as C
from math import isqrt
from typing import Optional

import torch
from torch import Tensor, nn

from . import _args, _lib
from ._args import ptr
from .transform import _NAMES, _check_scene, _index, _split, apply_records, transform_records

MAX_TRANSFORMS = _lib.POSE_MAX_TRANSFORMS


def _check_poses(quaternions, translations, log_scales, what: str):
    for name, t in (("quaternions", quaternions), ("translations", translations), ("log_scales", log_scales)):
        if t is None and name == "log_scales":
            continue
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError(f"{what} needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    T = quaternions.shape[0]
    if quaternions.dim() != 2 or quaternions.shape[1] != 4 or tuple(translations.shape) != (T, 3) or \
            (log_scales is not None and tuple(log_scales.shape) != (T,)):
        raise _lib.LsrError("quaternions must be (T, 4), translations (T, 3) and log_scales (T,) or None")
    if T < 1:
        raise _lib.LsrError("at least one transform is needed")
    devs = {quaternions.device, translations.device} | ({log_scales.device} if log_scales is not None else set())
    if len(devs) != 1:
        raise _lib.LsrError("the pose tensors must be on one device")
    return T


def _pose_matrices(q: Tensor, t: Tensor, ls: Optional[Tensor]) -> Tensor:
    T = q.shape[0]
    out = torch.empty((T, 4, 4), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.call("lsr_pose_matrices", T, ptr(q), ptr(t), ptr(ls), ptr(out), _args.stream(q))
    return out


def pose_matrices(quaternions: Tensor, translations: Tensor, log_scales: Optional[Tensor] = None) -> Tensor:
    """``lsr_pose_matrices``: the float32 similarities ``(T, 4, 4)`` of raw quaternions ``(T, 4)`` (w,x,y,z, any non-zero
    norm), translations ``(T, 3)`` and log-scales ``(T,)`` (``None``: ``s = 1``), evaluated in double in one small launch.
    Values only (no gradient: :func:`pose_scene` is the differentiable op).  float32 ROCm tensors."""
    _check_poses(quaternions, translations, log_scales, "pose_matrices")
    return _pose_matrices(quaternions.detach().contiguous(), translations.detach().contiguous(),
                          None if log_scales is None else log_scales.detach().contiguous())


class _PoseScene(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, features_rest, scaling, rotation, quaternions, translations, log_scales, idx):
        ctx.set_materialize_grads(False)
        n, K = xyz.shape[0], features_rest.shape[1] + 1
        q = quaternions.detach().contiguous()
        matrices = _pose_matrices(q, translations.detach().contiguous(),
                                  None if log_scales is None else log_scales.detach().contiguous())
        records = transform_records(matrices, isqrt(K) - 1, check=False)
        ins = dict(xyz=xyz.detach().contiguous(), features_rest=features_rest.detach().contiguous(),
                   scaling=scaling.detach().contiguous(), rotation=_args.quad(rotation.detach().contiguous()))
        outs = {k: torch.empty_like(t) for k, t in ins.items()}
        apply_records(records, idx, ins, outs, n, K)
        adjoint = transform_records(matrices, isqrt(K) - 1, adjoint=True, check=False) if any(ctx.needs_input_grad[:4]) else None
        posed = any(ctx.needs_input_grad[4:7])
        ctx.save_for_backward(adjoint, idx, *((records, q, ins["xyz"], outs["rotation"], outs["features_rest"]) if posed else ()))
        ctx.dims = (n, K, q.shape[0])
        return tuple(outs[k] for k in _NAMES)

    @staticmethod
    def backward(ctx, *grads):
        n, K, T = ctx.dims
        adjoint, idx = ctx.saved_tensors[:2]
        ins, outs = {}, {}
        for k, need, g in zip(_NAMES, ctx.needs_input_grad, grads):
            if need and g is not None:
                g = g.detach().contiguous()
                ins[k] = _args.quad(g) if k == "rotation" else g
                outs[k] = torch.empty_like(g)
        if outs:
            apply_records(adjoint, idx, ins, outs, n, K)
        pose = [None, None, None]
        if any(ctx.needs_input_grad[4:7]):
            records, q, xyz, rot, rest = ctx.saved_tensors[2:]
            dev = q.device
            g = {k: (None if v is None else v.detach().contiguous()) for k, v in zip(_NAMES, grads)}
            if g["rotation"] is not None:
                g["rotation"] = _args.quad(g["rotation"])
            shapes = ((T, 4), (T, 3), (T,))
            pose = [torch.empty(s, dtype=torch.float32, device=dev) if need else None
                    for s, need in zip(shapes, ctx.needs_input_grad[4:7])]
            lib = _lib.load()
            ws = _args.workspace(max(int(lib.lsr_pose_grad_workspace_bytes(n, K, T)), 8), dev)
            dims = _lib.TransformDims(n=n, sh_coeffs=K, num_transforms=T, reserved0=0, reserved1=0)
            gin = _lib.PoseGradIn(xyz=ptr(xyz), rotation=ptr(rot), features_rest=ptr(rest), g_xyz=ptr(g["xyz"]),
                                  g_features_rest=ptr(g["features_rest"]), g_scaling=ptr(g["scaling"]),
                                  g_rotation=ptr(g["rotation"]))
            with torch.cuda.device(dev):
                _lib.call("lsr_scene_pose_grad", C.byref(dims), ptr(records), ptr(idx), ptr(q), C.byref(gin), ptr(ws),
                          ws.numel(), ptr(pose[0]), ptr(pose[1]), ptr(pose[2]), _args.stream(dev))
        return tuple(outs.get(k) for k in _NAMES) + tuple(pose) + (None,)


def pose_scene(xyz: Tensor, features_rest: Tensor, scaling: Tensor, rotation: Tensor, quaternions: Tensor,
               translations: Tensor, log_scales: Optional[Tensor] = None, idx: Optional[Tensor] = None):
    """The raw parameters of a scene moved by the poses ``(quaternions (T, 4), translations (T, 3), log_scales (T,) or
    None)``: ``(xyz', features_rest', scaling', rotation')``, the same bits as ``transform_scene`` with
    :func:`pose_matrices` of the poses, differentiable in all seven tensors.  ``idx`` as in ``transform_scene`` (``None``:
    transform 0 for every Gaussian; out of range: passes through and contributes nothing to any pose).

    The four scene gradients come from the adjoint launch of ``transform_scene`` (the same bits); the pose gradients from
    ``lsr_scene_pose_grad`` (one pass over the scene and one small launch, only when a pose tensor needs a gradient; no
    atomics: the same bits every call).  The gradient of ``quaternions`` is orthogonal to each quaternion (its norm is not
    a degree of freedom).  Nothing is read back to the host.  At most ``LSR_POSE_MAX_TRANSFORMS`` transforms; float32 ROCm
    tensors only."""
    n, K = _check_scene(xyz, features_rest, scaling, rotation)
    T = _check_poses(quaternions, translations, log_scales, "pose_scene")
    if quaternions.device != xyz.device:
        raise _lib.LsrError(f"the poses must be on the scene's device {xyz.device} (no CPU fallback)")
    if T > MAX_TRANSFORMS:
        raise _lib.LsrError(f"{T} transforms: pose_scene is unsupported beyond LSR_POSE_MAX_TRANSFORMS = {MAX_TRANSFORMS} per call")
    return _PoseScene.apply(xyz, features_rest, scaling, rotation, quaternions, translations, log_scales,
                            _index(idx, n, xyz.device))


def _rotation_quaternion(R: Tensor) -> Tensor:
    """A unit quaternion (w,x,y,z), float64, of the rotation ``R (3, 3)``, by the largest of the four pivots."""
    m = R.tolist()
    tr = m[0][0] + m[1][1] + m[2][2]
    cand = [tr, m[0][0], m[1][1], m[2][2]]
    k = cand.index(max(cand))
    if k == 0:
        q = [1 + tr, m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1]]
    elif k == 1:
        q = [m[2][1] - m[1][2], 1 + m[0][0] - m[1][1] - m[2][2], m[0][1] + m[1][0], m[0][2] + m[2][0]]
    elif k == 2:
        q = [m[0][2] - m[2][0], m[0][1] + m[1][0], 1 - m[0][0] + m[1][1] - m[2][2], m[1][2] + m[2][1]]
    else:
        q = [m[1][0] - m[0][1], m[0][2] + m[2][0], m[1][2] + m[2][1], 1 - m[0][0] - m[1][1] + m[2][2]]
    q = torch.tensor(q, dtype=torch.float64)
    return q / q.norm()


class PartPoses(nn.Module):
    """The poses of ``num`` rigid parts as parameters: ``rotation (num, 4)`` (raw quaternions, identity), ``translation
    (num, 3)`` (zero) and, with ``learn_scale``, ``log_scale (num,)`` (zero).  ``forward`` poses a scene's raw parameters
    through :func:`pose_scene`, so a loss on the render reaches the poses; ``scene.render(..., poses=P, transform_idx=idx)``
    does the same inside a scene."""

    def __init__(self, num: int, learn_scale: bool = False):
        super().__init__()
        if not 1 <= int(num) <= MAX_TRANSFORMS:
            raise _lib.LsrError(f"PartPoses holds 1..{MAX_TRANSFORMS} poses (LSR_POSE_MAX_TRANSFORMS), not {num}")
        rot = torch.zeros(int(num), 4)
        rot[:, 0] = 1.0
        self.rotation = nn.Parameter(rot)
        self.translation = nn.Parameter(torch.zeros(int(num), 3))
        self.register_parameter("log_scale", nn.Parameter(torch.zeros(int(num))) if learn_scale else None)

    @property
    def num(self) -> int:
        return self.rotation.shape[0]

    def matrices(self) -> Tensor:
        """The float32 similarities ``(num, 4, 4)`` on the poses' ROCm device (:func:`pose_matrices`; values only)."""
        return pose_matrices(self.rotation, self.translation, self.log_scale)

    def forward(self, xyz: Tensor, features_rest: Tensor, scaling: Tensor, rotation: Tensor, idx: Optional[Tensor] = None):
        return pose_scene(xyz, features_rest, scaling, rotation, self.rotation, self.translation, self.log_scale, idx)

    def as_matrices(self) -> Tensor:
        """The similarities ``(num, 4, 4)`` as float64 on the CPU, in plain torch (runs anywhere)."""
        q = self.rotation.detach().to(device="cpu", dtype=torch.float64)
        w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        s = torch.ones(self.num, dtype=torch.float64) if self.log_scale is None else \
            self.log_scale.detach().to(device="cpu", dtype=torch.float64).exp()
        M = torch.zeros(self.num, 4, 4, dtype=torch.float64)
        M[:, :3, :3] = s[:, None, None] * R
        M[:, :3, 3] = self.translation.detach().to(device="cpu", dtype=torch.float64)
        M[:, 3, 3] = 1.0
        return M

    @classmethod
    def from_matrices(cls, M: Tensor, learn_scale: Optional[bool] = None) -> "PartPoses":
        """Poses that reproduce the similarities ``M (4, 4)`` or ``(T, 4, 4)`` (on the device of ``M``): unit quaternions of
        their rotations, their translations and the logs of their scales.  ``learn_scale=None`` keeps a ``log_scale`` only
        when some scale differs from 1; ``False`` refuses such matrices.  A new module: optimizer moments of another
        parametrisation do not carry over."""
        from .transform import _matrices
        M = _matrices(M, True)
        s, R, t = _split(M.to(device="cpu", dtype=torch.float64))
        scaled = bool((s - 1.0).abs().max() > 1e-6)
        if learn_scale is None:
            learn_scale = scaled
        if scaled and not learn_scale:
            raise _lib.LsrError("from_matrices: a scale other than 1 needs learn_scale=True")
        poses = cls(M.shape[0], learn_scale=learn_scale)
        with torch.no_grad():
            poses.rotation.copy_(torch.stack([_rotation_quaternion(r) for r in R]))
            poses.translation.copy_(t)
            if learn_scale:
                poses.log_scale.copy_(s.log())
        return poses.to(M.device)
