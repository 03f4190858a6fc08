"""Similarity transforms of a 3DGS scene: ``x' = s R x + t`` applied to the raw parameters a trainer holds, in HIP.

Moving a scene is more than moving its means.  For ``M = [[sR, t], [0, 1]]`` (``R`` a proper rotation, ``s > 0``):

* ``xyz`` becomes ``s R x + t``;
* ``rotation`` (w,x,y,z, any non-zero norm) becomes ``q_R (x) q``, the Hamilton product with the unit quaternion of ``R``;
* ``scaling`` (logs) becomes ``scaling + log s``;
* band ``l`` of ``features_rest`` (rows ``l^2 - 1 .. (l+1)^2 - 2``, each channel) becomes ``T_l(R) c_l``, where ``T_l`` is
  defined by ``B_l(R d) = T_l(R) B_l(d)`` for the ``"3dgs"`` colour basis ``B``: the moved scene shows along ``R d`` the
  colour the scene showed along ``d``.  A tool that leaves ``f_rest`` alone keeps the highlights glued to the old axes;
* ``features_dc`` and ``opacity`` do not change.

:func:`transform_scene` is that map as a ``torch.autograd.Function`` over ``lsr_transform_records`` /
``lsr_scene_transform`` (csrc/scene_transform.hip, C ABI include/lsr_transform.h): one launch over the parameters each
way, the backward being the same kernel on the records of the adjoint map.  Several transforms with a per-Gaussian index
pose the rigid parts of a scene in the same launch.  The transforms are data here: a 4x4 matrix is not a chart of the
similarity group and receives no gradient; :func:`latentsplat_amd.pose.pose_scene` is the same map with the poses as
quaternions, translations and log-scales, and differentiable in them.  Covariance-form scenes (``Scene3DGS``, the latent
``Gaussians``) are not covered.  The kernels take float32 ROCm tensors only; there is no CPU fallback.
:func:`similarity_matrix`, :func:`invert_similarity` and :func:`transform_cameras` are plain torch and run anywhere."""
from __future__ import annotations

import ctypes as C
from math import isqrt
from typing import Optional

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_NAMES = ("xyz", "features_rest", "scaling", "rotation")
SIMILARITY_TOLERANCE = 1e-5


def _as64(x, device=None) -> Tensor:
    return x.detach().to(dtype=torch.float64) if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float64, device=device)


def quaternion_matrix(q) -> Tensor:
    """The rotation matrix (3, 3), float64, of a w,x,y,z quaternion of any non-zero norm."""
    q = _as64(q)
    w, x, y, z = (q / q.norm()).unbind()
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)


def similarity_matrix(rotation=None, translation=None, scale: float = 1.0) -> Tensor:
    """``[[s R, t], [0, 1]]`` as a float64 ``(4, 4)`` tensor.  ``rotation`` is a 3x3 matrix or a w,x,y,z quaternion (any
    non-zero norm); ``None`` is the identity.  ``translation`` is ``(3,)``; ``None`` is zero."""
    M = torch.eye(4, dtype=torch.float64)
    if rotation is not None:
        r = _as64(rotation).cpu()
        if tuple(r.shape) == (4,):
            r = quaternion_matrix(r)
        if tuple(r.shape) != (3, 3):
            raise _lib.LsrError(f"rotation must be a 3x3 matrix or a w,x,y,z quaternion, got shape {tuple(r.shape)}")
        M[:3, :3] = r
    M[:3, :3] *= float(scale)
    if translation is not None:
        M[:3, 3] = _as64(translation).cpu().reshape(3)
    return M


def _split(M: Tensor):
    """``(s, R, t)`` of similarities ``(..., 4, 4)``: ``s = cbrt(det)`` of the linear part ``A`` and ``R`` the rotation
    nearest to ``A / s`` (its orthogonal polar factor, as ``lsr_transform_records`` takes it: a matrix of rounded entries
    is a similarity only to that rounding)."""
    A, t = M[..., :3, :3], M[..., :3, 3]
    det = torch.linalg.det(A)
    s = det.abs().pow(1.0 / 3.0) * det.sign()
    u, _, vh = torch.linalg.svd(A / s[..., None, None])
    return s, u @ vh, t


def invert_similarity(M: Tensor) -> Tensor:
    """The inverse of similarities ``(..., 4, 4)``: ``[[R^T / s, -R^T t / s], [0, 1]]``, in ``M``'s dtype, formed from the
    transpose (no general inverse)."""
    s, R, t = _split(M)
    out = torch.zeros_like(M)
    Ai = R.transpose(-1, -2) / s[..., None, None]
    out[..., :3, :3] = Ai
    out[..., :3, 3] = -(Ai @ t[..., None])[..., 0]
    out[..., 3, 3] = 1
    return out


def check_similarity(M: Tensor) -> None:
    """Refuse, with ``LsrError``, matrices ``(T, 4, 4)`` that are not similarities; one host read, float64.  With ``A`` the
    linear part and ``s^2 = trace(A^T A) / 3``: non-finite entries, a last row other than ``0 0 0 1``, ``det A <= 0`` (a
    reflection, or a singular matrix) and ``|A^T A - s^2 I| > 1e-5 s^2`` in any entry (shear, non-uniform scale) are
    refused.  The bound 1e-5 is roughly the float32 orthonormality of a rotation a user builds from float32 products (a few
    dozen roundings of 6e-8); an exactly orthonormal float64 matrix rounded to float32 is within 2e-7."""
    H = M.detach().to(device="cpu", dtype=torch.float64)
    for i, m in enumerate(H):
        where = f"transform {i}" if H.shape[0] > 1 else "the transform"
        if not bool(torch.isfinite(m).all()):
            raise _lib.LsrError(f"{where} has a non-finite entry")
        if m[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
            raise _lib.LsrError(f"{where} is not a similarity: its last row is {m[3].tolist()}, not 0 0 0 1")
        A = m[:3, :3]
        det = float(torch.linalg.det(A))
        if not det > 0.0:
            raise _lib.LsrError(f"{where} is not a similarity: the determinant of its linear part is {det:g} (a reflection or a "
                                "singular matrix); a scene can only be rotated, scaled uniformly and moved")
        gram = A.T @ A
        s2 = float(gram.diagonal().sum()) / 3.0
        dev = float((gram - s2 * torch.eye(3, dtype=torch.float64)).abs().max())
        if dev > SIMILARITY_TOLERANCE * s2:
            raise _lib.LsrError(f"{where} is not a similarity: |A^T A - s^2 I| = {dev / s2:.2g} s^2 exceeds {SIMILARITY_TOLERANCE:g} "
                                "s^2 (shear or non-uniform scale)")


def _matrices(M, check: bool) -> Tensor:
    """``(T, 4, 4)`` from ``(4, 4)`` or ``(T, 4, 4)``, shape-checked; with ``check`` held to :func:`check_similarity`."""
    if not torch.is_tensor(M) or M.dim() not in (2, 3) or tuple(M.shape[-2:]) != (4, 4) or not M.is_floating_point():
        raise _lib.LsrError("transforms must be a floating-point tensor of shape (4, 4) or (T, 4, 4)")
    M = M.detach().reshape(-1, 4, 4)
    if M.shape[0] < 1:
        raise _lib.LsrError("at least one transform is needed")
    if check:
        check_similarity(M)
    return M


def transform_records(M: Tensor, degree: int, adjoint: bool = False, check: bool = True) -> Tensor:
    """``lsr_transform_records``: the per-transform constants ``(T, LSR_TRANSFORM_RECORD_FLOATS(degree))`` the kernel reads,
    from similarities ``M (4, 4)`` or ``(T, 4, 4)`` on a ROCm device (any float dtype; the kernel reads float32).  A record
    holds the linear part ``sR``, ``t``, ``log s``, ``q_R`` and the band blocks ``T_1 .. T_degree``; with ``adjoint`` the
    constants of the adjoint map (``(sR)^T``, 0, 0, ``conj(q_R)``, ``T_l^T``).  One small launch, evaluated in double.

    ``check=True`` first refuses anything that is not a similarity (:func:`check_similarity`: reflections, shear,
    non-uniform scale, a bad last row, non-finite entries; orthonormality is held to ``1e-5 s^2``, roughly what float32
    products of a user-built rotation give) with one host read in float64.  ``check=False`` performs no host read."""
    if not 0 <= int(degree) <= _lib.TRANSFORM_MAX_DEGREE:
        raise _lib.LsrError(f"degree must be in 0..{_lib.TRANSFORM_MAX_DEGREE}")
    M = _matrices(M, check)
    if not M.is_cuda:
        raise _lib.LsrError("transform_records needs the transforms on a ROCm ('cuda') device (no CPU fallback)")
    M = M.to(torch.float32).contiguous()
    T = M.shape[0]
    out = torch.empty((T, _lib.transform_record_floats(int(degree))), dtype=torch.float32, device=M.device)
    with torch.cuda.device(M.device):
        _lib.call("lsr_transform_records", T, ptr(M), int(degree), 1 if adjoint else 0, ptr(out), _args.stream(M))
    return out


def _index(idx, n: int, dev) -> Optional[Tensor]:
    if idx is None:
        return None
    if not torch.is_tensor(idx) or idx.is_floating_point() or tuple(idx.shape) != (n,) or idx.device != dev:
        raise _lib.LsrError(f"idx must be an integer tensor of shape ({n},) on {dev}")
    return idx.detach().to(torch.int32).contiguous()


def apply_records(records: Tensor, idx: Optional[Tensor], inputs: dict, outputs: dict, n: int, K: int) -> None:
    """``lsr_scene_transform`` as it is (no autograd): ``inputs`` and ``outputs`` map some of ``xyz, features_rest, scaling,
    rotation`` to contiguous float32 ROCm tensors; an output may be its input (the in-place form)."""
    if n == 0:
        return
    dims = _lib.TransformDims(n=n, sh_coeffs=K, num_transforms=records.shape[0], reserved0=0, reserved1=0)
    tin = _lib.TransformIn(**{k: ptr(inputs.get(k)) for k in _NAMES})
    tout = _lib.TransformOut(**{k: ptr(outputs.get(k)) for k in _NAMES})
    dev = records.device
    with torch.cuda.device(dev):
        stream = _args.stream(dev)
        _lib.call("lsr_scene_transform", C.byref(dims), ptr(records), ptr(idx), C.byref(tin), C.byref(tout), stream)


def _check_scene(xyz: Tensor, features_rest: Tensor, scaling: Tensor, rotation: Tensor):
    given = (xyz, features_rest, scaling, rotation)
    for name, t in zip(_NAMES, given):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError(f"transform_scene needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    n = xyz.shape[0]
    if features_rest.dim() != 3 or features_rest.shape[0] != n or features_rest.shape[2] != 3:
        raise _lib.LsrError(f"features_rest must be (n, K - 1, 3), got {tuple(features_rest.shape)}")
    K = features_rest.shape[1] + 1
    if K not in (1, 4, 9, 16, 25):
        raise _lib.LsrError(f"{K} SH coefficients per channel: expected 1, 4, 9, 16 or 25")
    if tuple(xyz.shape) != (n, 3) or tuple(scaling.shape) != (n, 3) or tuple(rotation.shape) != (n, 4):
        raise _lib.LsrError("xyz must be (n, 3), scaling (n, 3) and rotation (n, 4)")
    if len({t.device for t in given}) != 1:
        raise _lib.LsrError("the scene's tensors must be on one device")
    return n, K


class _TransformScene(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, features_rest, scaling, rotation, matrices, idx):
        ctx.set_materialize_grads(False)
        n, K = xyz.shape[0], features_rest.shape[1] + 1
        records = transform_records(matrices, isqrt(K) - 1, check=False)
        ins = dict(xyz=xyz.detach().contiguous(), features_rest=features_rest.detach().contiguous(),
                   scaling=scaling.detach().contiguous(), rotation=_args.quad(rotation.detach().contiguous()))
        outs = {k: torch.empty_like(t) for k, t in ins.items()}
        apply_records(records, idx, ins, outs, n, K)
        # the backward's constants are fixed here, from the matrices the forward used (one more small launch, none later)
        adjoint = transform_records(matrices, isqrt(K) - 1, adjoint=True, check=False) if any(ctx.needs_input_grad[:4]) else None
        ctx.save_for_backward(adjoint, idx)
        ctx.dims = (n, K)
        return tuple(outs[k] for k in _NAMES)

    @staticmethod
    def backward(ctx, *grads):
        n, K = ctx.dims
        ins, outs = {}, {}
        for k, need, g in zip(_NAMES, ctx.needs_input_grad, grads):
            if need and g is not None:
                g = g.detach().contiguous()
                ins[k] = _args.quad(g) if k == "rotation" else g
                outs[k] = torch.empty_like(g)
        if outs:
            records, idx = ctx.saved_tensors
            apply_records(records, idx, ins, outs, n, K)
        return tuple(outs.get(k) for k in _NAMES) + (None, None)


def transform_scene(xyz: Tensor, features_rest: Tensor, scaling: Tensor, rotation: Tensor, transforms: Tensor,
                    idx: Optional[Tensor] = None, check: bool = True):
    """The raw parameters of a scene moved by similarities: ``(xyz', features_rest', scaling', rotation')``, differentiable
    in the four tensors (``features_dc`` and ``opacity`` do not change and are not taken).

    ``transforms`` is ``(4, 4)`` or ``(T, 4, 4)`` on the scene's device; ``idx`` (integer ``(n,)``, optional) names the
    transform of each Gaussian, ``None`` gives every Gaussian transform 0.  A Gaussian whose ``idx`` lies outside
    ``[0, T)`` passes through bit for bit, and so does its gradient.  ``check`` as in :func:`transform_records` (one host
    read; ``check=False`` for a training loop that poses parts every step).  One HIP launch over the parameters forward
    and one backward (the same kernel on the adjoint records, which the forward prepares) plus the small records launches.
    The transforms receive no gradient, also when they require one: a 4x4 matrix is not a chart of the similarity group.
    To fit poses use :func:`latentsplat_amd.pose.pose_scene` (quaternion, translation, log-scale per transform; the same
    forward bits).  float32 ROCm tensors only."""
    n, K = _check_scene(xyz, features_rest, scaling, rotation)
    M = _matrices(transforms, check)
    if M.device != xyz.device:
        raise _lib.LsrError(f"the transforms must be on the scene's device {xyz.device} (no CPU fallback)")
    return _TransformScene.apply(xyz, features_rest, scaling, rotation, M.to(torch.float32).contiguous(),
                                 _index(idx, n, xyz.device))


def transform_scene_(xyz: Tensor, features_rest: Tensor, scaling: Tensor, rotation: Tensor, transforms: Tensor,
                     idx: Optional[Tensor] = None, check: bool = True) -> None:
    """:func:`transform_scene` in place, without autograd: the four contiguous tensors are overwritten by one launch (a
    Gaussian's row is read whole before any of it is written).  The same bits as the out-of-place form."""
    n, K = _check_scene(xyz, features_rest, scaling, rotation)
    if not all(t.is_contiguous() for t in (xyz, features_rest, scaling, rotation)) or rotation.data_ptr() % 16:
        raise _lib.LsrError("transform_scene_ needs contiguous tensors (rotation 16-byte aligned)")
    M = _matrices(transforms, check)
    if M.device != xyz.device:
        raise _lib.LsrError(f"the transforms must be on the scene's device {xyz.device} (no CPU fallback)")
    records = transform_records(M, isqrt(K) - 1, check=False)
    t = dict(xyz=xyz.detach(), features_rest=features_rest.detach(), scaling=scaling.detach(), rotation=rotation.detach())
    apply_records(records, _index(idx, n, xyz.device), t, t, n, K)


def transform_cameras(extrinsics: Tensor, near: Tensor, far: Tensor, M: Tensor):
    """Cameras that see the moved scene as the given ones saw the scene: ``(extrinsics', near', far')`` for camera-to-world
    ``extrinsics (V, 4, 4)`` and one similarity ``M (4, 4)``.  The rotation becomes ``R R_c``, the position
    ``s R t_c + t``, ``near' = s near`` and ``far' = s far``.  With the default ``scale_invariant=True`` of
    ``build_view_table`` (the near cull lives in the ``1 / near``-scaled space) the moved scene under the moved cameras
    renders the same image.  Plain torch, in the dtype and on the device of ``extrinsics``."""
    M = M.detach().to(device=extrinsics.device, dtype=torch.float64)
    s, R, t = _split(M)
    E = extrinsics.to(torch.float64)
    out = E.clone()
    out[..., :3, :3] = R @ E[..., :3, :3]
    out[..., :3, 3] = (s * (R @ E[..., :3, 3:4]))[..., 0] + t
    sf = float(s)
    return out.to(extrinsics.dtype), near * sf, far * sf
