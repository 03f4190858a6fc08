"""Supervision of a trainable 3DGS scene's geometry by depth: the targets a photographed capture offers, and the loss in HIP
(csrc/depth_loss.hip; C ABI include/lsr_depth_loss.h).

Both published trainers supervise inverse depth with an L1:

* gsplat's ``depth_loss`` compares the rendered inverse depth with ``1 / z`` of the capture's own sparse points at the pixels
  they project to: :func:`sparse_inverse_depth` builds that map from the 2D observations of a
  :class:`latentsplat_amd.capture.ColmapModel` read with ``observations=True``;
* the 3DGS trainer compares it with a monocular inverse-depth prior per photograph, brought to the scene's scale by a
  per-image ``scale`` / ``offset`` computed from the same sparse points: :func:`load_depth_prior`,
  :func:`prepare_depth_priors` (the prior resampled onto the target camera through the unchanged
  :func:`latentsplat_amd.images.prepare_images`), :func:`align_depth_prior` and :func:`reliable_alignments`.

The targets are host numpy in float64, built once.  The per-step path is :func:`inverse_depth_loss`: one streaming HIP pass
over ``depth``, ``alpha`` and the target each way, float32 ROCm tensors only, no CPU fallback.

An inverse depth is positive, so in every target map ``> 0`` is the mask and no second map is stored."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

_WHO = "the inverse-depth loss"
_ALIGN = {"given": _lib.DEPTH_ALIGN_GIVEN, "fit": _lib.DEPTH_ALIGN_FIT}
_NORMALIZE = {"pixels": _lib.DEPTH_NORM_PIXELS, "weights": _lib.DEPTH_NORM_WEIGHTS}
PRIOR_EXTENSIONS = (".npy", ".pgm", ".png", ".tif", ".tiff")


# ---- targets: host, float64, one-time ----

def _rotation(qvec: np.ndarray) -> np.ndarray:
    w, x, y, z = np.asarray(qvec, np.float64) / np.linalg.norm(np.asarray(qvec, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def sparse_inverse_depth(model, image_row: int, H: int, W: int, fx: float, fy: float, near: float) -> np.ndarray:
    """``(H, W)`` float32: the inverse depths of the sparse points that image ``image_row`` (a row of ``model``, file order)
    observes, at the pixels they project to through the TARGET pinhole (centred, focal lengths ``fx, fy`` in output pixels),
    as both published tools project them; COLMAP's measured ``xy`` is not used.  In float64: ``p = R x + t`` with the
    normalised ``qvec`` (each component summed left to right); dropped when ``p.z <= near``; pixel ``j = floor(fx * p.x / p.z + W / 2)``,
    ``i = floor(fy * p.y / p.z + H / 2)``, dropped outside the image; the value is ``1 / p.z`` in the capture's units; where
    several land in one pixel the largest (the nearest) wins; pixels without a point hold 0."""
    if model.obs_offsets is None:
        raise _lib.LsrError("the model was read without its observations: read_colmap_model(path, observations=True)")
    lo, hi = int(model.obs_offsets[image_row]), int(model.obs_offsets[image_row + 1])
    out = np.zeros((int(H), int(W)), np.float64)
    if hi > lo:
        order = np.argsort(model.point_ids, kind="stable")
        rows = order[np.searchsorted(model.point_ids[order], model.obs_point_ids[lo:hi])]
        R, t, x = _rotation(model.qvec[image_row]), np.asarray(model.tvec[image_row], np.float64), model.xyz[rows]
        # (spelled out, left to right: one rounding per operation, whatever the BLAS would do with a product)
        p = np.stack([R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1] + R[k, 2] * x[:, 2] + t[k] for k in range(3)], axis=1)
        p = p[p[:, 2] > float(near)]
        j = np.floor(float(fx) * p[:, 0] / p[:, 2] + W / 2)
        i = np.floor(float(fy) * p[:, 1] / p[:, 2] + H / 2)
        inside = (j >= 0) & (j < W) & (i >= 0) & (i < H)
        np.maximum.at(out, (i[inside].astype(np.int64), j[inside].astype(np.int64)), 1.0 / p[inside, 2])
    return out.astype(np.float32)


def decode_pgm16(data: bytes, name: str = "<bytes>") -> np.ndarray:
    """A binary PGM (``P5``, maxval 65535, big-endian) as ``(H, W)`` uint16, with numpy alone.  ``#`` comments in the header
    are skipped; anything else, a truncated file included, is refused with ``name``."""
    pos, fields = 0, []
    while len(fields) < 4:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if pos < len(data) and data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] != b"\n":
                pos += 1
            continue
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace():
            pos += 1
        if start == pos:
            raise _lib.LsrError(f"{name}: the PGM header ends early")
        fields.append(data[start:pos])
    if fields[0] != b"P5" or not all(f.isdigit() for f in fields[1:]):
        raise _lib.LsrError(f"{name}: not a binary PGM (P5)")
    w, h, maxval = (int(f) for f in fields[1:])
    if maxval != 65535 or not (1 <= w <= _lib.IMAGE_MAX_EXTENT and 1 <= h <= _lib.IMAGE_MAX_EXTENT):
        raise _lib.LsrError(f"{name}: a PGM of maxval 65535 and extents in 1..{_lib.IMAGE_MAX_EXTENT} is needed, got {w} x {h}, maxval {maxval}")
    pos += 1                                     # the single whitespace byte after maxval
    if len(data) - pos != 2 * w * h:
        raise _lib.LsrError(f"{name}: {max(len(data) - pos, 0)} bytes of pixels, {w} x {h} x 2 needs {2 * w * h}")
    return np.frombuffer(data, ">u2", w * h, pos).reshape(h, w).astype(np.uint16)


def encode_pgm16(a: np.ndarray) -> bytes:
    """The inverse of :func:`decode_pgm16` for an ``(H, W)`` uint16 array."""
    a = np.asarray(a)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise _lib.LsrError(f"a PGM of maxval 65535 holds an (H, W) uint16 array, got {a.dtype} {a.shape}")
    return b"P5\n%d %d\n65535\n" % (a.shape[1], a.shape[0]) + a.astype(">u2").tobytes()


def load_depth_prior(path) -> np.ndarray:
    """``(Hs, Ws)`` uint16 from ``.npy`` (a uint16 array) or a binary ``.pgm`` (``P5``, maxval 65535), with numpy alone; any
    other format through PIL where it imports, and otherwise an error that names the file.  The value of a sample is
    ``u16 / 65536``: the published trainer's reading of its 16-bit files."""
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path, allow_pickle=False)
    elif ext == ".pgm":
        with open(path, "rb") as f:
            a = decode_pgm16(f.read(), path)
    else:
        try:
            from PIL import Image
        except ImportError as e:
            raise _lib.LsrError(f"{path}: only .npy (uint16) and binary .pgm are decoded without PIL, and PIL does not import "
                                f"({e}); convert the prior or install Pillow") from e
        with Image.open(path) as im:
            a = np.asarray(im)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise _lib.LsrError(f"{path}: a depth prior must be uint16 of shape (H, W), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def prepare_depth_priors(prior_u16, camera, H: int, W: int, fx: float, fy: float, device="cuda:0") -> Tensor:
    """``(B, H, W)`` float32 on ``device``: the priors ``prior_u16 (B, Hs, Ws)`` (uint16, numpy) of ONE source ``camera``
    (:class:`latentsplat_amd.images.SourceCamera`, in the priors' own pixels) resampled onto the centred target camera with
    the focal lengths ``fx, fy``, through the unchanged :func:`latentsplat_amd.images.prepare_images`: the high and the low
    bytes go in as two channels of a 3-channel uint8 image and come back as ``c_hi, c_lo``; the result is
    ``(65280 c_hi + 255 c_lo) / 65536``.  The operator is linear per channel, so this is the resampling of the 16-bit
    value over 65536.  0 where the prior covers nothing."""
    from .images import prepare_images
    a = np.asarray(prior_u16)
    if a.dtype != np.uint16 or a.ndim != 3:
        raise _lib.LsrError(f"prior_u16 must be uint16 of shape (B, Hs, Ws), got {a.dtype} {a.shape}")
    planes = np.stack([(a >> 8).astype(np.uint8), (a & 255).astype(np.uint8), np.zeros(a.shape, np.uint8)], axis=-1)
    image, _ = prepare_images(torch.from_numpy(planes).to(torch.device(device)), camera, H, W, fx, fy)
    return (65280.0 * image[:, 0] + 255.0 * image[:, 1]) / 65536.0


def align_depth_prior(sparse, prior) -> Tuple[float, float]:
    """``(scale, offset)`` that bring the inverse-depth ``prior (H, W)`` to the scale of the ``sparse (H, W)`` map
    (:func:`sparse_inverse_depth`): the published ``make_depth_scale`` rule.  Over the pixels where ``sparse > 0`` and
    ``prior > 0``, when there are more than 10 of them and ``max - min`` of the sparse values exceeds 1e-3: with
    ``t = median`` and ``s = mean |. - t|`` of each side, ``scale = s_sparse / s_prior`` and
    ``offset = t_sparse - t_prior * scale``.  Otherwise ``(0, 0)``.  float64 on the host."""
    a = np.asarray(sparse.detach().cpu() if torch.is_tensor(sparse) else sparse, np.float64)
    b = np.asarray(prior.detach().cpu() if torch.is_tensor(prior) else prior, np.float64)
    both = (a > 0) & (b > 0)
    a, b = a[both], b[both]
    if a.size <= 10 or not a.max() - a.min() > 1e-3:
        return 0.0, 0.0
    ta, tb = float(np.median(a)), float(np.median(b))
    sa, sb = float(np.mean(np.abs(a - ta))), float(np.mean(np.abs(b - tb)))
    if not sb > 0.0:
        return 0.0, 0.0
    scale = sa / sb
    return scale, ta - tb * scale


def reliable_alignments(affine) -> np.ndarray:
    """``(N, 2)`` float64: the per-image ``(scale, offset)`` rows of :func:`align_depth_prior` with the published "not
    reliable" rule applied over all images: a row whose scale is below 0.2 x or above 5 x the median of the non-zero scales
    becomes ``(0, 0)``."""
    out = np.array(affine, np.float64).reshape(-1, 2)
    used = out[:, 0] != 0
    if used.any():
        med = float(np.median(out[used, 0]))
        out[used & ((out[:, 0] < 0.2 * med) | (out[:, 0] > 5.0 * med))] = 0.0
    return out


# ---- the loss ----

def _inputs(depth, alpha, views, target, weight, align, normalize, alpha_min):
    depth = _args.f32(_WHO, "depth", depth)
    if depth.dim() != 3:
        raise _lib.LsrError(f"depth must be (V, H, W), got {tuple(depth.shape)}")
    V, H, W = depth.shape
    dev = depth.device
    alpha = _args.f32(_WHO, "alpha", alpha, (V, H, W), dev)
    target = _args.f32(_WHO, "target", target, (V, H, W), dev)
    if weight is not None:
        weight = _args.f32(_WHO, "weight", weight, (V, H, W), dev).detach().contiguous()
    views = _args.f32(_WHO, "views", views, (V, _lib.VIEW_FLOATS), dev)
    if align not in _ALIGN or normalize not in _NORMALIZE:
        raise _lib.LsrError(f"align is one of {sorted(_ALIGN)} and normalize one of {sorted(_NORMALIZE)}, got {align!r} and {normalize!r}")
    dims = _lib.DepthLossDims(num_views=V, height=H, width=W, align=_ALIGN[align], normalize=_NORMALIZE[normalize],
                              alpha_min=float(alpha_min), reserved0=0, reserved1=0)
    return depth.detach().contiguous(), alpha.detach().contiguous(), views.detach().contiguous(), target.detach().contiguous(), weight, dims


def workspace_bytes(V: int, H: int, W: int, align: str = "given") -> int:
    """``lsr_depth_loss_workspace_bytes`` (0 for shapes the loss refuses)."""
    dims = _lib.DepthLossDims(num_views=V, height=H, width=W, align=_ALIGN[align], normalize=0, alpha_min=0.0, reserved0=0, reserved1=0)
    return _lib.load().lsr_depth_loss_workspace_bytes(C.byref(dims))


def inverse_depth_forward(depth: Tensor, alpha: Tensor, views: Tensor, target: Tensor, weight: Optional[Tensor] = None,
                          affine: Optional[Tensor] = None, *, align: str = "given", normalize: str = "pixels",
                          alpha_min: float = 0.01, want=("loss",), out: Optional[dict] = None) -> dict:
    """``lsr_depth_loss_forward`` as it is: the outputs named in ``want`` (``loss (1,)``, ``per_view (V,)``,
    ``inverse_depth (V, H, W)``, ``affine (V, 2)``), written into the tensors of ``out`` where given, and ``workspace``: the
    uint8 tensor (``out["workspace"]`` when given) that holds the per-view table :func:`inverse_depth_backward` reads."""
    depth, alpha, views, target, weight, dims = _inputs(depth, alpha, views, target, weight, align, normalize, alpha_min)
    V, H, W = depth.shape
    dev = depth.device
    if affine is not None:
        affine = _args.f32(_WHO, "affine", affine, (V, 2), dev).detach().contiguous()
    shapes = {"loss": (1,), "per_view": (V,), "inverse_depth": (V, H, W), "affine": (V, 2)}
    res = _args.results(want, shapes, dev, out)
    for k in res:
        _args.f32(_WHO, k, res[k], shapes[k], dev, contiguous=True)
    ws = (out or {}).get("workspace")
    if ws is None:
        ws = _args.loss_workspace(_lib.load().lsr_depth_loss_workspace_bytes(C.byref(dims)), dev)
    with torch.cuda.device(dev):
        _lib.call("lsr_depth_loss_forward", C.byref(dims), ptr(depth), ptr(alpha), ptr(views), ptr(target), ptr(weight), ptr(affine),
                  ptr(ws), *(ptr(res.get(k)) for k in shapes), _args.stream(dev))
    res["workspace"] = ws
    return res


def inverse_depth_backward(depth: Tensor, alpha: Tensor, views: Tensor, target: Tensor, weight: Optional[Tensor], workspace: Tensor,
                           grad_loss: Optional[Tensor] = None, grad_per_view: Optional[Tensor] = None, *, align: str = "given",
                           normalize: str = "pixels", alpha_min: float = 0.01, want=("depth", "alpha"),
                           out: Optional[dict] = None) -> dict:
    """``lsr_depth_loss_backward`` as it is: the gradients named in ``want`` (``depth``, ``alpha``), written in full (into
    the tensors of ``out`` where given).  ``workspace`` is the forward's, untouched since; ``grad_loss`` (1 element) and
    ``grad_per_view (V,)`` are float32 tensors on the device, at least one of them given: the upstream gradient of view
    ``v`` is ``grad_loss / V + grad_per_view[v]``."""
    depth, alpha, views, target, weight, dims = _inputs(depth, alpha, views, target, weight, align, normalize, alpha_min)
    dev = depth.device
    if grad_loss is None and grad_per_view is None:
        raise _lib.LsrError("grad_loss or grad_per_view is needed")
    if grad_loss is not None:
        grad_loss = _args.f32(_WHO, "grad_loss", grad_loss, (1,), dev).detach().contiguous()
    if grad_per_view is not None:
        grad_per_view = _args.f32(_WHO, "grad_per_view", grad_per_view, (depth.shape[0],), dev).detach().contiguous()
    if not torch.is_tensor(workspace) or workspace.device != dev or workspace.dtype != torch.uint8:
        raise _lib.LsrError("workspace must be the uint8 tensor inverse_depth_forward returned")
    like = {"depth": depth, "alpha": alpha}
    res = {k: (out[k] if out is not None and k in out else torch.empty_like(like[k])) for k in want}
    for k in res:
        _args.f32(_WHO, f"grad_{k}", res[k], tuple(depth.shape), dev, contiguous=True)
    with torch.cuda.device(dev):
        _lib.call("lsr_depth_loss_backward", C.byref(dims), ptr(depth), ptr(alpha), ptr(views), ptr(target), ptr(weight),
                  ptr(workspace), ptr(grad_loss), ptr(grad_per_view), *(ptr(res.get(k)) for k in like), _args.stream(dev))
    return res


class _InverseDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, views, target, weight, affine, align, normalize, alpha_min, outputs):
        want = ("loss",) if outputs is None else ("loss", "per_view", "inverse_depth", "affine")
        res = inverse_depth_forward(depth, alpha, views, target, weight, affine, align=align, normalize=normalize,
                                    alpha_min=alpha_min, want=want)
        ctx.save_for_backward(depth, alpha, views, target, weight, res["workspace"])
        ctx.modes = (align, normalize, alpha_min)
        if outputs is not None:
            outputs.update({k: res[k] for k in want[1:]})
        return res["loss"].reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        depth, alpha, views, target, weight, ws = ctx.saved_tensors
        align, normalize, alpha_min = ctx.modes
        names = ("depth", "alpha")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad) if need)
        # the upstream gradient stays on the device: the kernel reads it there
        g = inverse_depth_backward(depth, alpha, views, target, weight, ws, grad_loss.reshape(1).float(), align=align,
                                   normalize=normalize, alpha_min=alpha_min, want=want) if want else {}
        return tuple(g.get(k) for k in names) + (None,) * 8


def inverse_depth_loss(depth: Tensor, alpha: Tensor, views: Tensor, target: Tensor, weight: Optional[Tensor] = None,
                       affine: Optional[Tensor] = None, *, align: str = "given", normalize: str = "pixels",
                       alpha_min: float = 0.01, outputs: Optional[dict] = None) -> Tensor:
    """The inverse-depth loss, a scalar, differentiable in ``depth`` and ``alpha``.

    ``depth (V, H, W)`` is the rendered depth of depth mode NATIVE (sum of alpha T tz), ``alpha (V, H, W)`` the rendered
    mask (sum of alpha T), ``views (V, 44)`` the table they were rendered with, ``target (V, H, W)`` an inverse depth (or a
    prior to be aligned) and ``weight (V, H, W)`` optional.  Per view ``v`` and pixel ``p``::

        s      = views[v, 40]                                    (tz = s z, as in the normal regulariser)
        I(p)   = s alpha / depth   where alpha > alpha_min, depth > 0 and both are finite; 0 elsewhere, without a gradient
        w(p)   = weight(p) if given, else 1 where target > 0 and 0 elsewhere
        r(p)   = w(p) (I(p) - (a_v target(p) + b_v))
        per_view[v] = sum_p |r(p)| / N_v,   N_v = H W ("pixels") or sum_p w(p) ("weights"; 0 gives 0)
        loss   = mean_v per_view[v]

    An unrendered pixel is "infinitely far", as in both published losses: it is penalised and not excused, so transparency
    is never rewarded.  ``align="given"``: ``(a_v, b_v) = affine[v]`` (``None``: ``(1, 0)``); a row with ``a_v == 0`` means
    "no usable target for this view": ``per_view = 0`` and no gradient.  ``align="fit"``: the weighted least-squares
    ``(a_v, b_v)`` of ``a target + b`` against ``I`` over the view's pixels, solved in double; they are constants in the
    backward; when fewer than two pixels weigh in or the target is flat to float32 precision the row is ``(0, 0)``.
    ``sign(0) = 0`` in the backward.  ``alpha_min = 0.01`` is a default, not a measurement.

    ``outputs``: a dict that receives ``per_view (V,)``, ``inverse_depth (V, H, W)`` and ``affine (V, 2)`` (values only).

    The loss reads the scene scale from slot 40 of ``views`` and has no gradient for the table: a ``views`` that requires
    grad is refused, since a silent partial pose gradient is worse than a refusal (pass ``views.detach()``).

    Two HIP launches forward (four with ``"fit"``) and one backward; no atomics: the same bits every call, and a view's
    numbers do not depend on which other views share the call."""
    if torch.is_tensor(views) and views.requires_grad:
        raise _lib.LsrError("inverse_depth_loss: views requires grad, and this operator has no pose gradient (pass "
                            "views.detach(); the rasterizer hands the table its own)")
    return _InverseDepth.apply(depth, alpha, views, target, weight, affine, align, normalize, float(alpha_min), outputs)
