"""The 3DGS photometric loss, ``(1 - lambda) * L1 + lambda * (1 - SSIM)``, as HIP kernels (csrc/photometric.hip, C ABI
include/lsr_loss.h).

:func:`photometric_loss` is a ``torch.autograd.Function`` over ``lsr_photometric_forward`` / ``lsr_photometric_backward``:
one forward call that also saves the three derivative maps, one backward call; differentiable in the rendered image only.
:func:`ssim` and :func:`l1` return values only.  :func:`compute_ssim` is the reference's evaluation metric
(``skimage.metrics.structural_similarity`` with an 11-pixel Gaussian window, ``data_range=1``) as a mode of the same
kernel: sample covariance and the mean over the pixels at least 5 from every border.

SSIM here is the published trainer's: the normalised 11-tap Gaussian window of sigma 1.5, zero padding, ``C1 = 0.01^2``,
``C2 = 0.03^2``, values taken as they are (no clamping).  The kernels take float32 ROCm tensors only; there is no CPU
fallback."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr


def _prepare(what: str, image: Tensor, target: Tensor):
    """Checked, detached, contiguous ``(V, C, H, W)`` views of both images."""
    for name, t in (("image", image), ("target", target)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.LsrError(f"{what} needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    if image.shape != target.shape or image.dim() not in (3, 4) or image.numel() == 0:
        raise _lib.LsrError(f"{what} takes two images of one shape, (V, C, H, W) or (C, H, W), got {tuple(image.shape)} and "
                            f"{tuple(target.shape)}")
    if image.device != target.device:
        raise _lib.LsrError("image and target must be on one device")
    x, y = image.detach().contiguous(), target.detach().contiguous()
    if x.dim() == 3:
        x, y = x[None], y[None]
    return x, y


def _dims(shape, lambda_dssim: float = 0.0, cov_norm: float = 1.0, crop: int = 0) -> _lib.PhotometricDims:
    V, Ch, H, W = shape
    return _lib.PhotometricDims(num_images=V, channels=Ch, height=H, width=W, lambda_dssim=float(lambda_dssim),
                                cov_norm=float(cov_norm), crop=int(crop), reserved0=0)


def photometric_forward(image: Tensor, target: Tensor, lambda_dssim: float = 0.2, *, cov_norm: float = 1.0, crop: int = 0,
                        want=("loss", "l1", "ssim")) -> dict:
    """``lsr_photometric_forward`` as it is (no autograd): the outputs named in ``want`` out of ``loss (1,)``, ``l1 (V,)``,
    ``ssim (V,)``, ``ssim_map (V, C, H, W)`` and ``saved (3, V, C, H, W)`` as a dict."""
    x, y = _prepare("photometric_forward", image, target)
    V = x.shape[0]
    shapes = dict(loss=(1,), l1=(V,), ssim=(V,), ssim_map=tuple(x.shape), saved=(3,) + tuple(x.shape))
    unknown = [k for k in want if k not in shapes]
    if unknown:
        raise _lib.LsrError(f"unknown outputs {unknown}; expected some of {list(shapes)}")
    lib = _lib.load()
    dims = _dims(x.shape, lambda_dssim, cov_norm, crop)
    out = _args.results([k for k in shapes if k in want], shapes, x.device)
    workspace = _args.loss_workspace(lib.lsr_photometric_workspace_bytes(C.byref(dims)), x.device)
    with torch.cuda.device(x.device):
        _lib.call("lsr_photometric_forward", C.byref(dims), ptr(x), ptr(y), ptr(workspace),
                  *(ptr(out.get(k)) for k in shapes), _args.stream(x))
    return out


def photometric_backward(image: Tensor, target: Tensor, saved: Tensor, grad_loss: Tensor, lambda_dssim: float = 0.2) -> Tensor:
    """``lsr_photometric_backward`` as it is: ``grad_loss * d loss / d image`` as ``(V, C, H, W)``, from the ``saved`` maps
    of :func:`photometric_forward` for the same images.  ``grad_loss`` is a one-element float32 tensor on the device."""
    x, y = _prepare("photometric_backward", image, target)
    for name, t, n in (("saved", saved, 3 * x.numel()), ("grad_loss", grad_loss, 1)):
        if not torch.is_tensor(t) or t.device != x.device or t.dtype != torch.float32 or t.numel() != n:
            raise _lib.LsrError(f"{name} must be a float32 tensor of {n} elements on the images' device")
    saved, grad_loss = saved.detach().contiguous(), grad_loss.detach().contiguous()
    grad = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call("lsr_photometric_backward", C.byref(_dims(x.shape, lambda_dssim)), ptr(x), ptr(y), ptr(saved),
                  ptr(grad_loss), ptr(grad), _args.stream(x))
    return grad


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, lambda_dssim):
        out = photometric_forward(image, target, lambda_dssim, want=("loss", "saved"))
        ctx.save_for_backward(image, target, out["saved"])
        ctx.lambda_dssim = lambda_dssim
        return out["loss"].reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        image, target, saved = ctx.saved_tensors
        # the upstream gradient stays on the device: the kernel reads it there
        grad = photometric_backward(image, target, saved, grad_loss, ctx.lambda_dssim)
        return grad.reshape(image.shape), None, None


def photometric_loss(image: Tensor, target: Tensor, lambda_dssim: float = 0.2) -> Tensor:
    """``(1 - lambda_dssim) * mean |image - target| + lambda_dssim * (1 - SSIM(image, target))`` as a scalar, differentiable
    in ``image``: the objective of the published 3DGS trainer at its ``lambda_dssim = 0.2`` (``1.0``: ``1 - SSIM``, ``0.0``:
    the L1 mean).  ``image`` and ``target`` are float32 ROCm tensors of one shape, ``(V, C, H, W)`` or ``(C, H, W)``; SSIM is
    the mean over every value of every image.  One HIP forward call, one backward call."""
    if torch.is_tensor(target) and target.requires_grad:
        raise _lib.LsrError("photometric_loss is differentiable in image only: target requires grad (detach it)")
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise _lib.LsrError(f"lambda_dssim must be in [0, 1], got {lambda_dssim}")
    _prepare("photometric_loss", image, target)
    return _PhotometricLoss.apply(image.contiguous(), target.contiguous(), float(lambda_dssim))


@torch.no_grad()
def ssim(image: Tensor, target: Tensor, *, per_image: bool = False, return_map: bool = False, cov_norm: float = 1.0,
         crop: int = 0):
    """SSIM of ``image`` against ``target`` (values only): the mean over all images, or ``(V,)`` with ``per_image``; with
    ``return_map`` also the map ``S`` in the images' shape.  ``cov_norm`` scales the (co)variances (1: the trainer's;
    121 / 120: sample covariance); ``crop=5`` takes the mean over the pixels at least 5 from every border."""
    out = photometric_forward(image, target, 1.0, cov_norm=cov_norm, crop=crop, want=("ssim", "ssim_map") if return_map else ("ssim",))
    value = out["ssim"] if per_image else out["ssim"].mean()
    return (value, out["ssim_map"].reshape(image.shape)) if return_map else value


@torch.no_grad()
def l1(image: Tensor, target: Tensor, per_image: bool = False) -> Tensor:
    """Mean of ``|image - target|`` (values only): over all images, or ``(V,)`` with ``per_image``."""
    out = photometric_forward(image, target, 0.0, want=("l1",))["l1"]
    return out if per_image else out.mean()


def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """The reference's ``src/evaluation/metrics.py`` ``compute_ssim``: ``(batch, channel, height, width)`` images in [0, 1]
    to ``(batch,)`` SSIM values, on the device.  It restates ``skimage.metrics.structural_similarity(win_size=11,
    gaussian_weights=True, channel_axis=0, data_range=1)``: the same window, sample covariance, the mean over the pixels at
    least 5 from every border (whose windows never see the padding).  Needs height and width of at least 11."""
    return ssim(predicted, ground_truth, per_image=True, cov_norm=121.0 / 120.0, crop=5)
