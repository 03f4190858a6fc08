"""What every wrapper hands the library and checks before it does: pointers, the stream, float32 / int32 ROCm tensors.

``who`` is the calling module's phrase ("density control", "adam_step", ...): the sentences are the product's, and the
tests match on them."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from ._lib import LsrError


def ptr(t: Optional[Tensor]) -> Optional[C.c_void_p]:
    """What ctypes passes as NULL for ``None`` and for a tensor without elements, the address otherwise.  torch reports
    ``data_ptr() == 0`` for an empty tensor itself, on the host and on a ROCm device (the tests hold it to that), and
    ``None`` is ctypes' own NULL, as an argument and in a structure field: the latency path pays for no second look."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(where) -> C.c_void_p:
    """The current stream of a device, or of a tensor's device."""
    return C.c_void_p(torch.cuda.current_stream(where.device if torch.is_tensor(where) else where).cuda_stream)


def _typed(dtype, kind: str, who: str, name: str, t, shape, device, contiguous: bool) -> Tensor:
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype:
        raise LsrError(f"{who} needs {kind} ROCm tensors (no CPU fallback): {name} is not one")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise LsrError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if device is not None and t.device != device:
        raise LsrError(f"{name} must be on {device}")
    if contiguous and not t.is_contiguous():
        raise LsrError(f"{name} is updated in place and must be contiguous (it is not copied)")
    return t


def f32(who: str, name: str, t, shape: Optional[tuple] = None, device=None, contiguous: bool = False) -> Tensor:
    return _typed(torch.float32, "float32", who, name, t, shape, device, contiguous)


def i32(who: str, name: str, t, shape: Optional[tuple] = None, device=None, contiguous: bool = False) -> Tensor:
    return _typed(torch.int32, "int32", who, name, t, shape, device, contiguous)


def quad(t: Tensor) -> Tensor:
    """(the kernels move a quaternion as one 16-byte quad)"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def workspace(nbytes: int, dev) -> Tensor:
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def loss_workspace(nbytes: int, dev) -> Tensor:
    """The workspace of an image loss: never empty (``lsr_*_workspace_bytes`` is 0 for refused dims, and the call that
    names the refusal wants a pointer), and 16 bytes are what torch aligns to 16."""
    return workspace(max(nbytes, 16), dev)


def upstream(name: str, t, device, what: str = "1 element on the images' device") -> Tensor:
    """The upstream gradient of a scalar loss, which the kernel reads on the device: a one-element float32 tensor there,
    detached and contiguous."""
    if not torch.is_tensor(t) or t.device != device or t.dtype != torch.float32 or t.numel() != 1:
        raise LsrError(f"{name} must be a float32 tensor of {what}")
    return t.detach().contiguous()


def results(want, shapes: dict, dev, out: Optional[dict] = None) -> dict:
    """The tensors a forward writes, one per name in ``want``: the caller's from ``out`` where given, else a fresh one of
    ``shapes[k]``, float32 (``valid`` is a uint8 mask)."""
    return {k: out[k] if out is not None and k in out else
            torch.empty(shapes[k], dtype=torch.uint8 if k == "valid" else torch.float32, device=dev) for k in want}
