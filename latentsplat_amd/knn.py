"""Exact three-nearest-neighbour distances over a point cloud, in HIP (csrc/knn.hip, C ABI include/lsr_knn.h): what the
published 3DGS trainer's ``create_from_pcd`` takes every Gaussian's initial scale from.

:func:`knn3` returns, for every point, the squared distances to its three nearest neighbours (ascending) and their
indices; :func:`mean_knn_dist2` the mean of the three.  Neighbours are every other point *by index*: coincident points
count, at distance 0.  Where distances tie the lower index comes first.  The search is exact (a Morton sort, boxes over
chunks of the sorted cloud, and a workgroup-wide bound that skips only what cannot hold a closer point).

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr


def _points(points: Tensor) -> Tensor:
    if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.float32:
        raise _lib.LsrError("the nearest-neighbour search needs a float32 ROCm tensor (no CPU fallback)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.LsrError(f"points must be (n, 3), got {tuple(points.shape)}")
    n = points.shape[0]
    if 1 <= n <= 3 or n > _lib.KNN_MAX_POINTS:
        raise _lib.LsrError(f"{n} points: three neighbours need at least 4 points (and at most {_lib.KNN_MAX_POINTS})")
    return points.detach().contiguous()


def _run(points: Tensor, want_mean: bool, want_dist2: bool, want_index: bool):
    p = _points(points)
    n, dev = p.shape[0], p.device
    mean = torch.empty((n,), dtype=torch.float32, device=dev) if want_mean else None
    dist2 = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_dist2 else None
    index = torch.empty((n, 3), dtype=torch.int32, device=dev) if want_index else None
    if n == 0:
        return mean, dist2, index
    lib = _lib.load()
    ws = _args.workspace(lib.lsr_knn3_workspace_bytes(n), dev)
    with torch.cuda.device(dev):
        _lib.call("lsr_knn3", n, ptr(p), ptr(mean), ptr(dist2), ptr(index), ptr(ws), _args.stream(dev))
    return mean, dist2, index


def knn3(points: Tensor) -> Tuple[Tensor, Tensor]:
    """``(dist2 (n, 3) float32 ascending, index (n, 3) int32)`` of the three nearest neighbours of every point of
    ``points (n, 3)``; asynchronous on the current stream.  A non-contiguous tensor is made contiguous."""
    _, dist2, index = _run(points, False, True, True)
    return dist2, index


def mean_knn_dist2(points: Tensor) -> Tensor:
    """``(n,)``: the mean squared distance of every point to its three nearest neighbours (the published
    ``distCUDA2``)."""
    return _run(points, True, False, False)[0]
