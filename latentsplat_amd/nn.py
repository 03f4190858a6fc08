"""The exact nearest neighbour of one cloud's points in ANOTHER cloud, in HIP (csrc/nn.hip, C ABI include/lsr_nn.h): the hot
path of the mesh metrics (:mod:`latentsplat_amd.mesh_eval`).

:class:`NearestIndex` builds a persistent index over a reference cloud once (a Morton sort, boxes over chunks of the
sorted cloud and over 64 chunks: the index of :func:`latentsplat_amd.knn.knn3`, kept); :meth:`NearestIndex.query` answers
any number of query sets against it.  :func:`nearest` is the one-shot form.  For every query: the smallest squared
distance to a reference point, in float32 from the caller's coordinates as ``dx dx + dy dy + dz dz`` (each operation
rounded once), and the lowest index among the reference points that attain it.  The search is exact.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr


def _cloud(name: str, points: Tensor) -> Tensor:
    if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.float32:
        raise _lib.LsrError(f"the nearest-neighbour query needs float32 ROCm tensors (no CPU fallback): {name} is not one")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.LsrError(f"{name} must be (n, 3), got {tuple(points.shape)}")
    if points.shape[0] > _lib.KNN_MAX_POINTS:
        raise _lib.LsrError(f"{name}: {points.shape[0]} points, at most {_lib.KNN_MAX_POINTS}")
    return points.detach().contiguous()


class NearestIndex:
    """A nearest-neighbour index over ``reference (n, 3)``, ``n >= 1``.  It holds its own sorted copy of the points: the
    caller's tensor may be freed or changed afterwards.  Built asynchronously on the current stream; a query on another
    stream has to be ordered after it, as with any tensor."""

    def __init__(self, reference: Tensor):
        r = _cloud("reference", reference)
        if r.shape[0] == 0:
            raise _lib.LsrError("the reference cloud is empty: there is no nearest neighbour")
        self.num_points = int(r.shape[0])
        self.device = r.device
        lib = _lib.load()
        self._mem = _args.workspace(lib.lsr_nn_index_bytes(self.num_points), self.device)
        ws = _args.workspace(lib.lsr_nn_build_workspace_bytes(self.num_points), self.device)
        with torch.cuda.device(self.device):
            _lib.call("lsr_nn_build", self.num_points, ptr(r), ptr(self._mem), ptr(ws), _args.stream(self.device))

    def _run(self, queries: Tensor, want_dist2: bool, want_index: bool):
        q = _cloud("queries", queries)
        if q.device != self.device:
            raise _lib.LsrError(f"queries must be on {self.device}, the reference's device")
        m = q.shape[0]
        dist2 = torch.empty((m,), dtype=torch.float32, device=self.device) if want_dist2 else None
        index = torch.empty((m,), dtype=torch.int32, device=self.device) if want_index else None
        if m == 0:
            return dist2, index
        ws = _args.workspace(_lib.load().lsr_nn_query_workspace_bytes(m), self.device)
        with torch.cuda.device(self.device):
            _lib.call("lsr_nn_query", self.num_points, ptr(self._mem), m, ptr(q), ptr(dist2), ptr(index), ptr(ws),
                      _args.stream(self.device))
        return dist2, index

    def query(self, queries: Tensor) -> Tuple[Tensor, Tensor]:
        """``(dist2 (m,) float32, index (m,) int32)`` for ``queries (m, 3)``: the squared distance to the nearest reference
        point and the lowest index that attains it; asynchronous on the current stream.  A non-contiguous tensor is made
        contiguous; ``(0, 3)`` queries give empty outputs.  The index is not consumed."""
        return self._run(queries, True, True)


def nearest(queries: Tensor, reference: Tensor) -> Tuple[Tensor, Tensor]:
    """``NearestIndex(reference).query(queries)``."""
    return NearestIndex(reference).query(queries)
