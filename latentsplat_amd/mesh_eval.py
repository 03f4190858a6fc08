"""What scores an extracted mesh against a ground-truth cloud: the step 2DGS, GOF, RaDe-GS and PGSR all end with.

:func:`cloud_metrics` gives accuracy, completeness and Chamfer as the DTU evaluation does, and precision, recall and
F-score at a threshold as Tanks and Temples does.  Its hot path is the nearest neighbour of every point of one cloud in
the other, which is HIP (:mod:`latentsplat_amd.nn`, csrc/nn.hip, exact); the reductions over the distances are plain
torch in float64 and the precision and recall counts are integers.  :func:`sample_mesh` draws the points to score from
a mesh, uniformly by area.

Dataset plumbing (DTU's observation masks, the alignment files of Tanks and Temples) is not here.  Values only: nothing
has a gradient.  float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _args, _lib
from .nn import NearestIndex

_WHO = "mesh evaluation"


def _means(dist2: Tensor, max_dist: Optional[float]):
    d2 = dist2.double()
    d = torch.sqrt(d2)
    if max_dist is not None:
        d, d2 = d.clamp(max=float(max_dist)), d2.clamp(max=float(max_dist) ** 2)
    return d, d.mean(), d2.mean()


def cloud_metrics(pred: Tensor, gt: Tensor, thresholds: Sequence[float] = (), max_dist: Optional[float] = None,
                  gt_index: Optional[NearestIndex] = None) -> dict:
    """Scores ``pred (np, 3)`` against ``gt (ng, 3)``, both non-empty.  With ``d = sqrt(float64(dist2))`` of the exact
    nearest neighbour in the other cloud:

    * ``accuracy`` = mean d(pred -> gt), ``completeness`` = mean d(gt -> pred), ``chamfer`` = their mean (DTU's
      "overall"); ``accuracy_sq`` / ``completeness_sq``: the means of ``dist2``;
    * per threshold tau, as lists in the order of ``thresholds``: ``precision`` = the share of pred with d < tau,
      ``recall`` = the share of gt with d < tau, ``fscore`` = 2 P R / (P + R), and 0 when P + R = 0; the integer counts
      behind them are ``precision_count`` and ``recall_count``, of ``num_pred`` and ``num_gt``.

    ``max_dist`` clips d (and ``dist2`` at its square) before the means only (DTU's 20 mm rule): precision and recall see
    the unclipped distances.  ``gt_index``: a :class:`NearestIndex` over ``gt`` built once by a caller that scores many
    meshes against the same ground truth.  One host read."""
    pred = _args.f32(_WHO, "pred", pred)
    gt = _args.f32(_WHO, "gt", gt, None, pred.device)
    for name, t in (("pred", pred), ("gt", gt)):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
            raise _lib.LsrError(f"{name} must be (n, 3) with n >= 1, got {tuple(t.shape)}")
    if gt_index is None:
        gt_index = NearestIndex(gt)
    elif gt_index.num_points != gt.shape[0] or gt_index.device != gt.device:
        raise _lib.LsrError("gt_index was not built over gt")
    taus = [float(t) for t in thresholds]
    to_gt = gt_index.query(pred)[0]
    to_pred = NearestIndex(pred).query(gt)[0]
    d_acc, acc, acc_sq = _means(to_gt, max_dist)
    d_comp, comp, comp_sq = _means(to_pred, max_dist)
    d_p, d_r = torch.sqrt(to_gt.double()), torch.sqrt(to_pred.double())
    counts = [c for tau in taus for c in ((d_p < tau).sum(), (d_r < tau).sum())]
    means = torch.stack([acc, comp, acc_sq, comp_sq]).tolist()
    counts = torch.stack(counts).tolist() if counts else []
    n_p, n_g = int(pred.shape[0]), int(gt.shape[0])
    out = dict(accuracy=means[0], completeness=means[1], chamfer=0.5 * (means[0] + means[1]), accuracy_sq=means[2],
               completeness_sq=means[3], num_pred=n_p, num_gt=n_g, max_dist=None if max_dist is None else float(max_dist),
               thresholds=taus, precision=[], recall=[], fscore=[], precision_count=[], recall_count=[])
    for k in range(len(taus)):
        cp, cr = int(counts[2 * k]), int(counts[2 * k + 1])
        p, r = cp / n_p, cr / n_g
        out["precision_count"].append(cp)
        out["recall_count"].append(cr)
        out["precision"].append(p)
        out["recall"].append(r)
        out["fscore"].append(2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


def sample_mesh(vertices: Tensor, faces: Tensor, m: int, generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """``(points (m, 3) float32, face (m,) int32)``: ``m`` points uniform by area on the mesh ``vertices (nv, 3)``,
    ``faces (nf, 3) int32``, and the face each lies on.

    Faces are drawn in proportion to their area through :func:`latentsplat_amd.mcmc.sample_by_weight` with weights
    area / largest area.  That rule quantises a weight to 30 bits, so a face below 2^-30 of the largest is never drawn
    (nor is a face of zero area).  The uniforms are ``torch.rand((3, m), dtype=float64, generator=generator)``: row 0
    picks the face, rows 1 and 2 the point ``(1 - sqrt(u1)) a + sqrt(u1) (1 - u2) b + sqrt(u1) u2 c``, evaluated in
    float64 and rounded once to float32.  The same generator state gives the same bits.  A mesh of zero (or non-finite)
    total area is refused.  One host read."""
    from .mcmc import sample_by_weight
    vertices = _args.f32(_WHO, "vertices", vertices)
    dev = vertices.device
    faces = _args.i32(_WHO, "faces", faces, None, dev)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.LsrError(f"vertices must be (nv, 3) and faces (nf, 3), got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    m = int(m)
    if m < 0:
        raise _lib.LsrError("m must not be negative")
    nv, nf = vertices.shape[0], faces.shape[0]
    if nf == 0 or nv == 0:
        raise _lib.LsrError("a mesh without faces has no area to sample")
    f = faces.detach().long()
    lo, hi = f.min(), f.max()
    v = vertices.detach().double()
    a, b, c = v[f[:, 0].clamp(0, nv - 1)], v[f[:, 1].clamp(0, nv - 1)], v[f[:, 2].clamp(0, nv - 1)]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    largest = area.max()
    lo, hi, top = torch.stack([lo.double(), hi.double(), largest]).tolist()
    if lo < 0 or hi >= nv:
        raise _lib.LsrError(f"faces name vertices {int(lo)}..{int(hi)}, outside 0..{nv - 1}")
    if not (top > 0.0 and top < float("inf")):
        raise _lib.LsrError("the mesh has zero (or non-finite) total area: nothing to sample")
    if m == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
    where = dev if generator is None else generator.device
    u = torch.rand((3, m), dtype=torch.float64, device=where, generator=generator).to(dev)
    weights = (area / largest).float()
    face = sample_by_weight(weights, u[0].contiguous())[0]
    pick = face.long()
    s = torch.sqrt(u[1])[:, None]
    t = u[2][:, None]
    points = (1.0 - s) * a[pick] + s * (1.0 - t) * b[pick] + s * t * c[pick]
    return points.float(), face
