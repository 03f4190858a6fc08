"""Codebook compression of a 3DGS scene: weighted k-means in HIP (csrc/vq.hip, C ABI include/lsr_vq.h).

A degree-3 scene is 59 floats per Gaussian and 45 of them are ``f_rest``.  Vector quantisation (Compact3D, "Compressed 3D
Gaussian Splatting") replaces the view-dependent colour rows and the shape rows (log-scales and rotation) by indices
into two small codebooks found by weighted k-means; positions, ``f_dc`` and opacities stay as they are.

:func:`vq_assign` is the assignment half of a Lloyd iteration: the nearest code of every row, fused distance and argmin on
the f32 matrix instruction, the ``n x k`` distances never in memory; ties go to the lowest index.  :func:`vq_update` is
the other half: weighted means in float64 in a fixed order (the same bits every call); a code nothing chose keeps its
previous row.  :func:`kmeans` drives the two for a fixed number of iterations with no host read in the loop.
:func:`quantize_scene` / :class:`QuantizedScene` are the scene level, :func:`contribution_weights` the usual importance
weights (how much each Gaussian contributes to a set of views).

The kernels take float32 ROCm tensors only; there is no CPU fallback.  A :class:`QuantizedScene` itself (``dequantize``,
``save``, ``load``) is plain gathers and a numpy file and lives on any device."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

MAX_DIM, MAX_CODES, MAX_ROWS = _lib.VQ_MAX_DIM, _lib.VQ_MAX_CODES, _lib.VQ_MAX_ROWS


def _rows(x: Tensor, what: str) -> Tensor:
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32:
        raise _lib.LsrError(f"vector quantisation needs float32 ROCm tensors (no CPU fallback): {what}")
    if x.dim() != 2 or not 1 <= x.shape[1] <= MAX_DIM or x.shape[0] > MAX_ROWS:
        raise _lib.LsrError(f"{what} must be (n, D) with 1 <= D <= {MAX_DIM} and n <= {MAX_ROWS}, got {tuple(x.shape)}")
    return x.detach().contiguous()


def _codes(codebook: Tensor, x: Tensor, what: str = "codebook") -> Tensor:
    c = _rows(codebook, what)
    if c.device != x.device or c.shape[1] != x.shape[1] or not 1 <= c.shape[0] <= MAX_CODES:
        raise _lib.LsrError(f"{what} must be (k, {x.shape[1]}) with 1 <= k <= {MAX_CODES} on {x.device}, got {tuple(c.shape)} on {c.device}")
    return c


def _vector(t: Tensor, x: Tensor, dtype, what: str) -> Tensor:
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype:
        raise _lib.LsrError(f"vector quantisation needs ROCm tensors (no CPU fallback): {what} must be {dtype}")
    if t.device != x.device or tuple(t.shape) != (x.shape[0],):
        raise _lib.LsrError(f"{what} must be ({x.shape[0]},) on {x.device}, got {tuple(t.shape)} on {t.device}")
    return t.detach().contiguous()


def _assign(x: Tensor, c: Tensor, idx: Tensor, dist2: Optional[Tensor], ws: Tensor) -> None:
    n, d = x.shape
    if n == 0:
        return
    dims = _lib.VqDims(n=n, k=c.shape[0], d=d)
    with torch.cuda.device(x.device):
        _lib.call("lsr_vq_assign", C.byref(dims), ptr(x), ptr(c), ptr(idx), ptr(dist2), ptr(ws), _args.stream(x))


def _update(x: Tensor, idx: Tensor, w: Optional[Tensor], prev: Tensor, out: Tensor, mass: Tensor, ws: Tensor) -> None:
    n, d = x.shape
    if n == 0:
        out.copy_(prev)
        mass.zero_()
        return
    dims = _lib.VqDims(n=n, k=prev.shape[0], d=d)
    with torch.cuda.device(x.device):
        _lib.call("lsr_vq_update", C.byref(dims), ptr(x), ptr(idx), ptr(w), ptr(prev), ptr(out), ptr(mass), ptr(ws),
                  _args.stream(x))


def vq_assign(x: Tensor, codebook: Tensor, want_dist: bool = False):
    """``idx (n,) int32``: for every row of ``x (n, D)`` the row of ``codebook (k, D)`` nearest to it; equal distances
    go to the lowest index.  ``want_dist=True`` returns ``(idx, dist2)`` with ``dist2 (n,)`` the squared distance to the
    chosen code, computed from the differences.  ``1 <= D <= 96``, ``1 <= k <= 65536``.  Asynchronous on the current
    stream; non-contiguous tensors are made contiguous; the inputs are expected to be finite."""
    x = _rows(x, "x")
    c = _codes(codebook, x)
    n, dev = x.shape[0], x.device
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    dist2 = torch.empty((n,), dtype=torch.float32, device=dev) if want_dist else None
    _assign(x, c, idx, dist2, _args.workspace(_lib.load().lsr_vq_workspace_bytes(n, c.shape[0], x.shape[1]), dev))
    return (idx, dist2) if want_dist else idx


def vq_update(x: Tensor, idx: Tensor, prev_codebook: Tensor, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``(codebook (k, D), mass (k,))``: ``codebook[j]`` is the mean of the rows of ``x (n, D)`` with ``idx == j``
    weighted by ``weights (n,)`` (``None``: ones) and ``mass[j]`` the sum of their weights.  A code of zero mass keeps
    ``prev_codebook[j]`` bit for bit; rows whose ``idx`` (int32) lies outside ``[0, k)`` are skipped, which is how a
    caller masks rows.  The sums are float64 in a fixed order: two calls give the same bits."""
    x = _rows(x, "x")
    prev = _codes(prev_codebook, x, "prev_codebook")
    idx = _vector(idx, x, torch.int32, "idx")
    w = None if weights is None else _vector(weights, x, torch.float32, "weights")
    out, mass = torch.empty_like(prev), torch.empty((prev.shape[0],), dtype=torch.float32, device=x.device)
    ws = _args.workspace(_lib.load().lsr_vq_workspace_bytes(x.shape[0], prev.shape[0], x.shape[1]), x.device)
    _update(x, idx, w, prev, out, mass, ws)
    return out, mass


def kmeans(x: Tensor, k: int, iters: int = 10, weights: Optional[Tensor] = None, init: Optional[Tensor] = None,
           generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """Weighted k-means (Lloyd): ``(codebook (k, D), idx (n,) int32)`` after exactly ``iters`` iterations of
    :func:`vq_assign` and :func:`vq_update`, then one more assignment, so that ``idx`` is the assignment against the
    returned codebook.  Nothing is read back inside the loop.  ``init (k, D)`` is the starting codebook; without it ``k``
    rows of ``x`` are drawn by ``torch.randperm(n, generator=generator)`` (wrapping around when ``n < k``).  The same
    inputs and the same generator state give the same bits."""
    x = _rows(x, "x")
    n, d = x.shape
    dev = x.device
    if not 1 <= int(k) <= MAX_CODES or int(iters) < 0:
        raise _lib.LsrError(f"kmeans: k must be in 1..{MAX_CODES} and iters >= 0")
    k = int(k)
    w = None if weights is None else _vector(weights, x, torch.float32, "weights")
    if init is not None:
        code = _codes(init, x, "init").clone()
        if code.shape[0] != k:
            raise _lib.LsrError(f"kmeans: init must be ({k}, {d}), got {tuple(code.shape)}")
    else:
        if n == 0:
            raise _lib.LsrError("kmeans: no rows to draw the initial codebook from; pass init")
        perm = torch.randperm(n, generator=generator, device=generator.device if generator is not None else "cpu")
        code = x.index_select(0, perm.to(dev)[torch.arange(k, device=dev) % n])
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    ws = _args.workspace(_lib.load().lsr_vq_workspace_bytes(n, k, d), dev)
    other, mass = torch.empty_like(code), torch.empty((k,), dtype=torch.float32, device=dev)
    for _ in range(int(iters)):
        _assign(x, code, idx, None, ws)
        _update(x, idx, w, code, other, mass, ws)
        code, other = other, code
    _assign(x, code, idx, None, ws)
    return code, idx


def shape_rows(scaling: Tensor, rotation: Tensor) -> Tensor:
    """The ``(n, 7)`` shape rows the shape codebook is built over: the three log-scales, then the unit quaternion with
    its sign fixed so that ``w >= 0`` (where ``w == 0`` the first non-zero component is positive): ``q`` and ``-q`` are one
    rotation and must not be two codes."""
    q = rotation.detach()
    q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-30)
    first = q[:, 3:4]                                   # the first non-zero component (0 for a zero row)
    for c in (2, 1, 0):
        first = torch.where(q[:, c:c + 1] != 0, q[:, c:c + 1], first)
    q = torch.where(first < 0, -q, q) + 0.0             # (+ 0.0: a negated zero component is +0.0 again, canonical in bits too)
    return torch.cat([scaling.detach(), q], dim=1).contiguous()


@dataclass
class QuantizedScene:
    """A scene whose view-dependent colour and shape are indices into codebooks.  ``xyz (n, 3)``, ``features_dc
    (n, 1, 3)`` and ``opacity (n, 1)`` are the scene's own tensors; ``rest_codebook (k_r, K - 1, 3)`` with ``rest_idx
    (n,)`` replaces ``_features_rest`` (both ``None`` at degree 0) and ``shape_codebook (k_s, 7)`` with ``shape_idx (n,)``
    replaces ``_scaling`` and ``_rotation`` (:func:`shape_rows`).  Indices are int32 in memory and uint16 in the file."""
    xyz: Tensor
    features_dc: Tensor
    opacity: Tensor
    rest_codebook: Optional[Tensor]
    rest_idx: Optional[Tensor]
    shape_codebook: Tensor
    shape_idx: Tensor
    max_sh_degree: int
    active_sh_degree: int

    @property
    def num_gaussians(self) -> int:
        return self.xyz.shape[0]

    def dequantize(self):
        """The :class:`~latentsplat_amd.scene_model.GaussianScene` the codebooks stand for: ``index_select`` gathers, on
        whatever device the tensors are."""
        from .scene_model import GaussianScene
        n = self.num_gaussians
        if self.rest_codebook is None:
            rest = torch.zeros((n, 0, 3), dtype=torch.float32, device=self.xyz.device)
        else:
            rest = self.rest_codebook.index_select(0, self.rest_idx.long())
        shape = self.shape_codebook.index_select(0, self.shape_idx.long())
        return GaussianScene(self.xyz, self.features_dc, rest, self.opacity, shape[:, :3], shape[:, 3:],
                             active_sh_degree=self.active_sh_degree)

    @property
    def nbytes(self) -> int:
        """Bytes of the quantised scene with 16-bit indices (what :meth:`save` stores before its general-purpose
        compression)."""
        floats = sum(t.numel() for t in (self.xyz, self.features_dc, self.opacity, self.shape_codebook))
        floats += 0 if self.rest_codebook is None else self.rest_codebook.numel()
        return 4 * floats + 2 * self.num_gaussians * (1 if self.rest_idx is None else 2)

    def save(self, path) -> None:
        """One ``numpy.savez_compressed`` file: the floats as they are, the indices as uint16."""
        import numpy as np
        host = lambda t: t.detach().cpu().numpy()
        arrays = dict(xyz=host(self.xyz), features_dc=host(self.features_dc), opacity=host(self.opacity),
                      shape_codebook=host(self.shape_codebook), shape_idx=host(self.shape_idx).astype(np.uint16),
                      sh_degrees=np.array([self.max_sh_degree, self.active_sh_degree], np.int32))
        if self.rest_codebook is not None:
            arrays.update(rest_codebook=host(self.rest_codebook), rest_idx=host(self.rest_idx).astype(np.uint16))
        with open(path, "wb") as f:
            np.savez_compressed(f, **arrays)

    @classmethod
    def load(cls, path, device="cpu") -> "QuantizedScene":
        """What :meth:`save` wrote, bit for bit, on ``device``."""
        import numpy as np
        with np.load(path) as z:
            dev = torch.device(device)
            f = lambda name: torch.from_numpy(z[name]).to(dev)
            i = lambda name: torch.from_numpy(z[name].astype(np.int32)).to(dev)
            rest = "rest_codebook" in z.files
            return cls(xyz=f("xyz"), features_dc=f("features_dc"), opacity=f("opacity"),
                       rest_codebook=f("rest_codebook") if rest else None, rest_idx=i("rest_idx") if rest else None,
                       shape_codebook=f("shape_codebook"), shape_idx=i("shape_idx"),
                       max_sh_degree=int(z["sh_degrees"][0]), active_sh_degree=int(z["sh_degrees"][1]))


def quantize_scene(scene, rest_codes: int = 4096, shape_codes: int = 4096, iters: int = 10, weights: Optional[Tensor] = None,
                   generator: Optional[torch.Generator] = None, rest_init: Optional[Tensor] = None,
                   shape_init: Optional[Tensor] = None) -> QuantizedScene:
    """Two weighted k-means runs (:func:`kmeans`) over a :class:`~latentsplat_amd.scene_model.GaussianScene` on a ROCm
    device: ``rest_codes`` codes over the ``_features_rest`` rows flattened to ``(n, 3 (K - 1))`` (no such group at degree
    0) and ``shape_codes`` codes over the :func:`shape_rows`.  ``weights (n,)`` weights both (``None``: ones;
    :func:`contribution_weights`); ``rest_init (k_r, 3 (K - 1))`` / ``shape_init (k_s, 7)`` are starting codebooks,
    otherwise rows are drawn with ``generator``.  Positions, ``_features_dc`` and opacities are copied as they are."""
    if not scene._xyz.is_cuda:
        raise _lib.LsrError("a GaussianScene is quantised on the MI355X: move it to a ROCm ('cuda') device; there is no CPU fallback")
    if not 1 <= int(rest_codes) <= MAX_CODES or not 1 <= int(shape_codes) <= MAX_CODES:
        raise _lib.LsrError(f"quantize_scene: the codebooks hold 1..{MAX_CODES} codes")
    n = scene.num_gaussians
    rest_width = 3 * scene._features_rest.shape[1]
    with torch.no_grad():
        rest_codebook = rest_idx = None
        if rest_width:
            rest_codebook, rest_idx = kmeans(scene._features_rest.detach().reshape(n, rest_width), rest_codes, iters, weights,
                                             rest_init, generator)
            rest_codebook = rest_codebook.reshape(-1, rest_width // 3, 3)
        shape_codebook, shape_idx = kmeans(shape_rows(scene._scaling, scene._rotation), shape_codes, iters, weights, shape_init,
                                           generator)
        keep = lambda t: t.detach().clone()
        return QuantizedScene(xyz=keep(scene._xyz), features_dc=keep(scene._features_dc), opacity=keep(scene._opacity),
                              rest_codebook=rest_codebook, rest_idx=rest_idx, shape_codebook=shape_codebook, shape_idx=shape_idx,
                              max_sh_degree=scene.max_sh_degree, active_sh_degree=scene.active_sh_degree)


def contribution_weights(scene, views: Tensor, height: int, width: int) -> Tensor:
    """``(n,)``: the sum over the pixels of ``views`` of ``alpha_i T_i``, how much Gaussian ``i`` contributes to the
    images: the gradient of the summed one-channel feature image with respect to a per-Gaussian feature of ones, through
    the rasterizer's own backward."""
    ones = torch.ones((scene.num_gaussians, 1), dtype=torch.float32, device=scene._xyz.device, requires_grad=True)
    with torch.enable_grad():
        feature = scene.render(views.detach(), height, width, features=ones)[1]
        grad, = torch.autograd.grad(feature.sum(), ones)
    return grad[:, 0].detach()
