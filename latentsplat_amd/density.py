"""Adaptive density control for a trainable 3DGS scene: the published trainer's densification statistics and its
clone / split / prune step, in HIP (csrc/density.hip, C ABI include/lsr_density.h).

:func:`accumulate_density_stats` is the per-step ``add_densification_stats`` and ``max_radii2D`` update over all views of
a step in one launch.  :func:`plan_densify` classifies every Gaussian, scans, and emits the row map of the new scene
(kept originals, then clones, then the children of the split ones); :func:`apply_densify` gathers every per-Gaussian
table — parameters and optimiser moments — through that map in one launch.  :class:`DensityControl` holds the statistics
of a :class:`latentsplat_amd.scene_model.GaussianScene` under the published names and puts the pieces together for a
``torch.optim.Adam`` / ``AdamW`` optimizer.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from functools import partial
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

RULES = dict(copy=_lib.DENSIFY_COPY, zero_new=_lib.DENSIFY_ZERO_NEW, xyz=_lib.DENSIFY_XYZ, scaling=_lib.DENSIFY_SCALING)
_FLT_MAX = 3.4028234663852886e38
_SCENE_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
_SCENE_RULES = dict(_xyz="xyz", _features_dc="copy", _features_rest="copy", _opacity="copy", _scaling="scaling", _rotation="copy")


_f32 = partial(_args.f32, "density control")


def accumulate_density_stats(means2D_grad: Tensor, radii: Tensor, grad_accum: Tensor, denom: Tensor, max_radii: Tensor) -> None:
    """``lsr_density_accumulate``: for each Gaussian and each view ``v`` in order, where ``radii[v, g] > 0``:
    ``grad_accum += |means2D_grad[v, g, :2]|``, ``denom += 1``, ``max_radii = max(max_radii, radii)``; in place, one
    launch, no host wait.  ``means2D_grad`` is the per-view ``(V, n, 3)`` gradient ``rasterize_views(..., means2D=)``
    delivers, taken as it is; ``radii`` its ``(V, n)`` int32 output; the statistics are contiguous float32 tensors of
    ``n`` elements (``(n,)`` or ``(n, 1)``)."""
    g = _f32("means2D_grad", means2D_grad)
    if g.dim() != 3 or g.shape[2] != 3:
        raise _lib.LsrError(f"means2D_grad must be the per-view (V, n, 3) gradient, got {tuple(g.shape)}")
    V, n = g.shape[0], g.shape[1]
    dev = g.device
    if not torch.is_tensor(radii) or radii.dtype != torch.int32 or tuple(radii.shape) != (V, n) or radii.device != dev:
        raise _lib.LsrError(f"radii must be the (V, n) = {(V, n)} int32 tensor of the same render, on the same device")
    for name, t in (("grad_accum", grad_accum), ("denom", denom), ("max_radii", max_radii)):
        _f32(name, t, device=dev)
        if t.numel() != n or not t.is_contiguous():
            raise _lib.LsrError(f"{name} must be a contiguous tensor of n = {n} elements (it is updated in place)")
    if V == 0 or n == 0:
        return
    g, radii = g.detach().contiguous(), radii.contiguous()
    with torch.cuda.device(dev):
        _lib.call("lsr_density_accumulate", V, n, ptr(g), ptr(radii), ptr(grad_accum), ptr(denom), ptr(max_radii),
                  _args.stream(dev))


def plan_densify(opacity: Tensor, scaling: Tensor, grad_accum: Tensor, denom: Tensor, max_radii: Tensor, *,
                 grad_threshold: float, dense_extent: float, min_opacity: float, max_screen_size: float = 0.0,
                 world_limit: float = 0.0, n_split: int = 2) -> Tuple[Tensor, Tensor]:
    """``lsr_densify_plan``: ``(map, counts)`` on the device, nothing read back.  ``map`` is an int32 tensor of
    ``n * max(2, n_split)`` words holding the unsigned ``parent | kind << 28`` (kind 0 kept, 1 clone, ``2 + c`` child
    ``c``) in its first ``n_out`` entries, the rest uninitialised; ``counts`` is int32 ``(4,)``: kept, clones, emitting
    split parents, ``n_out``.  ``opacity (n, 1)`` holds logits and ``scaling (n, 3)`` logs; the rules and the pinned
    output order are in include/lsr_density.h."""
    op = _f32("opacity", opacity)
    n, dev = op.shape[0], op.device
    _f32("opacity", op, (n, 1))
    sc = _f32("scaling", scaling, (n, 3), dev)
    stats = []
    for name, t in (("grad_accum", grad_accum), ("denom", denom), ("max_radii", max_radii)):
        _f32(name, t, device=dev)
        if t.numel() != n:
            raise _lib.LsrError(f"{name} must have n = {n} elements")
        stats.append(t.detach().contiguous())
    lib = _lib.load()
    params = _lib.DensifyParams(grad_threshold=grad_threshold, dense_extent=dense_extent, min_opacity=min_opacity,
                                max_screen_size=max_screen_size, world_limit=world_limit, n_split=int(n_split),
                                reserved0=0, reserved1=0)
    capacity = n * max(2, int(n_split))
    map_ = torch.empty(capacity, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    ws = _args.workspace(lib.lsr_densify_workspace_bytes(n), dev)
    op, sc = op.detach().contiguous(), sc.detach().contiguous()
    with torch.cuda.device(dev):
        _lib.call("lsr_densify_plan", n, ptr(op), ptr(sc), *map(ptr, stats), C.byref(params), ptr(map_), capacity,
                  C.c_void_p(counts.data_ptr()), ptr(ws), _args.stream(dev))
    return map_, counts


def apply_densify(map_: Tensor, counts: Tensor, n_out: int, tables: Sequence[Tuple[Tensor, str]], *, n_split: int = 2,
                  scaling: Optional[Tensor] = None, rotation: Optional[Tensor] = None, eps: Optional[Tensor] = None) -> list:
    """``lsr_densify_apply``: every ``(tensor, rule)`` of ``tables`` gathered through the plan's map into a new tensor of
    ``n_out`` rows, all in one launch; the new tensors in order.  ``n_out`` is the host's copy of ``counts[3]``.  A
    tensor is ``(n, ...)``, its row everything behind the first dimension; ``rule`` is ``"copy"``, ``"zero_new"``
    (clones and children are 0: optimiser moments), ``"xyz"`` (children are ``xyz + R(q / |q|) (exp(scaling) * eps[r])``)
    or ``"scaling"`` (children are ``log(exp(s) / (0.8 n_split))``).  ``scaling (n, 3)``, ``rotation (n, 4)`` and the
    standard normals ``eps (n_split * counts[2], 3)`` go with the last two rules."""
    if not tables:
        return []
    n, dev = tables[0][0].shape[0], tables[0][0].device
    if len(tables) > _lib.DENSIFY_MAX_TABLES:
        raise _lib.LsrError(f"at most {_lib.DENSIFY_MAX_TABLES} tables per call")
    for name, t in (("map", map_), ("counts", counts)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise _lib.LsrError(f"{name} must be the contiguous int32 tensor plan_densify returned, on the tables' device")
    if counts.numel() != 4 or not 0 <= n_out <= map_.numel():
        raise _lib.LsrError("counts must hold four words and n_out must lie within the map")
    srcs, outs, desc = [], [], []
    for i, (t, rule) in enumerate(tables):
        _f32(f"table {i}", t, device=dev)
        if rule not in RULES:
            raise _lib.LsrError(f"unknown rule {rule!r}; expected one of {list(RULES)}")
        if t.dim() < 1 or t.shape[0] != n:
            raise _lib.LsrError(f"table {i} must have n = {n} rows")
        src = t.detach().contiguous()
        dst = torch.empty((n_out,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        outs.append(dst)
        width = math.prod(src.shape[1:])
        if width and n_out:      # (a table without columns, features_rest of a degree-0 scene, has nothing to move)
            srcs.append(src)
            desc.append(_lib.DensifyTable(src.data_ptr() if n else None, dst.data_ptr(), width, RULES[rule]))
    desc = (_lib.DensifyTable * max(len(desc), 1))(*desc)
    num_tables = len(srcs)
    extras = []
    for name, t, shape in (("scaling", scaling, (n, 3)), ("rotation", rotation, (n, 4)), ("eps", eps, None)):
        if t is not None:
            _f32(name, t, shape, dev)
            t = t.detach().contiguous()
        extras.append(t)
    eps_rows = 0
    if extras[2] is not None:
        if extras[2].dim() != 2 or extras[2].shape[1] != 3:
            raise _lib.LsrError("eps must be (n_split * split parents, 3)")
        eps_rows = extras[2].shape[0]
    with torch.cuda.device(dev):
        _lib.call("lsr_densify_apply", n, int(n_out), ptr(map_), ptr(counts), int(n_split), desc, num_tables,
                  *map(ptr, extras), eps_rows, _args.stream(dev))
    return outs


class DensityControl:
    """The densification state of a :class:`GaussianScene` under the published trainer's names: ``xyz_gradient_accum
    (n, 1)``, ``denom (n, 1)`` and ``max_radii2D (n,)``, float32 on the scene's device."""

    def __init__(self, scene):
        self.scene = scene
        self.last_map = None       # the row map of the last densify_and_prune: int32 words, parent | kind << 28 (unsigned)
        self._reset(scene.num_gaussians)

    def _reset(self, n: int) -> None:
        dev = self.scene._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        self.denom = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        self.max_radii2D = torch.zeros((n,), dtype=torch.float32, device=dev)

    def render(self, views: Tensor, height: int, width: int, absgrad: bool = False, **kw):
        """The densification render: ``scene.render(views, height, width, **kw)`` with the per-view ``(V, n, 3)`` leaf whose
        ``.grad`` :meth:`update` takes after the backward.  Returns ``(outputs, leaf)``.  ``absgrad=False``: the leaf is the
        render's ``means2D`` (the signed gradient, the published statistic); ``absgrad=True``: its ``means2D_abs`` (the
        absolute gradient of AbsGS, :func:`latentsplat_amd.rasterizer.rasterize_views`; colour-only renders, which a scene's
        are)."""
        leaf = torch.zeros((views.shape[0], self.scene.num_gaussians, 3), dtype=torch.float32, device=self.scene._xyz.device,
                           requires_grad=True)
        kw["means2D_abs" if absgrad else "means2D"] = leaf
        return self.scene.render(views, height, width, **kw), leaf

    def update(self, means2D_grad: Tensor, radii: Tensor) -> None:
        """One step's statistics, one launch.  ``means2D_grad`` is the PER-VIEW ``(V, n, 3)`` gradient: render with
        ``means2D=torch.zeros(V, n, 3, requires_grad=True)`` and pass its ``.grad``; ``radii`` is the render's ``(V, n)``
        output.  Each view counts as one published ``add_densification_stats`` call, and the gradient is taken as it
        arrives (a loss that is a mean over ``V`` views gives each view ``1 / V`` of the published single-view
        gradient: scale the threshold, not the statistics).  A shared ``(n, 3)`` tensor has already summed the views
        and is refused.

        The ABSOLUTE view-space gradient (AbsGS; gsplat's ``absgrad``) is fed the same way: render with
        ``means2D_abs=torch.zeros(V, n, 3, requires_grad=True)`` (:meth:`render` with ``absgrad=True`` does) and pass that
        leaf's ``.grad``.  Its per-pixel contributions do not cancel, so a large blurry splat reaches the threshold; the
        values are larger than the signed gradient's, and the threshold has to follow (gsplat documents 8e-4 next to the
        classic 2e-4)."""
        if torch.is_tensor(means2D_grad) and means2D_grad.dim() == 2:
            raise _lib.LsrError("DensityControl.update takes the per-view (V, n, 3) gradient; a shared (n, 3) means2D has "
                                "already summed the views")
        if not torch.is_tensor(means2D_grad) or means2D_grad.dim() != 3 or means2D_grad.shape[1] != self.denom.shape[0]:
            raise _lib.LsrError(f"means2D_grad must be (V, n, 3) with n = {self.denom.shape[0]}")
        accumulate_density_stats(means2D_grad, radii, self.xyz_gradient_accum, self.denom, self.max_radii2D)

    def densify_and_prune(self, optimizer, max_grad: float, min_opacity: float, extent: float, max_screen_size: float,
                          percent_dense: float = 0.01, n_split: int = 2, generator: Optional[torch.Generator] = None) -> dict:
        """The published ``densify_and_prune``: clone the selected small Gaussians, split the selected large ones into
        ``n_split`` children, prune by opacity and (with ``max_screen_size``, 0 or None = off) by size; then zero the
        statistics at the new size.  One plan, ONE host read (the four counts), ``torch.randn`` with ``generator`` for
        the children's offsets, one gather over the six parameters and, for a ``torch.optim.Adam`` / ``AdamW``
        optimizer, their ``exp_avg`` / ``exp_avg_sq`` (new rows start at 0).  The scene gets fresh parameters
        (:meth:`GaussianScene.replace_parameters_`); the optimizer's ``param_groups`` and ``state`` are re-keyed to them
        and keep ``step``.  An optimizer of another class is refused unless it has no state yet.  ``max_grad = inf``
        means "select nothing" (it is passed as the largest float32).  Returns the counts as a dict."""
        scene = self.scene
        params = {k: getattr(scene, k) for k in _SCENE_PARAMS}
        n, dev = scene.num_gaussians, scene._xyz.device
        adam = isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW))
        by_id = {id(p): k for k, p in params.items()}
        held = {}          # name -> (group, index) for the scene's parameters the optimizer holds
        for group in (optimizer.param_groups if optimizer is not None else ()):
            for i, p in enumerate(group["params"]):
                if id(p) in by_id:
                    held[by_id[id(p)]] = (group, i)
        if optimizer is not None and not adam and any(len(optimizer.state.get(params[k], {})) for k in held):
            raise _lib.LsrError(f"densify_and_prune re-keys the state of torch.optim.Adam / AdamW only; {type(optimizer).__name__} "
                                "holds state for the scene's parameters")
        size = float(max_screen_size or 0.0)
        map_, counts = plan_densify(scene._opacity, scene._scaling, self.xyz_gradient_accum, self.denom, self.max_radii2D,
                                    grad_threshold=min(float(max_grad), _FLT_MAX), dense_extent=percent_dense * extent,
                                    min_opacity=min_opacity, max_screen_size=size, world_limit=0.1 * extent, n_split=n_split)
        kept, clones, parents, n_out = (int(c) for c in counts.tolist())          # the one host read
        eps = torch.randn((n_split * parents, 3), dtype=torch.float32, generator=generator,
                          device=dev if generator is None else generator.device).to(dev)
        tables = [(params[k].detach(), _SCENE_RULES[k]) for k in _SCENE_PARAMS]
        moments = []       # (name, state key)
        for k in held:
            state = optimizer.state.get(params[k], {})
            for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                if torch.is_tensor(state.get(key)):
                    tables.append((state[key], "zero_new"))
                    moments.append((k, key))
        new = apply_densify(map_, counts, n_out, tables, n_split=n_split, scaling=scene._scaling, rotation=scene._rotation,
                            eps=eps)
        old = dict(params)
        scene.replace_parameters_(**{k[1:]: t for k, t in zip(_SCENE_PARAMS, new)})
        new_moments = {}
        for (k, key), t in zip(moments, new[len(_SCENE_PARAMS):]):
            new_moments.setdefault(k, {})[key] = t
        for k, (group, i) in held.items():
            p_new = getattr(scene, k)
            state = optimizer.state.pop(old[k], None)
            group["params"][i] = p_new
            if state is not None and len(state):
                state.update(new_moments.get(k, {}))
                optimizer.state[p_new] = state
        self._reset(n_out)
        self.last_map = map_[:n_out]
        return dict(kept=kept, clones=clones, split_parents=parents, n_out=n_out, n_in=n)

    def reset_opacity(self, optimizer, value: float = 0.01) -> None:
        """The published ``reset_opacity``: logits become ``min(opacity, logit(value))`` and the optimizer's two moments
        of the opacity are zeroed.  Plain torch: one ``(n, 1)`` tensor every few thousand steps."""
        p = self.scene._opacity
        with torch.no_grad():
            p.clamp_(max=math.log(value / (1.0 - value)))
        state = optimizer.state.get(p, {}) if optimizer is not None else {}
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            if torch.is_tensor(state.get(key)):
                state[key].zero_()
