"""The MCMC densification strategy for a trainable 3DGS scene ("3D Gaussian Splatting as Markov Chain Monte Carlo",
Kheradmand et al., 2024) in HIP (csrc/mcmc.hip, C ABI include/lsr_mcmc.h): dead Gaussians are relocated onto live ones
drawn in proportion to their opacity, the scene grows by a fixed factor up to a hard cap, and every optimizer step adds
covariance-shaped noise to the positions.  No gradient statistics are needed.

:func:`sample_by_weight` draws row indices by inverse CDF in exact integer arithmetic from the caller's float64 uniforms;
:func:`relocation_values` is the opacity / scale a Gaussian and its copies take so that their sum renders as the original
did; :func:`inject_noise` is the per-step noise in one launch.  :class:`MCMCControl` puts the pieces together for a
:class:`latentsplat_amd.scene_model.GaussianScene` and a ``torch.optim.Adam`` / ``AdamW`` /
:class:`latentsplat_amd.optim.SceneAdam` optimizer.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import math
from functools import partial
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib
from ._args import ptr

ROLES = dict(copy=_lib.MCMC_COPY, opacity=_lib.MCMC_OPACITY, scaling=_lib.MCMC_SCALING, moment=_lib.MCMC_MOMENT)
_SCENE_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
_SCENE_ROLES = dict(_xyz="copy", _features_dc="copy", _features_rest="copy", _opacity="opacity", _scaling="scaling", _rotation="copy")
_MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


_f32 = partial(_args.f32, "the MCMC strategy")


def _i32(name: str, t, numel: int, device) -> Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.device != device or t.numel() != numel or not t.is_contiguous():
        raise _lib.LsrError(f"{name} must be a contiguous int32 tensor of {numel} elements on {device}")
    return t


def _rows(n: int) -> int:
    if n >= _lib.MCMC_MAX_ROWS:
        raise _lib.LsrError(f"the MCMC strategy takes fewer than 2^28 rows, got {n}")
    return n


def dead_logit(min_opacity: float) -> float:
    """``logit(min_opacity)`` in double, rounded to float32: the threshold ``lsr_mcmc_classify`` compares logits with."""
    if not 0.0 <= min_opacity < 1.0:
        raise _lib.LsrError(f"min_opacity must be in [0, 1), got {min_opacity}")
    if min_opacity == 0.0:
        return -math.inf
    return float(np.float32(math.log(min_opacity / (1.0 - min_opacity))))


def classify_dead(opacity: Tensor, threshold_logit: float, want_dead: bool = True):
    """``lsr_mcmc_classify``: ``weights (n,)`` = 0 for a dead row (``opacity <= threshold_logit``) and ``sigmoid(opacity)``
    otherwise; with ``want_dead`` also ``dead (n,)`` int32, whose first ``counts[0]`` entries are the dead rows in index
    order, and ``counts (2,)`` int32 = {dead, alive}, all on the device (nothing is read back).  Returns ``(weights, dead,
    counts)``, the last two ``None`` without ``want_dead``."""
    op = _f32("opacity", opacity)
    n, dev = _rows(op.shape[0] if op.dim() else 1), op.device
    if op.numel() != n:
        raise _lib.LsrError(f"opacity must be (n,) or (n, 1), got {tuple(op.shape)}")
    op = op.detach().contiguous()
    lib = _lib.load()
    weights = torch.empty(n, dtype=torch.float32, device=dev)
    dead = torch.empty(n, dtype=torch.int32, device=dev) if want_dead else None
    counts = torch.zeros(2, dtype=torch.int32, device=dev) if want_dead else None
    ws = _args.workspace(lib.lsr_mcmc_workspace_bytes(n, 0), dev) if want_dead else None
    if n == 0:
        return weights, dead, counts
    with torch.cuda.device(dev):
        _lib.call("lsr_mcmc_classify", n, ptr(op), float(threshold_logit), ptr(weights), ptr(dead), ptr(counts), ptr(ws),
                  _args.stream(dev))
    return weights, dead, counts


def sample_by_weight(weights: Tensor, uniforms: Tensor, return_total: bool = False):
    """``lsr_mcmc_sample``: ``(idx, count)`` — ``idx (m,)`` int32, row ``idx[j]`` drawn with probability in proportion to
    ``clamp(weights, 0, 1)`` quantised to 30 bits, by inverse CDF of the caller's ``uniforms (m,)`` float64
    (``torch.rand(m, dtype=torch.float64, generator=...)``); ``count (n,)`` int32, how often each row was drawn.  A row of
    weight 0 (or NaN, or below 2^-30) is never drawn; when every weight is 0, every ``idx`` is -1.  The rule is exact
    integer arithmetic (include/lsr_mcmc.h): the same inputs give the same draws on any device and at any size, and
    there is no 2^24-category limit.  ``return_total``: also the ``(1,)`` int64 sum of the quanta."""
    w = _f32("weights", weights)
    dev = w.device
    n = _rows(w.numel())
    if w.dim() != 1:
        raise _lib.LsrError(f"weights must be (n,), got {tuple(w.shape)}")
    if not torch.is_tensor(uniforms) or uniforms.dtype != torch.float64 or uniforms.dim() != 1 or uniforms.device != dev:
        raise _lib.LsrError("uniforms must be a float64 (m,) ROCm tensor on the weights' device (no CPU fallback)")
    m = uniforms.shape[0]
    if n == 0 and m > 0:
        raise _lib.LsrError("cannot draw from no rows")
    w, u = w.detach().contiguous(), uniforms.contiguous()
    lib = _lib.load()
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _args.workspace(lib.lsr_mcmc_workspace_bytes(n, m), dev)
    with torch.cuda.device(dev):
        _lib.call("lsr_mcmc_sample", n, ptr(w), m, ptr(u), ptr(idx), ptr(count), ptr(total), ptr(ws),
                  _args.stream(dev))
    return (idx, count, total) if return_total else (idx, count)


def apply_relocation(tables: Sequence[Tuple[Tensor, str]], n: int, idx: Tensor, count: Tensor, dest: Optional[Tensor] = None,
                     min_opacity: float = 0.005) -> None:
    """``lsr_mcmc_apply``, in place over every ``(tensor, role)`` of ``tables``; ``role`` is ``"copy"``, ``"opacity"``,
    ``"scaling"`` or ``"moment"``.  ``idx (m,)`` and ``count (n,)`` are those of one :func:`sample_by_weight` call.  With
    ``dest (m,)`` int32 (distinct rows below ``n``, none of them drawn) row ``dest[j]`` becomes a copy of row ``idx[j]``
    and keeps its own moments: a relocation, tensors of ``n`` rows.  Without it row ``n + j`` does, with moments of 0: a
    growth, tensors of ``n + m`` rows whose first ``n`` are the scene.  Sources (``count > 0``) take their new opacity and
    scaling and lose their moments either way.  Tensors must be contiguous: they are not copied."""
    if not tables:
        return
    dev = tables[0][0].device
    _rows(n)
    m = idx.shape[0]
    _i32("idx", idx, m, dev)
    _i32("count", count, n, dev)
    if dest is not None:
        _i32("dest", dest, m, dev)
        if m == 0:
            dest = None                    # (nothing to place; the sources are still updated)
    total_rows = n + m if dest is None else n
    _rows(total_rows)
    if len(tables) > _lib.MCMC_MAX_TABLES:
        raise _lib.LsrError(f"at most {_lib.MCMC_MAX_TABLES} tables per call")
    desc = []
    for i, (t, role) in enumerate(tables):
        _f32(f"table {i}", t, device=dev)
        if role not in ROLES:
            raise _lib.LsrError(f"unknown role {role!r}; expected one of {list(ROLES)}")
        if t.dim() < 1 or t.shape[0] != total_rows or not t.is_contiguous():
            raise _lib.LsrError(f"table {i} must be contiguous with {total_rows} rows (it is updated in place)")
        width = math.prod(t.shape[1:])
        if width and total_rows:      # (a table without columns, features_rest of a degree-0 scene, has nothing to move)
            desc.append(_lib.McmcTable(t.data_ptr(), width, ROLES[role]))
    if n == 0:
        return
    lib = _lib.load()
    arr = (_lib.McmcTable * max(len(desc), 1))(*desc)
    ws = _args.workspace(lib.lsr_mcmc_workspace_bytes(n, m), dev)
    with torch.cuda.device(dev):
        _lib.call("lsr_mcmc_apply", n, m, ptr(idx), ptr(count), ptr(dest), arr, len(desc), float(min_opacity), ptr(ws),
                  _args.stream(dev))


def relocation_values(opacity: Tensor, scaling: Tensor, count: Tensor, min_opacity: float = 0.005) -> Tuple[Tensor, Tensor]:
    """``(opacity', scaling')``: for every row with ``count > 0`` the logit and log-scales the Gaussian and its ``count``
    copies take (``N = min(count + 1, 50)``; the formulas are in include/lsr_mcmc.h, evaluated in double); rows with
    ``count == 0`` are copied bit for bit.  ``opacity (n, 1)`` or ``(n,)`` logits, ``scaling (n, 3)`` logs, ``count (n,)``
    int32."""
    op = _f32("opacity", opacity)
    n, dev = (op.shape[0] if op.dim() else 1), op.device
    if op.numel() != n:
        raise _lib.LsrError(f"opacity must be (n,) or (n, 1), got {tuple(op.shape)}")
    sc = _f32("scaling", scaling, (n, 3), dev)
    new_op, new_sc = op.detach().clone(memory_format=torch.contiguous_format), sc.detach().clone(memory_format=torch.contiguous_format)
    apply_relocation([(new_op, "opacity"), (new_sc, "scaling")], n, torch.empty(0, dtype=torch.int32, device=dev), count,
                     None, min_opacity)
    return new_op, new_sc


def inject_noise(xyz: Tensor, opacity: Tensor, scaling: Tensor, rotation: Tensor, eps: Tensor, step_scale: float) -> None:
    """``lsr_mcmc_noise``: ``xyz += Sigma (eps * f)`` in place, one launch, no host wait; ``Sigma = R S S^T R^T`` from
    ``rotation (n, 4)`` (normalised here, ``w, x, y, z``) and ``exp(scaling (n, 3))``, ``f = step_scale / (1 +
    exp(-100 ((1 - sigmoid(opacity)) - 0.995)))``: opaque Gaussians stay put.  ``eps (n, 3)`` are the caller's standard
    normals, ``step_scale = noise_lr * lr_xyz``.  A row whose increment is not finite is left as it is.  ``xyz`` must be
    contiguous (it is not copied); a ``Parameter`` is updated through its data."""
    x = _f32("xyz", xyz)
    n, dev = _rows(x.shape[0] if x.dim() else 0), x.device
    _f32("xyz", x, (n, 3))
    if not x.is_contiguous():
        raise _lib.LsrError("xyz is updated in place and must be contiguous (it is not copied)")
    op = _f32("opacity", opacity, device=dev)
    if op.numel() != n:
        raise _lib.LsrError(f"opacity must have n = {n} elements")
    sc, rot, e = _f32("scaling", scaling, (n, 3), dev), _f32("rotation", rotation, (n, 4), dev), _f32("eps", eps, (n, 3), dev)
    if not math.isfinite(step_scale):
        raise _lib.LsrError("step_scale must be finite")
    if n == 0:
        return
    op, sc, rot, e = (t.detach().contiguous() for t in (op, sc, rot, e))
    with torch.cuda.device(dev):
        _lib.call("lsr_mcmc_noise", n, ptr(x.detach()), ptr(op), ptr(sc), ptr(rot), ptr(e), float(step_scale),
                  _args.stream(dev))


def _held_parameters(scene, optimizer, what: str):
    """``(params, held)``: the scene's six parameters by name, and ``name -> (group, index)`` for those the optimizer
    holds.  An optimizer other than Adam / AdamW (SceneAdam is an Adam) that holds state for them is refused, as
    ``DensityControl.densify_and_prune`` refuses it."""
    params = {k: getattr(scene, k) for k in _SCENE_PARAMS}
    by_id = {id(p): k for k, p in params.items()}
    held = {}
    for group in (optimizer.param_groups if optimizer is not None else ()):
        for i, p in enumerate(group["params"]):
            if id(p) in by_id:
                held[by_id[id(p)]] = (group, i)
    adam = isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW))
    if optimizer is not None and not adam and any(len(optimizer.state.get(params[k], {})) for k in held):
        raise _lib.LsrError(f"{what} moves the state of torch.optim.Adam / AdamW only; {type(optimizer).__name__} holds state "
                            "for the scene's parameters")
    return params, held


def _moments(optimizer, params, held):
    """``[(name, key, tensor)]`` of the Adam moments the optimizer holds for the scene's parameters."""
    out = []
    for k in held:
        state = optimizer.state.get(params[k], {})
        for key in _MOMENTS:
            if torch.is_tensor(state.get(key)):
                out.append((k, key, state[key]))
    return out


class MCMCControl:
    """The MCMC strategy for a :class:`GaussianScene`: ``cap_max`` is the hard limit on the number of Gaussians,
    ``min_opacity`` the opacity at or below which a Gaussian is dead, ``growth`` the factor by which :meth:`add_new` grows
    the scene.  Call :meth:`step` every densification interval and :meth:`inject_noise` after every optimizer step, and
    add :meth:`regularizer` to the loss."""

    def __init__(self, scene, cap_max: int, min_opacity: float = 0.005, growth: float = 1.05):
        if cap_max < 1 or not growth >= 1.0:
            raise _lib.LsrError("cap_max must be positive and growth at least 1")
        _f32("the scene's positions", scene._xyz)
        self.scene = scene
        self.cap_max = int(cap_max)
        self.min_opacity = float(min_opacity)
        self.growth = float(growth)
        self.dead_logit = dead_logit(self.min_opacity)

    def _uniforms(self, m: int, generator: Optional[torch.Generator]) -> Tensor:
        dev = self.scene._xyz.device
        return torch.rand(m, dtype=torch.float64, generator=generator, device=dev if generator is None else generator.device).to(dev)

    def relocate(self, optimizer, generator: Optional[torch.Generator] = None) -> dict:
        """The published ``relocate_gs``: every dead Gaussian (``sigmoid(opacity) <= min_opacity``) becomes a copy of a
        live one drawn in proportion to its opacity; a Gaussian drawn ``c`` times and its copies take the opacity and
        scale of :func:`relocation_values` and it loses its Adam moments (a relocated row keeps its own, as in the
        published trainer).  In place on ``param.data``: the parameters stay the same objects and the optimizer is not
        touched beyond its moments.  ONE host read (the two counts).  Returns ``dict(dead, alive, relocated)``."""
        scene = self.scene
        params, held = _held_parameters(scene, optimizer, "relocate")
        n = scene.num_gaussians
        weights, dead, counts = classify_dead(scene._opacity, self.dead_logit)
        n_dead, n_alive = (int(c) for c in counts.tolist())                       # the one host read
        if n_dead == 0 or n_alive == 0:
            return dict(dead=n_dead, alive=n_alive, relocated=0)
        idx, count = sample_by_weight(weights, self._uniforms(n_dead, generator))
        tables = [(params[k].data, _SCENE_ROLES[k]) for k in _SCENE_PARAMS]
        tables += [(t, "moment") for _, _, t in _moments(optimizer, params, held)]
        apply_relocation(tables, n, idx, count, dead[:n_dead], self.min_opacity)
        return dict(dead=n_dead, alive=n_alive, relocated=n_dead)

    def add_new(self, optimizer, generator: Optional[torch.Generator] = None) -> dict:
        """The published ``add_new_gs``: the scene grows to ``min(cap_max, int(growth * n))`` rows (known on the host: no
        device read); each new Gaussian is a copy of one drawn in proportion to ``sigmoid(opacity)``, with the opacity
        and scale of :func:`relocation_values`, and starts with Adam moments of 0.  The scene gets fresh parameters
        (:meth:`GaussianScene.replace_parameters_`); the optimizer's ``param_groups`` and ``state`` are re-keyed to them
        and keep ``step``, as ``DensityControl.densify_and_prune`` does it.  At the cap nothing is touched.  Returns
        ``dict(added, n_in, n_out)``."""
        scene = self.scene
        params, held = _held_parameters(scene, optimizer, "add_new")
        n, dev = scene.num_gaussians, scene._xyz.device
        m = max(0, min(self.cap_max, int(self.growth * n)) - n)
        if m == 0 or n == 0:
            return dict(added=0, n_in=n, n_out=n)
        _rows(n + m)
        weights, _, _ = classify_dead(scene._opacity, -math.inf, want_dead=False)
        idx, count = sample_by_weight(weights, self._uniforms(m, generator))

        def grown(t: Tensor) -> Tensor:
            out = torch.empty((n + m,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
            out[:n].copy_(t.detach())
            return out

        new = {k: grown(params[k]) for k in _SCENE_PARAMS}
        moments = [(k, key, grown(t)) for k, key, t in _moments(optimizer, params, held)]
        tables = [(new[k], _SCENE_ROLES[k]) for k in _SCENE_PARAMS] + [(t, "moment") for _, _, t in moments]
        apply_relocation(tables, n, idx, count, None, self.min_opacity)
        scene.replace_parameters_(**{k[1:]: new[k] for k in _SCENE_PARAMS})
        new_moments = {}
        for k, key, t in moments:
            new_moments.setdefault(k, {})[key] = t
        for k, (group, i) in held.items():
            p_new = getattr(scene, k)
            state = optimizer.state.pop(params[k], None)
            group["params"][i] = p_new
            if state is not None and len(state):
                state.update(new_moments.get(k, {}))
                optimizer.state[p_new] = state
        return dict(added=m, n_in=n, n_out=n + m)

    def step(self, optimizer, generator: Optional[torch.Generator] = None) -> dict:
        """:meth:`relocate`, then :meth:`add_new`: the published order.  Returns ``dict(dead, relocated, added, n_in, n_out)``."""
        moved = self.relocate(optimizer, generator)
        added = self.add_new(optimizer, generator)
        return dict(dead=moved["dead"], relocated=moved["relocated"], added=added["added"], n_in=added["n_in"], n_out=added["n_out"])

    def inject_noise(self, lr_xyz: float, noise_lr: float = 5e5, generator: Optional[torch.Generator] = None) -> None:
        """The published per-step noise, after the optimizer step: ``torch.randn`` with ``generator`` and one launch
        (:func:`inject_noise` with ``step_scale = noise_lr * lr_xyz``; ``lr_xyz`` is the current position rate)."""
        scene = self.scene
        dev = scene._xyz.device
        eps = torch.randn((scene.num_gaussians, 3), dtype=torch.float32, generator=generator,
                          device=dev if generator is None else generator.device).to(dev)
        inject_noise(scene._xyz.data, scene._opacity, scene._scaling, scene._rotation, eps, float(noise_lr) * float(lr_xyz))

    def regularizer(self, opacity_reg: float = 0.01, scale_reg: float = 0.01) -> Tensor:
        """``opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scaling))``: the published trainer's two
        regularisers, without which nothing dies and nothing is relocated.  Plain torch with autograd."""
        scene = self.scene
        return opacity_reg * torch.sigmoid(scene._opacity).mean() + scale_reg * torch.exp(scene._scaling).mean()
