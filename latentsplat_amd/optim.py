"""The optimizer step of a trainable 3DGS scene in HIP: Adam over every parameter tensor of every group in one launch
(csrc/optim.hip, C ABI include/lsr_optim.h), densely or only on the Gaussians a visibility mask names.

:func:`adam_step` is the raw call.  :class:`SceneAdam` is a ``torch.optim.Adam`` whose ``step`` is that call: its state
keys and layout are stock Adam's, so :class:`latentsplat_amd.density.DensityControl` re-keys it like any Adam and a
``state_dict`` moves between the two classes.  :func:`expon_lr` is the customary 3DGS position-rate schedule (host
only) and :func:`visible_from_radii` the mask of a render.

The semantics of the sparse step are defined here, by include/lsr_optim.h, and not by appeal to any trainer: a row
whose mask byte is 0 keeps its parameter and both moments bit for bit, and is not read; the step count advances for
the tensor as a whole.  3DGS trainers that offer a visibility-masked step are commonly run without bias correction;
that is ``bias_correction=False`` here, a choice of the caller.

float32 ROCm tensors only; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from functools import partial
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _args, _lib


def expon_lr(step: int, lr_init: float, lr_final: float, max_steps: int, delay_steps: int = 0, delay_mult: float = 1.0) -> float:
    """The customary exponential 3DGS learning-rate schedule, on the host: log-linear from ``lr_init`` at step 0 to
    ``lr_final`` at ``max_steps`` and constant beyond, times a delay factor that rises from ``delay_mult`` at step 0 to
    1 at ``delay_steps`` along a quarter sine.  0 for a negative step or when both rates are 0.  With
    ``t = clip(step / max_steps, 0, 1)`` the value is ``delay_rate * exp((1 - t) * log(lr_init) + t * log(lr_final))``;
    the two ends (``t`` 0 and 1) return ``delay_rate * lr_init`` and ``delay_rate * lr_final`` themselves."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if delay_steps > 0:
        delay_rate = delay_mult + (1.0 - delay_mult) * math.sin(0.5 * math.pi * min(max(step / delay_steps, 0.0), 1.0))
    else:
        delay_rate = 1.0
    t = min(max(step / max_steps, 0.0), 1.0) if max_steps > 0 else 1.0
    if t == 0.0:
        return delay_rate * lr_init
    if t == 1.0:
        return delay_rate * lr_final
    return delay_rate * math.exp((1.0 - t) * math.log(lr_init) + t * math.log(lr_final))


def visible_from_radii(radii: Tensor) -> Tensor:
    """The ``(n,)`` bool mask of the Gaussians that were on screen in any view of a render: ``(radii > 0).any(0)`` for
    the ``(V, n)`` radii ``rasterize_views`` / ``GaussianScene.render`` return.  Plain torch."""
    if not torch.is_tensor(radii) or radii.dim() != 2:
        raise _lib.LsrError("radii must be the (V, n) tensor of a render")
    return (radii > 0).any(0)


def adam_scalars(lr: float, betas, step: int, bias_correction: bool = True):
    """``(step_size, inv_sqrt_bc2)`` of ``lsr_adam_table`` for step ``step`` (1 for the first), in double, as
    ``torch.optim.Adam`` computes them."""
    if not bias_correction:
        return float(lr), 1.0
    if step < 1:
        raise _lib.LsrError(f"the step count of an Adam step with bias correction starts at 1, got {step}")
    return float(lr) / (1.0 - float(betas[0]) ** step), 1.0 / math.sqrt(1.0 - float(betas[1]) ** step)


_f32 = partial(_args.f32, "adam_step")


def adam_step(tables: Sequence[dict], visible: Optional[Tensor] = None) -> None:
    """``lsr_adam_step``: one Adam step over every table, in place, one launch per ``LSR_ADAM_MAX_TABLES`` = 24 tables,
    no host wait.  A table is a dict: ``param``, ``grad``, ``exp_avg``, ``exp_avg_sq`` (float32 ROCm tensors of one
    shape; the three that are updated must be contiguous and are never copied, ``grad`` is made contiguous), ``lr``,
    ``betas``, ``eps``, ``step`` (the count of THIS step: 1 for the first) and ``bias_correction``.  Per element::

        m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * g * g
        p = p - step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)

    with ``step_size = lr / (1 - beta1^step)`` and ``inv_sqrt_bc2 = 1 / sqrt(1 - beta2^step)``, or ``lr`` and 1 without
    bias correction; these and ``1 - beta`` are computed here in double and rounded once, which gives a new gradient the
    weight ``torch.optim.Adam`` gives it (``float(1 - 0.999)``, not ``1 - float(0.999)``: 1.3e-5 apart).  ``visible``: a bool or uint8 ``(n,)`` tensor; every table then has ``n`` rows (its first
    dimension) and only rows with a non-zero byte are read and written.  Empty tensors are skipped."""
    if not tables:
        return
    dev = None
    desc, keep = [], []
    vis, n_vis = None, 0
    if visible is not None:
        if not torch.is_tensor(visible) or not visible.is_cuda or visible.dtype not in (torch.bool, torch.uint8) or visible.dim() != 1:
            raise _lib.LsrError("visible must be a bool or uint8 (n,) ROCm tensor (no CPU fallback)")
        vis = visible.contiguous()
        vis = vis.view(torch.uint8) if vis.dtype == torch.bool else vis
        n_vis, dev = vis.shape[0], vis.device
    for i, t in enumerate(tables):
        p = _f32(f"table {i} param", t["param"], contiguous=True)
        m = _f32(f"table {i} exp_avg", t["exp_avg"], contiguous=True)
        v = _f32(f"table {i} exp_avg_sq", t["exp_avg_sq"], contiguous=True)
        g = _f32(f"table {i} grad", t["grad"])
        dev = p.device if dev is None else dev
        if any(x.device != dev for x in (p, m, v, g)):
            raise _lib.LsrError(f"table {i}: every tensor of a call must be on {dev}")
        if not (p.shape == m.shape == v.shape == g.shape):
            raise _lib.LsrError(f"table {i}: param, grad, exp_avg and exp_avg_sq must have one shape, got {tuple(p.shape)}, "
                                f"{tuple(g.shape)}, {tuple(m.shape)} and {tuple(v.shape)}")
        if p.numel() == 0:
            continue
        rows = p.shape[0] if p.dim() else 1
        width = p.numel() // rows
        if vis is not None:
            if p.dim() == 0 or rows != n_vis:
                raise _lib.LsrError(f"table {i} has {rows} rows, the visibility mask {n_vis}")
            if width > _lib.ADAM_MAX_WIDTH:
                raise _lib.LsrError(f"table {i}: at most {_lib.ADAM_MAX_WIDTH} floats per row with a visibility mask, got {width}")
        elif width > _lib.ADAM_MAX_WIDTH:
            rows, width = p.numel(), 1                   # (dense: rows mean nothing)
        g = g.detach().contiguous()
        keep.append(g)
        betas = t.get("betas", (0.9, 0.999))
        step_size, inv_sqrt_bc2 = adam_scalars(t["lr"], betas, int(t.get("step", 1)), bool(t.get("bias_correction", True)))
        desc.append(_lib.AdamTable(param=p.data_ptr(), grad=g.data_ptr(), exp_avg=m.data_ptr(), exp_avg_sq=v.data_ptr(),
                                   rows=rows, width=width, reserved=0, beta1=float(betas[0]), beta2=float(betas[1]),
                                   one_minus_beta1=1.0 - float(betas[0]), one_minus_beta2=1.0 - float(betas[1]),
                                   eps=float(t.get("eps", 1e-8)), step_size=step_size, inv_sqrt_bc2=inv_sqrt_bc2, reserved_f=0.0))
    if not desc:
        return
    with torch.cuda.device(dev):
        for at in range(0, len(desc), _lib.ADAM_MAX_TABLES):
            chunk = desc[at:at + _lib.ADAM_MAX_TABLES]
            arr = (_lib.AdamTable * len(chunk))(*chunk)
            _lib.call("lsr_adam_step", arr, len(chunk), C.c_void_p(None if vis is None or n_vis == 0 else vis.data_ptr()),
                      n_vis, _args.stream(dev))


class SceneAdam(torch.optim.Adam):
    """``torch.optim.Adam`` with the step in HIP: all tensors of all parameter groups in one ``lsr_adam_step`` launch (a
    second one only beyond 24 tensors), optionally only on the visible Gaussians.

    ``SceneAdam(params_or_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-15, bias_correction=True)``; groups carry their
    own ``lr`` / ``betas`` / ``eps`` / ``bias_correction`` as in torch.  ``weight_decay``, ``amsgrad`` and ``maximize``
    are refused.  The state is stock Adam's — ``step`` (a float32 scalar on the host), ``exp_avg``, ``exp_avg_sq``,
    created at a parameter's first step — so ``DensityControl.densify_and_prune`` / ``reset_opacity`` work on it
    unchanged and ``state_dict()`` loads into a ``torch.optim.Adam`` and back.

    ``step(visibility=None)``: parameters without a gradient are skipped as in torch; ``step`` advances by one for
    every parameter that had one, with a mask too; the host does not wait for the device.  ``visibility`` is a bool or
    uint8 ``(n,)`` tensor (:func:`visible_from_radii`): every parameter then has ``n`` rows, and rows whose byte is 0 keep
    parameter and moments bit for bit (stock Adam would go on moving them on their momentum).

    The step count and the rates reach the kernel as arguments computed on the host.  A captured graph therefore
    replays the step count and rates OF ITS CAPTURE: a replay is exact only with ``bias_correction=False`` and constant
    rates.  Take one eager step before capturing, so that the state exists outside the graph's memory pool."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-15, bias_correction: bool = True, **kw):
        for name, off in (("weight_decay", 0), ("amsgrad", False), ("maximize", False)):
            if kw.pop(name, off):
                raise _lib.LsrError(f"SceneAdam does not implement {name}; use torch.optim.Adam for it")
        if kw:
            raise TypeError(f"SceneAdam got unexpected arguments {sorted(kw)}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, foreach=False)
        self.defaults["bias_correction"] = bool(bias_correction)
        for group in self.param_groups:
            group.setdefault("bias_correction", bool(bias_correction))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:        # (a state_dict of a stock Adam does not carry the key)
            group.setdefault("bias_correction", self.defaults.get("bias_correction", True))

    @classmethod
    def for_scene(cls, scene, extent: float, lr_position: float = 1.6e-4, lr_dc: float = 2.5e-3, lr_rest: Optional[float] = None,
                  lr_opacity: float = 5e-2, lr_scaling: float = 5e-3, lr_rotation: float = 1e-3, **kw) -> "SceneAdam":
        """One group per parameter tensor of a :class:`GaussianScene`, named after it (``_xyz``, ``_features_dc``,
        ``_features_rest``, ``_opacity``, ``_scaling``, ``_rotation``), at the published trainer's customary rates:
        position ``lr_position * extent``, ``lr_rest`` defaulting to ``lr_dc / 20``.  Empty tensors (``_features_rest``
        of a degree-0 scene) are left out."""
        rates = dict(_xyz=lr_position * float(extent), _features_dc=lr_dc, _features_rest=lr_dc / 20 if lr_rest is None else lr_rest,
                     _opacity=lr_opacity, _scaling=lr_scaling, _rotation=lr_rotation)
        groups = [dict(params=[p], lr=rates[name], name=name) for name, p in scene.named_parameters() if p.numel()]
        return cls(groups, lr=0.0, **kw)

    def set_lr(self, name: str, lr: float) -> None:
        """The rate of the group(s) named ``name`` (:meth:`for_scene` names them) from the next step on."""
        found = [g for g in self.param_groups if g.get("name") == name]
        if not found:
            raise KeyError(f"no parameter group named {name!r}")
        for g in found:
            g["lr"] = float(lr)

    @torch.no_grad()
    def step(self, visibility: Optional[Tensor] = None, closure=None):
        if callable(visibility) and closure is None:       # step(closure), as torch's optimizers are called
            visibility, closure = None, visibility
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        tables = []
        for group in self.param_groups:
            for name in ("weight_decay", "amsgrad", "maximize"):
                if group.get(name):
                    raise _lib.LsrError(f"SceneAdam does not implement {name}; use torch.optim.Adam for it")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise _lib.LsrError("SceneAdam takes dense gradients")
                if not p.is_cuda or p.dtype != torch.float32:
                    raise _lib.LsrError("SceneAdam needs float32 ROCm parameters (no CPU fallback)")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                tables.append((group, p, state))
        # nothing is touched before every table has been checked
        desc = [dict(param=p, grad=p.grad, exp_avg=s["exp_avg"], exp_avg_sq=s["exp_avg_sq"], lr=g["lr"], betas=g["betas"],
                     eps=g["eps"], step=int(float(s["step"])) + 1, bias_correction=g.get("bias_correction", True))
                for g, p, s in tables]
        adam_step(desc, visibility)
        for _, _, s in tables:
            s["step"] += 1
        return loss
