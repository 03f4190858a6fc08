#!/usr/bin/env python
"""Device time of the MCMC strategy (csrc/mcmc.hip, include/lsr_mcmc.h, latentsplat_amd.mcmc) and of the stock-PyTorch
composition of the published sequence on the same card.

  noise        `lsr_mcmc_noise` through the C ABI (one launch, in place) against the stock composition:
               build_scaling_rotation, L L^T, two sigmoids, bmm — about a dozen launches and (n, 3, 3) temporaries.  68
               bytes per Gaussian move (xyz read and written, opacity, scaling, rotation, eps); the rate is given as a
               fraction of the 6.3 TB/s achievable.  Two arms: `warm`, the same arrays call after call (at both sizes they
               fit the 256 MB last-level cache: a cache figure), and `rotating`, over as many copies of the arrays as make
               1.1 GB, each call on the next copy — what a training step sees, where a whole render lies between two calls
  relocate     `MCMCControl.relocate` with 5 % of the Gaussians dead, over the six parameters and their twelve Adam
               moments (18 tables), through the public class, host read included; against `torch.multinomial` +
               `bincount` + the closed form of the new values in torch + indexing launches per table
  add_new      `MCMCControl.add_new` with 5 % growth, likewise; against multinomial + bincount + `torch.cat` per table
  regularizer  forward + backward of `MCMCControl.regularizer` (plain torch: it is not fused)

Sizes: 393 216 and 3 000 000 Gaussians at SH degree 3.  The noise samples are `--inner` back-to-back calls between two
device events, divided by their number; relocate and add_new change the scene, so each of their samples is ONE call on
a scene put back to its start outside the timed region.  Every figure is the median of `--samples` (>= 20) after
`--warmup` calls, with the smallest and the largest sample beside it.

usage: python tools/bench_mcmc.py [--samples 20] [--warmup 3] [--inner 5] [--json [profiles/mcmc_bench.json]]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (393_216, 3_000_000)
SH_REST = 15
ACHIEVABLE = 6.3e12
NOISE_BYTES = 68
MIN_OPACITY = 0.005
NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def _sample(fn, dev, inner=1, before=None):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before is not None:
        before()
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def _figures(t):
    return dict(ms=statistics.median(t), min_ms=min(t), max_ms=max(t), samples=len(t))


def _show(f):
    return f"{f['ms']:8.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]"


def make_tensors(n, dev, dead_fraction):
    gen = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.randn(s, device=dev, generator=gen)
    opacity = torch.rand((n, 1), device=dev, generator=gen) * 8.0 - 4.0
    dead = torch.rand(n, device=dev, generator=gen) < dead_fraction
    opacity[dead] = -7.0
    return dict(xyz=r(n, 3), features_dc=r(n, 1, 3), features_rest=r(n, SH_REST, 3), opacity=opacity,
                scaling=torch.rand((n, 3), device=dev, generator=gen) * 4.0 - 6.0, rotation=r(n, 4))


def stock_noise(xyz, opacity, scaling, rotation, eps, step_scale):
    s = torch.exp(scaling)
    q = rotation / rotation.norm(dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R @ torch.diag_embed(s)
    cov = L @ L.transpose(1, 2)
    f = torch.sigmoid(100.0 * ((1.0 - torch.sigmoid(opacity)) - 0.995))
    xyz.add_(torch.bmm(cov, (eps * f * step_scale).unsqueeze(-1)).squeeze(-1))


def stock_new_values(opacity_logit, scaling_log, ratio):
    """The closed form of the new values in torch, terms up to the largest ratio present (one host read)."""
    o = torch.sigmoid(opacity_logit)
    N = ratio.clamp(max=50).to(torch.float32)
    op = 1.0 - torch.pow(1.0 - o, 1.0 / N)
    D, coef, pw = torch.zeros_like(op), N.clone(), op.clone()          # coef = C(N, k + 1)
    for k in range(int(N.max())):
        D = D + coef * pw * ((-1.0) ** k / (k + 1) ** 0.5)
        coef = coef * (N - (k + 1)).clamp(min=0) / (k + 2)
        pw = pw * op
    new_scale = torch.log((o / D) * torch.exp(scaling_log))
    op = op.clamp(MIN_OPACITY, 1.0 - torch.finfo(torch.float32).eps)
    return torch.log(op / (1.0 - op)), new_scale


def stock_relocate(t, moments):
    o = torch.sigmoid(t["opacity"]).squeeze(1)
    dead = o <= MIN_OPACITY
    dead_idx, alive_idx = dead.nonzero(as_tuple=True)[0], (~dead).nonzero(as_tuple=True)[0]
    if dead_idx.numel() == 0:
        return
    sampled = alive_idx[torch.multinomial(o[alive_idx], dead_idx.numel(), replacement=True)]
    ratio = torch.bincount(sampled, minlength=o.numel())[sampled] + 1
    new_o, new_s = stock_new_values(t["opacity"][sampled], t["scaling"][sampled], ratio[:, None])
    for k in NAMES:
        t[k][dead_idx] = new_o if k == "opacity" else new_s if k == "scaling" else t[k][sampled]
    t["opacity"][sampled], t["scaling"][sampled] = new_o, new_s
    for m in moments:
        m[sampled] = 0


def stock_add_new(t, moments, m):
    o = torch.sigmoid(t["opacity"]).squeeze(1)
    sampled = torch.multinomial(o, m, replacement=True)
    ratio = torch.bincount(sampled, minlength=o.numel())[sampled] + 1
    new_o, new_s = stock_new_values(t["opacity"][sampled], t["scaling"][sampled], ratio[:, None])
    t["opacity"][sampled], t["scaling"][sampled] = new_o, new_s
    out = {k: torch.cat([t[k], t[k][sampled]]) for k in NAMES}
    return out, [torch.cat([x, torch.zeros((m,) + tuple(x.shape[1:]), device=x.device)]) for x in moments]


def _scene_and_optimizer(start, dev):
    from latentsplat_amd import GaussianScene
    scene = GaussianScene.from_tensors(**start).to(dev)
    opt = torch.optim.Adam([dict(params=[p], lr=1e-3, name=name) for name, p in scene.named_parameters()], eps=1e-15)
    for _, p in scene.named_parameters():
        opt.state[p] = dict(step=torch.tensor(1.0), exp_avg=torch.full_like(p, 0.5), exp_avg_sq=torch.full_like(p, 0.25))
    return scene, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "mcmc_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_mcmc needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import MCMCControl, _lib, inject_noise
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, calls_per_noise_sample=a.inner, sh_rest=SH_REST, dead_fraction=0.05, growth=1.05,
               noise_bytes_per_gaussian=NOISE_BYTES, achievable_bytes_per_s=ACHIEVABLE, device=torch.cuda.get_device_name(dev),
               baseline_note="the published trainer evaluates the new values in a kernel of its own; the baseline here uses the "
                             "closed form in torch, with as many terms as the largest ratio drawn")
    for n in a.sizes:
        entry = dict(n=n)
        # ---- noise ----
        t = make_tensors(n, dev, 0.05)
        eps = torch.randn((n, 3), device=dev)
        step_scale = 5e5 * 1.6e-4
        args = (t["opacity"], t["scaling"], t["rotation"], eps, step_scale)
        xyz = t["xyz"].clone()
        copies = max(2, math.ceil(1.1e9 / (NOISE_BYTES * n)))
        sets = [[x.clone() for x in (xyz, t["opacity"], t["scaling"], t["rotation"], eps)] for _ in range(copies)]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        calls = [lambda p=[C.c_void_p(x.data_ptr()) for x in one]: _lib.check(lib.lsr_mcmc_noise(n, *p, step_scale, stream), "lsr_mcmc_noise")
                 for one in sets]

        def rotating():
            for call in calls:
                call()
        stock = lambda: stock_noise(xyz, *args)
        for fn in (calls[0], rotating, stock):
            for _ in range(a.warmup):
                fn()
        warm, s = (_figures([_sample(fn, dev, a.inner) for _ in range(a.samples)]) for fn in (calls[0], stock))
        k = _figures([_sample(rotating, dev, 1) / copies for _ in range(a.samples)])
        rate, rate_warm = (NOISE_BYTES * n / (f["ms"] * 1e-3) for f in (k, warm))
        inject_noise(xyz, *args)                             # (the public wrapper runs the same launch)
        entry["noise"] = dict(kernel=k, kernel_warm=warm, stock=s, speedup=s["ms"] / k["ms"], bytes=NOISE_BYTES * n, copies=copies,
                              bytes_per_s=rate, fraction_of_achievable=rate / ACHIEVABLE, warm_fraction_of_achievable=rate_warm / ACHIEVABLE)
        print(f"n={n:8d} noise     rotating {_show(k)} {100 * rate / ACHIEVABLE:.0f} % of achievable  warm {_show(warm)} "
              f"{100 * rate_warm / ACHIEVABLE:.0f} %  stock {_show(s)}  x{s['ms'] / k['ms']:.1f}", flush=True)
        del xyz, eps, sets, calls
        torch.cuda.empty_cache()
        # ---- relocate: 5 % dead ----
        scene, opt = _scene_and_optimizer(t, dev)
        control = MCMCControl(scene, cap_max=int(1.05 * n), min_opacity=MIN_OPACITY)
        gen = torch.Generator(device=dev).manual_seed(1)
        restore = lambda: scene._opacity.data.copy_(t["opacity"])
        out = {}
        times = []
        for i in range(a.warmup + a.samples):
            ms = _sample(lambda: out.update(control.relocate(opt, gen)), dev, 1, restore)
            if i >= a.warmup:
                times.append(ms)
        k = _figures(times)
        work = {name: v.clone() for name, v in t.items()}
        moments = [torch.full_like(work[name], 0.5) for name in NAMES for _ in range(2)]
        restore = lambda: work["opacity"].copy_(t["opacity"])
        times = [_sample(lambda: stock_relocate(work, moments), dev, 1, restore) for _ in range(a.warmup + a.samples)][a.warmup:]
        s = _figures(times)
        entry["relocate"] = dict(kernel=k, stock=s, speedup=s["ms"] / k["ms"], dead=out["dead"], tables=18)
        print(f"n={n:8d} relocate  public {_show(k)}  stock {_show(s)}  x{s['ms'] / k['ms']:.1f}  ({out['dead']} dead)", flush=True)
        del work, moments, scene, opt, control
        torch.cuda.empty_cache()
        # ---- add_new: 5 % growth ----
        times = []
        for i in range(a.warmup + a.samples):
            scene, opt = _scene_and_optimizer(t, dev)
            control = MCMCControl(scene, cap_max=int(1.05 * n), min_opacity=MIN_OPACITY)
            ms = _sample(lambda: out.update(control.add_new(opt, gen)), dev, 1)
            if i >= a.warmup:
                times.append(ms)
            del scene, opt, control
        k = _figures(times)
        m = int(1.05 * n) - n
        times = []
        for i in range(a.warmup + a.samples):
            work = {name: v.clone() for name, v in t.items()}
            moments = [torch.full_like(work[name], 0.5) for name in NAMES for _ in range(2)]
            ms = _sample(lambda: stock_add_new(work, moments, m), dev, 1)
            if i >= a.warmup:
                times.append(ms)
            del work, moments
        s = _figures(times)
        entry["add_new"] = dict(kernel=k, stock=s, speedup=s["ms"] / k["ms"], added=out["added"], tables=18)
        print(f"n={n:8d} add_new   public {_show(k)}  stock {_show(s)}  x{s['ms'] / k['ms']:.1f}  ({out['added']} added)", flush=True)
        torch.cuda.empty_cache()
        # ---- the regulariser: forward + backward, plain torch ----
        scene, opt = _scene_and_optimizer(t, dev)
        control = MCMCControl(scene, cap_max=n)

        def reg():
            scene._opacity.grad = scene._scaling.grad = None
            control.regularizer().backward()
        for _ in range(a.warmup):
            reg()
        r = _figures([_sample(reg, dev, a.inner) for _ in range(a.samples)])
        entry["regularizer_forward_backward"] = r
        print(f"n={n:8d} regularizer forward + backward {_show(r)}", flush=True)
        res[f"n_{n}"] = entry
        del scene, opt, control, t
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
