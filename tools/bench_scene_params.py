#!/usr/bin/env python
"""Device time of the 3DGS activation map (`lsr_scene_activate_forward` / `_backward`, csrc/scene_params.hip) against the
stock-PyTorch composition of the same outputs, alternated in one process.

  fused   one launch forward, one backward, through the C ABI into buffers allocated once (`fused_autograd_ms` is the
          public path on top of it: `activate_scene` + `torch.autograd.backward`, allocations and Python included)
  torch   what a scene optimiser writes by hand: `torch.cat` of f_dc and f_rest, `sigmoid`, `exp`, the normalise and the
          `rasterizer._covariance_from_scale_rotation` formula; autograd for the backward
  legs    forward under `no_grad`; forward + backward with upstream gradients on all three outputs
  shape   degree 3 (K = 16) at n = 393 216 (the encoder-shaped cloud) and n = 3 000 000 (a trained scene)

Each sample is `--inner` back-to-back calls between two device events, divided by their number; the figure is the median
of `--samples` (>= 20) after `--warmup` calls, the variants alternated sample by sample.  The byte model is what the math
must move per Gaussian: the forward reads (3 K + 8) * 4 and writes (3 K + 7) * 4 bytes, the backward reads (3 K + 7 + 8) * 4
and writes (3 K + 8) * 4; the rate is that over the time, as a fraction of the 6.3 TB/s achievable HBM rate of the
MI355X.  `fused_*_first_half_ms` / `_second_half_ms` (the medians of the two halves of the samples) and min / max say
how far the kernel's own figure moved inside the run.

usage: python tools/bench_scene_params.py [--samples 30] [--warmup 5] [--inner 5] [--json [profiles/scene_params_bench.json]]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12     # bytes / s
K = 16
SIZES = (393_216, 3_000_000)


def model_bytes(n: int, k: int) -> dict:
    fwd = n * 4 * ((3 * k + 8) + (3 * k + 7))
    bwd = n * 4 * ((3 * k + 7 + 8) + (3 * k + 8))
    return dict(forward=fwd, forward_backward=fwd + bwd)


def torch_composition(dc, rest, opacity, scaling, rotation, m=1.0):
    from latentsplat_amd.rasterizer import _covariance_from_scale_rotation
    shs = torch.cat([dc, rest], dim=1)
    return shs, torch.sigmoid(opacity), _covariance_from_scale_rotation(torch.exp(scaling), rotation, m)


def _sample(fn, dev, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def _alternate(fused, stock, dev, a):
    for _ in range(a.warmup):
        fused(); stock()
    torch.cuda.synchronize(dev)
    tf, ts = [], []
    for _ in range(a.samples):
        tf.append(_sample(fused, dev, a.inner))
        ts.append(_sample(stock, dev, a.inner))
    return tf, ts


def _median_of(fn, dev, a):
    for _ in range(a.warmup):
        fn()
    return statistics.median(_sample(fn, dev, a.inner) for _ in range(a.samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "scene_params_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_scene_params needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    from latentsplat_amd.scene_model import activate_scene
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(sh_coeffs=K, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
    p = lambda t: C.c_void_p(t.data_ptr())
    for n in SIZES:
        gen = torch.Generator(device=dev).manual_seed(n)
        r = lambda *s: torch.randn(s, device=dev, generator=gen)
        params = [r(n, 1, 3), r(n, K - 1, 3), 3 * r(n, 1), 2 * r(n, 3) - 3, r(n, 4)]
        ups = [r(n, K, 3), r(n, 1), r(n, 6)]
        outs = [torch.empty_like(u) for u in ups]
        grads = [torch.empty_like(t) for t in params]
        dims = _lib.SceneDims(n=n, sh_coeffs=K, scale_modifier=1.0, reserved0=0, reserved1=0)
        c_params, c_outs = _lib.SceneParams(*map(p, params)), _lib.SceneOutputs(p(outs[0]), p(outs[1]), p(outs[2]), None, None)
        c_ups, c_grads = _lib.SceneOutGrads(*map(p, ups)), _lib.SceneInGrads(*map(p, grads))
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def fused_fwd():
            _lib.check(lib.lsr_scene_activate_forward(C.byref(dims), C.byref(c_params), C.byref(c_outs), stream), "forward")

        def fused_fwd_bwd():
            fused_fwd()
            _lib.check(lib.lsr_scene_activate_backward(C.byref(dims), C.byref(c_params), C.byref(c_ups), C.byref(c_grads), stream), "backward")

        leaves = [t.clone().requires_grad_(True) for t in params]

        def stock_fwd():
            with torch.no_grad():
                torch_composition(*params)

        def stock_fwd_bwd():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(torch_composition(*leaves), ups)

        def public_fwd_bwd():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(activate_scene(*leaves), ups)

        # the two compute the same thing
        fused_fwd_bwd(); stock_fwd_bwd()
        with torch.no_grad():
            want = torch_composition(*params)
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
        diff = dict(shs=rel(outs[0], want[0]), opacities=rel(outs[1], want[1]), cov3D=rel(outs[2], want[2]),
                    **{f"d_{k}": rel(g, t.grad) for k, g, t in zip(("features_dc", "features_rest", "opacity", "scaling", "rotation"), grads, leaves)})
        del want
        nb = model_bytes(n, K)
        entry = dict(n=n, model_bytes=nb, max_rel_diff_vs_torch=diff)
        for leg, fused, stock in (("forward", fused_fwd, stock_fwd), ("forward_backward", fused_fwd_bwd, stock_fwd_bwd)):
            tf, ts = _alternate(fused, stock, dev, a)
            mf, ms = statistics.median(tf), statistics.median(ts)
            half = len(tf) // 2
            rate = nb[leg] / (mf * 1e-3)
            entry[leg] = dict(fused_ms=mf, torch_ms=ms, speedup=ms / mf, fused_min_ms=min(tf), fused_max_ms=max(tf),
                              fused_first_half_ms=statistics.median(tf[:half]), fused_second_half_ms=statistics.median(tf[half:]),
                              torch_min_ms=min(ts), torch_max_ms=max(ts), fused_bytes_per_s=rate,
                              fused_fraction_of_achievable_hbm=rate / HBM_ACHIEVABLE,
                              faster_than_torch_in_every_sample=bool(max(tf) < min(ts)))
            print(f"n={n:8d} {leg:17s} fused {mf:7.4f} ms [{min(tf):.4f}, {max(tf):.4f}]  torch {ms:8.4f} ms [{min(ts):.4f}, {max(ts):.4f}]  "
                  f"x{ms / mf:.1f}  model {nb[leg] / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:.1f} % of 6.3 TB/s", flush=True)
        entry["forward_backward"]["fused_autograd_ms"] = _median_of(public_fwd_bwd, dev, a)
        print(f"n={n:8d} public path (activate_scene + autograd.backward) {entry['forward_backward']['fused_autograd_ms']:.4f} ms", flush=True)
        print(f"n={n:8d} fused vs torch, max relative difference: " + ", ".join(f"{k} {v:.1e}" for k, v in diff.items()), flush=True)
        res[f"n_{n}"] = entry
        del params, ups, outs, grads, leaves
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
