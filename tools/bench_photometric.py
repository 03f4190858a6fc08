#!/usr/bin/env python
"""Device time of the photometric loss (`lsr_photometric_forward` / `_backward`, csrc/photometric.hip) against the
stock-PyTorch composition of the same loss, alternated in one process.

  fused   the forward (two launches: tiles, then the per-image sums) and the backward (one launch) through the C ABI into
          buffers allocated once; `fused_autograd_ms` is the public path on top of it (`photometric_loss` + `backward`,
          allocations and Python included)
  torch   what a 3DGS trainer writes by hand: five grouped 11 x 11 `conv2d` calls over x, y, x^2, y^2, xy, the SSIM map
          and the L1 term elementwise, autograd for the backward.  If the composition does not run on the device the
          entry says so (`torch_error`) and carries no number for it
  legs    forward: the loss value alone (no maps written); forward + backward: the forward that saves the three
          derivative maps, then the backward with a device-side upstream gradient
  shapes  16 x 3 x 256 x 256 (the headline render's views) and 4 x 3 x 1024 x 1024, lambda 0.2, uniform noise images

Each sample is `--inner` back-to-back calls between two device events, divided by their number; the figure is the median
of `--samples` (>= 20) after `--warmup` calls, the variants alternated sample by sample; `fused_first_half_ms` /
`_second_half_ms` and min / max say how far the kernel's own figure moved inside the run.  The byte model is what the
kernels must move per value (4 bytes each): the forward reads both images (8 B); the saving forward also writes three maps
(20 B); the backward reads the three maps and both images and writes the gradient (24 B).  The rate is that over the
time, as a fraction of the 6.3 TB/s achievable HBM rate of the MI355X (both shapes fit the 256 MiB Infinity Cache, so this
is a rate, not a claim about HBM).  `render_*_ms` is the rasterizer's own time for the headline shape's 16 views from
profiles/r06_bench.json (`path_step`), for scale.

usage: python tools/bench_photometric.py [--samples 30] [--warmup 5] [--inner 5] [--json [profiles/photometric_bench.json]]"""
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
SHAPES = ((16, 3, 256, 256), (4, 3, 1024, 1024))
LAMBDA = 0.2
HEADLINE = (16, 3, 256, 256)


def model_bytes(n: int) -> dict:
    return dict(forward=8 * n, forward_backward=(20 + 24) * n)


def torch_composition(x, y, window, lam=LAMBDA):
    import torch.nn.functional as F
    ch = x.shape[1]
    f = lambda t: F.conv2d(t, window, padding=5, groups=ch)
    mu1, mu2 = f(x), f(y)
    s1, s2, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return (1 - lam) * (x - y).abs().mean() + lam * (1 - ssim.mean())


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
        fused()
        if stock:
            stock()
    torch.cuda.synchronize(dev)
    tf, ts = [], []
    for _ in range(a.samples):
        tf.append(_sample(fused, dev, a.inner))
        if stock:
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
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "photometric_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_photometric needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    from latentsplat_amd.losses import photometric_loss
    dev = torch.device("cuda:0")
    lib = _lib.load()
    with open(os.path.join(ROOT, "profiles", "r06_bench.json")) as f:
        render = json.load(f)["path_step"]
    res = dict(lambda_dssim=LAMBDA, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner,
               hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.tensor([-(k - 5) ** 2 / (2 * 1.5 ** 2) for k in range(11)], dtype=torch.float64).exp()
    g = (g / g.sum()).float().to(dev)
    for shape in SHAPES:
        V, ch, H, W = shape
        n = V * ch * H * W
        gen = torch.Generator(device=dev).manual_seed(n)
        y = torch.rand(shape, device=dev, generator=gen)
        x = (y + 0.05 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1)
        window = (g[:, None] * g[None, :]).expand(ch, 1, 11, 11).contiguous()
        dims = _lib.PhotometricDims(num_images=V, channels=ch, height=H, width=W, lambda_dssim=LAMBDA, cov_norm=1.0, crop=0,
                                    reserved0=0)
        workspace = torch.empty(lib.lsr_photometric_workspace_bytes(C.byref(dims)), dtype=torch.uint8, device=dev)
        loss, up = torch.empty(1, device=dev), torch.ones(1, device=dev)
        saved, grad = torch.empty((3,) + shape, device=dev), torch.empty(shape, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def fused_fwd():
            _lib.check(lib.lsr_photometric_forward(C.byref(dims), p(x), p(y), p(workspace), p(loss), None, None, None, None, stream), "forward")

        def fused_fwd_bwd():
            _lib.check(lib.lsr_photometric_forward(C.byref(dims), p(x), p(y), p(workspace), p(loss), None, None, None, p(saved), stream), "forward")
            _lib.check(lib.lsr_photometric_backward(C.byref(dims), p(x), p(y), p(saved), p(up), p(grad), stream), "backward")

        leaf = x.clone().requires_grad_(True)

        def stock_fwd():
            with torch.no_grad():
                torch_composition(x, y, window)

        def stock_fwd_bwd():
            leaf.grad = None
            torch_composition(leaf, y, window).backward()

        def public_fwd_bwd():
            leaf.grad = None
            photometric_loss(leaf, y, LAMBDA).backward()

        nb = model_bytes(n)
        entry = dict(shape=list(shape), values=n, model_bytes=nb)
        fused_fwd_bwd()
        torch.cuda.synchronize(dev)
        try:                                         # the two compute the same thing, where the composition runs at all
            stock_fwd_bwd()
            with torch.no_grad():
                want = torch_composition(x, y, window)
            torch.cuda.synchronize(dev)
            entry["max_diff_vs_torch"] = dict(loss=float((loss[0] - want).abs()),
                                              grad_rel=float((grad - leaf.grad).abs().max() / leaf.grad.abs().max()))
            stock_ok = True
        except RuntimeError as e:
            entry["torch_error"] = f"{type(e).__name__}: {str(e).splitlines()[0][:300]}"
            stock_ok = False
            print(f"{shape}: the stock composition does not run here: {entry['torch_error']}", flush=True)
        for leg, fused, stock in (("forward", fused_fwd, stock_fwd), ("forward_backward", fused_fwd_bwd, stock_fwd_bwd)):
            tf, ts = _alternate(fused, stock if stock_ok else None, dev, a)
            mf = statistics.median(tf)
            half = len(tf) // 2
            rate = nb[leg] / (mf * 1e-3)
            e = dict(fused_ms=mf, fused_min_ms=min(tf), fused_max_ms=max(tf), fused_first_half_ms=statistics.median(tf[:half]),
                     fused_second_half_ms=statistics.median(tf[half:]), fused_bytes_per_s=rate,
                     fused_fraction_of_achievable_hbm=rate / HBM_ACHIEVABLE)
            line = (f"{shape} {leg:17s} fused {mf:7.4f} ms [{min(tf):.4f}, {max(tf):.4f}]  model {nb[leg] / 1e6:.1f} MB -> "
                    f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:.1f} % of 6.3 TB/s")
            if stock_ok:
                ms = statistics.median(ts)
                e.update(torch_ms=ms, torch_min_ms=min(ts), torch_max_ms=max(ts), speedup=ms / mf,
                         faster_than_torch_in_every_sample=bool(max(tf) < min(ts)))
                line += f"  torch {ms:8.4f} ms [{min(ts):.4f}, {max(ts):.4f}]  x{ms / mf:.1f}"
            if shape == HEADLINE:
                key = "forward_ms" if leg == "forward" else "forward_backward_ms"
                e.update(render_ms=render[key], fused_over_render=mf / render[key])
                if stock_ok:
                    e["torch_over_render"] = e["torch_ms"] / render[key]
                line += f"  render of the same 16 views {render[key]:.3f} ms"
            entry[leg] = e
            print(line, flush=True)
        entry["forward_backward"]["fused_autograd_ms"] = _median_of(public_fwd_bwd, dev, a)
        print(f"{shape} public path (photometric_loss + backward) {entry['forward_backward']['fused_autograd_ms']:.4f} ms", flush=True)
        if stock_ok:
            print(f"{shape} fused vs torch: " + ", ".join(f"{k} {v:.1e}" for k, v in entry["max_diff_vs_torch"].items()), flush=True)
        res["x".join(map(str, shape))] = entry
        del x, y, saved, grad, leaf
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
