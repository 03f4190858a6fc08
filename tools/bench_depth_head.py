#!/usr/bin/env python
"""Depth head of the encoder: the fused HIP path against a stock-PyTorch composition of the same math, alternated in
one process.

  fused   latentsplat_amd.depth_head.depth_head: one launch forward (logits -> depth, opacity, index), one backward
  torch   what a user of the reference runs behind the head's Linear (depth_predictor_monocular.py:52-81,
          discrete_probability_distribution.py:7-20, conversions.py:5-14, encoder_epipolar.py:113-126,190): strided
          split of the channels, softmax, sigmoid, sum and divide, cumsum, searchsorted, gathers, the relative-disparity
          arithmetic, the opacity map — and autograd's backward.  Both variants are handed the same uniforms, so the
          random generator is outside both timings.
  shape   the encoder's (config/model/encoder/epipolar.yaml:11-16): 2 context views x 65 536 rays, 32 buckets, 1 surface,
          3 samples per scene; 1 scene and 4 scenes; opacity exponent 2 ** 0.5, scale 1 / 3

Times are device events around `steps` calls (median over `rounds`, the two variants alternated, both warmed up first).
The byte model is the traffic the math needs per (row, surface): forward 4 * 2 S F read + 12 k written; backward
4 * 2 S F read and written + 12 k read (the indices and the two upstream gradients).  The rate is that over the time, as
a fraction of the 6.3 TB/s achievable HBM rate of the MI355X.

usage: python tools/bench_depth_head.py [--steps 50] [--rounds 7] [--json [profiles/depth_head_bench.json]]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12     # bytes / s
RAYS, S, F, K = 65536, 32, 1, 3
EXPONENT, SCALE = 2 ** 0.5, 1 / 3
EPS = torch.finfo(torch.float32).eps


def bytes_forward(rows):
    return rows * F * (4 * 2 * S + 12 * K)


def bytes_backward(rows):
    return rows * F * (2 * 4 * 2 * S + 12 * K)


def _time(fn, steps, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / steps


def torch_composition(logits, near, far, uniforms):
    """logits (cams, rays, 2 S F), near / far (cams,), uniforms (cams, rays, F, k) -> depth, opacity (cams, rays, F, k)."""
    x = logits.reshape(*logits.shape[:-1], S, F, 2)
    pdf = x[..., 0].transpose(-1, -2).softmax(dim=-1)
    offset = x[..., 1].transpose(-1, -2).sigmoid()
    normalized = pdf / (EPS + pdf.sum(dim=-1, keepdim=True))
    cdf = normalized.cumsum(dim=-1)
    index = torch.searchsorted(cdf, uniforms, right=True).clip(max=S - 1)
    density = normalized.gather(dim=-1, index=index)
    relative_disparity = (index + offset.gather(dim=-1, index=index)) / S
    near, far = near[:, None, None, None], far[:, None, None, None]
    disp_near, disp_far = 1 / (near + 1e-10), 1 / (far + 1e-10)
    depth = 1 / ((1 - relative_disparity) * (disp_near - disp_far) + disp_far + 1e-10)
    opacity = 0.5 * (1 - (1 - density) ** EXPONENT + density ** (1 / EXPONENT)) * SCALE
    return depth, opacity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "depth_head_bench.json"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_depth_head needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.depth_head import depth_head
    dev = torch.device("cuda:0")
    res = {}
    for scenes in (1, 4):
        cams = 2 * scenes
        gen = torch.Generator(device=dev).manual_seed(scenes)
        logits = (2 * torch.randn((cams, RAYS, 2 * S * F), device=dev, generator=gen)).requires_grad_()
        near = 0.5 + torch.rand((cams,), device=dev, generator=gen)
        far = near + 2 + 5 * torch.rand((cams,), device=dev, generator=gen)
        uniforms = torch.rand((cams, RAYS, F, K), device=dev, generator=gen)
        gd = torch.randn((cams, RAYS, F, K), device=dev, generator=gen)
        go = torch.randn((cams, RAYS, F, K), device=dev, generator=gen)

        def fused(backward):
            depth, opacity, _ = depth_head(logits, near, far, num_surfaces=F, uniforms=uniforms,
                                           opacity_exponent=EXPONENT, opacity_scale=SCALE)
            if backward:
                logits.grad = None
                torch.autograd.backward([depth, opacity], [gd, go])
            return depth, opacity

        def stock(backward):
            depth, opacity = torch_composition(logits, near, far, uniforms)
            if backward:
                logits.grad = None
                torch.autograd.backward([depth, opacity], [gd, go])
            return depth, opacity

        # same results (and warm-up of both variants)
        with torch.no_grad():
            df, of = fused(False)
            ds, os_ = stock(False)
            same = (df - ds).abs() <= 1e-4 * ds.abs()         # (a sample on a cumulative-sum edge may pick the neighbour)
            moved = float(1 - same.float().mean())
            diff = float(((of - os_).abs() * same).max())
        fused(True); g_fused = logits.grad.clone()
        stock(True); g_stock = logits.grad.clone()
        rows_same = same.all(-1).all(-1)
        gdiff = float((g_fused - g_stock)[rows_same].abs().max() / g_stock.abs().max())
        del df, of, ds, os_, g_fused, g_stock, same, rows_same
        rows = cams * RAYS
        nb_f, nb_fb = bytes_forward(rows), bytes_forward(rows) + bytes_backward(rows)
        entry = dict(cameras=cams, rows=rows, buckets=S, surfaces=F, samples=K, bytes_forward=nb_f,
                     bytes_forward_backward=nb_fb, share_of_samples_on_another_bucket=moved,
                     max_abs_diff_opacity=diff, max_rel_diff_grad=gdiff)
        for what, backward, nbytes in (("forward", False, nb_f), ("forward_backward", True, nb_fb)):
            tf, ts = [], []
            for _ in range(a.rounds):                      # alternated
                if backward:
                    tf.append(_time(lambda: fused(True), a.steps, dev))
                    ts.append(_time(lambda: stock(True), a.steps, dev))
                else:
                    with torch.no_grad():
                        tf.append(_time(lambda: fused(False), a.steps, dev))
                        ts.append(_time(lambda: stock(False), a.steps, dev))
            mf, ms = statistics.median(tf), statistics.median(ts)
            spread = max(max(ts) - min(ts), max(tf) - min(tf))
            entry[what] = dict(fused_ms=mf, torch_ms=ms, speedup=ms / mf, fused_all=tf, torch_all=ts,
                               torch_spread_ms=max(ts) - min(ts), fused_spread_ms=max(tf) - min(tf),
                               faster_by_more_than_the_spread=bool(ms - mf > spread),
                               fused_bytes_per_s=nbytes / (mf * 1e-3),
                               fused_fraction_of_achievable_hbm=nbytes / (mf * 1e-3) / HBM_ACHIEVABLE)
            e = entry[what]
            print(f"scenes={scenes} {what:17s} fused {mf:8.4f} ms  torch {ms:8.4f} ms  x{e['speedup']:.2f}  "
                  f"(spread fused {e['fused_spread_ms']:.4f} / torch {e['torch_spread_ms']:.4f} ms)  model {nbytes / 1e6:.1f} MB -> "
                  f"{e['fused_bytes_per_s'] / 1e12:.2f} TB/s = {100 * e['fused_fraction_of_achievable_hbm']:.1f} % of 6.3 TB/s",
                  flush=True)
        print(f"scenes={scenes} fused vs torch: opacity max |diff| {diff:.2e}, gradient max rel diff {gdiff:.2e}, "
              f"samples on another bucket {moved:.2e}", flush=True)
        res[f"encoder_{scenes}_scene" + ("s" if scenes > 1 else "")] = entry
        del logits, uniforms, gd, go
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
