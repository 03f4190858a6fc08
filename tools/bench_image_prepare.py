#!/usr/bin/env python
"""Device time of the image preparation (csrc/image_prepare.hip; include/lsr_image.h; latentsplat_amd.images) on the card it
runs on.

  prepare   `lsr_image_prepare` through the C ABI (one launch) into preallocated buffers
  stock     the stock composition in the same process: the sub-sample positions from elementwise torch operations,
            `F.grid_sample(bilinear, align_corners=False, padding_mode="border")` on the sub-sample grid, the coverage mask and
            `avg_pool2d` (tests/colmap_ref.py `stock_prepare`, the yardstick of the tests), uint8 -> float conversion included

Shapes: 16 x 1080 x 1920 x 3 -> 540 x 960 (PINHOLE, S = 2) and 4 x 3286 x 4946 x 3 -> 822 x 1236 (a quarter; PINHOLE and
OPENCV, S = 4), each with an off-centre principal point.  The pass must read every source byte once and write 16 bytes per
output pixel (three colour floats and the coverage): `bytes = 3 Hs Ws + 16 H W` per image, and `hbm_share` is that over the
time over the 6.3 TB/s achievable rate.  It is a byte-granular gather with 4 x C taps per sub-sample, so the share says how
far the gather is from a streaming copy, nothing more.

Every arm rotates over as many copies of its arrays as make more than the 256 MB last-level cache (at least two), each call on
the next copy; every timed shape is warmed up; every figure is the median of `--samples` (>= 20) samples with the smallest and
the largest beside it.

usage: python tools/bench_image_prepare.py [--samples 20] [--warmup 3] [--json [profiles/image_prepare_bench.json]]"""
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

CACHE_BYTES = 256e6
HBM_BYTES_PER_S = 6.3e12
# label, B, Hs, Ws, H, W, r, COLMAP model, parameters
SHAPES = (
    ("1080p_half_pinhole", 16, 1080, 1920, 540, 960, 2.0, 1, [1500.0, 1498.0, 967.3, 533.8]),
    ("16mp_quarter_pinhole", 4, 3286, 4946, 822, 1236, 4.0, 1, [4200.0, 4195.0, 2481.6, 1637.2]),
    ("16mp_quarter_opencv", 4, 3286, 4946, 822, 1236, 4.0, 4, [4200.0, 4195.0, 2481.6, 1637.2, -0.04, 0.01, 0.0005, -0.0003]),
)


def _sample(fn, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end)


def _figures(t):
    med = statistics.median(t)
    return dict(ms=med, min_ms=min(t), max_ms=max(t), samples=len(t), spread=(max(t) - min(t)) / med)


def _show(f):
    return f"{f['ms']:8.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]"


def bench_shape(shape, dev, a, lib):
    from latentsplat_amd import _lib
    from latentsplat_amd.images import SourceCamera
    from tests.colmap_ref import camera_numbers, stock_prepare, subsamples
    label, B, Hs, Ws, H, W, r, model, params = shape
    camera = SourceCamera.from_colmap(model, params)
    cam = camera_numbers(model, params)
    fxo, fyo = cam["fx"] / r, cam["fy"] / r
    nbytes = B * (3 * Hs * Ws + 16 * H * W)
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / nbytes))
    gen = torch.Generator(device=dev).manual_seed(B * Hs)
    src = [torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(copies)]
    image = [torch.empty((B, 3, H, W), device=dev) for _ in range(copies)]
    cover = [torch.empty((B, H, W), device=dev) for _ in range(copies)]
    dims = _lib.ImageDims(batch=B, src_height=Hs, src_width=Ws, channels=3, height=H, width=W, fx=fxo, fy=fyo)
    cs = camera.struct()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())

    def mine():
        for s, i, c in zip(src, image, cover):
            _lib.check(lib.lsr_image_prepare(C.byref(dims), C.byref(cs), P(s), None, P(i), P(c), stream), "lsr_image_prepare")

    at = [0]

    def stock():
        at[0] = (at[0] + 1) % copies
        return stock_prepare(src[at[0]], cam, H, W, fxo, fyo)

    res = dict(label=label, batch=B, src=[Hs, Ws], out=[H, W], model=_lib.COLMAP_MODELS[model][0], subsamples=subsamples(cam, fxo, fyo),
               copies=copies, bytes=nbytes)
    for name, fn, per in (("prepare", mine, copies), ("stock", stock, 1)):
        for _ in range(a.warmup):
            fn()
        res[name] = _figures([_sample(fn, dev) / per for _ in range(a.samples)])
    theirs = stock_prepare(src[0], cam, H, W, fxo, fyo)
    mine()
    torch.cuda.synchronize(dev)
    res.update(speedup=res["stock"]["ms"] / res["prepare"]["ms"], bytes_per_s=nbytes / (res["prepare"]["ms"] * 1e-3),
               max_abs_difference_from_stock=float((image[0] - theirs[0]).abs().max()),
               coverage_disagreements=int((cover[0] != theirs[1]).sum()))
    res["hbm_share"] = res["bytes_per_s"] / HBM_BYTES_PER_S
    print(f"{label:22s} S={res['subsamples']}  prepare {_show(res['prepare'])}  stock {_show(res['stock'])}  x{res['speedup']:.1f}  "
          f"{res['bytes_per_s'] / 1e12:.3f} TB/s = {100 * res['hbm_share']:.1f} % of {HBM_BYTES_PER_S / 1e12} TB/s  "
          f"(max |difference| from stock {res['max_abs_difference_from_stock']:.2e})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "image_prepare_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_image_prepare needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               hbm_bytes_per_s=HBM_BYTES_PER_S, bytes_note="3 Hs Ws + 16 H W per image: every source byte once, 16 bytes per output pixel",
               baseline_note="the stock arm is grid_sample on the sub-sample grid plus avg_pool2d, with the uint8 -> float conversion")
    for shape in SHAPES:
        res[shape[0]] = bench_shape(shape, dev, a, lib)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
