#!/usr/bin/env python
"""Device time of the bilateral-grid operator (csrc/bilagrid.hip, include/lsr_bilagrid.h, latentsplat_amd.bilagrid) on the
card it runs on.

  hip          `lsr_bilagrid_slice_forward`, and forward + `lsr_bilagrid_slice_backward`, through the C ABI into buffers
               allocated once
  stock        the stock composition in the same process: a 5-D `F.grid_sample` of `grids[idx]` (bilinear, border,
               align_corners) and an einsum, and with autograd in the grids and the image
  photometric  `lsr_photometric_forward` (saving) and forward + `lsr_photometric_backward` on the same images at lambda 0.2:
               the loss the operator precedes, measured in the same run
  tv           `lsr_bilagrid_tv_forward` + `lsr_bilagrid_tv_backward` of all the grids

Shapes: 16 x 3 x 256 x 256 and 4 x 3 x 1024 x 1024 images; 200 grids of 16 x 16 x 8 (the published size) and of 1 x 1 x 1 (one
affine per image); the views of a call take consecutive grids, the next call the next ones.  Every arm rotates over as many
copies of its image-sized arrays as make more than the 256 MB last-level cache even for the forward alone, which touches 24
bytes per pixel (at least two copies), each call on the next copy;
every timed shape is warmed up; every figure is the median of `--samples` (>= 20) samples with the smallest and the largest
beside it.  Each hip figure is also given as a fraction of the photometric one and as a multiple of the time HBM needs for the
bytes that must move (24 B per pixel forward, 48 more backward, at 6.3 TB/s).

usage: python tools/bench_bilateral_grid.py [--samples 20] [--warmup 3] [--json [profiles/bilateral_grid_bench.json]]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGES = ((16, 256, 256), (4, 1024, 1024))
GRIDS = ((8, 16, 16), (1, 1, 1))             # (L, Y, X)
NUM_GRIDS = 200
CACHE_BYTES = 256e6
HBM_BYTES_PER_S = 6.3e12
FWD_BYTES, BWD_BYTES = 24, 48                # per pixel: image read, out written; image and grad_out read, grad_image written (and image re-read)
LAMBDA = 0.2


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


def stock_slice(grids, image, idx):
    V, _, H, W = image.shape
    x = ((torch.arange(W, device=image.device, dtype=image.dtype) + 0.5) / W)[None, None, :].expand(V, H, W)
    y = ((torch.arange(H, device=image.device, dtype=image.dtype) + 0.5) / H)[None, :, None].expand(V, H, W)
    luma = 0.299 * image[:, 0] + 0.587 * image[:, 1] + 0.114 * image[:, 2]
    coords = torch.stack((x, y, luma), -1)[:, None] * 2 - 1
    A = F.grid_sample(grids[idx.long()], coords, mode="bilinear", padding_mode="border", align_corners=True)
    A = A.reshape(V, 3, 4, H, W)
    return torch.einsum("vrkhw,vkhw->vrhw", A[:, :, :3], image) + A[:, :, 3]


def bench(shape, grid, dev, a, lib):
    from latentsplat_amd import _lib
    V, H, W = shape
    L, Y, X = grid
    pixels = V * H * W
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (pixels * FWD_BYTES)))     # sized for the forward arm, which moves the fewest bytes
    gen = torch.Generator(device=dev).manual_seed(pixels + L)
    grids = torch.eye(3, 4, device=dev).reshape(1, 12, 1, 1, 1) + 0.3 * torch.randn((NUM_GRIDS, 12, L, Y, X), device=dev, generator=gen)
    grad_grids = torch.empty_like(grids)
    sets = []
    for k in range(copies):
        image = torch.rand((V, 3, H, W), device=dev, generator=gen)
        # smooth luminance, as a photograph has: a low-resolution field upsampled, plus a little noise
        smooth = F.interpolate(torch.rand((V, 3, H // 16, W // 16), device=dev, generator=gen), size=(H, W), mode="bilinear", align_corners=False)
        image = (0.9 * smooth + 0.1 * image).contiguous()
        idx = ((torch.arange(V, device=dev) + k * V) % NUM_GRIDS).to(torch.int32)
        sets.append(dict(image=image, idx=idx, target=torch.rand((V, 3, H, W), device=dev, generator=gen), out=torch.empty_like(image),
                         grad_out=torch.randn((V, 3, H, W), device=dev, generator=gen), grad_image=torch.empty_like(image),
                         saved=torch.empty((3, V, 3, H, W), device=dev)))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    dims = _lib.BilagridDims(num_views=V, height=H, width=W, num_grids=NUM_GRIDS, grid_l=L, grid_y=Y, grid_x=X, reserved0=0)
    pdims = _lib.PhotometricDims(num_images=V, channels=3, height=H, width=W, lambda_dssim=LAMBDA, cov_norm=1.0, crop=0, reserved0=0)
    pws = torch.empty(max(lib.lsr_photometric_workspace_bytes(C.byref(pdims)), 16), dtype=torch.uint8, device=dev)
    tws = torch.empty(max(lib.lsr_bilagrid_tv_workspace_bytes(C.byref(dims)), 16), dtype=torch.uint8, device=dev)
    loss, one, tv = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty(1, device=dev)

    def hip(backward):
        def run():
            for s in sets:
                _lib.check(lib.lsr_bilagrid_slice_forward(C.byref(dims), P(grids), P(s["image"]), P(s["idx"]), P(s["out"]), stream), "fwd")
                if backward:
                    _lib.check(lib.lsr_bilagrid_slice_backward(C.byref(dims), P(grids), P(s["image"]), P(s["idx"]), P(s["grad_out"]),
                                                               P(s["grad_image"]), P(grad_grids), stream), "bwd")
        return run

    def photo(backward):
        def run():
            for s in sets:
                _lib.check(lib.lsr_photometric_forward(C.byref(pdims), P(s["image"]), P(s["target"]), P(pws), P(loss), None, None, None,
                                                       P(s["saved"]), stream), "photometric fwd")
                if backward:
                    _lib.check(lib.lsr_photometric_backward(C.byref(pdims), P(s["image"]), P(s["target"]), P(s["saved"]), P(one),
                                                            P(s["grad_image"]), stream), "photometric bwd")
        return run

    def total_variation():
        _lib.check(lib.lsr_bilagrid_tv_forward(C.byref(dims), P(grids), P(tws), P(tv), stream), "tv fwd")
        _lib.check(lib.lsr_bilagrid_tv_backward(C.byref(dims), P(grids), P(one), P(grad_grids), stream), "tv bwd")

    turn = [0]

    def stock(backward):
        def run():
            turn[0] = (turn[0] + 1) % copies
            s = sets[turn[0]]
            if not backward:
                with torch.no_grad():
                    return stock_slice(grids, s["image"], s["idx"])
            g, x = grids.detach().requires_grad_(True), s["image"].detach().requires_grad_(True)
            stock_slice(g, x, s["idx"]).backward(s["grad_out"])
        return run

    res = dict(views=V, height=H, width=W, grid=dict(l=L, y=Y, x=X), num_grids=NUM_GRIDS, copies=copies,
               path=lib.lsr_bilagrid_slice_path(C.byref(dims)))
    arms = (("hip_forward", hip(False), copies), ("hip_forward_backward", hip(True), copies), ("photometric_forward", photo(False), copies),
            ("photometric_forward_backward", photo(True), copies), ("stock_forward", stock(False), 1), ("stock_forward_backward", stock(True), 1),
            ("tv_forward_backward", total_variation, 1))
    for name, fn, per in arms:
        for _ in range(a.warmup):
            fn()
        res[name] = _figures([_sample(fn, dev) / per for _ in range(a.samples)])
    for what, nbytes in (("forward", FWD_BYTES), ("forward_backward", FWD_BYTES + BWD_BYTES)):
        f = res["hip_" + what]
        f["of_photometric"] = f["ms"] / res["photometric_" + what]["ms"]
        f["hbm_ms"] = 1e3 * nbytes * pixels / HBM_BYTES_PER_S
        f["times_hbm"] = f["ms"] / f["hbm_ms"]
        f["speedup_over_stock"] = res["stock_" + what]["ms"] / f["ms"]
    # the two agree
    s = sets[0]
    lib.lsr_bilagrid_slice_forward(C.byref(dims), P(grids), P(s["image"]), P(s["idx"]), P(s["out"]), stream)
    res["max_abs_difference_from_stock"] = float((s["out"] - stock_slice(grids, s["image"], s["idx"])).abs().max())
    print(f"{V}x3x{H}x{W} grid {X}x{Y}x{L} path {res['path']}: forward {_show(res['hip_forward'])} (stock {_show(res['stock_forward'])}, "
          f"photometric {_show(res['photometric_forward'])}, x{res['hip_forward']['times_hbm']:.1f} HBM)\n"
          f"    forward+backward {_show(res['hip_forward_backward'])} (stock {_show(res['stock_forward_backward'])}, photometric "
          f"{_show(res['photometric_forward_backward'])}, {res['hip_forward_backward']['of_photometric']:.2f} of it, "
          f"x{res['hip_forward_backward']['times_hbm']:.1f} HBM)  tv {_show(res['tv_forward_backward'])}  "
          f"differs from stock by {res['max_abs_difference_from_stock']:.2e}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "bilateral_grid_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_bilateral_grid needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               hbm_bytes_per_s=HBM_BYTES_PER_S, bytes_per_pixel=dict(forward=FWD_BYTES, backward=BWD_BYTES), lambda_dssim=LAMBDA,
               baseline_note="stock: F.grid_sample of grids[idx] (5-D, bilinear, border, align_corners=True) and an einsum, autograd for "
                             "the gradients; photometric: lsr_photometric_forward (saving) / _backward on the same images",
               results=[])
    for shape in IMAGES:
        for grid in GRIDS:
            res["results"].append(bench(shape, grid, dev, a, lib))
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
