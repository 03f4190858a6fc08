#!/usr/bin/env python
"""Device time of the 3D smoothing filter (csrc/filter3d.hip, csrc/scene_params.hip; include/lsr_filter3d.h,
include/lsr_scene.h; latentsplat_amd.filter3d) on the card it runs on.

  pass         `lsr_filter3d_compute` through the C ABI (three launches) into preallocated buffers, both modes, against
               the stock-PyTorch composition of the published per-camera loop (a Python loop over the cameras, about
               fifteen elementwise launches and two masked updates each) in the same process.  The pass reads 12 bytes
               and writes 4 per Gaussian whatever the number of cameras, so it is bound by its vector instructions: the
               figure given is (Gaussian, camera) pairs per second
  activation   `lsr_scene_activate_filtered_forward` and forward + backward against the UNFILTERED kernels timed in the
               same run, samples alternating between the two, at SH degree 3, writing shs, opacities and cov3D (what a
               render takes).  The filtered map moves 4 bytes per Gaussian more each way; `byte_ratio` is that, `ratio`
               the measured one, `spread` the (max - min) / median of each arm in this run

Sizes: 393 216 Gaussians x 100 cameras and 3 000 000 x 200.  Every arm rotates over as many copies of its arrays as make
more than the 256 MB last-level cache (at least two), each call on the next copy; every timed shape is warmed up; every
figure is the median of `--samples` (>= 20) samples with the smallest and the largest beside it.

usage: python tools/bench_filter3d.py [--samples 20] [--warmup 3] [--json [profiles/filter3d_bench.json]]"""
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

SIZES = ((393_216, 100), (3_000_000, 200))
SH_COEFFS = 16
WIDTH = 1024
CACHE_BYTES = 256e6
PASS_BYTES = 16                  # xyz read, filter written
FWD_BYTES = 4 * ((3 * SH_COEFFS + 8) + (3 * SH_COEFFS + 7))        # parameters read; shs, opacities, cov3D written
BWD_BYTES = 4 * ((3 * SH_COEFFS + 7) + 8 + (3 * SH_COEFFS + 8))     # upstream read, opacity / scaling / rotation read, gradients written


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


def _copies(bytes_per_copy):
    return max(2, math.ceil(1.2 * CACHE_BYTES / bytes_per_copy))


def circle_table(V, dev):
    """V cameras on a circle of radius 4 around the origin looking at it, tanfov 0.5: a (V, 44) view table."""
    from latentsplat_amd.rasterizer import build_view_table
    ang = torch.arange(V, dtype=torch.float32) * (2 * math.pi / V)
    zero, one = torch.zeros_like(ang), torch.ones_like(ang)
    offset = torch.stack([torch.cos(ang), zero, torch.sin(ang)], -1)
    down = torch.stack([zero, one, zero], -1)
    ext = torch.zeros((V, 4, 4))
    ext[:, :3, 0], ext[:, :3, 1], ext[:, :3, 2] = torch.linalg.cross(down, -offset), down, -offset
    ext[:, :3, 3] = 4.0 * offset
    ext[:, 3, 3] = 1
    intr = torch.tensor([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1.0]]).repeat(V, 1, 1)
    near, far = torch.full((V,), 0.1), torch.full((V,), 100.0)
    return build_view_table(ext.to(dev), intr.to(dev), near.to(dev), far.to(dev), torch.zeros(3, device=dev), scale_invariant=False)


def stock_filter(xyz, cams, width, height):
    """The published per-camera loop, composed of stock PyTorch operations: `cams` is a list of (R (3, 3), T (3,), focal_x,
    focal_y) with p = xyz @ R + T."""
    distance = torch.full((xyz.shape[0],), 100000.0, device=xyz.device)
    valid_points = torch.zeros(xyz.shape[0], dtype=torch.bool, device=xyz.device)
    focal_length = 0.0
    for R, T, fx, fy in cams:
        p = xyz @ R + T[None, :]
        valid_depth = p[:, 2] > 0.2
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * fx + width / 2.0
        y = y / z * fy + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15),
                                      torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        focal_length = max(focal_length, fx)
    distance[~valid_points] = distance[valid_points].max()
    return distance / focal_length * (0.2 ** 0.5)


def bench_pass(n, V, dev, a, lib):
    from latentsplat_amd import _lib, compute_filter_3d
    views = circle_table(V, dev)
    gen = torch.Generator(device=dev).manual_seed(n)
    copies = _copies(PASS_BYTES * n)
    xyz = [(torch.rand((n, 3), device=dev, generator=gen) * 6.0 - 3.0) for _ in range(copies)]
    out = [torch.empty((n, 1), device=dev) for _ in range(copies)]
    ws = torch.empty(lib.lsr_filter3d_workspace_bytes(n, V), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())

    def arm(mode):
        def run():
            for x, o in zip(xyz, out):
                _lib.check(lib.lsr_filter3d_compute(n, P(x), V, P(views), WIDTH, 0.15, 0.2, mode, P(o), None, P(ws), stream),
                           "lsr_filter3d_compute")
        return run

    table = views.cpu()
    cams = [(table[v, :16].reshape(4, 4)[:3, :3].contiguous().to(dev), table[v, 12:15].contiguous().to(dev),
             WIDTH / (2 * float(table[v, 35])), WIDTH / (2 * float(table[v, 36]))) for v in range(V)]
    stock_i = [0]

    def stock():
        stock_i[0] = (stock_i[0] + 1) % copies
        return stock_filter(xyz[stock_i[0]], cams, WIDTH, WIDTH)

    res = {}
    for name, fn, per in (("published", arm(_lib.FILTER3D_PUBLISHED), copies), ("per_view", arm(_lib.FILTER3D_PER_VIEW), copies),
                          ("stock", stock, 1)):
        for _ in range(a.warmup):
            fn()
        res[name] = _figures([_sample(fn, dev) / per for _ in range(a.samples)])
    # the two agree (equal focal lengths here; the stock loop clamps and divides where the kernel does not)
    mine = compute_filter_3d(xyz[0], views, WIDTH)[:, 0]
    theirs = stock_filter(xyz[0], cams, WIDTH, WIDTH)
    agree = float(((mine - theirs).abs() <= 1e-5 * theirs.abs()).float().mean())
    pairs = n * V / (res["published"]["ms"] * 1e-3)
    res.update(n=n, views=V, copies=copies, pairs_per_s=pairs, speedup=res["stock"]["ms"] / res["published"]["ms"],
               fraction_agreeing_with_stock=agree)
    print(f"n={n:8d} V={V:3d} pass  published {_show(res['published'])}  per_view {_show(res['per_view'])}  stock {_show(res['stock'])}  "
          f"x{res['speedup']:.0f}  {pairs / 1e9:.1f} G pairs/s  agree {100 * agree:.2f} %", flush=True)
    return res


def bench_activation(n, dev, a, lib):
    from latentsplat_amd import _lib
    K = SH_COEFFS
    copies = _copies((FWD_BYTES + BWD_BYTES) * n)
    gen = torch.Generator(device=dev).manual_seed(n + 1)
    r = lambda *s: torch.randn(s, device=dev, generator=gen)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    dims = _lib.SceneDims(n=n, sh_coeffs=K, scale_modifier=1.0, reserved0=0, reserved1=0)
    sets = []
    for _ in range(copies):
        p = dict(dc=r(n, 1, 3), rest=r(n, K - 1, 3), opacity=r(n, 1), scaling=torch.rand((n, 3), device=dev, generator=gen) * 4.0 - 6.0,
                 rotation=r(n, 4), filt=torch.exp(torch.rand((n,), device=dev, generator=gen) * 6.0 - 8.0))
        outs = dict(shs=torch.empty((n, K, 3), device=dev), opacities=torch.empty((n, 1), device=dev), cov3D=torch.empty((n, 6), device=dev))
        ups = dict(shs=r(n, K, 3), opacities=r(n, 1), cov3D=r(n, 6))
        grads = {k: torch.empty_like(p[k]) for k in ("dc", "rest", "opacity", "scaling", "rotation")}
        params = _lib.SceneParams(P(p["dc"]), P(p["rest"]), P(p["opacity"]), P(p["scaling"]), P(p["rotation"]))
        so = _lib.SceneOutputs(shs=P(outs["shs"]), opacities=P(outs["opacities"]), cov3D=P(outs["cov3D"]))
        sg = _lib.SceneOutGrads(P(ups["shs"]), P(ups["opacities"]), P(ups["cov3D"]))
        si = _lib.SceneInGrads(P(grads["dc"]), P(grads["rest"]), P(grads["opacity"]), P(grads["scaling"]), P(grads["rotation"]))
        sets.append((p, outs, ups, grads, params, so, sg, si))

    def fwd(filtered, backward):
        def run():
            for p, _, _, _, params, so, sg, si in sets:
                if filtered:
                    _lib.check(lib.lsr_scene_activate_filtered_forward(C.byref(dims), C.byref(params), P(p["filt"]), C.byref(so), stream), "fwd")
                    if backward:
                        _lib.check(lib.lsr_scene_activate_filtered_backward(C.byref(dims), C.byref(params), P(p["filt"]), C.byref(sg),
                                                                            C.byref(si), stream), "bwd")
                else:
                    _lib.check(lib.lsr_scene_activate_forward(C.byref(dims), C.byref(params), C.byref(so), stream), "fwd")
                    if backward:
                        _lib.check(lib.lsr_scene_activate_backward(C.byref(dims), C.byref(params), C.byref(sg), C.byref(si), stream), "bwd")
        return run

    res = dict(n=n, sh_coeffs=K, copies=copies)
    for what, backward, nbytes in (("forward", False, FWD_BYTES), ("forward_backward", True, FWD_BYTES + BWD_BYTES)):
        plain, filt = fwd(False, backward), fwd(True, backward)
        for fn in (plain, filt):
            for _ in range(a.warmup):
                fn()
        tp, tf = [], []
        for _ in range(a.samples):                           # alternating: both arms see the same machine
            tp.append(_sample(plain, dev) / copies)
            tf.append(_sample(filt, dev) / copies)
        fp, ff = _figures(tp), _figures(tf)
        extra = 4 * (2 if backward else 1)
        res[what] = dict(unfiltered=fp, filtered=ff, ratio=ff["ms"] / fp["ms"], byte_ratio=(nbytes + extra) / nbytes,
                         bytes_per_gaussian_unfiltered=nbytes, unfiltered_bytes_per_s=nbytes * n / (fp["ms"] * 1e-3),
                         filtered_bytes_per_s=(nbytes + extra) * n / (ff["ms"] * 1e-3))
        print(f"n={n:8d} {what:16s} unfiltered {_show(fp)}  filtered {_show(ff)}  ratio {res[what]['ratio']:.4f} "
              f"(bytes {res[what]['byte_ratio']:.4f}; spreads {fp['spread']:.3f} / {ff['spread']:.3f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "filter3d_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_filter3d needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, width=WIDTH, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               pass_bytes_per_gaussian=PASS_BYTES,
               baseline_note="the stock arm is the published per-camera loop composed of stock PyTorch operations; it clamps the depth "
                             "and divides where the kernel compares without a division")
    for n, V in SIZES:
        entry = dict(filter_pass=bench_pass(n, V, dev, a, lib))
        torch.cuda.empty_cache()
        entry["activation"] = bench_activation(n, dev, a, lib)
        torch.cuda.empty_cache()
        res[f"n_{n}"] = entry
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
