#!/usr/bin/env python
"""Device time of mesh extraction (csrc/tsdf.hip, include/lsr_mesh.h, latentsplat_amd.mesh) on the card it runs on.

  fusion      `TSDFVolume.integrate` of V views in ONE call, with colour, at 256^3 x 16 views of 256 x 256 and at
              512^3 x 64 views of 512 x 512: depth maps of an analytic sphere seen from cameras on a circle, the volume a
              box around it
  stock       the stock float32 PyTorch composition of the same rule (include/lsr_mesh.h, steps 1..11), one view at a time
              over the whole volume, in the same process on the same card
  extraction  `lsr_mesh_count` and `lsr_mesh_count` + `lsr_mesh_emit` (through `TSDFVolume.extract_mesh`, its one host read
              included) on the fused volumes

Every arm rotates over as many copies of the volume as make more than the 256 MB last-level cache, each call on the next
copy; every timed shape is warmed up; every figure is the median of `--samples` (>= 20) samples with the smallest and the
largest beside it.  Fusion is also given in (lattice point, view) pairs per second, and every HIP figure as the fraction of
the 6.3 TB/s achievable rate that the bytes the call must move amount to: fusion reads 20 B per lattice point and writes 20 B
per touched one, and reads the 20 B per pixel of its images once; counting reads 8 B and writes 9 B per lattice point;
emission reads those 17 B and writes 24 B per vertex and 12 B per face.

usage: python tools/bench_tsdf.py [--samples 20] [--warmup 2] [--json [profiles/tsdf_bench.json]]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((256, 16, 256), (512, 64, 512))       # lattice edge, views, image edge
CACHE_BYTES = 256e6
HBM_BYTES_PER_S = 6.3e12
RADIUS, CAMERA_DISTANCE, FOCAL = 1.0, 3.0, 0.8


def _sample(fn, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end)


def _figures(t, nbytes=None):
    med = statistics.median(t)
    f = dict(ms=med, min_ms=min(t), max_ms=max(t), samples=len(t))
    if nbytes is not None:
        f.update(bytes=nbytes, fraction_of_hbm=nbytes / HBM_BYTES_PER_S / (1e-3 * med))
    return f


def _show(f):
    tail = f", {100 * f['fraction_of_hbm']:.0f} % of HBM" if "fraction_of_hbm" in f else ""
    return f"{f['ms']:9.3f} ms [{f['min_ms']:.3f}, {f['max_ms']:.3f}]{tail}"


def _time(fn, dev, samples, warmup, nbytes=None):
    for _ in range(warmup):
        fn()
    return _figures([_sample(fn, dev) for _ in range(samples)], nbytes)


def circle_views(V, dev):
    """A (V, 44) table of cameras on a circle around the origin, looking at it, through build_view_table (near 1: scale 1)."""
    from latentsplat_amd.rasterizer import build_view_table
    ang = torch.arange(V, device=dev, dtype=torch.float32) * (2 * math.pi / V) + 0.1
    zero, one = torch.zeros_like(ang), torch.ones_like(ang)
    offset = torch.stack([torch.cos(ang), zero, torch.sin(ang)], -1)
    down = torch.stack([zero, one, zero], -1)
    ext = torch.zeros((V, 4, 4), device=dev)
    ext[:, :3, 0], ext[:, :3, 1], ext[:, :3, 2] = torch.linalg.cross(down, -offset), down, -offset
    ext[:, :3, 3] = CAMERA_DISTANCE * offset
    ext[:, 3, 3] = 1
    intr = torch.tensor([[FOCAL, 0, 0.5], [0, FOCAL, 0.5], [0, 0, 1.0]], device=dev).repeat(V, 1, 1)
    near, far = torch.full((V,), 1.0, device=dev), torch.full((V,), 100.0, device=dev)
    return build_view_table(ext, intr, near, far, torch.zeros(3, device=dev))


def sphere_images(V, size, dev, gen):
    """(depth, alpha, color): what the rasterizer would render of an opaque sphere of RADIUS at the origin (the same from every
    camera of the circle): depth = z alpha along the optical axis, alpha 1 on the sphere and 0 beside it."""
    u = (torch.arange(size, device=dev, dtype=torch.float32) + 0.5) / size
    ry, rx = torch.meshgrid((u - 0.5) / FOCAL, (u - 0.5) / FOCAL, indexing="ij")
    d2 = rx * rx + ry * ry + 1.0
    disc = CAMERA_DISTANCE ** 2 - d2 * (CAMERA_DISTANCE ** 2 - RADIUS ** 2)
    hit = disc > 0
    z = torch.where(hit, (CAMERA_DISTANCE - torch.sqrt(disc.clamp_min(0))) / d2, torch.zeros_like(d2))
    alpha = hit.float()
    return ((z * alpha).expand(V, size, size).contiguous(), alpha.expand(V, size, size).contiguous(),
            torch.rand((V, 3, size, size), device=dev, generator=gen))


def stock_integrate(vol, depth, alpha, views, color, alpha_min=0.5):
    """include/lsr_mesh.h steps 1..11 in stock float32 PyTorch, one view at a time over the whole volume, in place."""
    nx, ny, nz = vol.dims
    dev = vol.device
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float32), torch.arange(ny, device=dev, dtype=torch.float32),
                             torch.arange(nx, device=dev, dtype=torch.float32), indexing="ij")
    x, y, z0 = (vol.origin[0] + vol.voxel_size * i, vol.origin[1] + vol.voxel_size * j, vol.origin[2] + vol.voxel_size * k)
    V, H, W = depth.shape
    for v in range(V):
        view = views[v]
        s = view[40]
        px, py, pz = s * x, s * y, s * z0
        row = lambda m, r: m[r] * px + m[4 + r] * py + m[8 + r] * pz + m[12 + r]
        z, cx, cy, cw = row(view[:16], 2), row(view[16:32], 0), row(view[16:32], 1), row(view[16:32], 3)
        live = (z > 0) & (cw > 0)
        ix = torch.floor(((cx / cw + 1) * W - 1) / 2 + 0.5)
        iy = torch.floor(((cy / cw + 1) * H - 1) / 2 + 0.5)
        live &= (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        pixel = torch.where(live, iy * W + ix, torch.zeros_like(ix)).long()
        a = alpha[v].reshape(-1)[pixel]
        live &= a > alpha_min
        D = depth[v].reshape(-1)[pixel] / a
        live &= torch.isfinite(D) & (D > 0)
        sdf = (D - z) / s
        live &= ~(sdf < -vol.trunc)
        d = torch.clamp_max(sdf / vol.trunc, 1.0)
        w1 = vol.weight + 1
        vol.tsdf.copy_(torch.where(live, (vol.tsdf * vol.weight + d) / w1, vol.tsdf))
        for c in range(3):
            vol.color[c].copy_(torch.where(live, (vol.color[c] * vol.weight + color[v, c].reshape(-1)[pixel]) / w1, vol.color[c]))
        vol.weight.copy_(torch.where(live, w1, vol.weight))


def bench_shape(n, V, size, dev, a):
    from latentsplat_amd import _lib
    from latentsplat_amd.mesh import TSDFVolume
    gen = torch.Generator(device=dev).manual_seed(n + V)
    views = circle_views(V, dev)
    depth, alpha, color = sphere_images(V, size, dev, gen)
    voxels, pixels = n ** 3, V * size * size
    half = 1.25 * RADIUS
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (20 * voxels)))
    vols = [TSDFVolume((-half,) * 3, 2 * half / (n - 1), (n, n, n), device=dev) for _ in range(copies)]
    turn = [0]

    def next_empty():
        turn[0] = (turn[0] + 1) % copies
        for k in range(copies):                  # the target first: the other copies then pass through the cache behind it
            vols[(turn[0] + k) % copies].reset()
        torch.cuda.synchronize(dev)

    def fuse():
        vols[turn[0]].integrate(depth, alpha, views, color=color)

    # (the reset is outside the timed window: every sample fuses into an empty volume, as the first batch of a run does)
    def sample_fusion(fn):
        out = []
        for _ in range(a.warmup):
            next_empty()
            fn()
        for _ in range(a.samples):
            next_empty()
            out.append(_sample(fn, dev))
        return out

    res = dict(lattice=n, views=V, image=size, copies=copies, pairs=voxels * V)
    t = sample_fusion(fuse)
    touched = int((vols[turn[0]].weight > 0).sum())
    res["touched_fraction"] = touched / voxels
    res["hip_fusion"] = _figures(t, 20 * voxels + 20 * touched + 20 * pixels)
    res["hip_fusion"]["pairs_per_s"] = voxels * V / (1e-3 * res["hip_fusion"]["ms"])
    t = sample_fusion(lambda: stock_integrate(vols[turn[0]], depth, alpha, views, color))
    res["stock_fusion"] = _figures(t)
    res["stock_fusion"]["pairs_per_s"] = voxels * V / (1e-3 * res["stock_fusion"]["ms"])
    res["speedup"] = res["stock_fusion"]["ms"] / res["hip_fusion"]["ms"]
    # the two agree: the last stock volume against a HIP fusion of the same views
    stock_vol, hip_vol = vols[turn[0]], vols[(turn[0] + 1) % copies]
    hip_vol.reset()
    hip_vol.integrate(depth, alpha, views, color=color)
    # (random inputs keep no distance from the rounding of the nearest pixel: a point that projects onto a pixel boundary reads
    # one pixel here and its neighbour there; the tests' reference leaves such points out, this counts them)
    diff = (stock_vol.tsdf - hip_vol.tsdf).abs()
    other_pixel = (stock_vol.weight != hip_vol.weight) | (diff > 1e-4)
    res["points_that_read_another_pixel_than_stock"] = int(other_pixel.sum())
    res["max_abs_tsdf_difference_from_stock_elsewhere"] = float(diff[~other_pixel].max())
    print(f"fusion {n}^3 x {V} views of {size}^2: HIP {_show(res['hip_fusion'])}, {res['hip_fusion']['pairs_per_s']:.3e} pairs/s\n"
          f"    stock {_show(res['stock_fusion'])}, {res['stock_fusion']['pairs_per_s']:.3e} pairs/s: x{res['speedup']:.1f}; touched "
          f"{res['touched_fraction']:.3f}; {res['points_that_read_another_pixel_than_stock']} of {voxels} points read another pixel "
          f"than stock, tsdf elsewhere differs by at most {res['max_abs_tsdf_difference_from_stock_elsewhere']:.2e}", flush=True)

    # extraction, on the fused volumes (every copy fused the same views)
    for vol in vols:
        vol.reset()
        vol.integrate(depth, alpha, views, color=color)
    lib = _lib.load()
    ws = torch.empty(lib.lsr_mesh_workspace_bytes(C.byref(vols[0]._dims)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ptr = lambda t_: C.c_void_p(t_.data_ptr())

    def count():
        turn[0] = (turn[0] + 1) % copies
        vol = vols[turn[0]]
        _lib.call("lsr_mesh_count", C.byref(vol._dims), ptr(vol.tsdf), ptr(vol.weight), 1.0, ptr(ws), ptr(counts),
                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    res["hip_count"] = _time(count, dev, a.samples, a.warmup, 17 * voxels)
    nv, nf = counts.tolist()
    res["vertices"], res["faces"] = nv, nf

    def extract():
        turn[0] = (turn[0] + 1) % copies
        return vols[turn[0]].extract_mesh()

    for _ in range(a.warmup):
        extract()
    t = []
    for _ in range(a.samples):                   # a host clock: the call ends in its own host read and allocates its outputs
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        extract()
        torch.cuda.synchronize(dev)
        t.append(1e3 * (time.perf_counter() - t0))
    res["hip_extract_mesh"] = _figures(t, 34 * voxels + 24 * nv + 12 * nf)
    print(f"extraction {n}^3: count {_show(res['hip_count'])}; extract_mesh (count + host read + emit) {_show(res['hip_extract_mesh'])}; "
          f"{nv} vertices, {nf} faces", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "tsdf_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_tsdf needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               hbm_bytes_per_s=HBM_BYTES_PER_S,
               bytes_note="fusion: 20 B per lattice point read + 20 B per touched point written + 20 B per pixel read; count: 8 B read + "
                          "9 B written per lattice point; extract_mesh: count, those 17 B read again, 24 B per vertex and 12 B per face written",
               baseline_note="stock: the float32 PyTorch composition of steps 1..11 of include/lsr_mesh.h (tools/bench_tsdf.py), one view "
                             "at a time over the whole volume, same process and card",
               shapes=[])
    for n, V, size in SHAPES:
        res["shapes"].append(bench_shape(n, V, size, dev, a))
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
