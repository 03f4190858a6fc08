#!/usr/bin/env python
"""Device time of the vector quantisation (csrc/vq.hip, include/lsr_vq.h, latentsplat_amd.vq) and of the stock-PyTorch
composition on the same card, in the same process.

  assign   `lsr_vq_assign` through the C ABI into preallocated outputs (pack kernel + fused distance-and-argmin kernel)
           against the stock route: `x @ c.T` in row chunks of at most 1 GiB of scores, the bias added, `argmin`.  The
           rate is 2 n k D floating-point operations over the call's time, as a fraction of the 157.3 TF f32 matrix peak
           and beside the 122 TF of an untuned LDS-tiled f32 MFMA GEMM; it is a whole-call rate, pack kernel included.
  update   `lsr_vq_update` (sort, float64 block sums, finish) against `index_add_` of the weighted rows and a divide
           (float32 atomics: neither reproducible nor accurate for large codes, which is why it is not what the library does).
           The update is bound by memory, so both sides rotate over as many copies of (x, idx, weights) as make 1.1 GB,
           more than the 256 MB last-level cache, each call on the next copy; a sample is one pass over all copies
  kmeans   one Lloyd iteration: the two together, through latentsplat_amd.vq's own launch helpers

Shapes (n, k, D): (3 000 000, 4096, 45) the rest rows of a large degree-3 scene, (393 216, 4096, 45) a small one,
(3 000 000, 4096, 7) the shape rows.  Rows are clustered (4096 centres, spread 0.1) and the assignment used by the update
is the kernel's own.  Every figure is the median of `--samples` (>= 20) samples after `--warmup` calls, the smallest and the
largest beside it; a sample is `inner` back-to-back calls between two device events, divided by their number.  The
assignment and the iteration reuse one set of arrays (they are bound by arithmetic: 10^11 to 10^12 operations on at most
540 MB); every buffer of both sides is allocated outside the timed region.

usage: python tools/bench_vq.py [--samples 20] [--warmup 3] [--json [profiles/vq_bench.json]]"""
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

SHAPES = ((3_000_000, 4096, 45), (393_216, 4096, 45), (3_000_000, 4096, 7))
PEAK_F32_MATRIX = 157.3e12
UNTUNED_GEMM = 122e12
SCORE_BYTES = 1 << 30
ROTATE_BYTES = 1.1e9


def _sample(fn, dev, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def _figures(fn, dev, a, inner, calls_per_fn=1):
    for _ in range(a.warmup):
        fn()
    t = [_sample(fn, dev, inner) / calls_per_fn for _ in range(a.samples)]
    return dict(ms=statistics.median(t), min_ms=min(t), max_ms=max(t), samples=len(t), calls_per_sample=inner * calls_per_fn)


def _show(f):
    return f"{f['ms']:9.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]"


def stock_assign(x, c, idx, chunk):
    bias = (c * c).sum(1)
    for a in range(0, x.shape[0], chunk):
        s = torch.addmm(bias, x[a:a + chunk], c.T, beta=1.0, alpha=-2.0)
        torch.argmin(s, dim=1, out=idx[a:a + chunk])


def stock_update(x, idx, w, prev, sums, mass):
    sums.zero_().index_add_(0, idx, x * w[:, None])
    mass.zero_().index_add_(0, idx, w)
    return torch.where(mass[:, None] > 0, sums / mass[:, None], prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "vq_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_vq needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib, vq
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), peak_f32_matrix_flops=PEAK_F32_MATRIX,
               untuned_f32_mfma_gemm_flops=UNTUNED_GEMM, stock_score_chunk_bytes=SCORE_BYTES, shapes=[])
    for n, k, d in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(n + d)
        c = 3.0 * torch.randn((k, d), device=dev, generator=gen)
        x = c[torch.randint(0, k, (n,), device=dev, generator=gen)] + 0.1 * torch.randn((n, d), device=dev, generator=gen)
        w = torch.rand(n, device=dev, generator=gen) + 0.5
        idx, dist2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
        ws = torch.empty(lib.lsr_vq_workspace_bytes(n, k, d), dtype=torch.uint8, device=dev)
        dims = _lib.VqDims(n=n, k=k, d=d)
        p = lambda t: C.c_void_p(None if t is None else t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        inner = 1 if n * k * d > 1e11 else 4
        flops = 2.0 * n * k * d

        def assign(dist=None):
            _lib.check(lib.lsr_vq_assign(C.byref(dims), p(x), p(c), p(idx), p(dist), p(ws), stream), "lsr_vq_assign")
        kern = _figures(assign, dev, a, inner)
        with_dist = _figures(lambda: assign(dist2), dev, a, inner)
        chunk = max(1, SCORE_BYTES // (4 * k))
        sidx = torch.empty(n, dtype=torch.int64, device=dev)
        stock = _figures(lambda: stock_assign(x, c, sidx, chunk), dev, a, inner)
        agree = float((sidx == idx.long()).float().mean())
        rate = flops / (kern["ms"] * 1e-3)
        entry = dict(n=n, k=k, d=d, flops=flops,
                     assign=dict(kernel=kern, kernel_with_dist2=with_dist, stock=stock, speedup=stock["ms"] / kern["ms"], flops_per_s=rate,
                                 fraction_of_f32_matrix_peak=rate / PEAK_F32_MATRIX, fraction_of_untuned_gemm=rate / UNTUNED_GEMM,
                                 stock_flops_per_s=flops / (stock["ms"] * 1e-3), stock_agrees_on_fraction_of_rows=agree))
        print(f"{n}x{k}x{d} assign  kernel {_show(kern)} = {rate / 1e12:.1f} TF ({100 * rate / PEAK_F32_MATRIX:.0f} % of peak, "
              f"{100 * rate / UNTUNED_GEMM:.0f} % of the untuned GEMM)  with dist2 {_show(with_dist)}  stock {_show(stock)}  x{stock['ms'] / kern['ms']:.2f}"
              f"  (stock agrees on {100 * agree:.3f} % of rows)", flush=True)
        del sidx
        out, mass = torch.empty_like(c), torch.empty(k, device=dev)
        copies = max(2, math.ceil(ROTATE_BYTES / (n * (4 * d + 8))))
        sets = [(x.clone(), idx.clone(), w.clone()) for _ in range(copies)]

        def update():
            for xs, ids, wts in sets:
                _lib.check(lib.lsr_vq_update(C.byref(dims), p(xs), p(ids), p(wts), p(c), p(out), p(mass), p(ws), stream), "lsr_vq_update")
        kern = _figures(update, dev, a, 1, copies)
        long_sets = [(xs, ids.long(), wts) for xs, ids, wts in sets]
        sums, smass = torch.empty_like(c), torch.empty(k, device=dev)

        def stock_update_all():
            for xs, ids, wts in long_sets:
                stock_update(xs, ids, wts, c, sums, smass)
        stock = _figures(stock_update_all, dev, a, 1, copies)
        worst = float((stock_update(*long_sets[-1], c, sums, smass) - out).abs().max())
        entry["update"] = dict(kernel=kern, stock=stock, speedup=stock["ms"] / kern["ms"], largest_difference_to_stock=worst, copies=copies,
                               rotated_bytes=copies * n * (4 * d + 8))
        print(f"{n}x{k}x{d} update  kernel {_show(kern)}  stock {_show(stock)}  x{stock['ms'] / kern['ms']:.2f}  (largest difference {worst:.2e}; "
              f"rotating over {copies} copies)", flush=True)
        del sets, long_sets
        torch.cuda.empty_cache()
        sidx = torch.empty(n, dtype=torch.int64, device=dev)

        def iteration():
            vq._assign(x, c, idx, None, ws)
            vq._update(x, idx, w, c, out, mass, ws)

        def stock_iteration():
            stock_assign(x, c, sidx, chunk)
            stock_update(x, sidx, w, c, sums, smass)
        kern, stock = _figures(iteration, dev, a, inner), _figures(stock_iteration, dev, a, inner)
        entry["kmeans_iteration"] = dict(kernel=kern, stock=stock, speedup=stock["ms"] / kern["ms"])
        print(f"{n}x{k}x{d} kmeans iteration  kernel {_show(kern)}  stock {_show(stock)}  x{stock['ms'] / kern['ms']:.2f}", flush=True)
        res["shapes"].append(entry)
        del x, c, w, idx, dist2, ws, out, mass, sidx, sums, smass
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
