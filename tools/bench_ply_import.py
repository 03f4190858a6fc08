#!/usr/bin/env python
"""Device time of the .ply import's unpack kernel (`lsr_ply_unpack`) against a stock-PyTorch composition of the same
outputs, alternated in one process.

  fused   latentsplat_amd.ply_import.unpack_table: one launch, rows (n, 62) -> means, shs, opacities, scales,
          rotations, cov3D
  torch   what a user writes by hand behind a .ply parser: column gathers (index_select by the same offsets), the
          (n, 3, K-1) -> (n, K-1, 3) transpose of the rest coefficients, sigmoid, exp, normalise and
          rasterizer._covariance_from_scale_rotation
  shape   degree 3 (K = 16, 62-float rows) at n = 393 216 (the encoder-shaped cloud) and n = 3 000 000 (a trained scene)

Each sample is `--inner` back-to-back calls between two device events, divided by their number, so that the device and
not the host's launch path is what is timed; the fused variant writes into outputs allocated once, the composition
allocates its results as PyTorch does.  The figure is the median of `--samples` (>= 20) after `--warmup` calls, the
variants alternated sample by sample.  The byte model is what
the math must move: n * 4 * (stride + 3 + 3 K + 1 + 3 + 4 + 6); the rate is that over the time, as a fraction of the
6.3 TB/s achievable HBM rate of the MI355X.  `--rows` also times the kernel at other rows-per-workgroup settings
(the LSR_PLY_UNPACK_ROWS development knob).

usage: python tools/bench_ply_import.py [--samples 30] [--warmup 5] [--inner 10] [--rows 64 256] [--json [profiles/ply_import_bench.json]]"""
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


def standard_names(k: int) -> list:
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
    names += [f"f_rest_{i}" for i in range(3 * (k - 1))] + ["opacity"]
    return names + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]


def model_bytes(n: int, stride: int, k: int) -> int:
    return n * 4 * (stride + 3 + 3 * k + 1 + 3 + 4 + 6)


def torch_composition(rows, idx):
    from latentsplat_amd.rasterizer import _covariance_from_scale_rotation
    n = rows.shape[0]
    means = rows.index_select(1, idx["xyz"])
    dc = rows.index_select(1, idx["f_dc"])
    rest = rows.index_select(1, idx["f_rest"]).reshape(n, 3, K - 1).transpose(1, 2)
    shs = torch.cat([dc[:, None, :], rest], dim=1).contiguous()
    opacities = torch.sigmoid(rows.index_select(1, idx["opacity"]))
    scales = torch.exp(rows.index_select(1, idx["scale"]))
    rot = rows.index_select(1, idx["rot"])
    rotations = rot / rot.norm(dim=-1, keepdim=True)
    cov = _covariance_from_scale_rotation(scales, rot, 1.0)
    return dict(means=means, shs=shs, opacities=opacities, scales=scales, rotations=rotations, cov3D=cov)


def _sample(fn, dev, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rows", type=int, nargs="*", default=[], help="other rows-per-workgroup settings to time")
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "ply_import_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_ply_import needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    from latentsplat_amd.ply_import import layout_from_names, unpack_table
    dev = torch.device("cuda:0")
    lib = _lib.load()
    names = standard_names(K)
    stride = len(names)
    at = names.index
    t = lambda xs: torch.tensor(xs, device=dev)
    idx = dict(xyz=t([at(k) for k in "xyz"]), f_dc=t([at(f"f_dc_{i}") for i in range(3)]),
               f_rest=t([at(f"f_rest_{i}") for i in range(3 * (K - 1))]), opacity=t([at("opacity")]),
               scale=t([at(f"scale_{i}") for i in range(3)]), rot=t([at(f"rot_{i}") for i in range(4)]))
    res = dict(sh_coeffs=K, stride=stride, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
    for n in SIZES:
        gen = torch.Generator(device=dev).manual_seed(n)
        rows = torch.randn((n, stride), device=dev, generator=gen)
        layout = layout_from_names(names, n)
        stock = lambda: torch_composition(rows, idx)
        with torch.no_grad():
            f, s = unpack_table(rows, layout), stock()
            diff = {k: float((f[k] - s[k]).abs().max() / s[k].abs().max().clamp_min(1e-30)) for k in f}
            del s
            ptrs = _lib.PlyOutputs(**{k: C.c_void_p(v.data_ptr()) for k, v in f.items()})
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            fused = lambda: _lib.check(lib.lsr_ply_unpack(C.byref(layout), C.c_void_p(rows.data_ptr()), 0, C.byref(ptrs),
                                                          stream), "lsr_ply_unpack")
            for _ in range(a.warmup):
                fused(); stock()
            torch.cuda.synchronize(dev)
            tf, ts = [], []
            for _ in range(a.samples):                       # alternated
                tf.append(_sample(fused, dev, a.inner))
                ts.append(_sample(stock, dev, a.inner))
            other = {}
            for r in a.rows:
                _lib.set_knob("LSR_PLY_UNPACK_ROWS", r)
                for _ in range(a.warmup):
                    fused()
                other[str(r)] = statistics.median(_sample(fused, dev, a.inner) for _ in range(a.samples))
            if a.rows:
                _lib.set_knob("LSR_PLY_UNPACK_ROWS", 128)
        mf, ms = statistics.median(tf), statistics.median(ts)
        nb = model_bytes(n, stride, K)
        entry = dict(n=n, model_bytes=nb, fused_ms=mf, torch_ms=ms, speedup=ms / mf, fused_min_ms=min(tf), fused_max_ms=max(tf),
                     torch_min_ms=min(ts), torch_max_ms=max(ts), fused_bytes_per_s=nb / (mf * 1e-3),
                     fused_fraction_of_achievable_hbm=nb / (mf * 1e-3) / HBM_ACHIEVABLE,
                     faster_than_torch_in_every_sample=bool(max(tf) < min(ts)), max_rel_diff_vs_torch=diff)
        if other:
            entry["fused_ms_by_rows_per_workgroup"] = other
        print(f"n={n:8d}  fused {mf:7.4f} ms [{min(tf):.4f}, {max(tf):.4f}]  torch {ms:8.4f} ms [{min(ts):.4f}, {max(ts):.4f}]  "
              f"x{ms / mf:.1f}  model {nb / 1e6:.1f} MB -> {nb / (mf * 1e-3) / 1e12:.2f} TB/s = "
              f"{100 * entry['fused_fraction_of_achievable_hbm']:.1f} % of 6.3 TB/s" + (f"  rows/wg {other}" if other else ""),
              flush=True)
        print(f"n={n:8d}  fused vs torch, max relative difference: " + ", ".join(f"{k} {v:.1e}" for k, v in diff.items()), flush=True)
        res[f"n_{n}"] = entry
        del rows, f
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
