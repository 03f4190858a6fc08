#!/usr/bin/env python
"""Device time of the scene export's packing kernel (`lsr_ply_pack_scene`) against a stock-PyTorch composition of the same
rows, alternated in one process.

  fused   one launch: means (n,3), opacities (n,), colour SH (n,3,K) in the "reference" convention, covariances (n,3,3)
          -> rows (n, 14 + 3K) of the published layout, into a table allocated once
  torch   what a user writes by hand: torch.linalg.eigh over the (n,3,3) batch (each matrix scaled by its largest entry,
          without which the ROCm eigh is wrong for small covariances), descending order, the clamp, the
          determinant fix, matrix to quaternion (largest-of-four candidates with torch.where), logit, the SH basis change
          as a (25,25) matmul and the channel-major flatten, zeros for the normals, and torch.cat
  shape   degree 3 (K = 16, 62-float rows) at n = 393 216 (the encoder-shaped cloud) and n = 3 000 000 (a trained scene)

Each sample is `--inner` back-to-back calls between two device events, divided by their number (the composition's samples
take fewer calls, down to one, when a call of it takes longer than 100 ms / `--inner`); the figure is the median of
`--samples` (>= 20) after `--warmup` calls, the variants alternated sample by sample.  The byte model is what the math
must move: n * 4 * (3 + 1 + 3K + 9 + 14 + 3K); the rate is that over the time, as a fraction of the 6.3 TB/s achievable
HBM rate of the MI355X.

usage: python tools/bench_ply_export.py [--samples 30] [--warmup 5] [--inner 10] [--json [profiles/ply_export_bench.json]]"""
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


def model_bytes(n: int, k: int) -> int:
    return n * 4 * (3 + 1 + 3 * k + 9 + 14 + 3 * k)


def make_inputs(n: int, dev, seed: int):
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(s, device=dev, generator=gen)
    u = lambda *s: torch.rand(s, device=dev, generator=gen)
    q = torch.nn.functional.normalize(r(n, 4), dim=-1)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    s = torch.exp(u(n, 1) * -6.9) * torch.exp(u(n, 3) * -3.4)            # overall 1e-3..1, ratios down to 1/30
    cov = (R * (s * s)[:, None, :]) @ R.transpose(1, 2)
    cov = 0.5 * (cov + cov.transpose(1, 2))
    return r(n, 3), u(n) * 0.998 + 0.001, r(n, 3, K), cov.contiguous()


def torch_composition(means, opac, shs_cm, cov, M):
    n = means.shape[0]
    # (each matrix is divided by its largest entry first: on ROCm the batched eigh stops at an absolute tolerance and
    # returns wrong eigenpairs for about 28 % of covariances of this range — entries of 1e-9 ... 1e-6 — as they are)
    big = cov.reshape(n, 9).abs().amax(1).clamp_min(1e-37)
    lam, V = torch.linalg.eigh(cov / big[:, None, None])                  # ascending
    lam, V = lam.flip(-1) * big[:, None], V.flip(-1)
    lam = torch.maximum(lam, (1e-12 * lam[:, :1]).clamp_min(1e-37))
    det = torch.linalg.det(V)
    V = torch.cat([V[:, :, :2], V[:, :, 2:] * torch.where(det < 0, -1.0, 1.0)[:, None, None]], dim=2)
    m = V.reshape(n, 9).unbind(-1)
    tw, tx, ty, tz = 1 + m[0] + m[4] + m[8], 1 + m[0] - m[4] - m[8], 1 - m[0] + m[4] - m[8], 1 - m[0] - m[4] + m[8]
    cand = torch.stack([torch.stack([tw, m[7] - m[5], m[2] - m[6], m[3] - m[1]], -1),
                        torch.stack([m[7] - m[5], tx, m[1] + m[3], m[2] + m[6]], -1),
                        torch.stack([m[2] - m[6], m[1] + m[3], ty, m[5] + m[7]], -1),
                        torch.stack([m[3] - m[1], m[2] + m[6], m[5] + m[7], tz], -1)], 1)
    pick = torch.stack([tw, tx, ty, tz], -1).argmax(-1)
    q = cand.gather(1, pick[:, None, None].expand(n, 1, 4))[:, 0]
    q = torch.nn.functional.normalize(q, dim=-1)
    q = q * torch.where(q[:, :1] < 0, -1.0, 1.0)
    logit = torch.logit(opac).clamp(-20, 20)[:, None]
    sh = shs_cm @ M.T                                                     # (n,3,K): c' = M c per channel
    return torch.cat([means, torch.zeros_like(means), sh[:, :, 0], sh[:, :, 1:].reshape(n, -1), logit, 0.5 * torch.log(lam), q], dim=1)


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
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "ply_export_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_ply_export needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    import numpy as np
    from latentsplat_amd import _lib
    from latentsplat_amd.ply_export import pack_scene
    dev = torch.device("cuda:0")
    lib = _lib.load()
    M64 = np.zeros(625)
    _lib.check(lib.lsr_ply_sh_axes_matrix(M64.ctypes.data_as(C.c_void_p)), "lsr_ply_sh_axes_matrix")
    M = torch.tensor(M64.reshape(25, 25)[:K, :K], dtype=torch.float32, device=dev)
    stride = _lib.ply_scene_row_floats(K)
    res = dict(sh_coeffs=K, stride=stride, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
    for n in SIZES:
        means, opac, shs, cov = make_inputs(n, dev, n)
        stock = lambda: torch_composition(means, opac, shs, cov, M)
        with torch.no_grad():
            rows = pack_scene(means, opac, shs, covariances=cov, convention="reference", channel_major=True)
            s = stock()
            o = 6 + 3 * K
            # eigenvectors are not unique: the geometry columns are compared through the covariance they rebuild
            from latentsplat_amd.rasterizer import _covariance_from_scale_rotation
            cov6 = cov.reshape(n, 9)[:, [0, 1, 2, 4, 5, 8]]
            big = cov6.abs().amax(1, keepdim=True)
            rebuild_err = lambda t: float(((_covariance_from_scale_rotation(torch.exp(t[:, o + 1:o + 4]), t[:, o + 4:o + 8], 1.0) - cov6).abs() / big).max())
            diff = dict(sh_and_opacity_columns_max_abs=float((rows[:, :o + 1] - s[:, :o + 1]).abs().max()),
                        fused_cov_rebuild_rel=rebuild_err(rows), torch_cov_rebuild_rel=rebuild_err(s))
            del s, cov6, big
            p = lambda t: C.c_void_p(t.data_ptr())
            inp = _lib.PlySceneInputs(p(means), p(opac), p(shs), p(cov), None, None, K, 1, 9, 0)
            opts = _lib.PlySceneOpts(_lib.SH_AXES_REFERENCE, K, 0, 0)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            fused = lambda: _lib.check(lib.lsr_ply_pack_scene(n, C.byref(inp), C.byref(opts), p(rows), stream), "lsr_ply_pack_scene")
            # (a composition call of tens of milliseconds needs no batching to hide the launch path: its samples take
            # fewer calls, so that a run stays within minutes)
            stock_inner = max(1, min(a.inner, int(100.0 / max(_sample(stock, dev, 1), 1e-3))))
            for _ in range(a.warmup):
                fused(); stock()
            torch.cuda.synchronize(dev)
            tf, ts = [], []
            for _ in range(a.samples):                       # alternated
                tf.append(_sample(fused, dev, a.inner))
                ts.append(_sample(stock, dev, stock_inner))
        mf, ms = statistics.median(tf), statistics.median(ts)
        nb = model_bytes(n, K)
        entry = dict(n=n, model_bytes=nb, torch_calls_per_sample=stock_inner, fused_ms=mf, torch_ms=ms, speedup=ms / mf, fused_min_ms=min(tf), fused_max_ms=max(tf),
                     torch_min_ms=min(ts), torch_max_ms=max(ts), fused_bytes_per_s=nb / (mf * 1e-3),
                     fused_fraction_of_achievable_hbm=nb / (mf * 1e-3) / HBM_ACHIEVABLE,
                     faster_than_torch_in_every_sample=bool(max(tf) < min(ts)), differences=diff)
        print(f"n={n:8d}  fused {mf:7.4f} ms [{min(tf):.4f}, {max(tf):.4f}]  torch {ms:8.4f} ms [{min(ts):.4f}, {max(ts):.4f}]  "
              f"x{ms / mf:.1f}  model {nb / 1e6:.1f} MB -> {nb / (mf * 1e-3) / 1e12:.2f} TB/s = "
              f"{100 * entry['fused_fraction_of_achievable_hbm']:.1f} % of 6.3 TB/s", flush=True)
        print(f"n={n:8d}  " + ", ".join(f"{k} {v:.1e}" for k, v in diff.items()), flush=True)
        res[f"n_{n}"] = entry
        del means, opac, shs, cov, rows
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
