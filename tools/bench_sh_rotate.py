#!/usr/bin/env python
"""SH coefficient rotation of the Gaussian adapter: the fused HIP path against a stock-PyTorch composition of the same
math, alternated in one process.

  fused   latentsplat_amd.sh_rotate.rotate_harmonics: lsr_sh_rotation_matrices + one launch forward, one backward
          (masks, both tensors, sample broadcast), reading the strided view of the encoder's Linear output in place
  torch   what the reference does once it has its Wigner matrices (gaussian_adapter.py:90-93,107-108,
          sh_utils.py:100-120): broadcast multiply by the masks, one einsum per band with the tables of
          lsr_sh_rotation_matrices, cat — per tensor, autograd's backward
  shape   the encoder's (config/model/encoder/epipolar.yaml:12-22): 2 context views x 65 536 rays x 3 samples per scene,
          colour SH degree 4, 4 latent channels of degree 2, rows of 120 floats with the harmonics 9 floats in;
          1 scene and 4 scenes

Times are device events around `steps` calls (median over `rounds`, the two variants alternated); the bytes model is the
traffic the math needs (forward: one read of the raw harmonics, one write of both outputs; backward: the reverse), and the
rate is that over the time, as a fraction of the 6.3 TB/s achievable HBM rate of the MI355X.

usage: python tools/bench_sh_rotate.py [--steps 50] [--rounds 7] [--json [profiles/sh_rotate_bench.json]]"""
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
RAYS, SAMPLES, KC, C, KF, ROW_FLOATS, ROW_OFFSET = 65536, 3, 25, 4, 9, 120, 9


def _time(fn, steps, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / steps


def _mask(degree, dev):
    m = torch.ones((degree + 1) ** 2)
    for l in range(1, degree + 1):
        m[l * l:(l + 1) ** 2] = 0.1 * 0.25 ** l
    return m.to(dev)


def torch_composition(view, tables, cmask, fmask):
    """view (cams, rays, 3 Kc + C Kf), tables (cams, 165) -> colour (cams, rays, S, 3, Kc), feature (cams, rays, S, C, Kf)."""
    cams, rays, _ = view.shape
    out = []
    for lo, ch, K, mask in ((0, 3, KC, cmask), (3 * KC, C, KF, fmask)):
        x = view[..., lo:lo + ch * K].reshape(cams, rays, 1, ch, K).broadcast_to(cams, rays, SAMPLES, ch, K) * mask
        bands, off = [], 0
        for l in range(int(K ** 0.5)):
            n = 2 * l + 1
            D = tables[:, off:off + n * n].reshape(cams, 1, 1, 1, n, n)
            bands.append(torch.einsum("...ij,...j->...i", D, x[..., l * l:(l + 1) ** 2]))
            off += n * n
        out.append(torch.cat(bands, dim=-1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "sh_rotate_bench.json"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sh_rotate needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.sh_rotate import rotate_harmonics, sh_rotation_matrices
    dev = torch.device("cuda:0")
    res = {}
    for scenes in (1, 4):
        cams = 2 * scenes
        gen = torch.Generator(device=dev).manual_seed(scenes)
        linear_out = torch.randn((cams, RAYS, ROW_FLOATS), device=dev, generator=gen).requires_grad_()
        view = linear_out[..., ROW_OFFSET:ROW_OFFSET + 3 * KC + C * KF]
        q = torch.nn.functional.normalize(torch.randn((cams, 4), device=dev, generator=gen), dim=-1)
        x, y, z, w = q.unbind(-1)
        rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                           2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                           2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(cams, 3, 3)
        cmask, fmask = _mask(4, dev), _mask(2, dev)
        tables = sh_rotation_matrices(rot, 4)
        gc = torch.randn((cams, RAYS, SAMPLES, 3, KC), device=dev, generator=gen)
        gf = torch.randn((cams, RAYS, SAMPLES, C, KF), device=dev, generator=gen)

        def fused(backward):
            color, feature = rotate_harmonics(view, rot, SAMPLES, KC, C, KF, cmask, fmask)
            if backward:
                linear_out.grad = None
                torch.autograd.backward([color, feature], [gc, gf])
            return color, feature

        def stock(backward):
            color, feature = torch_composition(view, tables, cmask, fmask)
            if backward:
                linear_out.grad = None
                torch.autograd.backward([color, feature], [gc, gf])
            return color, feature

        # same results (and warm-up of every variant)
        with torch.no_grad():
            cf, ff = fused(False)
            cs, fs = stock(False)
            diff = max(float((cf - cs).abs().max()), float((ff - fs).abs().max()))
        fused(True); g_fused = linear_out.grad.clone()
        stock(True); g_stock = linear_out.grad.clone()
        gdiff = float((g_fused - g_stock).abs().max() / g_stock.abs().max())
        del cf, ff, cs, fs, g_fused, g_stock
        rows = cams * RAYS
        width = 3 * KC + C * KF
        bytes_fwd = 4 * rows * width * (1 + SAMPLES)
        bytes_fwd_bwd = 2 * bytes_fwd                      # + one read of both upstream gradients, one write of the dense rows
        entry = dict(cameras=cams, rows=rows, samples=SAMPLES, bytes_forward=bytes_fwd, bytes_forward_backward=bytes_fwd_bwd,
                     max_abs_diff_forward=diff, max_rel_diff_grad=gdiff)
        for what, backward, nbytes in (("forward", False, bytes_fwd), ("forward_backward", True, bytes_fwd_bwd)):
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
            entry[what] = dict(fused_ms=mf, torch_ms=ms, speedup=ms / mf, fused_all=tf, torch_all=ts,
                               torch_spread_ms=max(ts) - min(ts), fused_spread_ms=max(tf) - min(tf),
                               faster_by_more_than_torch_spread=bool(ms - mf > max(ts) - min(ts)),
                               fused_bytes_per_s=nbytes / (mf * 1e-3),
                               fused_fraction_of_achievable_hbm=nbytes / (mf * 1e-3) / HBM_ACHIEVABLE)
            e = entry[what]
            print(f"scenes={scenes} {what:17s} fused {mf:8.4f} ms  torch {ms:8.4f} ms  x{e['speedup']:.2f}  "
                  f"(torch spread {e['torch_spread_ms']:.4f} ms)  model {nbytes / 1e6:.1f} MB -> "
                  f"{e['fused_bytes_per_s'] / 1e12:.2f} TB/s = {100 * e['fused_fraction_of_achievable_hbm']:.1f} % of 6.3 TB/s",
                  flush=True)
        print(f"scenes={scenes} fused vs torch: forward max |diff| {diff:.2e}, gradient max rel diff {gdiff:.2e}", flush=True)
        res[f"encoder_{scenes}_scene" + ("s" if scenes > 1 else "")] = entry
        del linear_out, view, gc, gf
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
