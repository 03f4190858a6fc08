#!/usr/bin/env python
"""Device time of the pose gradient of a scene's rigid parts (`lsr_scene_pose_grad`, csrc/scene_pose.hip) against the
stock-PyTorch float32 autograd composition of the same gradients, against the existing adjoint launch of
`lsr_scene_transform`, and against the HBM time of the bytes that must move, in one process on one card.

  fused      `lsr_scene_pose_grad` through the C ABI into outputs and a workspace allocated once: the pass over the scene
             and the finishing launch
  adjoint    `lsr_scene_transform` on the adjoint records over the same upstream gradients (what the scene gradients cost)
  autograd   the public op, forward and backward, only the poses requiring grad: `pose_scene` + `torch.autograd.grad`
             (records launches, allocations and Python included)
  torch      the same forward and backward from a float32 restatement of the map (`stock_pose_scene`): R(p / |p|), exp(l),
             T_l(R) built differentiably per band from the basis definition (a fixed pseudo-inverse times the basis at the
             rotated directions), gathered per Gaussian with an index, `matmul` / `einsum` / `cat`
  patterns   uniform (no index); 64 contiguous parts (what `merge` produces); 64 parts with shuffled rows
  shape      degree 3 (K = 16) at n = 393 216 and n = 3 000 000

Each sample is `--inner` back-to-back calls between two device events, divided by their number; every call of every leg
takes the next of several buffer sets whose inputs alone exceed twice the 256 MiB last-level cache.  The figure is the
median of `--samples` (>= 20) after `--warmup` calls with the fastest and slowest beside it, the legs alternated sample by
sample.  Bytes that must move per Gaussian: 4 * (3 + 4 + 3 (K - 1)) read of x, q', c' and 4 * (3 + 3 (K - 1) + 3 + 4) of the
upstream gradients (+ 4 with an index): 428 at K = 16; the HBM time is that over the 6.3 TB/s achievable rate of the MI355X.

usage: python tools/bench_pose_grad.py [--samples 20] [--warmup 3] [--inner 2] [--json [profiles/pose_grad_bench.json]]"""
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
LLC_BYTES = 256 << 20
K, DEGREE = 16, 3
SIZES = (393_216, 3_000_000)
PARTS = 64
NAMES = ("xyz", "features_rest", "scaling", "rotation")


def pose_grad_bytes(n: int, indexed: bool = False, K: int = K) -> int:
    return n * (4 * ((3 + 4 + 3 * (K - 1)) + (3 + 3 * (K - 1) + 3 + 4)) + (4 if indexed else 0))


def basis(d: torch.Tensor) -> torch.Tensor:
    """The "3dgs" colour basis (csrc/lsr_sh.h) to degree 4 at directions (..., 3) -> (..., 25), differentiable."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C1 = 0.4886025119029199
    b = [0.28209479177387814 * torch.ones_like(x),
         -C1 * y, C1 * z, -C1 * x,
         1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * (2 * zz - xx - yy),
         -1.0925484305920792 * xz, 0.5462742152960396 * (xx - yy),
         -0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z,
         -0.4570457994644658 * y * (4 * zz - xx - yy), 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
         -0.4570457994644658 * x * (4 * zz - xx - yy), 1.445305721320277 * z * (xx - yy),
         -0.5900435899266435 * x * (xx - 3 * yy),
         2.5033429417967046 * xy * (xx - yy), -1.7701307697799304 * yz * (3 * xx - yy),
         0.9461746957575601 * xy * (7 * zz - 1), -0.6690465435572892 * yz * (7 * zz - 3),
         0.10578554691520431 * (zz * (35 * zz - 30) + 3), -0.6690465435572892 * xz * (7 * zz - 3),
         0.47308734787878004 * (xx - yy) * (7 * zz - 1), -1.7701307697799304 * xz * (xx - 3 * yy),
         0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(b, dim=-1)


class StockPose:
    """The float32 stock-PyTorch composition of the posed map, differentiable in everything.  The constants (64 unit
    directions and the pseudo-inverse of each band of the basis there, computed in float64) are made once."""

    def __init__(self, degree: int, device):
        g = torch.Generator().manual_seed(5)
        d = torch.randn(64, 3, generator=g, dtype=torch.float64)
        d = d / d.norm(dim=1, keepdim=True)
        B = basis(d)
        self.degree = degree
        self.dirs = d.float().to(device)
        self.pinv = [torch.linalg.pinv(B[:, l * l:(l + 1) ** 2]).float().to(device) for l in range(degree + 1)]

    def __call__(self, xyz, features_rest, scaling, rotation, p, t, ls=None, idx=None):
        ph = p / p.norm(dim=1, keepdim=True)
        w, x, y, z = ph.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        s = ls.exp() if ls is not None else torch.ones_like(w)
        A = s[:, None, None] * R
        Bm = basis(torch.einsum("tij,nj->tni", R, self.dirs)) if self.degree else None      # (T, N, 25)
        bands = [(self.pinv[l] @ Bm[:, :, l * l:(l + 1) ** 2]).transpose(1, 2) for l in range(1, self.degree + 1)]
        if idx is None:
            pick = lambda v: v[0]
            xo = xyz @ A[0].T + t[0]
            rest = [torch.einsum("ij,njc->nic", Tl[0], features_rest[:, l * l - 1:(l + 1) ** 2 - 1])
                    for l, Tl in zip(range(1, self.degree + 1), bands)]
        else:
            i = idx.long()
            pick = lambda v: v[i]
            xo = torch.einsum("nij,nj->ni", A[i], xyz) + t[i]
            rest = [torch.einsum("nij,njc->nic", Tl[i], features_rest[:, l * l - 1:(l + 1) ** 2 - 1])
                    for l, Tl in zip(range(1, self.degree + 1), bands)]
        q = pick(ph)
        aw, ax, ay, az = (q[..., k:k + 1] for k in range(4))
        bw, bx, by, bz = (rotation[:, k:k + 1] for k in range(4))
        rot = torch.cat([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                         aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=1)
        so = scaling + (pick(ls)[..., None] if ls is not None else 0.0)
        return xo, (torch.cat(rest, dim=1) if rest else features_rest), so, rot


def _sample(fn, dev, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def _stats(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def _alternate(fns, dev, a):
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize(dev)
    ts = [[] for _ in fns]
    for _ in range(a.samples):
        for t, fn in zip(ts, fns):
            t.append(_sample(fn, dev, a.inner))
    return [_stats(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "pose_grad_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_pose_grad needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    from latentsplat_amd.pose import pose_matrices, pose_scene
    from latentsplat_amd.transform import transform_records, transform_scene
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(7)
    quat = torch.randn(PARTS, 4, device=dev, generator=gen)
    # the largest component positive: the sign the records' q_R takes, so that the stock composition (which multiplies by
    # +p / |p|) computes the same q' and with it the same gradients
    quat = quat * quat.gather(1, quat.abs().argmax(dim=1, keepdim=True)).sign()
    trans = torch.randn(PARTS, 3, device=dev, generator=gen) * 3
    logs = (torch.rand(PARTS, device=dev, generator=gen) - 0.5) * 0.4
    stock = StockPose(DEGREE, dev)
    res = dict(sh_coeffs=K, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE,
               last_level_cache_bytes=LLC_BYTES, parts=PARTS, max_transforms=_lib.POSE_MAX_TRANSFORMS)
    for n in SIZES:
        g = torch.Generator(device=dev).manual_seed(n)
        r = lambda *s: torch.randn(s, device=dev, generator=g)
        sets = max(2, -(-2 * LLC_BYTES // pose_grad_bytes(n)) + 1)                   # inputs alone exceed twice the cache
        ins = [[3 * r(n, 3), 0.3 * r(n, K - 1, 3), r(n, 3) - 3, r(n, 4)] for _ in range(sets)]
        ups = [[r(n, 3), r(n, K - 1, 3), r(n, 3), r(n, 4)] for _ in range(sets)]
        adj_out = [torch.empty_like(t) for t in ins[0]]
        contiguous = (torch.arange(n, device=dev) * PARTS // n).to(torch.int32)
        shuffled = contiguous[torch.randperm(n, device=dev, generator=g)].contiguous()
        entry = dict(n=n, buffer_sets=sets)
        for pattern, idx, T in (("uniform", None, 1), ("contiguous_64", contiguous, PARTS), ("shuffled_64", shuffled, PARTS)):
            q, t, ls = quat[:T].contiguous(), trans[:T].contiguous(), logs[:T].contiguous()
            mats = pose_matrices(q, t, ls)
            rec, adj = transform_records(mats, DEGREE, check=False), transform_records(mats, DEGREE, adjoint=True, check=False)
            with torch.no_grad():
                moved = [transform_scene(*s, mats, idx, check=False) for s in ins]
            dims = _lib.TransformDims(n=n, sh_coeffs=K, num_transforms=T, reserved0=0, reserved1=0)
            ws = torch.empty(int(lib.lsr_pose_grad_workspace_bytes(n, K, T)), dtype=torch.uint8, device=dev)
            gq, gt, gl = torch.empty(T, 4, device=dev), torch.empty(T, 3, device=dev), torch.empty(T, device=dev)
            c_gin = [_lib.PoseGradIn(xyz=p(s[0]), rotation=p(m[3]), features_rest=p(m[1]), g_xyz=p(u[0]), g_features_rest=p(u[1]),
                                     g_scaling=p(u[2]), g_rotation=p(u[3])) for s, m, u in zip(ins, moved, ups)]
            c_adj_in = [_lib.TransformIn(**{k: p(v) for k, v in zip(NAMES, u)}) for u in ups]
            c_adj_out = _lib.TransformOut(**{k: p(v) for k, v in zip(NAMES, adj_out)})
            ip = None if idx is None else p(idx)
            turn = [0]

            def nxt():
                turn[0] = (turn[0] + 1) % sets
                return turn[0]

            def fused():
                _lib.check(lib.lsr_scene_pose_grad(C.byref(dims), p(rec), ip, p(q), C.byref(c_gin[nxt()]), p(ws), ws.numel(), p(gq), p(gt),
                                                   p(gl), stream), "pose_grad")

            def adjoint():
                _lib.check(lib.lsr_scene_transform(C.byref(dims), p(adj), ip, C.byref(c_adj_in[nxt()]), C.byref(c_adj_out), stream), "adjoint")

            leaves = [v.clone().requires_grad_(True) for v in (q, t, ls)]

            def fused_autograd():
                i = nxt()
                return torch.autograd.grad(pose_scene(*ins[i], *leaves, idx), leaves, ups[i])

            def stock_autograd():
                i = nxt()
                return torch.autograd.grad(stock(*ins[i], *leaves, idx), leaves, ups[i])

            # the two compute the same thing
            fused()
            i = turn[0]
            want = torch.autograd.grad(stock(*ins[i], *leaves, idx), leaves, ups[i])
            rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
            diff = dict(quaternion=rel(gq, want[0]), translation=rel(gt, want[1]), log_scale=rel(gl, want[2]))
            del want
            fu, ad = _alternate((fused, adjoint), dev, a)
            fa, sa = _alternate((fused_autograd, stock_autograd), dev, a)
            nb = pose_grad_bytes(n, idx is not None)
            hbm_ms = nb / HBM_ACHIEVABLE * 1e3
            e = dict(fused=fu, adjoint_launch=ad, fused_autograd=fa, torch_autograd=sa, model_bytes=nb, hbm_ms=hbm_ms,
                     fused_over_hbm=fu["median_ms"] / hbm_ms, fused_over_adjoint=fu["median_ms"] / ad["median_ms"],
                     autograd_speedup=sa["median_ms"] / fa["median_ms"], max_rel_diff_vs_torch=diff)
            entry[pattern] = e
            print(f"n={n:8d} {pattern:14s} fused {fu['median_ms']:8.4f} ms [{fu['min_ms']:.4f}, {fu['max_ms']:.4f}]  = {e['fused_over_hbm']:.2f} x HBM "
                  f"time {hbm_ms:.4f} ms, {e['fused_over_adjoint']:.2f} x adjoint {ad['median_ms']:.4f} ms [{ad['min_ms']:.4f}, {ad['max_ms']:.4f}];  "
                  f"autograd fused {fa['median_ms']:.4f} ms [{fa['min_ms']:.4f}, {fa['max_ms']:.4f}] torch {sa['median_ms']:.4f} ms "
                  f"[{sa['min_ms']:.4f}, {sa['max_ms']:.4f}] x{e['autograd_speedup']:.1f};  max rel diff " +
                  ", ".join(f"{k} {v:.1e}" for k, v in diff.items()), flush=True)
            del moved, c_gin, c_adj_in, ws, leaves
        res[f"n_{n}"] = entry
        del ins, ups, adj_out, contiguous, shuffled
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
