#!/usr/bin/env python
"""Device time of the similarity transform of a scene (`lsr_scene_transform`, csrc/scene_transform.hip) against the
stock-PyTorch composition of the same map and against the activation kernel, in one process on one card.

  fused   one launch over the raw parameters through the C ABI into buffers allocated once: a uniform transform out of
          place and in place, 64 transforms with a random per-Gaussian index, and forward + backward through the public
          autograd op (`transform_scene` + `torch.autograd.backward`: records launches, allocations and Python included)
  torch   the same map from the same records: a `matmul` for the positions, the quaternion product written out, an add for
          the log-scales, one `einsum` per band and a `cat`.  Indexed: the rows sorted by transform, that composition on each
          part's slice, the results scattered back (`torch_gathered_records` beside it: the records gathered per Gaussian
          and batched einsums: somewhat faster at 393 216 rows, six times slower at 3 000 000)
  yardstick  `lsr_scene_activate_forward` at the same row count in the same run, both normalised by the bytes that must move
  shape   degree 3 (K = 16) at n = 393 216 and n = 3 000 000

Each sample is `--inner` back-to-back calls between two device events, divided by their number; every call of every leg
takes the next of several buffer sets (inputs, outputs, and for the autograd leg leaves and upstream gradients) whose
inputs alone exceed twice the 256 MiB last-level cache, so that no call finds its inputs there.  The
figure is the median of `--samples` (>= 20) after `--warmup` calls with the fastest and slowest beside it, fused and torch
alternated sample by sample.  Bytes that must move per Gaussian, out of place: 2 * 4 * (3 + 3 (K - 1) + 3 + 4) (+ 4 with an
index); the rate is that over the time, as a fraction of the 6.3 TB/s achievable HBM rate of the MI355X.

usage: python tools/bench_scene_transform.py [--samples 20] [--warmup 3] [--inner 4] [--json [profiles/scene_transform_bench.json]]"""
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


def transform_bytes(n: int, indexed: bool = False) -> int:
    return n * (2 * 4 * (3 + 3 * (K - 1) + 3 + 4) + (4 if indexed else 0))


def activation_bytes(n: int) -> int:
    return n * 4 * ((3 * K + 8) + (3 * K + 7))


def torch_composition(rec, xyz, features_rest, scaling, rotation, idx=None):
    """The map from one record (or, with idx, from the records gathered per Gaussian)."""
    r = rec[0] if idx is None else rec[idx.long()]
    A, t, ls, q = r[..., :9].reshape(*r.shape[:-1], 3, 3), r[..., 9:12], r[..., 12:13], r[..., 13:17]
    if idx is None:
        x = xyz @ A.T + t
    else:
        x = torch.einsum("nij,nj->ni", A, xyz) + t
    aw, ax, ay, az = q[..., 0:1], q[..., 1:2], q[..., 2:3], q[..., 3:4]
    bw, bx, by, bz = rotation[:, 0:1], rotation[:, 1:2], rotation[:, 2:3], rotation[:, 3:4]
    rot = torch.cat([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=1)
    bands, off = [], 20
    for l in range(1, DEGREE + 1):
        m = 2 * l + 1
        T = r[..., off:off + m * m].reshape(*r.shape[:-1], m, m)
        c = features_rest[:, l * l - 1:(l + 1) ** 2 - 1]
        bands.append(torch.einsum("ij,njc->nic" if idx is None else "nij,njc->nic", T, c))
        off += m * m
    return x, torch.cat(bands, dim=1), scaling + ls, rot


def torch_composition_by_part(rec, xyz, features_rest, scaling, rotation, idx):
    """The indexed map as a stock composition would do it: the rows sorted by their transform (one argsort, one host read of
    the counts), the uniform composition on each part's contiguous slice, the results scattered back."""
    given = (xyz, features_rest, scaling, rotation)
    order = torch.argsort(idx.long())
    counts = torch.bincount(idx.long(), minlength=rec.shape[0]).tolist()
    gathered = [t[order] for t in given]
    parts, start = [], 0
    for k, count in enumerate(counts):
        if count:
            parts.append(torch_composition(rec[k:k + 1], *(t[start:start + count] for t in gathered)))
            start += count
    outs = []
    for j, t in enumerate(given):
        o = torch.empty_like(t)
        o[order] = torch.cat([part[j] for part in parts], dim=0)
        outs.append(o)
    return tuple(outs)


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
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "scene_transform_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_scene_transform needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    from latentsplat_amd.transform import similarity_matrix, transform_records, transform_scene
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator().manual_seed(7)
    mats = torch.stack([similarity_matrix(torch.randn(4, generator=gen), torch.randn(3, generator=gen) * 10,
                                          float(torch.empty(1).uniform_(0.5, 2.0, generator=gen))) for _ in range(PARTS)]).to(dev)
    rec1, rec64 = transform_records(mats[:1], DEGREE), transform_records(mats, DEGREE)
    res = dict(sh_coeffs=K, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE,
               last_level_cache_bytes=LLC_BYTES, transforms_indexed=PARTS)
    for n in SIZES:
        g = torch.Generator(device=dev).manual_seed(n)
        r = lambda *s: torch.randn(s, device=dev, generator=g)
        sets = max(2, -(-2 * LLC_BYTES // (transform_bytes(n) // 2)) + 1)         # inputs alone exceed twice the cache
        ins = [dict(xyz=3 * r(n, 3), features_rest=0.3 * r(n, K - 1, 3), scaling=r(n, 3) - 3, rotation=r(n, 4)) for _ in range(sets)]
        extra = [(r(n, 1, 3), 3 * r(n, 1)) for _ in range(sets)]                       # features_dc, opacity: the activation's
        outs = [{k: torch.empty_like(t) for k, t in s.items()} for s in ins]          # the outputs rotate with the inputs
        acts_out = [dict(shs=torch.empty((n, K, 3), device=dev), opacities=torch.empty((n, 1), device=dev),
                         cov3D=torch.empty((n, 6), device=dev)) for _ in range(sets)]
        idx = torch.randint(0, PARTS, (n,), device=dev, generator=g, dtype=torch.int32)
        c_in = [_lib.TransformIn(**{k: p(t) for k, t in s.items()}) for s in ins]
        c_out = [_lib.TransformOut(**{k: p(t) for k, t in o.items()}) for o in outs]
        c_inplace = [_lib.TransformOut(**{k: p(t) for k, t in s.items()}) for s in ins]
        c_params = [_lib.SceneParams(p(e[0]), p(s["features_rest"]), p(e[1]), p(s["scaling"]), p(s["rotation"])) for s, e in zip(ins, extra)]
        c_act = [_lib.SceneOutputs(p(o["shs"]), p(o["opacities"]), p(o["cov3D"]), None, None) for o in acts_out]
        d1 = _lib.TransformDims(n=n, sh_coeffs=K, num_transforms=1, reserved0=0, reserved1=0)
        d64 = _lib.TransformDims(n=n, sh_coeffs=K, num_transforms=PARTS, reserved0=0, reserved1=0)
        dact = _lib.SceneDims(n=n, sh_coeffs=K, scale_modifier=1.0, reserved0=0, reserved1=0)
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % sets
            return turn[0]

        def fused_uniform():
            i = nxt()
            _lib.check(lib.lsr_scene_transform(C.byref(d1), p(rec1), None, C.byref(c_in[i]), C.byref(c_out[i]), stream), "transform")

        def fused_inplace():
            i = nxt()
            _lib.check(lib.lsr_scene_transform(C.byref(d1), p(rec1), None, C.byref(c_in[i]), C.byref(c_inplace[i]), stream), "transform")

        def fused_indexed():
            i = nxt()
            _lib.check(lib.lsr_scene_transform(C.byref(d64), p(rec64), p(idx), C.byref(c_in[i]), C.byref(c_out[i]), stream), "transform")

        def activation():
            i = nxt()
            _lib.check(lib.lsr_scene_activate_forward(C.byref(dact), C.byref(c_params[i]), C.byref(c_act[i]), stream), "activate")

        def stock_uniform():
            with torch.no_grad():
                torch_composition(rec1, **ins[nxt()])

        def stock_indexed():
            with torch.no_grad():
                torch_composition_by_part(rec64, **ins[nxt()], idx=idx)

        def stock_indexed_gathered():
            with torch.no_grad():
                torch_composition(rec64, **ins[nxt()], idx=idx)

        # forward + backward: leaves and upstream gradients rotate over as many sets as the other legs
        ups = [[torch.randn_like(s[k]) for k in NAMES] for s in ins]
        leaves = [[s[k].clone().requires_grad_(True) for k in NAMES] for s in ins]

        def fused_fwd_bwd():
            i = nxt()
            for t in leaves[i]:
                t.grad = None
            torch.autograd.backward(transform_scene(*leaves[i], mats[:1], check=False), ups[i])

        def stock_fwd_bwd():
            i = nxt()
            for t in leaves[i]:
                t.grad = None
            torch.autograd.backward(torch_composition(rec1, *leaves[i]), ups[i])

        # the two compute the same thing
        fused_uniform()
        with torch.no_grad():
            want = torch_composition(rec1, **ins[turn[0]])
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
        diff = {k: rel(outs[turn[0]][k], w) for k, w in zip(NAMES, want)}
        fused_indexed()
        with torch.no_grad():
            want = torch_composition_by_part(rec64, **ins[turn[0]], idx=idx)
            same = torch_composition(rec64, **ins[turn[0]], idx=idx)
        diff.update({k + "_indexed": rel(outs[turn[0]][k], w) for k, w in zip(NAMES, want)})
        diff.update({k + "_indexed_gathered": rel(outs[turn[0]][k], w) for k, w in zip(NAMES, same)})
        del want, same
        entry = dict(n=n, buffer_sets=sets, max_rel_diff_vs_torch=diff)
        nb, nbi, nba = transform_bytes(n), transform_bytes(n, True), activation_bytes(n)
        uni, sto, acts = _alternate((fused_uniform, stock_uniform, activation), dev, a)
        inp, = _alternate((fused_inplace,), dev, a)
        for s in ins:                                   # (the in-place leg moved every set: bring the values back to scale)
            s["xyz"].normal_(); s["scaling"].normal_().sub_(3)
        ind, sti, stg = _alternate((fused_indexed, stock_indexed, stock_indexed_gathered), dev, a)
        fb, sfb = _alternate((fused_fwd_bwd, stock_fwd_bwd), dev, a)
        frac = lambda b, st: b / (st["median_ms"] * 1e-3) / HBM_ACHIEVABLE
        entry["uniform_out_of_place"] = dict(fused=uni, torch=sto, speedup=sto["median_ms"] / uni["median_ms"], model_bytes=nb,
                                             fused_fraction_of_achievable_hbm=frac(nb, uni))
        entry["uniform_in_place"] = dict(fused=inp, model_bytes=nb, fused_fraction_of_achievable_hbm=frac(nb, inp))
        entry["indexed_64"] = dict(fused=ind, torch=sti, torch_gathered_records=stg, speedup=sti["median_ms"] / ind["median_ms"], model_bytes=nbi,
                                   fused_fraction_of_achievable_hbm=frac(nbi, ind))
        entry["forward_backward_autograd"] = dict(fused=fb, torch=sfb, speedup=sfb["median_ms"] / fb["median_ms"], model_bytes=2 * nb,
                                                  fused_fraction_of_achievable_hbm=frac(2 * nb, fb))
        entry["activation_yardstick"] = dict(fused=acts, model_bytes=nba, fused_fraction_of_achievable_hbm=frac(nba, acts),
                                             transform_rate_over_activation_rate=frac(nb, uni) / frac(nba, acts))
        for leg in ("uniform_out_of_place", "uniform_in_place", "indexed_64", "forward_backward_autograd", "activation_yardstick"):
            e = entry[leg]
            f = e["fused"]
            line = f"n={n:8d} {leg:26s} fused {f['median_ms']:8.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]  {100 * e['fused_fraction_of_achievable_hbm']:5.1f} % of 6.3 TB/s"
            if "torch" in e:
                t = e["torch"]
                line += f"  torch {t['median_ms']:9.4f} ms [{t['min_ms']:.4f}, {t['max_ms']:.4f}]  x{e['speedup']:.1f}"
            print(line, flush=True)
        print(f"n={n:8d} transform rate / activation rate (bytes-normalised): {entry['activation_yardstick']['transform_rate_over_activation_rate']:.3f}", flush=True)
        print(f"n={n:8d} fused vs torch, max relative difference: " + ", ".join(f"{k} {v:.1e}" for k, v in diff.items()), flush=True)
        res[f"n_{n}"] = entry
        del ins, extra, outs, acts_out, idx, leaves, ups, c_in, c_out, c_act, c_inplace, c_params
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
