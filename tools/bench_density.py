#!/usr/bin/env python
"""Device time of adaptive density control (csrc/density.hip, include/lsr_density.h) against the stock-PyTorch composition
of the published sequence, alternated in one process.

  accumulate   the densification statistics of one step over V = 16 views: `lsr_density_accumulate`, one launch, against
               the published per-view update (`update_filter = radii > 0`, boolean-index `+=` on `xyz_gradient_accum` and
               `denom`, `max` on `max_radii2D`) run once per view
  densify      `plan_densify` -> one host read of the counts -> `torch.randn` -> `apply_densify` over the six parameters
               and their twelve Adam moments (the public wrappers, allocations and the host read included), against
               `densify_and_clone` -> `densify_and_split` -> `prune_points` with `cat_tensors_to_optimizer` /
               `_prune_optimizer` written in torch as published: boolean masks, `cat`, `repeat`, `bmm`
  apply        `lsr_densify_apply` alone through the C ABI into buffers allocated once: the gather's own time, and the
               bytes it must move (per table: the rows it reads plus the rows it writes, plus the map once) as a share of
               the 6.3 TB/s achievable HBM rate of the MI355X
  shape        degree 3 (K = 16) at n = 393 216 and n = 3 000 000; statistics drawn so that roughly 10 % of the Gaussians
               are cloned, 10 % split (N = 2) and 5 % pruned

Each sample is `--inner` back-to-back calls between two device events, divided by their number; the figure is the median
of `--samples` (>= 20) after `--warmup` calls, the variants alternated sample by sample.

usage: python tools/bench_density.py [--samples 20] [--warmup 3] [--inner 3] [--json [profiles/density_bench.json]]"""
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
V = 16
N_SPLIT = 2
SIZES = (393_216, 3_000_000)
THR = dict(grad_threshold=2e-4, dense_extent=0.05, min_opacity=0.005)
NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def _sample(fn, dev, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def _alternate(fused, stock, dev, a):
    for _ in range(a.warmup):
        fused(); stock()
    torch.cuda.synchronize(dev)
    tf, ts = [], []
    for _ in range(a.samples):
        tf.append(_sample(fused, dev, a.inner))
        ts.append(_sample(stock, dev, a.inner))
    return tf, ts


def _figures(tf, ts):
    mf, ms = statistics.median(tf), statistics.median(ts)
    return dict(fused_ms=mf, torch_ms=ms, speedup=ms / mf, fused_min_ms=min(tf), fused_max_ms=max(tf), torch_min_ms=min(ts),
                torch_max_ms=max(ts), faster_than_torch_in_every_sample=bool(max(tf) < min(ts)))


def stock_accumulate(grad, radii, acc, den, mr):
    for v in range(grad.shape[0]):
        vis = radii[v] > 0
        mr[vis] = torch.max(mr[vis], radii[v][vis].float())
        acc[vis] += torch.norm(grad[v][vis, :2], dim=-1, keepdim=True)
        den[vis] += 1


def _build_rotation(r):
    q = r / torch.sqrt((r * r).sum(1))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def stock_densify(params, moments, acc, den, thr, N):
    """The published sequence on a dict of tensors and their Adam moments (no size pruning); returns the new ones."""
    t = dict(params)
    m = {k: list(v) for k, v in moments.items()}

    def postfix(new):
        for k in NAMES:
            m[k] = [torch.cat((s, torch.zeros_like(new[k])), dim=0) for s in m[k]]
            t[k] = torch.cat((t[k], new[k]), dim=0)

    def prune(mask):
        valid = ~mask
        for k in NAMES:
            m[k] = [s[valid] for s in m[k]]
            t[k] = t[k][valid]

    grads = acc / den
    grads[grads.isnan()] = 0.0
    sel = torch.logical_and(torch.norm(grads, dim=-1) >= thr["grad_threshold"],
                            torch.max(torch.exp(t["scaling"]), dim=1).values <= thr["dense_extent"])
    postfix({k: t[k][sel] for k in NAMES})
    padded = torch.zeros(t["xyz"].shape[0], device=grads.device)
    padded[:grads.shape[0]] = grads.squeeze()
    sel = torch.logical_and(padded >= thr["grad_threshold"], torch.max(torch.exp(t["scaling"]), dim=1).values > thr["dense_extent"])
    stds = torch.exp(t["scaling"][sel]).repeat(N, 1)
    samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
    rots = _build_rotation(t["rotation"][sel]).repeat(N, 1, 1)
    new = {k: t[k][sel].repeat(N, *([1] * (t[k].dim() - 1))) for k in NAMES}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][sel].repeat(N, 1)
    new["scaling"] = torch.log(torch.exp(t["scaling"][sel]).repeat(N, 1) / (0.8 * N))
    postfix(new)
    prune(torch.cat((sel, torch.zeros(N * int(sel.sum()), device=sel.device, dtype=torch.bool))))
    prune((torch.sigmoid(t["opacity"]) < thr["min_opacity"]).squeeze())
    return t, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "density_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_density needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    from latentsplat_amd.density import RULES, accumulate_density_stats, apply_densify, plan_densify
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(sh_coeffs=K, views=V, n_split=N_SPLIT, samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner,
               hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, thresholds=THR)
    for n in SIZES:
        gen = torch.Generator(device=dev).manual_seed(n)
        r = lambda *s: torch.randn(s, device=dev, generator=gen)
        u = lambda *s: torch.rand(s, device=dev, generator=gen)
        entry = dict(n=n)

        # ---- accumulate ----
        grad = r(V, n, 3) * 1e-4
        radii = torch.where(u(V, n) < 0.4, 0, (u(V, n) * 40).int()).int()
        stats = [torch.zeros(n, 1, device=dev), torch.zeros(n, 1, device=dev), torch.zeros(n, device=dev)]
        stock_stats = [t.clone() for t in stats]
        accumulate_density_stats(grad, radii, *stats)
        stock_accumulate(grad, radii, stock_stats[0], stock_stats[1], stock_stats[2])
        same = dict(grad_accum=float((stats[0] - stock_stats[0]).abs().max() / stock_stats[0].abs().max()),
                    denom=bool(torch.equal(stats[1], stock_stats[1])), max_radii=bool(torch.equal(stats[2], stock_stats[2])))
        tf, ts = _alternate(lambda: accumulate_density_stats(grad, radii, *stats),
                            lambda: stock_accumulate(grad, radii, stock_stats[0], stock_stats[1], stock_stats[2]), dev, a)
        nbytes = V * n * (12 + 4) + 2 * 3 * n * 4          # whole cache lines of the gradient, the radii, the statistics in and out
        entry["accumulate"] = dict(_figures(tf, ts), model_bytes=nbytes, agrees_with_torch=same,
                                   fused_fraction_of_achievable_hbm=nbytes / (statistics.median(tf) * 1e-3) / HBM_ACHIEVABLE)
        print(f"n={n:8d} accumulate V={V}  fused {statistics.median(tf):7.4f} ms  torch {statistics.median(ts):8.4f} ms  "
              f"x{statistics.median(ts) / statistics.median(tf):.1f}  {entry['accumulate']['fused_fraction_of_achievable_hbm'] * 100:.1f} % of 6.3 TB/s  {same}", flush=True)
        del grad, radii, stock_stats

        # ---- plan + apply: roughly 10 % cloned, 10 % split, 5 % pruned ----
        params = dict(xyz=r(n, 3), features_dc=r(n, 1, 3), features_rest=0.2 * r(n, K - 1, 3), opacity=3.3 * r(n, 1) + 0.14,
                      scaling=torch.log(THR["dense_extent"] * torch.exp(1.5 * (r(n, 3) - 0.82))), rotation=r(n, 4))
        moments = {k: [0.01 * r(*t.shape), 1e-4 * u(*t.shape)] for k, t in params.items()}
        den = torch.full((n, 1), float(V), device=dev)
        acc = den * THR["grad_threshold"] * torch.exp(r(n, 1) - 0.84)          # P(avg >= threshold) ~ 0.2
        mr = torch.zeros(n, device=dev)
        rules = dict(xyz="xyz", scaling="scaling")
        tables = [(params[k], rules.get(k, "copy")) for k in NAMES] + [(s, "zero_new") for k in NAMES for s in moments[k]]
        plan_kw = dict(max_screen_size=0.0, world_limit=0.0, n_split=N_SPLIT, **THR)

        def fused():
            map_, counts = plan_densify(params["opacity"], params["scaling"], acc, den, mr, **plan_kw)
            c = counts.tolist()
            eps = torch.randn((N_SPLIT * c[2], 3), device=dev)
            return map_, counts, c, eps, apply_densify(map_, counts, c[3], tables, n_split=N_SPLIT, scaling=params["scaling"],
                                                       rotation=params["rotation"], eps=eps)

        def stock():
            return stock_densify(params, moments, acc, den, THR, N_SPLIT)

        map_, counts, c, eps, out = fused()
        t_new, _ = stock()
        kept, clones, parents, n_out = c
        entry["outcome"] = dict(kept=kept, clones=clones, split_parents=parents, n_out=n_out,
                                cloned_share=clones / n, split_share=parents / n, dropped_share=1 - (kept + parents) / n,
                                torch_sequence_rows=int(t_new["xyz"].shape[0]),
                                copy_tables_equal_torch=bool(all(torch.equal(o, t_new[k]) for k, o in zip(NAMES, out) if k not in rules)))
        print(f"n={n:8d} outcome {entry['outcome']}", flush=True)
        del t_new
        tf, ts = _alternate(fused, stock, dev, a)
        entry["densify"] = _figures(tf, ts)
        print(f"n={n:8d} densify (plan + read + randn + apply, 18 tables)  fused {statistics.median(tf):7.4f} ms [{min(tf):.4f}, {max(tf):.4f}]  "
              f"torch {statistics.median(ts):8.4f} ms [{min(ts):.4f}, {max(ts):.4f}]  x{statistics.median(ts) / statistics.median(tf):.1f}", flush=True)

        # ---- the gather alone, through the C ABI into buffers allocated once ----
        desc = (_lib.DensifyTable * len(tables))(*[_lib.DensifyTable(t.data_ptr(), o.data_ptr(), t[0].numel(), RULES[rule])
                                                   for (t, rule), o in zip(tables, out)])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())

        def apply_only():
            _lib.check(lib.lsr_densify_apply(n, n_out, p(map_), p(counts), N_SPLIT, desc, len(tables), p(params["scaling"]),
                                             p(params["rotation"]), p(eps), eps.shape[0], stream), "lsr_densify_apply")

        ws = torch.empty(lib.lsr_densify_workspace_bytes(n), dtype=torch.uint8, device=dev)
        dp = _lib.DensifyParams(reserved0=0, reserved1=0, **plan_kw)
        map2, counts2 = torch.empty_like(map_), torch.empty_like(counts)

        def plan_only():
            _lib.check(lib.lsr_densify_plan(n, p(params["opacity"]), p(params["scaling"]), p(acc), p(den), p(mr), C.byref(dp), p(map2),
                                            map2.numel(), p(counts2), p(ws), stream), "lsr_densify_plan")

        ta, tp = _alternate(apply_only, plan_only, dev, a)
        nbytes = 4 * n_out + sum(4 * t[0].numel() * (n_out + (kept if rule == "zero_new" else n_out)) for t, rule in tables)
        ma = statistics.median(ta)
        entry["apply"] = dict(ms=ma, min_ms=min(ta), max_ms=max(ta), model_bytes=nbytes, bytes_per_s=nbytes / (ma * 1e-3),
                              fraction_of_achievable_hbm=nbytes / (ma * 1e-3) / HBM_ACHIEVABLE, tables=len(tables))
        entry["plan"] = dict(ms=statistics.median(tp), min_ms=min(tp), max_ms=max(tp), launches=3)
        print(f"n={n:8d} apply alone {ma:7.4f} ms [{min(ta):.4f}, {max(ta):.4f}]  model {nbytes / 1e6:.1f} MB -> "
              f"{nbytes / (ma * 1e-3) / 1e12:.2f} TB/s = {100 * entry['apply']['fraction_of_achievable_hbm']:.1f} % of 6.3 TB/s;  "
              f"plan alone {entry['plan']['ms']:.4f} ms", flush=True)
        res[f"n_{n}"] = entry
        del params, moments, tables, out, map_, eps, desc
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
