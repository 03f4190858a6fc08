#!/usr/bin/env python
"""Time the optimizer step of a degree-3 3DGS scene: `SceneAdam.step()` (one HIP launch, csrc/optim.hip) against
`torch.optim.Adam(..., foreach=True)` and `torch.optim.Adam(..., fused=True)` on the same card in the same process, and
the visibility-sparse step at visible fractions 1.0, 0.25 and 0.05 under a uniformly random mask and a mask of
contiguous runs.

Every figure is the time of `step()` through the public class, host work included, as a training loop pays it:
gradients and state are allocated and the state created before anything is timed.  A window is `--steps` calls between
two device events; the variants take turns, window by window, `--windows` times each, so that drift of the card or the
host reaches all of them alike.  Reported per variant: the median window in ms per step, the fastest and slowest
window (the run-to-run spread), the ratio to each stock baseline (baseline / this: above 1 is faster than the
baseline), and the share of 6.3 TB/s that 28 bytes per UPDATED element (four reads, three writes) amounts to: for a
sparse step that is the useful traffic, not what the memory system moved — rows of 3 floats share 128-byte lines, so a
random mask saves little on the narrow tables.

Writes profiles/scene_adam_bench.json.

usage: python tools/bench_scene_adam.py [--gaussians 393216 3000000] [--steps 100] [--windows 9] [--out profiles/scene_adam_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = lambda n: dict(_xyz=(n, 3), _features_dc=(n, 1, 3), _features_rest=(n, 15, 3), _opacity=(n, 1), _scaling=(n, 3), _rotation=(n, 4))
RATES = dict(_xyz=1.6e-4, _features_dc=2.5e-3, _features_rest=2.5e-3 / 20, _opacity=5e-2, _scaling=5e-3, _rotation=1e-3)
FLOATS_PER_GAUSSIAN = 59
BYTES_PER_ELEMENT = 28            # p, g, m, v read; p, m, v written
ACHIEVABLE = 6.3e12               # bytes / s: the rate the README's other rows are measured against
RUN = 1024                        # rows per contiguous run of the "runs" mask


def make(n, dev, kind):
    from latentsplat_amd import SceneAdam
    gen = torch.Generator(device=dev).manual_seed(0)
    params = {k: torch.nn.Parameter(torch.randn(s, device=dev, generator=gen)) for k, s in SHAPES(n).items()}
    for p in params.values():
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 0.1
    groups = [dict(params=[p], lr=RATES[k], name=k) for k, p in params.items()]
    if kind == "scene_adam":
        opt = SceneAdam(groups, lr=0.0, eps=1e-15)
    elif kind == "scene_adam_nobc":
        opt = SceneAdam(groups, lr=0.0, eps=1e-15, bias_correction=False)
    else:
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15, **{kind: True})
    return opt


def masks(n, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for frac in (1.0, 0.25, 0.05):
        out[f"random_{frac}"] = torch.rand(n, device=dev, generator=gen) < frac
        runs = torch.rand((n + RUN - 1) // RUN, device=dev, generator=gen) < frac
        out[f"runs_{frac}"] = runs.repeat_interleave(RUN)[:n].contiguous()
    return out


def window(fn, steps, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gaussians", type=int, nargs="+", default=[393216, 3_000_000])
    ap.add_argument("--steps", type=int, default=100, help="step() calls per timed window")
    ap.add_argument("--windows", type=int, default=9, help="windows per variant, taken in turns")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_adam_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_scene_adam needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, steps_per_window=a.steps, windows=a.windows,
               bytes_per_updated_element=BYTES_PER_ELEMENT, achievable_bytes_per_s=ACHIEVABLE, run_rows=RUN, sizes=[])
    for n in a.gaussians:
        variants = {}
        for kind in ("scene_adam", "foreach", "fused"):
            opt = make(n, dev, kind)
            variants[kind] = (opt.step, n)
        sparse_opt = make(n, dev, "scene_adam_nobc")
        for name, m in masks(n, dev).items():
            variants["sparse_" + name] = ((lambda m=m: sparse_opt.step(visibility=m)), int(m.sum()))
        for fn, _ in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in variants}
        for _ in range(a.windows):
            for k, (fn, _) in variants.items():
                times[k].append(window(fn, a.steps, dev))
        rows = {}
        for k, ts in times.items():
            med = statistics.median(ts)
            updated = variants[k][1] * FLOATS_PER_GAUSSIAN
            rows[k] = dict(ms=med, ms_min=min(ts), ms_max=max(ts), spread=(max(ts) - min(ts)) / med, updated_gaussians=variants[k][1],
                           share_of_achievable=updated * BYTES_PER_ELEMENT / (med * 1e-3) / ACHIEVABLE)
        for k, r in rows.items():
            r["vs_foreach"] = rows["foreach"]["ms"] / r["ms"]
            r["vs_fused"] = rows["fused"]["ms"] / r["ms"]
            print(f"n={n:8d} {k:20s} {r['ms']:8.4f} ms  [{r['ms_min']:.4f}, {r['ms_max']:.4f}]  x{r['vs_foreach']:.2f} foreach  "
                  f"x{r['vs_fused']:.2f} fused  {100 * r['share_of_achievable']:5.1f} % of 6.3 TB/s on updated bytes")
        res["sizes"].append(dict(gaussians=n, floats_per_gaussian=FLOATS_PER_GAUSSIAN, variants=rows))
        del variants, sparse_opt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(out=a.out)))
    return res


if __name__ == "__main__":
    main()
