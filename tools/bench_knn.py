#!/usr/bin/env python
"""Device time of the exact three-nearest-neighbour search (csrc/knn.hip, include/lsr_knn.h) that initialises a scene
from a point cloud, and of the stock-PyTorch alternative on the same card.

  knn3         `lsr_knn3` through the C ABI into outputs and a workspace allocated once, mean_dist2 alone (what
               `GaussianScene.from_point_cloud` asks for) and all three outputs
  clouds       `uniform`: U(0, 1)^3;  `clustered`: eight centres, per-point scales exp(U(-7, 0)) around them
  sizes        393 216 and 3 000 000 points
  baseline     at 393 216 only: `torch.cdist` of a chunk of queries against the cloud, then `torch.topk(4, largest=False)`
               (the point itself is the first hit), chunk by chunk.  At 3 000 000 that is 9 x 10^12 pair evaluations and a
               distance matrix of 36 TB in chunks: it is left out
  phases       the per-kernel split is taken by a run of its own under `rocprofv3 --kernel-trace --stats`:
                   rocprofv3 --kernel-trace --stats -d DIR -o knn -- python tools/bench_knn.py --trace-run
                   python tools/bench_knn.py --merge-phases DIR/knn_results.db --json profiles/knn_bench.json

Each sample is `--inner` back-to-back calls between two device events, divided by their number; the figure is the median
of `--samples` (>= 20) after `--warmup` calls, with the smallest and the largest sample beside it.  The baseline takes
seconds per call: it is sampled `--baseline-samples` times, one call each.

usage: python tools/bench_knn.py [--samples 20] [--warmup 3] [--inner 3] [--baseline-samples 5] [--skip-baseline] [--json [profiles/knn_bench.json]]"""
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

SIZES = (393_216, 3_000_000)
CLOUDS = ("uniform", "clustered")
BASELINE_SIZE = 393_216
BASELINE_CHUNK = 2048
TRACE_CALLS = 5
PHASES = (("bbox", "k_knn_bbox"), ("keys", "k_knn_keys"), ("gather", "k_knn_gather"), ("group_boxes", "k_knn_group_boxes"),
          ("search", "k_knn_search"))


def make_cloud(kind: str, n: int, dev) -> torch.Tensor:
    gen = torch.Generator(device=dev).manual_seed(n + len(kind))
    if kind == "uniform":
        return torch.rand((n, 3), device=dev, generator=gen)
    centres = torch.randn((8, 3), device=dev, generator=gen) * 4.0
    which = torch.randint(0, 8, (n,), device=dev, generator=gen)
    scale = torch.exp(-7.0 * torch.rand((n, 1), device=dev, generator=gen))
    return (centres[which] + torch.randn((n, 3), device=dev, generator=gen) * scale).contiguous()


def _sample(fn, dev, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / inner


def _figures(t):
    return dict(ms=statistics.median(t), min_ms=min(t), max_ms=max(t), samples=len(t))


def stock_mean_dist2(p: torch.Tensor) -> torch.Tensor:
    out = torch.empty(p.shape[0], device=p.device)
    for lo in range(0, p.shape[0], BASELINE_CHUNK):
        d = torch.cdist(p[lo:lo + BASELINE_CHUNK], p)
        out[lo:lo + BASELINE_CHUNK] = (torch.topk(d, 4, dim=1, largest=False).values[:, 1:] ** 2).mean(1)
    return out


def _caller(lib, p, dev, all_outputs: bool):
    n = p.shape[0]
    mean = torch.empty(n, device=dev)
    dist2 = torch.empty((n, 3), device=dev) if all_outputs else None
    index = torch.empty((n, 3), device=dev, dtype=torch.int32) if all_outputs else None
    ws = torch.empty(lib.lsr_knn3_workspace_bytes(n), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    from latentsplat_amd import _lib

    def call():
        _lib.check(lib.lsr_knn3(n, ptr(p), ptr(mean), ptr(dist2), ptr(index), ptr(ws), stream), "lsr_knn3")
    return call, mean


def merge_phases(db: str, path: str) -> None:
    """Per-phase mean device time of every (size, cloud) case from the rocpd database of a `--trace-run`."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    rows = [(n, e - s) for n, s, e in rows if "k_knn_" in n or "rocprim" in n]
    calls, cur = [], {}
    for name, ns in rows:
        phase = next((label for label, key in PHASES if key in name), "sort")
        cur[phase] = cur.get(phase, 0) + ns
        if phase == "search":
            calls.append(cur)
            cur = {}
    cases = [(n, kind) for n in SIZES for kind in CLOUDS]
    if len(calls) != TRACE_CALLS * len(cases):
        sys.exit(f"{db}: {len(calls)} lsr_knn3 calls, expected {TRACE_CALLS * len(cases)} (is it the database of a --trace-run?)")
    res = json.load(open(path))
    for i, (n, kind) in enumerate(cases):
        mine = calls[TRACE_CALLS * i + 1:TRACE_CALLS * (i + 1)]          # (the first call of a case is its warm-up)
        phases = {label: statistics.mean(c.get(label, 0) for c in mine) * 1e-6 for label in [p for p, _ in PHASES] + ["sort"]}
        res[f"n_{n}"][kind]["phases_ms"] = dict(phases, total=sum(phases.values()), calls=len(mine),
                                               source="rocprofv3 --kernel-trace --stats, a run of its own (mean_dist2 alone)")
        print(f"n={n:8d} {kind:9s} phases (ms): " + "  ".join(f"{k} {v:.4f}" for k, v in phases.items()), flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--baseline-samples", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true", help="leave the torch baseline out (kernel A/B runs)")
    ap.add_argument("--trace-run", action="store_true", help=f"{TRACE_CALLS} calls per case and nothing else: the run rocprofv3 traces")
    ap.add_argument("--merge-phases", default=None, help="rocpd database of a --trace-run: add the per-phase split to --json")
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "knn_bench.json"), default=None)
    a = ap.parse_args()
    if a.merge_phases:
        return merge_phases(a.merge_phases, a.json or os.path.join(ROOT, "profiles", "knn_bench.json"))
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_knn needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, baseline_chunk=BASELINE_CHUNK,
               device=torch.cuda.get_device_name(dev))
    for n in SIZES:
        entry = dict(n=n, workspace_bytes=int(lib.lsr_knn3_workspace_bytes(n)))
        for kind in CLOUDS:
            p = make_cloud(kind, n, dev)
            if a.trace_run:
                call, _ = _caller(lib, p, dev, False)
                for _ in range(TRACE_CALLS):
                    call()
                torch.cuda.synchronize(dev)
                continue
            case = {}
            for label, all_outputs in (("mean_only", False), ("all_outputs", True)):
                call, mean = _caller(lib, p, dev, all_outputs)
                for _ in range(a.warmup):
                    call()
                case[label] = _figures([_sample(call, dev, a.inner) for _ in range(a.samples)])
            case["points_per_s"] = n / (case["mean_only"]["ms"] * 1e-3)
            line = f"n={n:8d} {kind:9s} knn3 mean only {case['mean_only']['ms']:8.4f} ms [{case['mean_only']['min_ms']:.4f}, {case['mean_only']['max_ms']:.4f}]  " \
                   f"all outputs {case['all_outputs']['ms']:8.4f} ms"
            if n == BASELINE_SIZE and not a.skip_baseline:
                want = stock_mean_dist2(p)
                rel = ((mean - want).abs() / want.clamp_min(1e-30))
                case["baseline_agreement"] = dict(median_relative_difference=float(rel.median()), max_relative_difference=float(rel.max()),
                                                  note="cdist computes in the expanded form |a|^2 + |b|^2 - 2 a.b: the difference is its error")
                base = _figures([_sample(lambda: stock_mean_dist2(p), dev, 1) for _ in range(a.baseline_samples)])
                case["torch_cdist_topk"] = base
                case["speedup"] = base["ms"] / case["mean_only"]["ms"]
                line += f"  torch cdist + topk {base['ms']:9.2f} ms [{base['min_ms']:.2f}, {base['max_ms']:.2f}]  x{case['speedup']:.0f}"
            else:
                case["torch_cdist_topk"] = None      # 9 x 10^12 pair evaluations: left out
            print(line, flush=True)
            entry[kind] = case
            del p
            torch.cuda.empty_cache()
        res[f"n_{n}"] = entry
    if a.json and not a.trace_run:
        os.makedirs(os.path.dirname(a.json), exist_ok=True)
        if os.path.exists(a.json):         # the recorded A/B arms of the design are not this tool's to measure
            old = json.load(open(a.json))
            if "design_ab" in old:
                res["design_ab"] = old["design_ab"]
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
