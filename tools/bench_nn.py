#!/usr/bin/env python
"""Device time of the cross-cloud nearest-neighbour query (csrc/nn.hip, include/lsr_nn.h) behind the mesh metrics, of
`knn3` on the same cloud in the same process (the yardstick), of a stock-PyTorch baseline, and of the connected
components of the two meshes `tools/bench_tsdf.py` extracts.

  build        `lsr_nn_build` through the C ABI into index memory and a workspace allocated once
  query        `lsr_nn_query` into preallocated `dist2` and `index`, workspace allocated once
  self         build + query of a cloud against itself (n = m), and `lsr_knn3` (mean_dist2 alone, its cheapest form) on
               that cloud: `self_over_knn3` is the ratio of the two medians.  A self query finds distance 0 in its seed
               chunk and visits nothing else, so `near_build_plus_query_over_knn3` (the medians of build and of the near
               query, added, over knn3's) is recorded beside it
  rotation     every call takes the next of several copies of its inputs (reference clouds, query clouds, indexes), enough
               of them that a round exceeds the 256 MB last-level cache: no call finds its input there from the call before
  references   `uniform`: U(0, 1)^3;  `clustered`: eight centres, per-point scales exp(U(-7, 0)) around them (those of
               tools/bench_knn.py);  `sphere`: points on the unit sphere (surface-like)
  queries      `near`: drawn as the reference is (another seed);  `far5`: the same with 5 % of the queries moved 10 to 20
               reference extents away, in random directions (`far_over_near` is the seed's price)
  sizes        (n, m) = (393 216, 393 216) and (3 000 000, 3 000 000)
  baseline     at 393 216 only: `torch.cdist` of a chunk of queries against the reference, then `min`, chunk by chunk.  At
               3 000 000 that is 9 x 10^12 pair evaluations: it is left out
  components   `mesh_components` on the meshes of the 256^3 and 512^3 sphere volumes of tools/bench_tsdf.py: rounds used and
               time, against `extract_mesh` on the same volume
  phases       the per-kernel split is taken by a run of its own under `rocprofv3 --kernel-trace --stats`:
                   rocprofv3 --kernel-trace --stats -d DIR -o nn -- python tools/bench_nn.py --trace-run

Each sample is `--inner` back-to-back calls between two device events, divided by their number; the figure is the median
of `--samples` (>= 20) after `--warmup` calls, with the smallest and the largest sample beside it.

usage: python tools/bench_nn.py [--samples 20] [--warmup 3] [--inner 3] [--baseline-samples 3] [--skip-baseline]
                                [--skip-components] [--json [profiles/nn_bench.json]]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = ((393_216, 393_216), (3_000_000, 3_000_000))
REFERENCES = ("uniform", "clustered", "sphere")
QUERIES = ("near", "far5")
BASELINE_SIZE = 393_216
BASELINE_CHUNK = 2048
CACHE_BYTES = 256e6
TRACE_CALLS = 5


def make_cloud(kind: str, n: int, dev, seed: int) -> torch.Tensor:
    gen = torch.Generator(device=dev).manual_seed(1000 * seed + n % 997 + len(kind))
    if kind == "uniform":
        return torch.rand((n, 3), device=dev, generator=gen)
    if kind == "sphere":
        g = torch.randn((n, 3), device=dev, generator=gen)
        return (g / g.norm(dim=1, keepdim=True).clamp_min(1e-20)).contiguous()
    centres = torch.randn((8, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(n + len(kind))) * 4.0
    which = torch.randint(0, 8, (n,), device=dev, generator=gen)
    scale = torch.exp(-7.0 * torch.rand((n, 1), device=dev, generator=gen))
    return (centres[which] + torch.randn((n, 3), device=dev, generator=gen) * scale).contiguous()


def make_queries(kind: str, mode: str, m: int, dev, seed: int) -> torch.Tensor:
    q = make_cloud(kind, m, dev, seed)
    if mode == "far5":
        gen = torch.Generator(device=dev).manual_seed(seed + 77)
        extent = float((q.max(dim=0).values - q.min(dim=0).values).max())
        far = torch.rand((m,), device=dev, generator=gen) < 0.05
        way = torch.randn((m, 3), device=dev, generator=gen)
        way = way / way.norm(dim=1, keepdim=True).clamp_min(1e-20) * (extent * (10.0 + 10.0 * torch.rand((m, 1), device=dev, generator=gen)))
        q = torch.where(far[:, None], q + way, q).contiguous()
    return q


def copies_for(nbytes: int) -> int:
    return max(2, math.ceil(1.2 * CACHE_BYTES / max(nbytes, 1)))


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


def _show(f):
    return f"{f['ms']:8.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]"


def _time(fn, dev, a, samples=None, inner=None, warmup=None):
    for _ in range(a.warmup if warmup is None else warmup):
        fn()
    return _figures([_sample(fn, dev, inner or a.inner) for _ in range(samples or a.samples)])


def stock_nearest(q: torch.Tensor, r: torch.Tensor):
    dist = torch.empty(q.shape[0], device=q.device)
    index = torch.empty(q.shape[0], device=q.device, dtype=torch.int64)
    for lo in range(0, q.shape[0], BASELINE_CHUNK):
        d, i = torch.cdist(q[lo:lo + BASELINE_CHUNK], r).min(dim=1)
        dist[lo:lo + BASELINE_CHUNK], index[lo:lo + BASELINE_CHUNK] = d, i
    return dist, index


class Case:
    """The rotating inputs of one (n, m, reference kind) and the calls over them."""

    def __init__(self, lib, kind, n, m, dev):
        from latentsplat_amd import _lib
        self.lib, self.check, self.n, self.m, self.dev = lib, _lib.check, n, m, dev
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.index_bytes = int(lib.lsr_nn_index_bytes(n))
        self.refs = [make_cloud(kind, n, dev, s) for s in range(copies_for(12 * n))]
        self.mems = [torch.empty(self.index_bytes, dtype=torch.uint8, device=dev) for _ in range(copies_for(self.index_bytes))]
        self.build_ws = torch.empty(lib.lsr_nn_build_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.query_ws = torch.empty(lib.lsr_nn_query_workspace_bytes(max(n, m)), dtype=torch.uint8, device=dev)
        self.knn_ws = torch.empty(lib.lsr_knn3_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.dist2 = torch.empty(max(n, m), device=dev)
        self.index = torch.empty(max(n, m), device=dev, dtype=torch.int32)
        self.turn = 0
        for k in range(len(self.mems)):                             # every index holds a built reference from the start
            self._build(self.refs[k % len(self.refs)], self.mems[k])
        torch.cuda.synchronize(dev)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def _build(self, ref, mem):
        self.check(self.lib.lsr_nn_build(self.n, self._p(ref), self._p(mem), self._p(self.build_ws), self.stream), "lsr_nn_build")

    def _query(self, mem, q):
        self.check(self.lib.lsr_nn_query(self.n, self._p(mem), q.shape[0], self._p(q), self._p(self.dist2), self._p(self.index),
                                         self._p(self.query_ws), self.stream), "lsr_nn_query")

    def build(self):
        self.turn += 1
        self._build(self.refs[self.turn % len(self.refs)], self.mems[self.turn % len(self.mems)])

    def query_of(self, queries):
        def call():
            self.turn += 1
            self._query(self.mems[self.turn % len(self.mems)], queries[self.turn % len(queries)])
        return call

    def self_query(self):
        self.turn += 1
        ref, mem = self.refs[self.turn % len(self.refs)], self.mems[self.turn % len(self.mems)]
        self._build(ref, mem)
        self._query(mem, ref)

    def knn3(self):
        self.turn += 1
        ref = self.refs[self.turn % len(self.refs)]
        self.check(self.lib.lsr_knn3(self.n, self._p(ref), self._p(self.dist2), None, None, self._p(self.knn_ws), self.stream), "lsr_knn3")


def bench_case(lib, kind, n, m, dev, a) -> dict:
    case = Case(lib, kind, n, m, dev)
    res = dict(index_bytes=case.index_bytes, reference_copies=len(case.refs), index_copies=len(case.mems))
    if a.trace_run:
        near = [make_queries(kind, "near", m, dev, 100)]
        for fn in (case.build, case.query_of(near), case.self_query, case.knn3):
            for _ in range(TRACE_CALLS):
                fn()
        torch.cuda.synchronize(dev)
        return res
    res["build"] = _time(case.build, dev, a)
    for mode in QUERIES:
        queries = [make_queries(kind, mode, m, dev, 100 + s) for s in range(copies_for(12 * m))]
        res[f"query_{mode}"] = _time(case.query_of(queries), dev, a)
        res[f"query_{mode}"]["queries_per_s"] = m / (res[f"query_{mode}"]["ms"] * 1e-3)
        if mode == "near" and n == BASELINE_SIZE and not a.skip_baseline:
            q, r = queries[0], case.refs[0]
            case._build(r, case.mems[0])
            case._query(case.mems[0], q)
            want_d, want_i = stock_nearest(q, r)
            got_d, got_i = torch.sqrt(case.dist2[:m]), case.index[:m].long()
            rel = (got_d - want_d).abs() / want_d.clamp_min(1e-30)
            res["baseline_agreement"] = dict(median_relative_difference=float(rel.median()), max_relative_difference=float(rel.max()),
                                             indices_equal=float((got_i == want_i).float().mean()),
                                             note="cdist computes in the expanded form |a|^2 + |b|^2 - 2 a.b: the difference is its error")
            res["torch_cdist_min"] = _time(lambda: stock_nearest(q, r), dev, a, samples=a.baseline_samples, inner=1, warmup=1)
            res["speedup"] = res["torch_cdist_min"]["ms"] / res["query_near"]["ms"]
        del queries
    res["far_over_near"] = res["query_far5"]["ms"] / res["query_near"]["ms"]
    if n == m:
        res["self_build_and_query"] = _time(case.self_query, dev, a)
        res["knn3_mean_only"] = _time(case.knn3, dev, a)
        res["self_over_knn3"] = res["self_build_and_query"]["ms"] / res["knn3_mean_only"]["ms"]
        res["near_build_plus_query_over_knn3"] = (res["build"]["ms"] + res["query_near"]["ms"]) / res["knn3_mean_only"]["ms"]
    line = f"n={n:8d} m={m:8d} {kind:9s} build {_show(res['build'])}  query near {_show(res['query_near'])}  far5 {_show(res['query_far5'])} " \
           f"(x{res['far_over_near']:.2f})"
    if n == m:
        line += f"  self {_show(res['self_build_and_query'])}  knn3 {_show(res['knn3_mean_only'])}  ratio {res['self_over_knn3']:.2f}"
    if "torch_cdist_min" in res:
        line += f"  torch cdist + min {res['torch_cdist_min']['ms']:9.2f} ms  x{res['speedup']:.0f}"
    print(line, flush=True)
    return res


def bench_components(dev, a) -> dict:
    """mesh_components on the two meshes tools/bench_tsdf.py extracts, beside extract_mesh on the same volume."""
    import bench_tsdf as bt
    from latentsplat_amd.mesh import TSDFVolume, mesh_components
    out = {}
    for n, V, size in bt.SHAPES:
        gen = torch.Generator(device=dev).manual_seed(n + V)
        views = bt.circle_views(V, dev)
        depth, alpha, color = bt.sphere_images(V, size, dev, gen)
        half = 1.25 * bt.RADIUS
        vol = TSDFVolume((-half,) * 3, 2 * half / (n - 1), (n, n, n), device=dev)
        vol.integrate(depth, alpha, views, color=color)
        vertices, faces, _ = vol.extract_mesh()
        labels, rounds = mesh_components(faces, vertices.shape[0], return_rounds=True)
        res = dict(vertices=int(vertices.shape[0]), faces=int(faces.shape[0]), rounds=rounds, components=int(torch.unique(labels).numel()))
        res["extract_mesh"] = _time(lambda: vol.extract_mesh(), dev, a, inner=1)
        res["mesh_components"] = _time(lambda: mesh_components(faces, vertices.shape[0]), dev, a, inner=1)
        res["components_over_extraction"] = res["mesh_components"]["ms"] / res["extract_mesh"]["ms"]
        print(f"components {n}^3: {res['vertices']} vertices, {res['faces']} faces, {res['components']} components, {rounds} rounds; "
              f"mesh_components (range check, rounds, host reads) {_show(res['mesh_components'])}  extract_mesh {_show(res['extract_mesh'])}", flush=True)
        out[f"volume_{n}"] = res
        del vol, depth, alpha, color, vertices, faces
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--baseline-samples", type=int, default=3)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--skip-components", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help=f"{TRACE_CALLS} calls of each kind per case and nothing else: the run rocprofv3 traces")
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "nn_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_nn needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(samples=a.samples, warmup=a.warmup, calls_per_sample=a.inner, baseline_chunk=BASELINE_CHUNK,
               cache_bytes_rotated_over=1.2 * CACHE_BYTES, device=torch.cuda.get_device_name(dev))
    for n, m in SIZES:
        entry = dict(n=n, m=m)
        for kind in REFERENCES:
            entry[kind] = bench_case(lib, kind, n, m, dev, a)
            torch.cuda.empty_cache()
        res[f"n_{n}_m_{m}"] = entry
    if not a.skip_components and not a.trace_run:
        res["components"] = bench_components(dev, a)
    if a.json and not a.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
