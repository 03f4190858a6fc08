#!/usr/bin/env python
"""Cost of the absolute view-space gradient (AbsGS; `means2D_abs`, `lsr_backward_absgrad`) on the card it
runs on: forward + backward with and without `means2D_abs`, same inputs, same process.

  headline   `bench.py`'s headline shape reduced to colour alone: 16 views x 300 000 Gaussians x 256 x 256, precomputed
             colours (the headline's 4 feature channels replaced by 3 colour channels: the absolute gradient is supported with
             at most 4 payload channels), one shared scene, through `rasterize_views`
  scene      a degree-3 `GaussianScene` of 393 216 Gaussians (a pixel-aligned encoder-shaped cloud,
             `GaussianScene.from_point_cloud`, all bands active), 4 views x 256 x 256, through `scene.render`

Both arms render with a per-view `(V, G, 3)` `means2D` leaf, as a densifying trainer does; the abs arm adds the `means2D_abs`
leaf.  The forward is the same call in both (the argument only reaches the backward), so only forward + backward is timed.
Samples alternate between the two arms, so both see the same machine; every figure is the median of `--samples` (>= 20)
samples with the fastest and the slowest beside it, `spread` their (max - min) / median, `ratio` abs / classic of the
medians.  Nothing is asserted: the figures are what was measured.

usage: python tools/bench_absgrad.py [--samples 20] [--warmup 5] [--json [profiles/absgrad_bench.json]]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sample(fn, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end)


def _figures(t):
    med = statistics.median(t)
    return dict(ms=med, min_ms=min(t), max_ms=max(t), samples=len(t), spread=(max(t) - min(t)) / med)


def _show(f):
    return f"{f['ms']:8.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]"


def _legs(name, render, leaves, shape, dev, a):
    """render(**kw) -> the tuple of rasterize_views; leaves: the tensors that receive a gradient; shape: (V, G)."""
    weights = None
    m2d = torch.zeros(*shape, 3, device=dev, requires_grad=True)
    mabs = torch.zeros(*shape, 3, device=dev, requires_grad=True)

    def forward_backward(absgrad):
        def run():
            nonlocal weights
            for t in leaves + [m2d, mabs]:
                t.grad = None
            out = [o for o in render(means2D=m2d, **(dict(means2D_abs=mabs) if absgrad else {}))[:4] if o is not None]
            if weights is None:
                gen = torch.Generator(device=dev).manual_seed(0)
                weights = [torch.randn(o.shape, device=dev, generator=gen) for o in out]
            sum((o * w).sum() for o, w in zip(out, weights)).backward()
        return run

    classic, absg = forward_backward(False), forward_backward(True)
    for fn in (classic, absg):
        for _ in range(a.warmup):
            fn()
    tc, ta = [], []
    for _ in range(a.samples):                           # alternating: both arms see the same machine
        tc.append(_sample(classic, dev))
        ta.append(_sample(absg, dev))
    fc, fa = _figures(tc), _figures(ta)
    res = dict(forward_backward=dict(classic=fc, absgrad=fa, ratio=fa["ms"] / fc["ms"]))
    print(f"{name:9s} forward_backward classic {_show(fc)}  absgrad {_show(fa)}  ratio {fa['ms'] / fc['ms']:.4f} "
          f"(spreads {fc['spread']:.3f} / {fa['spread']:.3f})", flush=True)
    return res


def bench_headline(dev, a):
    import bench
    from latentsplat_amd.rasterizer import rasterize_views
    G, V, S = 300_000, 16, 256
    inp = bench.build_inputs(G, V, S, dev, seed=1234)
    colors = torch.rand((G, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    leaves = [inp[k].requires_grad_(True) for k in ("means", "cov", "opac")] + [colors.requires_grad_(True)]
    render = lambda **kw: rasterize_views(inp["views"], S, S, 0, *leaves[:3], colors_precomp=leaves[3], **kw)
    return dict(_legs("headline", render, leaves, (V, G), dev, a), gaussians=G, views=V, size=S, colour_channels=3, feature_channels=0)


def bench_scene(dev, a):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.rasterizer import build_view_table
    from latentsplat_amd.synthetic import make_encoder_scene
    S, V = 256, 4
    sc = make_encoder_scene(context_views=2, size=S, samples=3, views=V, color_sh_degree=None, feature_channels=None)
    n = sc.means.shape[0]
    colors = torch.rand((n, 3), generator=torch.Generator().manual_seed(1))
    scene = GaussianScene.from_point_cloud(sc.means.to(dev), colors.to(dev), sh_degree=3)
    while scene.active_sh_degree < 3:
        scene.oneup_sh_degree()
    with torch.no_grad():
        scene._features_rest.add_(0.02 * torch.randn(scene._features_rest.shape, generator=torch.Generator().manual_seed(2)).to(dev))
    views = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                             torch.zeros(3, device=dev), True)
    leaves = [p for p in scene.parameters() if p.numel()]
    render = lambda **kw: scene.render(views, S, S, **kw)
    return dict(_legs("scene", render, leaves, (V, n), dev, a), gaussians=n, views=V, size=S, sh_degree=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "absgrad_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_absgrad needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev),
               note="classic and absgrad samples alternate in one process on the same inputs; both arms carry a means2D leaf; "
                    "ratio = absgrad / classic of the medians; nothing is asserted")
    res["headline"] = bench_headline(dev, a)
    torch.cuda.empty_cache()
    res["scene"] = bench_scene(dev, a)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
