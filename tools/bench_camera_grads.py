#!/usr/bin/env python
"""Cost of the camera gradient: one forward + backward step with and without dL/d(cameras), alternated in one process.

  bench shape : 16 views x 300 k Gaussians (one shared scene), 4 direct feature channels, 256 x 256 (bench.py's headline
                call through rasterize_views; the camera gradient is requested by a view table that requires grad)
  configs[4]  : DecoderSplattingCUDA.forward, 4 scenes x 4 views x 393 216 Gaussians, colour SH degree 4 + 4-channel latent SH
                degree 2 (bench.py decoder_step_timing's batch4 shape); the gradient goes to the extrinsics
usage: python tools/bench_camera_grads.py [--steps 30] [--rounds 5] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, steps, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / steps


def bench_shape(dev):
    from latentsplat_amd.decoder import cuda_splatting as cs
    from latentsplat_amd.rasterizer import rasterize_views
    from latentsplat_amd.synthetic import make_scene
    sc = make_scene(300_000, image_size=256, views=16, color_sh_degree=None, feature_channels=4).to(dev)
    views0 = cs._view_table(sc.extrinsics, sc.intrinsics, sc.near, sc.far, torch.zeros(3, device=dev), True)
    leaves = [t.clone().requires_grad_(True) for t in (sc.means, cs._pack_covariances(sc.covariances),
                                                        sc.opacities[:, None], sc.feature_sh[..., 0].contiguous())]
    gf = torch.randn((16, 4, 256, 256), device=dev)

    def step(cam):
        views = views0.clone().requires_grad_(cam)
        _, feat, mask, _, _ = rasterize_views(views, 256, 256, 0, leaves[0], leaves[1], leaves[2], features=leaves[3])
        torch.autograd.backward([feat, mask], [gf, torch.ones_like(mask)])
    return step


def configs4(dev):
    from latentsplat_amd import decoder as dec
    from latentsplat_amd.synthetic import make_scene
    scs = [make_scene(393_216, image_size=256, views=4, color_sh_degree=4, feature_channels=4, feature_sh_degree=2,
                      seed=4321 + i).to(dev) for i in range(4)]
    st = lambda name: torch.stack([getattr(sc, name) for sc in scs])
    leaf = lambda name: st(name).contiguous().requires_grad_(True)
    gauss = dec.Gaussians(leaf("means"), leaf("covariances"), leaf("opacities"), leaf("color_sh"), leaf("feature_sh"))
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), [0.0, 0.0, 0.0]).to(dev)
    ext0 = st("extrinsics")
    gc = torch.randn((4, 4, 3, 256, 256), device=dev)
    gf = torch.randn((4, 4, 4, 256, 256), device=dev)

    def step(cam):
        ext = ext0.clone().requires_grad_(cam)
        out = d.forward(gauss, ext, st("intrinsics"), st("near"), st("far"), (256, 256))
        torch.autograd.backward([out.color, out.feature_posterior.mean], [gc, gf])
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for name, make in (("bench_shape_16x300k_C4", bench_shape), ("configs4_decoder_4x4x393k", configs4)):
        step = make(dev)
        for cam in (False, True, False, True):     # warm-up of both variants (speculative sizing, allocator)
            step(cam)
        off, on = [], []
        for _ in range(a.rounds):                  # alternated
            off.append(_time(lambda: step(False), a.steps, dev))
            on.append(_time(lambda: step(True), a.steps, dev))
        res[name] = dict(ms_off=statistics.median(off), ms_on=statistics.median(on),
                         extra_ms=statistics.median(on) - statistics.median(off), off_all=off, on_all=on)
        print(name, json.dumps({k: (round(v, 4) if isinstance(v, float) else [round(x, 4) for x in v])
                                for k, v in res[name].items()}), flush=True)
        del step
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
