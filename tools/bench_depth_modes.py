#!/usr/bin/env python
"""Cost of a depth mode in the decoder: one ``DecoderSplattingCUDA.forward(depth_mode="disparity")`` + backward step (loss on
colour, latent mean and depth) at the decoder shapes of BASELINE configs[3] (1 scene x 4 views x 393 216 Gaussians) and
configs[4] (4 scenes x 4 views), colour SH degree 4 + 4-channel latent SH degree 2, 256 x 256.  Three variants, alternated in
one process:

  two_pass : the switch off (the default, and what the decoder did before the switch existed): one render for colour /
             features and a second, complete rasterization per scene for the depth image (``render_depth``);
  fused    : ``set_fused_depth_modes(True)``: the one render carries the mode, no second pass;
  no_mode  : ``depth_mode=None`` (the native depth output in the loss): the floor.

``--variants two_pass,no_mode`` runs a subset (e.g. this script copied into a checkout of an earlier commit, which has no
fused path).  usage: python tools/bench_depth_modes.py [--steps 20] [--rounds 5] [--json profiles/depth_modes_bench.json]"""
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


def decoder_shape(dev, scenes):
    from latentsplat_amd import decoder as dec
    from latentsplat_amd.synthetic import make_scene
    scs = [make_scene(393_216, image_size=256, views=4, color_sh_degree=4, feature_channels=4, feature_sh_degree=2,
                      seed=4321 + i).to(dev) for i in range(scenes)]
    st = lambda name: torch.stack([getattr(sc, name) for sc in scs])
    leaf = lambda name: st(name).contiguous().requires_grad_(True)
    gauss = dec.Gaussians(leaf("means"), leaf("covariances"), leaf("opacities"), leaf("color_sh"), leaf("feature_sh"))
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), [0.0, 0.0, 0.0]).to(dev)
    cams = (st("extrinsics"), st("intrinsics"), st("near"), st("far"))
    gc = torch.randn((scenes, 4, 3, 256, 256), device=dev)
    gf = torch.randn((scenes, 4, 4, 256, 256), device=dev)
    gd = torch.randn((scenes, 4, 256, 256), device=dev)

    # (a checkout from before the switch existed, measured for comparison with --variants two_pass,no_mode, has no setter)
    set_fused = getattr(dec, "set_fused_depth_modes", lambda on: None)

    def step(variant):
        set_fused(variant == "fused")
        try:
            out = d.forward(gauss, *cams, (256, 256), depth_mode=None if variant == "no_mode" else "disparity")
        finally:
            set_fused(False)
        torch.autograd.backward([out.color, out.feature_posterior.mean, out.depth], [gc, gf, gd])
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="two_pass,fused,no_mode")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    variants = a.variants.split(",")
    dev = torch.device("cuda:0")
    res = {}
    for name, scenes in (("configs3_decoder_1x4x393k", 1), ("configs4_decoder_4x4x393k", 4)):
        step = decoder_shape(dev, scenes)
        for _ in range(2):                         # warm-up of every variant (speculative sizing, allocator)
            for v in variants:
                step(v)
        ms = {v: [] for v in variants}
        for _ in range(a.rounds):                  # alternated
            for v in variants:
                ms[v].append(_time(lambda: step(v), a.steps, dev))
        r = {f"ms_{v}": statistics.median(ms[v]) for v in variants}
        r.update({f"{v}_all": ms[v] for v in variants})
        if "two_pass" in ms and "fused" in ms:
            r["two_pass_over_fused"] = r["ms_two_pass"] / r["ms_fused"]
        if "no_mode" in ms and "fused" in ms:
            r["fused_over_no_mode"] = r["ms_fused"] / r["ms_no_mode"]
        res[name] = r
        print(name, json.dumps({k: (round(v, 4) if isinstance(v, float) else [round(x, 4) for x in v]) for k, v in r.items()}), flush=True)
        del step
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
