#!/usr/bin/env python
"""Device time of the depth distortion regulariser (csrc/distortion.hip, include/lsr_distortion.h, latentsplat_amd.distortion)
on the card it runs on.

  A       `lsr_scene_depth_moments_forward`, and forward + `_backward`, through the Python layer into outputs allocated once,
          at 393 216 and 3 000 000 Gaussians x 4 and 16 views (space ndc, a pivot per view)
  B       `lsr_distortion_loss_forward` (the loss alone), and forward + `_backward` (both gradients), likewise, at
          16 x 256 x 256 and 4 x 1024 x 1024
  stock   the stock float32 PyTorch composition of the same definitions in the same process on the same card, and with autograd
  scene   a degree-3 scene of 393 216 Gaussians at 4 views of 512 x 512, forward + backward, alternating in one process:
          `render` + L1 against `render_with_distortion` + L1 + the loss; `render_with_normals` + the normal loss against
          `render_surface` + both losses; and the `torch.cat` that joins the two payloads in `render_surface`, alone
  pivot   the accuracy figures of tests/test_distortion_gpu.py::test_the_pivot_takes_the_cancellation_out
          (tests/distortion_ref.py::pivot_errors)

Every arm rotates over as many copies of its large arrays as make more than the 256 MB last-level cache, each call on the next
copy; every timed shape is warmed up; every figure is the median of `--samples` (>= 20) samples with the smallest and the
largest beside it.  Each HIP figure is also given as the fraction of the 6.3 TB/s achievable rate that the bytes the kernel must
move amount to: A forward writes 8 B per (view, Gaussian) and reads 12 B per Gaussian, its backward reads the 8 and the 12 and
writes 12 B per Gaussian; B forward reads 12 B per pixel (two moments, alpha), its backward reads them again and writes 12.

usage: python tools/bench_distortion.py [--samples 20] [--warmup 3] [--json [profiles/distortion_bench.json]] [--skip-scene]"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_normals import ALPHA_MIN, CACHE_BYTES, HBM_BYTES_PER_S, _figures, _sample, _show, _time, circle_views  # noqa: E402

GAUSSIANS, VIEWS = (393_216, 3_000_000), (4, 16)
IMAGES = ((16, 256, 256), (4, 1024, 1024))
NEAR, FAR = 1.0, 100.0


# ---- the stock float32 composition of the definitions of include/lsr_distortion.h ----

def stock_moments(views, xyz, pivot):
    s = views[:, 40, None]
    row = torch.stack([views[:, 2], views[:, 6], views[:, 10]], -1)
    z = (torch.einsum("vj,nj->vn", row, xyz) * s + views[:, 14, None]) / s
    ok = torch.isfinite(z) & (z > 0)
    zs = torch.where(ok, z, torch.ones_like(z))
    n, f = views[:, 42, None], views[:, 43, None]
    mp = f / (f - n) * (1.0 - n / zs) - pivot[:, None]
    out = torch.stack([mp, mp * mp], -1)
    return torch.where(ok[..., None], out, torch.zeros_like(out))


def stock_loss(moment_map, alpha):
    d = alpha * moment_map[:, 1] - moment_map[:, 0] * moment_map[:, 0]
    return (d.sum((1, 2)) / (alpha.shape[1] * alpha.shape[2])).mean()


# ---- arms ----

def bench_A(n, V, dev, a):
    from latentsplat_amd.distortion import depth_moments_backward, depth_moments_forward, depth_pivot, with_near_far
    gen = torch.Generator(device=dev).manual_seed(n + V)
    views = with_near_far(circle_views(V, dev), NEAR, FAR)
    pivot = depth_pivot(views, (0.0, 0.0, 0.0), "ndc").to(dev)
    out_bytes, row_bytes = 8 * V * n, 12 * n
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (out_bytes + row_bytes)))
    sets = [dict(xyz=torch.rand((n, 3), device=dev, generator=gen) * 2 - 1, out=torch.empty((V, n, 2), device=dev),
                 grad=torch.empty((n, 3), device=dev)) for _ in range(copies)]
    ups = [torch.randn((V, n, 2), device=dev, generator=gen) for _ in range(copies)]

    def hip(backward):
        def run():
            for s, up in zip(sets, ups):
                depth_moments_forward(views, s["xyz"], "ndc", pivot, out=s["out"], check=False)
                if backward:
                    depth_moments_backward(views, s["xyz"], up, "ndc", pivot, out=s["grad"])
        return run

    turn = [0]

    def stock(backward):
        def run():
            turn[0] = (turn[0] + 1) % copies
            s = sets[turn[0]]
            if not backward:
                with torch.no_grad():
                    return stock_moments(views, s["xyz"], pivot)
            x = s["xyz"].detach().requires_grad_(True)
            stock_moments(views, x, pivot).backward(ups[turn[0]])
        return run

    res = dict(gaussians=n, views=V, copies=copies)
    res["hip_forward"] = _time(hip(False), dev, a, copies, out_bytes + row_bytes)
    res["hip_forward_backward"] = _time(hip(True), dev, a, copies, 2 * (out_bytes + row_bytes) + 12 * n)
    res["stock_forward"] = _time(stock(False), dev, a)
    res["stock_forward_backward"] = _time(stock(True), dev, a)
    s = sets[0]
    res["max_abs_difference_from_stock"] = float((depth_moments_forward(views, s["xyz"], "ndc", pivot) - stock_moments(views, s["xyz"], pivot)).abs().max())
    print(f"A {n} x {V}: forward {_show(res['hip_forward'])} (stock {_show(res['stock_forward'])})\n"
          f"    forward+backward {_show(res['hip_forward_backward'])} (stock {_show(res['stock_forward_backward'])})  "
          f"differs from stock by {res['max_abs_difference_from_stock']:.2e}", flush=True)
    return res


def bench_B(shape, dev, a):
    import ctypes as C

    from latentsplat_amd import _lib
    from latentsplat_amd.distortion import distortion_loss_backward, distortion_loss_forward
    V, H, W = shape
    pixels = V * H * W
    gen = torch.Generator(device=dev).manual_seed(pixels)
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (12 * pixels)))
    sets = []
    for _ in range(copies):
        alpha = 0.1 + 0.89 * torch.rand((V, H, W), device=dev, generator=gen)
        mean = torch.rand((V, H, W), device=dev, generator=gen) - 0.5
        var = 0.05 * torch.rand((V, H, W), device=dev, generator=gen)
        mm = torch.stack([alpha * mean, alpha * (mean * mean + var)], 1).contiguous()
        sets.append(dict(mm=mm, alpha=alpha, out=dict(loss=torch.empty(1, device=dev)),
                         grads=dict(moment_map=torch.empty_like(mm), alpha=torch.empty_like(alpha))))
    one = torch.ones(1, device=dev)
    dims = _lib.DistortionDims(num_images=V, height=H, width=W, reserved0=0, reserved1=0, reserved2=0)
    workspace = torch.empty(max(_lib.load().lsr_distortion_loss_workspace_bytes(C.byref(dims)), 16), dtype=torch.uint8, device=dev)
    for s in sets:
        s["out"]["workspace"] = workspace

    def hip(backward):
        def run():
            for s in sets:
                distortion_loss_forward(s["mm"], s["alpha"], None, out=s["out"])
                if backward:
                    distortion_loss_backward(s["mm"], s["alpha"], one, None, out=s["grads"])
        return run

    turn = [0]

    def stock(backward):
        def run():
            turn[0] = (turn[0] + 1) % copies
            s = sets[turn[0]]
            if not backward:
                with torch.no_grad():
                    return stock_loss(s["mm"], s["alpha"])
            leaves = [s[k].detach().requires_grad_(True) for k in ("mm", "alpha")]
            stock_loss(*leaves).backward()
        return run

    res = dict(views=V, height=H, width=W, copies=copies)
    res["hip_forward"] = _time(hip(False), dev, a, copies, 12 * pixels)
    res["hip_forward_backward"] = _time(hip(True), dev, a, copies, 36 * pixels)
    res["stock_forward"] = _time(stock(False), dev, a)
    res["stock_forward_backward"] = _time(stock(True), dev, a)
    s = sets[0]
    res["loss"] = float(distortion_loss_forward(s["mm"], s["alpha"])["loss"])
    res["stock_loss"] = float(stock_loss(s["mm"], s["alpha"]))
    print(f"B {V} x {H} x {W}: forward {_show(res['hip_forward'])} (stock {_show(res['stock_forward'])})\n"
          f"    forward+backward {_show(res['hip_forward_backward'])} (stock {_show(res['stock_forward_backward'])})  "
          f"loss {res['loss']:.6e} (stock {res['stock_loss']:.6e})", flush=True)
    return res


def bench_scene(dev, a, n=393_216, V=4, size=512):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.distortion import depth_pivot, distortion_loss, with_near_far
    from latentsplat_amd.normals import normal_consistency_loss
    gen = torch.Generator(device=dev).manual_seed(7)
    r = lambda *s: torch.rand(s, device=dev, generator=gen)
    # the shell of small flat Gaussians of tools/bench_normals.py: a surface for the depth to describe
    direction = torch.nn.functional.normalize(torch.randn((n, 3), device=dev, generator=gen), dim=-1)
    scaling = torch.log(torch.stack([0.004 + 0.006 * r(n), 0.004 + 0.006 * r(n), 0.0005 + 0.001 * r(n)], -1))
    scene = GaussianScene.from_tensors(xyz=direction * (0.9 + 0.2 * r(n, 1)), features_dc=r(n, 1, 3) - 0.5, features_rest=0.1 * (r(n, 15, 3) - 0.5),
                                       opacity=2.0 * r(n, 1), scaling=scaling, rotation=torch.randn((n, 4), device=dev, generator=gen)).to(dev)
    views = with_near_far(circle_views(V, dev, radius=3.0), NEAR, FAR)
    pivot = depth_pivot(views, (0.0, 0.0, 0.0), "ndc")
    kw = dict(space="ndc", pivot=pivot, check_near_far=False)
    target = r(V, 3, size, size)

    def plain():
        color = scene.render(views, size, size)[0]
        (color - target).abs().mean().backward()
        scene.zero_grad(set_to_none=True)

    def with_distortion():
        color, mm, mask, _, _ = scene.render_with_distortion(views, size, size, **kw)
        ((color - target).abs().mean() + distortion_loss(mm, mask)).backward()
        scene.zero_grad(set_to_none=True)

    def with_normals():
        color, nmap, mask, depth, _ = scene.render_with_normals(views, size, size)
        ((color - target).abs().mean() + 0.05 * normal_consistency_loss(nmap, depth, mask, views, ALPHA_MIN)).backward()
        scene.zero_grad(set_to_none=True)

    def surface():
        color, nmap, mm, mask, depth, _ = scene.render_surface(views, size, size, **kw)
        ((color - target).abs().mean() + 0.05 * normal_consistency_loss(nmap, depth, mask, views, ALPHA_MIN) + distortion_loss(mm, mask)).backward()
        scene.zero_grad(set_to_none=True)

    normals, moments = torch.randn((V, n, 3), device=dev, generator=gen), torch.randn((V, n, 2), device=dev, generator=gen)

    def cat():
        torch.cat((normals, moments), dim=-1)

    arms = dict(render=plain, render_with_distortion_and_loss=with_distortion, render_with_normals_and_loss=with_normals,
                render_surface_and_both_losses=surface)
    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    for _ in range(a.samples):                  # alternating, in one process
        for k, fn in arms.items():
            times[k].append(_sample(fn, dev))
    res = dict(gaussians=n, views=V, size=size, sh_degree=3, space="ndc")
    res.update({k + "_forward_backward": _figures(t) for k, t in times.items()})
    res["payload_cat_forward"] = _time(cat, dev, a, 1, 2 * 20 * V * n)
    with torch.no_grad():
        _, nmap, mm, mask, depth, _ = scene.render_surface(views, size, size, **kw)
        res["distortion_loss"] = float(distortion_loss(mm, mask))
        res["covered_fraction"] = float((mask > ALPHA_MIN).float().mean())
    ms = lambda k: res[k + "_forward_backward"]["ms"]
    res["ratio_distortion_over_render"] = ms("render_with_distortion_and_loss") / ms("render")
    res["ratio_surface_over_normals"] = ms("render_surface_and_both_losses") / ms("render_with_normals_and_loss")
    print(f"scene {n} x {V} at {size}: render {_show(res['render_forward_backward'])}, with distortion + loss "
          f"{_show(res['render_with_distortion_and_loss_forward_backward'])}: x{res['ratio_distortion_over_render']:.3f}\n"
          f"    with normals + loss {_show(res['render_with_normals_and_loss_forward_backward'])}, surface + both losses "
          f"{_show(res['render_surface_and_both_losses_forward_backward'])}: x{res['ratio_surface_over_normals']:.3f}\n"
          f"    the payload cat alone {_show(res['payload_cat_forward'])}  (distortion loss {res['distortion_loss']:.3e}, "
          f"covered {res['covered_fraction']:.2f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-scene", action="store_true")
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "distortion_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_distortion needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               hbm_bytes_per_s=HBM_BYTES_PER_S,
               bytes_note="A forward: 8 B per (view, Gaussian) written + 12 B per Gaussian read; A backward: the same read + 12 B per "
                          "Gaussian written; B forward: 12 B per pixel read; B backward: 12 read + 12 written",
               baseline_note="stock: the float32 PyTorch composition of the definitions of include/lsr_distortion.h "
                             "(tools/bench_distortion.py), autograd for the gradients, same process and card",
               A=[], B=[])
    for n in GAUSSIANS:
        for V in VIEWS:
            res["A"].append(bench_A(n, V, dev, a))
            torch.cuda.empty_cache()
    for shape in IMAGES:
        res["B"].append(bench_B(shape, dev, a))
        torch.cuda.empty_cache()
    if not a.skip_scene:
        res["scene"] = bench_scene(dev, a)
    from tests import distortion_ref as dref
    res["pivot"] = dref.pivot_errors(dev)
    print(f"pivot: error with pivot 0 {res['pivot']['err_pivot_0']:.3e}, pivoted {res['pivot']['err_pivoted']:.3e}, ratio "
          f"{res['pivot']['ratio']:.3g} (largest D {res['pivot']['max_distortion']:.3e})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
