#!/usr/bin/env python
"""Device time of the inverse-depth loss (csrc/depth_loss.hip, include/lsr_depth_loss.h, latentsplat_amd.depth_sup) on the card
it runs on.

  loss    `lsr_depth_loss_forward` (the loss alone), and forward + `_backward` (both gradients), through the Python layer into
          outputs allocated once, at 16 x 256 x 256 and 4 x 1024 x 1024, with `align="given"` and `align="fit"`, a weight
          map given (16 B per pixel read forward)
  stock   the stock float32 PyTorch composition of the same definition in the same process on the same card, and with autograd
  photo   `photometric_loss` (forward, and forward + backward) on colour images of the same V x H x W in the same run: the loss
          a training step already pays for
  scene   a degree-3 scene of 393 216 Gaussians at 4 views of 512 x 512: `render` + L1, forward + backward, against `render` +
          L1 + this loss on the depth and mask the render returns anyway, alternating in one process

Every arm rotates over as many copies of its arrays as make more than the 256 MB last-level cache, each call on the next
copy; every timed shape is warmed up; every figure is the median of `--samples` (>= 20) samples with the smallest and the
largest beside it.  Each HIP figure is also given as the fraction of the 6.3 TB/s achievable rate that the bytes the pass must
move amount to: "given" forward reads 16 B per pixel (depth, alpha, target, weight); "fit" reads them twice (the moments pass,
then the residuals); the backward reads the 16 again and writes 8.

usage: python tools/bench_depth_loss.py [--samples 20] [--warmup 3] [--json [profiles/depth_loss_bench.json]] [--skip-scene]"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGES = ((16, 256, 256), (4, 1024, 1024))
CACHE_BYTES = 256e6
HBM_BYTES_PER_S = 6.3e12
ALPHA_MIN = 0.01


def _sample(fn, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end)


def _figures(t, nbytes=None):
    med = statistics.median(t)
    f = dict(ms=med, min_ms=min(t), max_ms=max(t), samples=len(t))
    if nbytes is not None:
        f.update(bytes=nbytes, hbm_ms=1e3 * nbytes / HBM_BYTES_PER_S, fraction_of_hbm=nbytes / HBM_BYTES_PER_S / (1e-3 * med))
    return f


def _show(f):
    tail = f", {100 * f['fraction_of_hbm']:.0f} % of HBM" if "fraction_of_hbm" in f else ""
    return f"{f['ms']:8.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]{tail}"


def _time(fn, dev, a, per=1, nbytes=None):
    for _ in range(a.warmup):
        fn()
    return _figures([_sample(fn, dev) / per for _ in range(a.samples)], nbytes)


def circle_views(V, dev, radius=4.0):
    """A (V, 44) table of cameras on a circle around the origin through build_view_table."""
    from latentsplat_amd.rasterizer import build_view_table
    ang = torch.arange(V, device=dev, dtype=torch.float32) * (2 * math.pi / V) + 0.1
    zero, one = torch.zeros_like(ang), torch.ones_like(ang)
    offset = torch.stack([torch.cos(ang), zero, torch.sin(ang)], -1)
    down = torch.stack([zero, one, zero], -1)
    ext = torch.zeros((V, 4, 4), device=dev)
    ext[:, :3, 0], ext[:, :3, 1], ext[:, :3, 2] = torch.linalg.cross(down, -offset), down, -offset
    ext[:, :3, 3] = radius * offset
    ext[:, 3, 3] = 1
    intr = torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]], device=dev).repeat(V, 1, 1)
    near, far = torch.full((V,), 1.0, device=dev), torch.full((V,), 100.0, device=dev)
    return build_view_table(ext, intr, near, far, torch.zeros(3, device=dev))


# ---- the stock float32 composition of the definition of include/lsr_depth_loss.h ----

def stock_loss(depth, alpha, views, target, weight, affine, align, alpha_min=ALPHA_MIN):
    s = views[:, 40].reshape(-1, 1, 1)
    ok = (alpha > alpha_min) & (depth > 0) & torch.isfinite(alpha) & torch.isfinite(depth)
    inv = torch.where(ok, s * torch.where(ok, alpha, torch.zeros_like(alpha)) / torch.where(ok, depth, torch.ones_like(depth)),
                      torch.zeros_like(depth))
    w = weight
    if align == "fit":
        with torch.no_grad():
            sm = lambda x: x.sum((1, 2))
            Sw, St, SI, Stt, StI = sm(w), sm(w * target), sm(w * inv), sm(w * target * target), sm(w * target * inv)
            det = Sw * Stt - St * St
            good = (sm((w > 0).float()) >= 2) & (det > 2.0 ** -24 * Sw * Stt)
            a = torch.where(good, (Sw * StI - St * SI) / torch.where(good, det, torch.ones_like(det)), torch.zeros_like(det))
            b = torch.where(good, (SI - a * St) / torch.where(good, Sw, torch.ones_like(Sw)), torch.zeros_like(det))
    else:
        a, b = affine[:, 0], affine[:, 1]
    r = w * (inv - (a.reshape(-1, 1, 1) * target + b.reshape(-1, 1, 1)))
    per_view = torch.where(a != 0, r.abs().sum((1, 2)) / (depth.shape[1] * depth.shape[2]), torch.zeros_like(a))
    return per_view.mean()


# ---- arms ----

def bench_loss(shape, dev, a):
    from latentsplat_amd.depth_sup import inverse_depth_backward, inverse_depth_forward, workspace_bytes
    from latentsplat_amd.losses import photometric_loss
    V, H, W = shape
    pixels = V * H * W
    gen = torch.Generator(device=dev).manual_seed(pixels)
    views = circle_views(V, dev)
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (16 * pixels)))
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    scale = views[:, 40].reshape(-1, 1, 1)
    sets = []
    for k in range(copies):
        z = 3.0 + 0.002 * xs + 0.001 * ys + 0.3 * torch.sin(0.05 * xs + k) * torch.cos(0.04 * ys) + 0.05 * torch.rand((V, H, W), device=dev, generator=gen)
        alpha = 0.3 + 0.69 * torch.rand((V, H, W), device=dev, generator=gen)
        alpha[:, H // 3:H // 3 + 8, W // 4:W // 4 + 40] = 0.0
        target = ((1.0 / z + 0.02 * (torch.rand((V, H, W), device=dev, generator=gen) - 0.5)) - 0.03) / 1.7
        weight = (torch.rand((V, H, W), device=dev, generator=gen) > 0.1).float()
        sets.append(dict(depth=(scale * z * alpha).contiguous(), alpha=alpha.contiguous(), target=target.contiguous(), weight=weight,
                         out=dict(loss=torch.empty(1, device=dev)), grads=dict(depth=torch.empty_like(alpha), alpha=torch.empty_like(alpha))))
    affine = torch.tensor([[1.7, 0.03]], device=dev).repeat(V, 1)
    one = torch.ones(1, device=dev)
    res = dict(views=V, height=H, width=W, copies=copies)

    for align in ("given", "fit"):
        workspace = torch.empty(workspace_bytes(V, H, W, align), dtype=torch.uint8, device=dev)
        for s in sets:
            s["out"]["workspace"] = workspace
        modes = dict(align=align, normalize="pixels", alpha_min=ALPHA_MIN)

        def hip(backward):
            def run():
                for s in sets:
                    inverse_depth_forward(s["depth"], s["alpha"], views, s["target"], s["weight"], affine if align == "given" else None,
                                          out=s["out"], **modes)
                    if backward:
                        inverse_depth_backward(s["depth"], s["alpha"], views, s["target"], s["weight"], workspace, one, out=s["grads"], **modes)
            return run

        turn = [0]

        def stock(backward):
            def run():
                turn[0] = (turn[0] + 1) % copies
                s = sets[turn[0]]
                if not backward:
                    with torch.no_grad():
                        return stock_loss(s["depth"], s["alpha"], views, s["target"], s["weight"], affine, align)
                d, al = s["depth"].detach().requires_grad_(True), s["alpha"].detach().requires_grad_(True)
                stock_loss(d, al, views, s["target"], s["weight"], affine, align).backward()
            return run

        fwd_bytes = (32 if align == "fit" else 16) * pixels
        r = dict(hip_forward=_time(hip(False), dev, a, copies, fwd_bytes),
                 hip_forward_backward=_time(hip(True), dev, a, copies, fwd_bytes + 24 * pixels),
                 stock_forward=_time(stock(False), dev, a), stock_forward_backward=_time(stock(True), dev, a))
        s = sets[0]
        got = inverse_depth_forward(s["depth"], s["alpha"], views, s["target"], s["weight"], affine if align == "given" else None, **modes)["loss"]
        r["loss"], r["stock_loss"] = float(got), float(stock_loss(s["depth"], s["alpha"], views, s["target"], s["weight"], affine, align))
        res[align] = r
        print(f"{align:5s} {V} x {H} x {W}: forward {_show(r['hip_forward'])} (stock {_show(r['stock_forward'])})\n"
              f"    forward+backward {_show(r['hip_forward_backward'])} (stock {_show(r['stock_forward_backward'])})  "
              f"loss {r['loss']:.6f} (stock {r['stock_loss']:.6f})", flush=True)

    # photometric_loss on colour images of the same V x H x W, rotating likewise
    pcopies = max(2, math.ceil(1.2 * CACHE_BYTES / (24 * pixels)))
    images = [(torch.rand((V, 3, H, W), device=dev, generator=gen), torch.rand((V, 3, H, W), device=dev, generator=gen)) for _ in range(pcopies)]

    def photo(backward):
        def run():
            for x, y in images:
                if not backward:
                    with torch.no_grad():
                        photometric_loss(x, y, 0.2)
                else:
                    leaf = x.detach().requires_grad_(True)
                    photometric_loss(leaf, y, 0.2).backward()
        return run

    res["photometric_forward"] = _time(photo(False), dev, a, pcopies)
    res["photometric_forward_backward"] = _time(photo(True), dev, a, pcopies)
    print(f"photometric_loss {V} x 3 x {H} x {W}: forward {_show(res['photometric_forward'])}, forward+backward "
          f"{_show(res['photometric_forward_backward'])}", flush=True)
    return res


def bench_scene(dev, a, n=393_216, V=4, size=512):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.depth_sup import inverse_depth_loss
    gen = torch.Generator(device=dev).manual_seed(7)
    r = lambda *s: torch.rand(s, device=dev, generator=gen)
    # a shell of small flat Gaussians around the origin: a surface for the depth to describe
    direction = torch.nn.functional.normalize(torch.randn((n, 3), device=dev, generator=gen), dim=-1)
    scaling = torch.log(torch.stack([0.004 + 0.006 * r(n), 0.004 + 0.006 * r(n), 0.0005 + 0.001 * r(n)], -1))
    scene = GaussianScene.from_tensors(xyz=direction * (0.9 + 0.2 * r(n, 1)), features_dc=r(n, 1, 3) - 0.5, features_rest=0.1 * (r(n, 15, 3) - 0.5),
                                       opacity=2.0 * r(n, 1), scaling=scaling, rotation=torch.randn((n, 4), device=dev, generator=gen)).to(dev)
    views = circle_views(V, dev, radius=3.0)
    target = r(V, 3, size, size)
    with torch.no_grad():
        _, _, mask, depth, _ = scene.render(views, size, size)
        prior = torch.where(mask > 0.5, views[:, 40].reshape(-1, 1, 1) * mask / depth.clamp_min(1e-6), torch.zeros_like(mask)) * 0.5 + 0.01
    cover = torch.ones_like(mask)

    def plain():
        color = scene.render(views, size, size)[0]
        (color - target).abs().mean().backward()
        scene.zero_grad(set_to_none=True)

    def with_depth(align):
        def run():
            color, _, m, d, _ = scene.render(views, size, size)
            ((color - target).abs().mean() + 0.1 * inverse_depth_loss(d, m, views, prior, cover, align=align)).backward()
            scene.zero_grad(set_to_none=True)
        return run

    arms = dict(render=plain, given=with_depth("given"), fit=with_depth("fit"))
    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    t = {k: [] for k in arms}
    for _ in range(a.samples):                  # alternating, in one process
        for k, fn in arms.items():
            t[k].append(_sample(fn, dev))
    res = dict(gaussians=n, views=V, size=size, sh_degree=3, render_forward_backward=_figures(t["render"]),
               with_depth_loss_given_forward_backward=_figures(t["given"]), with_depth_loss_fit_forward_backward=_figures(t["fit"]))
    res["ratio_given"] = res["with_depth_loss_given_forward_backward"]["ms"] / res["render_forward_backward"]["ms"]
    res["ratio_fit"] = res["with_depth_loss_fit_forward_backward"]["ms"] / res["render_forward_backward"]["ms"]
    print(f"scene {n} x {V} at {size}: render + L1 {_show(res['render_forward_backward'])}; + depth loss (given) "
          f"{_show(res['with_depth_loss_given_forward_backward'])}: x{res['ratio_given']:.3f}; (fit) "
          f"{_show(res['with_depth_loss_fit_forward_backward'])}: x{res['ratio_fit']:.3f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-scene", action="store_true")
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "depth_loss_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_depth_loss needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               hbm_bytes_per_s=HBM_BYTES_PER_S, alpha_min=ALPHA_MIN,
               bytes_note="given forward: 16 B per pixel read (depth, alpha, target, weight); fit forward: 32 (two passes); backward: "
                          "16 read + 8 written",
               baseline_note="stock: the float32 PyTorch composition of the definition of include/lsr_depth_loss.h "
                             "(tools/bench_depth_loss.py), autograd for the gradients; photometric_loss on (V, 3, H, W); same process and card",
               loss=[])
    for shape in IMAGES:
        res["loss"].append(bench_loss(shape, dev, a))
        torch.cuda.empty_cache()
    if not a.skip_scene:
        res["scene"] = bench_scene(dev, a)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
