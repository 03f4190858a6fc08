#!/usr/bin/env python
"""Device time of the depth-normal consistency regulariser (csrc/normals.hip, include/lsr_normals.h, latentsplat_amd.normals)
on the card it runs on.

  A       `lsr_scene_normals_forward`, and forward + `_backward`, through the Python layer into outputs allocated once, at
          393 216 and 3 000 000 Gaussians x 4 and 16 views
  B       `lsr_normal_consistency_forward` (the loss alone), and forward + `_backward` (all three gradients), likewise, at
          16 x 256 x 256 and 4 x 1024 x 1024
  stock   the stock float32 PyTorch composition of the same definitions in the same process on the same card, and with autograd
  scene   a degree-3 scene of 393 216 Gaussians at 4 views of 512 x 512: `render_with_normals` + the loss, forward + backward,
          alternating with plain `render` (forward + backward of a colour loss) in one process: the cost of the three extra
          payload channels plus the loss

Every arm rotates over as many copies of its large arrays as make more than the 256 MB last-level cache, each call on the next
copy; every timed shape is warmed up; every figure is the median of `--samples` (>= 20) samples with the smallest and the
largest beside it.  Each HIP figure is also given as the fraction of the 6.3 TB/s achievable rate that the bytes the kernel must
move amount to: A forward writes 12 B per (view, Gaussian) and reads 40 B per Gaussian, its backward reads the 12 and the 40
and writes 16 B per Gaussian; B forward reads 20 B per pixel (normal map, depth, alpha), its backward reads them again and
writes 20.

usage: python tools/bench_normals.py [--samples 20] [--warmup 3] [--json [profiles/normals_bench.json]] [--skip-scene]"""
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

GAUSSIANS, VIEWS = (393_216, 3_000_000), (4, 16)
IMAGES = ((16, 256, 256), (4, 1024, 1024))
CACHE_BYTES = 256e6
HBM_BYTES_PER_S = 6.3e12
ALPHA_MIN = 0.5


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
        f.update(bytes=nbytes, fraction_of_hbm=nbytes / HBM_BYTES_PER_S / (1e-3 * med))
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


# ---- the stock float32 composition of the definitions of include/lsr_normals.h ----

def stock_normals(views, xyz, scaling, rotation):
    q = rotation / rotation.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    k = torch.argmin(scaling, dim=-1)
    a = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1))[..., 0]
    W3 = views[:, :16].reshape(-1, 4, 4).transpose(1, 2)[:, :3, :3]
    c = torch.sqrt((W3 * W3).sum((1, 2)) / 3.0)
    d = (a[None] * (views[:, None, 32:35] - views[:, None, 40:41] * xyz[None])).sum(-1)
    sign = torch.where(d < 0, -1.0, 1.0)
    o = sign[..., None] * torch.einsum("vij,nj->vni", W3, a) / c[:, None, None]
    ok = torch.isfinite(d) & torch.isfinite(o).all(-1)
    return torch.where(ok[..., None], o, torch.zeros_like(o))


def stock_rays(views, H, W):
    dev = views.device
    A = views[:, :16].reshape(-1, 4, 4).transpose(1, 2)[:, :3, :3]
    Q = views[:, 16:32].reshape(-1, 4, 4).transpose(1, 2)[:, [0, 1, 3], :3] @ torch.linalg.inv(A)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    nx, ny = ((2 * xs + 1) / W - 1)[None], ((2 * ys + 1) / H - 1)[None]
    q = lambda i, j: Q[:, i, j, None, None]
    m00, m01, b0 = q(0, 0) - nx * q(2, 0), q(0, 1) - nx * q(2, 1), nx * q(2, 2) - q(0, 2)
    m10, m11, b1 = q(1, 0) - ny * q(2, 0), q(1, 1) - ny * q(2, 1), ny * q(2, 2) - q(1, 2)
    det = m00 * m11 - m01 * m10
    rx, ry = (b0 * m11 - m01 * b1) / det, (m00 * b1 - b0 * m10) / det
    jac = (rx[:, 0, 1] - rx[:, 0, 0]) * (ry[:, 1, 0] - ry[:, 0, 0]) - (rx[:, 1, 0] - rx[:, 0, 0]) * (ry[:, 0, 1] - ry[:, 0, 0])
    return torch.stack([rx, ry, torch.ones_like(rx)], -1), torch.where(jac > 0, -1.0, 1.0)


def stock_consistency(normal_map, depth, alpha, views, alpha_min=ALPHA_MIN):
    V, H, W = depth.shape
    rays, sigma = stock_rays(views, H, W)
    ok = alpha > alpha_min
    D = torch.where(ok, depth, torch.zeros_like(depth)) / torch.where(ok, alpha, torch.ones_like(alpha))
    P = D[..., None] * rays
    a = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    b = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    m = torch.linalg.cross(a, b, dim=-1)
    norm = m.norm(dim=-1)
    tiny, huge = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).max
    valid = (ok[:, 1:-1, 1:-1] & ok[:, 1:-1, 2:] & ok[:, 1:-1, :-2] & ok[:, 2:, 1:-1] & ok[:, :-2, 1:-1] & (norm >= tiny) & (norm <= huge))
    n = sigma[:, None, None, None] * m / torch.where(valid, norm, torch.ones_like(norm))[..., None]
    dot = (normal_map.permute(0, 2, 3, 1)[:, 1:-1, 1:-1] * n).sum(-1)
    e = torch.where(valid, alpha.detach()[:, 1:-1, 1:-1] - dot, torch.zeros_like(dot))
    return (e.sum((1, 2)) / (H * W)).mean()


# ---- arms ----

def bench_A(n, V, dev, a):
    from latentsplat_amd.normals import normals_backward, normals_forward
    gen = torch.Generator(device=dev).manual_seed(n + V)
    views = circle_views(V, dev)
    out_bytes, row_bytes = 12 * V * n, 40 * n
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (out_bytes + row_bytes)))
    sets = [dict(xyz=torch.rand((n, 3), device=dev, generator=gen) * 2 - 1, scaling=torch.randn((n, 3), device=dev, generator=gen) - 3,
                 rotation=torch.randn((n, 4), device=dev, generator=gen), out=torch.empty((V, n, 3), device=dev),
                 grad=torch.empty((n, 4), device=dev)) for _ in range(copies)]
    ups = [torch.randn((V, n, 3), device=dev, generator=gen) for _ in range(copies)]

    def hip(backward):
        def run():
            for s, up in zip(sets, ups):
                normals_forward(views, s["xyz"], s["scaling"], s["rotation"], out=s["out"])
                if backward:
                    normals_backward(views, s["xyz"], s["scaling"], s["rotation"], up, out=s["grad"])
        return run

    turn = [0]

    def stock(backward):
        def run():
            turn[0] = (turn[0] + 1) % copies
            s = sets[turn[0]]
            if not backward:
                with torch.no_grad():
                    return stock_normals(views, s["xyz"], s["scaling"], s["rotation"])
            q = s["rotation"].detach().requires_grad_(True)
            stock_normals(views, s["xyz"], s["scaling"], q).backward(ups[turn[0]])
        return run

    res = dict(gaussians=n, views=V, copies=copies)
    res["hip_forward"] = _time(hip(False), dev, a, copies, out_bytes + row_bytes)
    res["hip_forward_backward"] = _time(hip(True), dev, a, copies, 2 * (out_bytes + row_bytes) + 16 * n)
    res["stock_forward"] = _time(stock(False), dev, a)
    res["stock_forward_backward"] = _time(stock(True), dev, a)
    s = sets[0]
    # the two agree, up to the pairs whose axis lies within float32 rounding of perpendicular to the view direction: there the
    # sign is either way (random inputs keep no distance from that threshold; the tests' builders do)
    diff = (normals_forward(views, s["xyz"], s["scaling"], s["rotation"]) - stock_normals(views, s["xyz"], s["scaling"], s["rotation"])).abs().amax(-1)
    flipped = diff > 1.0
    res["pairs_with_the_other_sign"] = int(flipped.sum())
    res["max_abs_difference_from_stock"] = float(diff[~flipped].max())
    print(f"A {n} x {V}: forward {_show(res['hip_forward'])} (stock {_show(res['stock_forward'])})\n"
          f"    forward+backward {_show(res['hip_forward_backward'])} (stock {_show(res['stock_forward_backward'])})  "
          f"differs from stock by {res['max_abs_difference_from_stock']:.2e} ({res['pairs_with_the_other_sign']} of {V * n} pairs on the sign's threshold)",
          flush=True)
    return res


def bench_B(shape, dev, a):
    import ctypes as C

    from latentsplat_amd import _lib
    from latentsplat_amd.normals import normal_consistency_backward, normal_consistency_forward
    V, H, W = shape
    pixels = V * H * W
    gen = torch.Generator(device=dev).manual_seed(pixels)
    views = circle_views(V, dev)
    copies = max(2, math.ceil(1.2 * CACHE_BYTES / (20 * pixels)))
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    sets = []
    for k in range(copies):
        D = 3.0 + 0.002 * xs + 0.001 * ys + 0.05 * torch.sin(0.05 * xs + k) * torch.cos(0.04 * ys) + 1e-3 * torch.rand((V, H, W), device=dev, generator=gen)
        alpha = 0.55 + 0.44 * torch.rand((V, H, W), device=dev, generator=gen)
        alpha[:, H // 3:H // 3 + 8, W // 4:W // 4 + 40] = 0.1
        N = torch.randn((V, 3, H, W), device=dev, generator=gen) * 0.2
        N[:, 2] -= 1.0
        N = N / N.norm(dim=1, keepdim=True) * alpha[:, None]
        sets.append(dict(N=N.contiguous(), depth=(D * alpha).contiguous(), alpha=alpha.contiguous(),
                         out=dict(loss=torch.empty(1, device=dev)),
                         grads=dict(normal_map=torch.empty_like(N), depth=torch.empty_like(alpha), alpha=torch.empty_like(alpha))))
    one = torch.ones(1, device=dev)
    dims = _lib.NormalDims(num_images=V, height=H, width=W, alpha_min=ALPHA_MIN, reserved0=0, reserved1=0)
    workspace = torch.empty(max(_lib.load().lsr_normal_consistency_workspace_bytes(C.byref(dims)), 16), dtype=torch.uint8, device=dev)
    for s in sets:
        s["out"]["workspace"] = workspace

    def hip(backward):
        def run():
            for s in sets:
                normal_consistency_forward(s["N"], s["depth"], s["alpha"], views, ALPHA_MIN, out=s["out"])
                if backward:
                    normal_consistency_backward(s["N"], s["depth"], s["alpha"], views, one, ALPHA_MIN, out=s["grads"])
        return run

    turn = [0]

    def stock(backward):
        def run():
            turn[0] = (turn[0] + 1) % copies
            s = sets[turn[0]]
            if not backward:
                with torch.no_grad():
                    return stock_consistency(s["N"], s["depth"], s["alpha"], views)
            leaves = [s[k].detach().requires_grad_(True) for k in ("N", "depth", "alpha")]
            stock_consistency(*leaves, views).backward()
        return run

    res = dict(views=V, height=H, width=W, copies=copies)
    res["hip_forward"] = _time(hip(False), dev, a, copies, 20 * pixels)
    res["hip_forward_backward"] = _time(hip(True), dev, a, copies, 60 * pixels)
    res["stock_forward"] = _time(stock(False), dev, a)
    res["stock_forward_backward"] = _time(stock(True), dev, a)
    s = sets[0]
    got = normal_consistency_forward(s["N"], s["depth"], s["alpha"], views, ALPHA_MIN)["loss"]
    res["loss"], res["stock_loss"] = float(got), float(stock_consistency(s["N"], s["depth"], s["alpha"], views))
    print(f"B {V} x {H} x {W}: forward {_show(res['hip_forward'])} (stock {_show(res['stock_forward'])})\n"
          f"    forward+backward {_show(res['hip_forward_backward'])} (stock {_show(res['stock_forward_backward'])})  "
          f"loss {res['loss']:.6f} (stock {res['stock_loss']:.6f})", flush=True)
    return res


def bench_scene(dev, a, n=393_216, V=4, size=512):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.normals import normal_consistency_loss
    gen = torch.Generator(device=dev).manual_seed(7)
    r = lambda *s: torch.rand(s, device=dev, generator=gen)
    # a shell of small flat Gaussians around the origin: a surface for the depth to describe
    direction = torch.nn.functional.normalize(torch.randn((n, 3), device=dev, generator=gen), dim=-1)
    scaling = torch.log(torch.stack([0.004 + 0.006 * r(n), 0.004 + 0.006 * r(n), 0.0005 + 0.001 * r(n)], -1))
    scene = GaussianScene.from_tensors(xyz=direction * (0.9 + 0.2 * r(n, 1)), features_dc=r(n, 1, 3) - 0.5, features_rest=0.1 * (r(n, 15, 3) - 0.5),
                                       opacity=2.0 * r(n, 1), scaling=scaling, rotation=torch.randn((n, 4), device=dev, generator=gen)).to(dev)
    views = circle_views(V, dev, radius=3.0)
    target = r(V, 3, size, size)

    def plain():
        color = scene.render(views, size, size)[0]
        (color - target).abs().mean().backward()
        scene.zero_grad(set_to_none=True)

    def with_normals():
        color, nmap, mask, depth, _ = scene.render_with_normals(views, size, size)
        ((color - target).abs().mean() + 0.05 * normal_consistency_loss(nmap, depth, mask, views, ALPHA_MIN)).backward()
        scene.zero_grad(set_to_none=True)

    for _ in range(a.warmup):
        plain()
        with_normals()
    t_plain, t_normals = [], []
    for _ in range(a.samples):                  # alternating, in one process
        t_plain.append(_sample(plain, dev))
        t_normals.append(_sample(with_normals, dev))
    with torch.no_grad():
        color, nmap, mask, depth, _ = scene.render_with_normals(views, size, size)
        loss = float(normal_consistency_loss(nmap, depth, mask, views, ALPHA_MIN))
        covered = float((mask > ALPHA_MIN).float().mean())
    res = dict(gaussians=n, views=V, size=size, sh_degree=3, render_forward_backward=_figures(t_plain),
               render_with_normals_and_loss_forward_backward=_figures(t_normals), normal_loss=loss, covered_fraction=covered)
    res["ratio"] = res["render_with_normals_and_loss_forward_backward"]["ms"] / res["render_forward_backward"]["ms"]
    print(f"scene {n} x {V} at {size}: render {_show(res['render_forward_backward'])}, with normals + loss "
          f"{_show(res['render_with_normals_and_loss_forward_backward'])}: x{res['ratio']:.3f}  (loss {loss:.4f}, covered {covered:.2f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-scene", action="store_true")
    ap.add_argument("--json", nargs="?", const=os.path.join(ROOT, "profiles", "normals_bench.json"), default=None)
    a = ap.parse_args()
    if a.samples < 20:
        sys.exit("at least 20 samples")
    if not torch.cuda.is_available():
        sys.exit("bench_normals needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = dict(samples=a.samples, warmup=a.warmup, device=torch.cuda.get_device_name(dev), cache_bytes=CACHE_BYTES,
               hbm_bytes_per_s=HBM_BYTES_PER_S, alpha_min=ALPHA_MIN,
               bytes_note="A forward: 12 B per (view, Gaussian) written + 40 B per Gaussian read; A backward: the same read + 16 B per "
                          "Gaussian written; B forward: 20 B per pixel read; B backward: 20 read + 20 written",
               baseline_note="stock: the float32 PyTorch composition of the definitions of include/lsr_normals.h (tools/bench_normals.py), "
                             "autograd for the gradients, same process and card",
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
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
