#!/usr/bin/env python
"""Train a 3DGS scene from a photographed capture: a COLMAP sparse model and its photographs.

  1. `Capture.load(ROOT, --sparse, --images, --resolution)`: the model through the library's host reader, the photographs
     resampled in HIP onto the centred, distortion-free camera the rasterizer implements (`lsr_image_prepare`), with a
     coverage map per image; every `--hold`-th image by sorted name is held out (the published rule; 0: none);
  2. the scene starts from the model's points: `capture.initial_scene(--sh-degree)` (`GaussianScene.from_point_cloud`);
  3. each step draws `--batch` training views of one output size from a seeded shuffle (every view once per epoch) and
     minimises `photometric_loss(render * coverage, target * coverage, --lambda-dssim)`: where the photograph has nothing to
     say both sides are 0;
  4. `SceneAdam`, one parameter group per tensor at the published trainer's customary rates (position 1.6e-4 -> 1.6e-6 times
     `cameras_extent` on the `expon_lr` schedule over the run, f_dc 2.5e-3, f_rest f_dc / 20, opacity 5e-2, scaling 5e-3,
     rotation 1e-3; eps 1e-15): defaults, not measurements;
  5. `--strategy adc` (the default): `DensityControl` every `--densify-interval` steps between `--densify-from` and
     `--densify-until`, opacity resets every `--opacity-reset-interval`; the loss is a mean over the batch, so the
     threshold defaults to `2e-4 / batch`.  `--strategy mcmc`: `MCMCControl` on the same schedule up to `--cap-max`, its two
     regularisers in the loss, position noise after every step.  `--densify-interval 0` turns either off;
  6. `--sh-degree-interval I`: one more SH band every I steps (0: never).  `--antialiasing`: the rasterizer's opacity
     compensation.  `--filter-3d`: the 3D smoothing filter over the training cameras, recomputed after every density event
     and every `--filter-3d-interval` steps (per output size, the smallest filter wins);
  7. `point_cloud.ply` and `metrics.json` in `--out`: `loss_first`, `loss_last`, `gaussians`, `ms_per_step` (after a
     warm-up), and on the held-out views `psnr` and `ssim` (`compute_ssim`) over the covered pixels: the render and the target
     multiplied by the coverage, the squared error averaged over the covered values only;
  8. depth supervision, both off by default and both `inverse_depth_loss` on the depth and mask the
     render already returns.  `--depth-sparse W`: the L1 on inverse depth at the pixels the model's own sparse points project
     to (`capture.sparse_depth`), a mean over those points, times W times `cameras_extent` (gsplat's `depth_loss`; its
     customary W is 1e-2).  `--depth-priors DIR`: one 16-bit monocular inverse-depth prior per image under the image's name
     in DIR, brought to the scene's scale by the per-image scale and offset from the sparse points (`--depth-align given`,
     the published rule) or by a least-squares fit against the render every step (`--depth-align fit`), a mean over the
     pixels weighted by the coverage, times a weight on the `expon_lr` schedule from `--depth-prior-weight` to
     `--depth-prior-weight-final` over the run.  `metrics.json` then also holds `depth_loss_first` / `depth_loss_last`: the
     weighted depth terms of the first and the last step;
  9. the two geometric regularisers, both off by default, from step `--reg-from` on.
     `--normal-reg W`: W times `normal_consistency_loss` at the pixels covered more than `--normal-alpha-min`.  `--dist-reg W`:
     W times `distortion_loss` with the capture's coverage map as the weight, the depths in `--dist-space` (default ndc, with
     the capture's near / far) about `depth_pivot` at the centroid of the capture's sparse points.  One render carries what is
     asked for: `render_with_normals`, `render_with_distortion`, or `render_surface` for both.  `metrics.json` then holds the
     settings and `normal_loss_first / _last`, `dist_loss_first / _last`: the unweighted terms of the first and last step
     they were on.

usage: python tools/train_colmap.py ROOT --out DIR [--sparse sparse/0] [--images images] [--resolution 1] [--hold 8] [--steps 30000]
                                    [--batch 1] [--seed 0] [--lambda-dssim 0.2] [--sh-degree 3] [--sh-degree-interval 1000]
                                    [--strategy adc|mcmc] [--densify-interval 100] [--densify-from 500] [--densify-until 15000]
                                    [--densify-grad-threshold 2e-4/BATCH] [--min-opacity 0.005] [--opacity-reset-interval 3000]
                                    [--cap-max N] [--noise-lr 5e5] [--opacity-reg 0.01] [--scale-reg 0.01]
                                    [--antialiasing] [--filter-3d] [--filter-3d-interval 100]
                                    [--depth-sparse 0] [--depth-priors DIR] [--depth-prior-weight 1.0]
                                    [--depth-prior-weight-final 0.01] [--depth-align given|fit]
                                    [--normal-reg 0] [--dist-reg 0] [--reg-from 0] [--normal-alpha-min 0.5]
                                    [--dist-space ndc|linear|disparity]"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARMUP_STEPS = 5            # steps left out of the time per step (fewer when there are fewer than 10 steps)
EVAL_BATCH = 4


def batches(groups: dict, batch: int, rng: random.Random):
    """One epoch: every view once, in batches of at most `batch` views of one output size, batches in a seeded order."""
    out = []
    for size in sorted(groups):
        idx = list(groups[size])
        rng.shuffle(idx)
        out += [(size, idx[at:at + batch]) for at in range(0, len(idx), batch)]
    rng.shuffle(out)
    return out


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                 epilog="The learning rates and schedules are the published trainer's customary defaults, not measurements.")
    ap.add_argument("root")
    ap.add_argument("--out", required=True)
    ap.add_argument("--sparse", default="sparse/0")
    ap.add_argument("--images", default="images")
    ap.add_argument("--resolution", type=float, default=1.0, help="reduce the photographs by this factor (targets of round(W / r) x round(H / r))")
    ap.add_argument("--hold", type=int, default=8, help="every this-many-th image by sorted name is held out for testing (0: none)")
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--batch", type=int, default=1, help="training views per step, all of one output size")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lambda-dssim", type=float, default=0.2)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--sh-degree-interval", type=int, default=1000, help="render one more SH band every this many steps (0: never)")
    ap.add_argument("--lr-position", type=float, default=1.6e-4, help="times cameras_extent")
    ap.add_argument("--lr-position-final", type=float, default=1.6e-6, help="times cameras_extent, reached at --steps")
    ap.add_argument("--lr-dc", type=float, default=2.5e-3)
    ap.add_argument("--lr-opacity", type=float, default=5e-2)
    ap.add_argument("--lr-scaling", type=float, default=5e-3)
    ap.add_argument("--lr-rotation", type=float, default=1e-3)
    ap.add_argument("--strategy", choices=("adc", "mcmc"), default="adc")
    ap.add_argument("--densify-interval", type=int, default=100, help="a density event every this many steps (0: never)")
    ap.add_argument("--densify-from", type=int, default=500)
    ap.add_argument("--densify-until", type=int, default=15000)
    ap.add_argument("--densify-grad-threshold", type=float, default=None, help="adc: on the mean view-space gradient (default 2e-4 / --batch)")
    ap.add_argument("--min-opacity", type=float, default=0.005)
    ap.add_argument("--opacity-reset-interval", type=int, default=3000, help="adc: reset the opacities every this many steps (0: never)")
    ap.add_argument("--cap-max", type=int, default=1_000_000, help="mcmc: the largest number of Gaussians")
    ap.add_argument("--noise-lr", type=float, default=5e5, help="mcmc: position noise, times the position rate")
    ap.add_argument("--opacity-reg", type=float, default=0.01, help="mcmc: weight of mean(sigmoid(opacity)) in the loss")
    ap.add_argument("--scale-reg", type=float, default=0.01, help="mcmc: weight of mean(exp(scaling)) in the loss")
    ap.add_argument("--antialiasing", action="store_true")
    ap.add_argument("--filter-3d", action="store_true")
    ap.add_argument("--filter-3d-interval", type=int, default=100)
    ap.add_argument("--depth-sparse", type=float, default=0.0, help="weight of the sparse-point inverse-depth loss, times cameras_extent (0: off; customary 1e-2)")
    ap.add_argument("--depth-priors", default=None, help="a directory of 16-bit monocular inverse-depth priors, one per image name (default: off)")
    ap.add_argument("--depth-prior-weight", type=float, default=1.0)
    ap.add_argument("--depth-prior-weight-final", type=float, default=0.01, help="reached at --steps")
    ap.add_argument("--depth-align", choices=("given", "fit"), default="given", help="priors: the per-image scale / offset from the sparse points, or a fit per step")
    ap.add_argument("--normal-reg", type=float, default=0.0, help="weight of the depth-normal consistency loss (0: off, the default)")
    ap.add_argument("--dist-reg", type=float, default=0.0, help="weight of the depth distortion loss (0: off, the default)")
    ap.add_argument("--reg-from", type=int, default=0, help="neither regulariser before this step")
    ap.add_argument("--normal-alpha-min", type=float, default=0.5, help="(a default, not a measurement)")
    ap.add_argument("--dist-space", choices=("ndc", "linear", "disparity"), default="ndc")
    a = ap.parse_args(argv)
    if a.normal_reg < 0 or a.dist_reg < 0 or a.reg_from < 0 or not a.normal_alpha_min > 0:
        sys.exit("--normal-reg, --dist-reg and --reg-from must not be negative and --normal-alpha-min must be positive")
    if a.steps < 1 or a.batch < 1 or a.hold < 0 or a.densify_interval < 0 or a.sh_degree_interval < 0 or a.filter_3d_interval < 1:
        sys.exit("--steps, --batch and --filter-3d-interval must be positive; --hold and the intervals must not be negative")
    if not 0.0 <= a.lambda_dssim <= 1.0 or not 0 <= a.sh_degree <= 4 or not a.resolution > 0:
        sys.exit("--lambda-dssim must be in [0, 1], --sh-degree in 0..4, --resolution positive")
    if a.depth_sparse < 0 or not a.depth_prior_weight > 0 or not a.depth_prior_weight_final > 0:
        sys.exit("--depth-sparse must not be negative; the two prior weights must be positive")
    if not torch.cuda.is_available():
        sys.exit("train_colmap needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.capture import Capture
    from latentsplat_amd.losses import compute_ssim, photometric_loss
    from latentsplat_amd.optim import SceneAdam, expon_lr
    dev = torch.device("cuda:0")
    depth_on = a.depth_sparse > 0 or a.depth_priors is not None
    capture = Capture.load(a.root, a.sparse, a.images, a.resolution, dev, observations=depth_on)
    if depth_on:
        from latentsplat_amd.depth_sup import inverse_depth_loss
    priors_found = capture.load_depth_priors(a.depth_priors) if a.depth_priors is not None else 0
    if a.depth_priors is not None and priors_found == 0:
        sys.exit(f"--depth-priors {a.depth_priors}: no prior was found for any of the {len(capture)} images")
    train, test = capture.split(a.hold)
    if not train:
        sys.exit(f"--hold {a.hold} leaves no training image among {len(capture)}")
    extent = capture.cameras_extent
    black = torch.zeros(3, device=dev)
    scene = capture.initial_scene(a.sh_degree)
    gaussians_first = scene.num_gaussians
    rates = dict(_xyz=a.lr_position * extent, _features_dc=a.lr_dc, _features_rest=a.lr_dc / 20, _opacity=a.lr_opacity,
                 _scaling=a.lr_scaling, _rotation=a.lr_rotation)
    opt = SceneAdam([dict(params=[p], lr=rates[name], name=name) for name, p in scene.named_parameters() if p.numel()], lr=0.0, eps=1e-15)
    xyz_group = next(g for g in opt.param_groups if g["name"] == "_xyz")
    gen_dev = torch.Generator(device=dev).manual_seed(a.seed)
    rng = random.Random(a.seed)
    control = mcmc = None
    if a.densify_interval > 0 and a.strategy == "adc":
        from latentsplat_amd.density import DensityControl
        control = DensityControl(scene)
        threshold = 2e-4 / a.batch if a.densify_grad_threshold is None else a.densify_grad_threshold
    if a.strategy == "mcmc":
        from latentsplat_amd.mcmc import MCMCControl
        mcmc = MCMCControl(scene, max(a.cap_max, scene.num_gaussians), a.min_opacity)
    if a.normal_reg > 0:
        from latentsplat_amd.normals import normal_consistency_loss
    if a.dist_reg > 0:
        from latentsplat_amd.distortion import depth_pivot, distortion_loss, with_near_far
        centroid = torch.from_numpy(capture.model.xyz.astype("float64").mean(axis=0))
    normal_losses, dist_losses = [], []
    groups = capture.size_groups(train)
    group_views = {size: capture.views(idx, black) for size, idx in groups.items()}
    filter_3d, events = None, []

    def refresh_filter():
        nonlocal filter_3d
        if a.filter_3d:
            per_size = [scene.compute_filter_3d(v, size[1]) for size, v in group_views.items()]
            filter_3d = per_size[0] if len(per_size) == 1 else torch.stack(per_size).amin(dim=0)

    refresh_filter()
    warm = min(WARMUP_STEPS, a.steps // 2)
    losses, depth_losses, queue, t0 = [], [], [], None
    for step in range(a.steps):
        if step == warm:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        if not queue:
            queue = batches(groups, a.batch, rng)
        (H, W), idx = queue.pop()
        views = capture.views(idx, black)
        target, cover = capture.targets(idx), capture.coverage(idx)[:, None]
        opt.zero_grad(set_to_none=True)
        collect = control is not None and step < a.densify_until
        means2D = torch.zeros((len(idx), scene.num_gaussians, 3), device=dev, requires_grad=True) if collect else None
        kw = dict(means2D=means2D) if collect else {}
        with_normals, with_dist = a.normal_reg > 0 and step >= a.reg_from, a.dist_reg > 0 and step >= a.reg_from
        if with_dist:       # near / far where space="ndc" reads them (the NATIVE render does not), and the pivot of these views
            views = with_near_far(views, capture.near[idx], capture.far[idx])
            dist_kw = dict(space=a.dist_space, pivot=depth_pivot(views, centroid, a.dist_space), check_near_far=False)
        if with_dist and with_normals:
            render, normal_map, moment_map, mask, depth, radii = scene.render_surface(views, H, W, filter_3d=filter_3d,
                                                                                      antialiasing=a.antialiasing, **dist_kw, **kw)
        elif with_dist:
            render, moment_map, mask, depth, radii = scene.render_with_distortion(views, H, W, filter_3d=filter_3d,
                                                                                  antialiasing=a.antialiasing, **dist_kw, **kw)
        elif with_normals:
            render, normal_map, mask, depth, radii = scene.render_with_normals(views, H, W, filter_3d=filter_3d,
                                                                               antialiasing=a.antialiasing, **kw)
        else:               # (neither: the call it was)
            render, _, mask, depth, radii = scene.render(views, H, W, filter_3d=filter_3d, antialiasing=a.antialiasing, **kw)
        loss = photometric_loss(render * cover, target * cover, a.lambda_dssim)
        if with_normals:
            normal_losses.append(normal_consistency_loss(normal_map, depth, mask, views, a.normal_alpha_min))
            loss = loss + a.normal_reg * normal_losses[-1]
            normal_losses[-1] = normal_losses[-1].detach()
        if with_dist:
            dist_losses.append(distortion_loss(moment_map, mask, cover[:, 0].contiguous()))
            loss = loss + a.dist_reg * dist_losses[-1]
            dist_losses[-1] = dist_losses[-1].detach()
        if depth_on:
            depth_term = 0.0
            if a.depth_sparse > 0:
                depth_term = a.depth_sparse * extent * inverse_depth_loss(depth, mask, views, capture.sparse_depth(idx), normalize="weights")
            if a.depth_priors is not None:
                prior, affine = capture.depth_priors(idx)
                weight = expon_lr(step, a.depth_prior_weight, a.depth_prior_weight_final, a.steps)
                depth_term = depth_term + weight * inverse_depth_loss(depth, mask, views, prior, cover[:, 0].contiguous(),
                                                                      affine if a.depth_align == "given" else None,
                                                                      align=a.depth_align, normalize="pixels")
            loss = loss + depth_term
            depth_losses.append(depth_term.detach())
        if mcmc is not None:
            loss = loss + mcmc.regularizer(a.opacity_reg, a.scale_reg)
        loss.backward()
        xyz_group["lr"] = expon_lr(step, a.lr_position * extent, a.lr_position_final * extent, a.steps)
        opt.step()
        losses.append(loss.detach())
        done = step + 1
        event = a.densify_interval > 0 and a.densify_from < done <= a.densify_until and done % a.densify_interval == 0
        if collect:
            control.update(means2D.grad, radii)
            if event:
                size = 20.0 if a.opacity_reset_interval and done > a.opacity_reset_interval else 0.0
                events.append(dict(step=done, **control.densify_and_prune(opt, threshold, a.min_opacity, extent, size, generator=gen_dev)))
                refresh_filter()
        if mcmc is not None:
            if event:
                events.append(dict(step=done, **mcmc.step(opt, gen_dev)))
                refresh_filter()
            mcmc.inject_noise(xyz_group["lr"], a.noise_lr, gen_dev)
        if control is not None and a.opacity_reset_interval and done % a.opacity_reset_interval == 0 and done <= a.densify_until:
            control.reset_opacity(opt)
        if a.sh_degree_interval and done % a.sh_degree_interval == 0:
            scene.oneup_sh_degree()
        if a.filter_3d and done % a.filter_3d_interval == 0 and not event:
            refresh_filter()
    torch.cuda.synchronize(dev)
    per_step = (time.perf_counter() - t0) / (a.steps - warm)
    os.makedirs(a.out, exist_ok=True)
    scene.save_ply(os.path.join(a.out, "point_cloud.ply"))
    res = dict(loss_first=float(losses[0]), loss_last=float(losses[-1]), steps=a.steps, gaussians=scene.num_gaussians,
               gaussians_first=gaussians_first, ms_per_step=1e3 * per_step, timed_steps=a.steps - warm, images=len(capture),
               train_views=len(train), test_views=len(test), sizes=[list(s) for s in sorted(capture.size_groups())],
               resolution=a.resolution, hold=a.hold, batch=a.batch, seed=a.seed, cameras_extent=extent, lambda_dssim=a.lambda_dssim,
               strategy=a.strategy, density_events=events, sh_degree=a.sh_degree, active_sh_degree_last=scene.active_sh_degree,
               antialiasing=bool(a.antialiasing), filter_3d=bool(a.filter_3d), format=capture.model.format)
    if depth_on:
        res.update(depth_loss_first=float(depth_losses[0]), depth_loss_last=float(depth_losses[-1]), depth_sparse=a.depth_sparse,
                   depth_priors=priors_found, depth_align=a.depth_align)
    if a.normal_reg > 0 or a.dist_reg > 0:
        res.update(normal_reg=a.normal_reg, dist_reg=a.dist_reg, reg_from=a.reg_from, normal_alpha_min=a.normal_alpha_min,
                   dist_space=a.dist_space)
        if normal_losses:
            res.update(normal_loss_first=float(normal_losses[0]), normal_loss_last=float(normal_losses[-1]))
        if dist_losses:
            res.update(dist_loss_first=float(dist_losses[0]), dist_loss_last=float(dist_losses[-1]))
    if test:
        psnr, ssim, names = [], [], []
        with torch.no_grad():
            for (H, W), idx in sorted(capture.size_groups(test).items()):
                for at in range(0, len(idx), EVAL_BATCH):
                    part = idx[at:at + EVAL_BATCH]
                    cover = capture.coverage(part)[:, None]
                    render = scene.render(capture.views(part, black), H, W, filter_3d=filter_3d, antialiasing=a.antialiasing)[0].clamp(0.0, 1.0) * cover
                    target = capture.targets(part) * cover
                    mse = ((render - target) ** 2).sum(dim=(1, 2, 3)) / (3.0 * cover.sum(dim=(1, 2, 3))).clamp_min(1.0)
                    psnr += (-10.0 * torch.log10(mse.clamp_min(1e-12))).tolist()
                    ssim += compute_ssim(target, render).tolist() if min(H, W) >= 11 else [None] * len(part)     # (an 11 x 11 window)
                    names += [capture.names[k] for k in part]
        scored = [s for s in ssim if s is not None]
        res.update(psnr=sum(psnr) / len(psnr), ssim=sum(scored) / len(scored) if scored else None, test=dict(names=names, psnr=psnr, ssim=ssim))
    with open(os.path.join(a.out, "metrics.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("test", "density_events")}))
    return res


if __name__ == "__main__":
    main()
