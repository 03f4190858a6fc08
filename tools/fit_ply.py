#!/usr/bin/env python
"""Fit a 3DGS scene file to renders of itself: the load -> optimise -> save loop of INTEGRATION.md §10, as a tool.

  1. `GaussianScene.from_ply(path, device)`: the file's raw parameters (log-scales, opacity logits, unnormalised
     quaternions, f_dc / f_rest) under the published trainer's names;
  2. target images: the loaded scene rendered under `no_grad` from the cameras of `tools/render_ply.py` (a circle around
     the median of the means, `--distance` scene extents away);
  3. the parameters are perturbed with seeded Gaussian noise scaled by `--noise`; unit noise is 0.1 on f_dc, 0.5 on the
     opacity logits, 0.05 on the log-scales, 0.05 on the quaternions and 0.002 x extent on the positions;
  4. `torch.optim.Adam`, one parameter group per tensor, minimising the mean L1 between render and target over all views
     each step.  Every step is one `lsr_scene_activate_forward`, the rasterizer, its backward and one
     `lsr_scene_activate_backward`.  `--lambda-dssim L` with L > 0 minimises the published trainer's objective instead,
     `(1 - L) * L1 + L * (1 - SSIM)` (its L is 0.2), through `latentsplat_amd.photometric_loss`: one HIP call each way;
  5. `fit.json` (`loss_first`, `loss_last`, `steps`, `lambda_dssim`, the wall time per step after a warm-up, the scene's
     size) and the fitted scene as `point_cloud.ply` in `--out`.

The learning rates default to the published trainer's customary ones (position 1.6e-4 x extent, f_dc 2.5e-3, f_rest
f_dc / 20, opacity 5e-2, scaling 5e-3, rotation 1e-3; Adam eps 1e-15).  They are defaults, not measurements: nothing here
tuned them.

`--optimizer fused` takes the step with `latentsplat_amd.SceneAdam`: all six tensors in one HIP launch.
`--optimizer sparse` is the same without bias correction and with the mask `visible_from_radii` of the step's render: only
Gaussians that were on screen in one of the step's views are updated.  `--optimizer torch`, the default, is
`torch.optim.Adam` as before.  `--lr-position-final F` turns on the customary exponential schedule of the position rate
(`expon_lr`): from `--lr-position` to F, both times the extent, over `--lr-position-max-steps` steps (default `--steps`).
`fit.json` names the optimizer.

Adaptive density control is off by default.  `--densify-interval I` with I > 0 turns it on: every step
renders with a per-view `(V, n, 3)` `means2D` and feeds its gradient and the radii to `DensityControl.update`; every I-th
step after `--densify-from` and up to `--densify-until` runs `DensityControl.densify_and_prune` (clone, split, prune; the
optimizer's moments travel with their rows), with size pruning (20 px, 0.1 x extent) once the first opacity reset is
behind; every `--opacity-reset-interval`-th step resets the opacities.  The loss here is a mean over the V views, so each
view's gradient is 1 / V of the published single-view one and `--densify-grad-threshold` defaults to `2e-4 / views`:
like the learning rates, a default and not a measurement.  `--drop F` removes a seeded fraction F of the Gaussians after
the targets are rendered, so that there is something to grow back.  With densification on, `fit.json` also holds
`gaussians_first`, `gaussians_last` and `densify_events` (the counts of every event).

`--from-points` starts the fit from the file's point cloud alone: after the targets are rendered the
scene is replaced by `GaussianScene.from_point_cloud(xyz, clamp(0.5 + 0.2820948 f_dc, 0, 1), sh_degree)` — the published
`create_from_pcd`: scales from the 3-nearest-neighbour distances (`lsr_knn3`), identity rotations, opacity 0.1, active SH
degree 0 — and `--noise` / `--drop` are ignored.  `--sh-degree-interval I` with I > 0 calls `oneup_sh_degree()` every I
steps (default 0: never), without which a scene that starts at active degree 0 never trains its higher bands.  `fit.json`
holds `from_points` and `active_sh_degree_last`.

`--strategy mcmc` replaces adaptive density control by the MCMC strategy (`latentsplat_amd.MCMCControl`):
`--densify-interval / --densify-from / --densify-until` then schedule `MCMCControl.step` (dead Gaussians are relocated onto
live ones, then the scene grows by 5 % up to `--cap-max`, default the file's own count); the opacity and scale regulariser
(`--opacity-reg`, `--scale-reg`) joins the loss; and after every optimizer step covariance-shaped noise is added to the
positions (`--noise-lr` times the current position rate).  No gradient statistics are gathered.  `fit.json` then holds
`strategy`, `cap_max`, `gaussians_first`, `gaussians_last` and `mcmc_events` (`step, dead, relocated, added, n_in, n_out` of
every event).  `--strategy adc`, the default, is everything above.

`--filter-3d` trains with the 3D smoothing filter of Mip-Splatting: `scene.compute_filter_3d(views,
size)` before the first step, after every densification / MCMC event (the filter of another row count is refused) and every
`--filter-3d-interval` steps (default 100, the published cadence); every render of the fit takes it (`filter_3d=`), the
targets do not.  Besides the raw `point_cloud.ply`, `point_cloud_fused.ply` holds the scene with the filter baked into
opacities and scales, which any viewer shows filtered.  `fit.json` then holds `filter_3d`, `filter_3d_interval`,
`filter_3d_events` (`step, reason, gaussians` of every computation) and `fused_ply`.

`--antialiasing` renders the targets and every step of the fit with the rasterizer's opacity compensation for its 0.3
screen-space low-pass (the published trainer's `--antialiasing`); `fit.json` holds `antialiasing`.

`--absgrad` (with `--densify-interval`) densifies on the ABSOLUTE view-space gradient of AbsGS (gsplat's
`absgrad`): the densification render also passes a per-view `(V, n, 3)` `means2D_abs`, and `DensityControl.update` gets ITS
gradient — the sum over the pixels of the magnitudes of their contributions, in which a large blurry splat's contributions do
not cancel.  `--densify-grad-threshold` then defaults to `8e-4 / views`, gsplat's documented companion value divided by the
views as above: a default, not a measurement.  `fit.json` holds `absgrad`.

`--bilateral-grid X Y L` trains with bilateral-grid appearance compensation (`latentsplat_amd.BilateralGrid`):
every fitted render goes through one X x Y x L grid of colour affines per view before the loss (`1 1 1`: one affine per view,
the published trainer's exposure compensation; `16 16 8`: the published grid), `--tv-weight` (default 10, the published one)
times the grids' total variation joins the loss, and the grids take their steps from a `torch.optim.Adam` of their own at
`--bilateral-grid-lr` (default 2e-3, the published one; like the other rates a default, not a measurement), so the scene's
optimizer and its re-keying at densification are untouched.  `--target-jitter S` with S > 0 gives every target view a seeded
per-channel affine (gain uniform in [1 - S, 1 + S], offset uniform in [-S / 4, S / 4]) from a generator of its own: photographs
that disagree, for the grids to absorb.  `fit.json` then holds `bilateral_grid`, `tv_weight` and `tv_last`, and/or
`target_jitter`; `bilateral_grids.pt` holds the module's state dict.

`--normal-reg W` with W > 0 adds W times the depth-normal consistency loss: from step `--normal-reg-from`
(default 0) on, every step renders with `GaussianScene.render_with_normals` and `normal_consistency_loss` compares the blended
normals with the normals of the rendered depth at the pixels covered more than `--normal-alpha-min` (default 0.5: a default,
not a measurement).  `--flatten-reg W` adds W times `flatten_loss`, the mean shortest extent.  Together with `--absgrad` the
normal term is refused (six payload channels).  `fit.json` then holds the four values and `normal_loss_first / _last`.
`--dist-reg W` with W > 0 adds W times the depth distortion loss: from step `--dist-reg-from` (default 0)
on, every step renders with `GaussianScene.render_with_distortion` (with `--normal-reg`: `render_surface`, both payloads in one
render) and `distortion_loss` takes the blended depth moments and the mask.  The depths are measured in `--dist-space`
(default ndc, the mapping of 2DGS, with the cameras' near / far) about `depth_pivot` at the mean of the scene's positions
at the start.  Together with `--absgrad` it is refused (five payload channels).  `fit.json` then holds `dist_reg`,
`dist_reg_from`, `dist_space` and `dist_loss_first / _last`.
Without the two weights the run is the one it was.

usage: python tools/fit_ply.py scene.ply --out DIR [--views 8] [--size 256] [--steps 200] [--noise 1.0] [--seed 0] [--distance 2.5]
                               [--lambda-dssim 0.0] [--drop 0.0] [--densify-interval 0] [--densify-from 0] [--densify-until STEPS]
                               [--densify-grad-threshold 2e-4/VIEWS] [--min-opacity 0.005] [--opacity-reset-interval 0]
                               [--optimizer torch|fused|sparse] [--lr-position-final F] [--lr-position-max-steps S]
                               [--from-points] [--sh-degree-interval 0]
                               [--strategy adc|mcmc] [--cap-max N] [--noise-lr 5e5] [--opacity-reg 0.01] [--scale-reg 0.01]
                               [--filter-3d] [--filter-3d-interval 100] [--antialiasing] [--absgrad]
                               [--bilateral-grid X Y L] [--bilateral-grid-lr 2e-3] [--tv-weight 10] [--target-jitter 0]
                               [--normal-reg 0] [--normal-reg-from 0] [--normal-alpha-min 0.5] [--flatten-reg 0]
                               [--dist-reg 0] [--dist-reg-from 0] [--dist-space ndc|linear|disparity]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from render_ply import circle_cameras, scene_extent  # noqa: E402

UNIT_NOISE = dict(_features_dc=0.1, _opacity=0.5, _scaling=0.05, _rotation=0.05)
POSITION_NOISE = 0.002      # x extent
WARMUP_STEPS = 5            # steps left out of the time per step (fewer when there are fewer than 10 steps)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                 epilog="The learning rates are the published trainer's customary defaults, not measurements.")
    ap.add_argument("ply")
    ap.add_argument("--out", required=True)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--noise", type=float, default=1.0, help="scale of the perturbation (0: start from the loaded scene)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--distance", type=float, default=2.5, help="circle radius in scene extents")
    ap.add_argument("--lambda-dssim", type=float, default=0.0,
                    help="weight of the D-SSIM term (0: plain L1, the default; the published trainer uses 0.2)")
    ap.add_argument("--lr-position", type=float, default=1.6e-4, help="times the scene's extent (a default, not a measurement)")
    ap.add_argument("--lr-dc", type=float, default=2.5e-3, help="(a default, not a measurement)")
    ap.add_argument("--lr-rest", type=float, default=None, help="default: --lr-dc / 20")
    ap.add_argument("--lr-opacity", type=float, default=5e-2, help="(a default, not a measurement)")
    ap.add_argument("--lr-scaling", type=float, default=5e-3, help="(a default, not a measurement)")
    ap.add_argument("--lr-rotation", type=float, default=1e-3, help="(a default, not a measurement)")
    ap.add_argument("--optimizer", choices=("torch", "fused", "sparse"), default="torch",
                    help="torch: torch.optim.Adam (the default); fused: SceneAdam, one HIP launch; sparse: SceneAdam without bias "
                         "correction, updating only the Gaussians visible in the step's views")
    ap.add_argument("--lr-position-final", type=float, default=None,
                    help="times the extent: decay the position rate exponentially to this (default: constant rate)")
    ap.add_argument("--lr-position-max-steps", type=int, default=None, help="steps over which the position rate decays (default: --steps)")
    ap.add_argument("--drop", type=float, default=0.0,
                    help="remove this fraction of the Gaussians (seeded) after the targets are rendered (default 0: none)")
    ap.add_argument("--densify-interval", type=int, default=0, help="densify and prune every this many steps (0: never, the default)")
    ap.add_argument("--densify-from", type=int, default=0, help="no densification before this step")
    ap.add_argument("--densify-until", type=int, default=None, help="no densification (and no statistics) after this step (default: --steps)")
    ap.add_argument("--densify-grad-threshold", type=float, default=None,
                    help="on the mean view-space gradient (default 2e-4 / --views, with --absgrad 8e-4 / --views: defaults, not measurements)")
    ap.add_argument("--min-opacity", type=float, default=0.005, help="Gaussians below it are pruned at a densification")
    ap.add_argument("--opacity-reset-interval", type=int, default=0, help="reset the opacities every this many steps (0: never)")
    ap.add_argument("--from-points", action="store_true",
                    help="start from the file's points and DC colours alone (GaussianScene.from_point_cloud); --noise and --drop are ignored")
    ap.add_argument("--sh-degree-interval", type=int, default=0, help="render one more SH band every this many steps (0: never, the default)")
    ap.add_argument("--strategy", choices=("adc", "mcmc"), default="adc",
                    help="what --densify-interval schedules: adc, adaptive density control (the default), or mcmc, relocation and growth to a cap")
    ap.add_argument("--cap-max", type=int, default=None, help="mcmc: the largest number of Gaussians (default: the file's count)")
    ap.add_argument("--noise-lr", type=float, default=5e5, help="mcmc: position noise, times the position rate (the published default)")
    ap.add_argument("--opacity-reg", type=float, default=0.01, help="mcmc: weight of mean(sigmoid(opacity)) in the loss")
    ap.add_argument("--scale-reg", type=float, default=0.01, help="mcmc: weight of mean(exp(scaling)) in the loss")
    ap.add_argument("--filter-3d", action="store_true",
                    help="train with the 3D smoothing filter of Mip-Splatting and also write point_cloud_fused.ply")
    ap.add_argument("--antialiasing", action="store_true",
                    help="render with opacity compensation for the 0.3 screen-space low-pass (default: the classic mode)")
    ap.add_argument("--absgrad", action="store_true",
                    help="densify on the absolute view-space gradient (AbsGS): means2D_abs of the render instead of means2D")
    ap.add_argument("--filter-3d-interval", type=int, default=100, help="recompute the 3D filter every this many steps (the published cadence)")
    ap.add_argument("--bilateral-grid", type=int, nargs=3, default=None, metavar=("X", "Y", "L"),
                    help="one X x Y x L bilateral grid of colour affines per view between render and loss (default: none; "
                         "1 1 1: one affine per view; 16 16 8: the published grid)")
    ap.add_argument("--bilateral-grid-lr", type=float, default=2e-3, help="Adam rate of the grids (the published default, not a measurement)")
    ap.add_argument("--tv-weight", type=float, default=10.0, help="weight of the grids' total variation in the loss (the published default)")
    ap.add_argument("--normal-reg", type=float, default=0.0,
                    help="weight of the depth-normal consistency loss (0: off, the default): every step renders the normals of "
                         "the Gaussians next to the colour and compares them with the normals of the rendered depth")
    ap.add_argument("--normal-reg-from", type=int, default=0, help="no normal consistency loss before this step")
    ap.add_argument("--normal-alpha-min", type=float, default=0.5,
                    help="pixels the scene covers less than this take no part in the normal loss (a default, not a measurement)")
    ap.add_argument("--flatten-reg", type=float, default=0.0, help="weight of mean(min_k exp(scaling)) in the loss (0: off, the default)")
    ap.add_argument("--dist-reg", type=float, default=0.0,
                    help="weight of the depth distortion loss (0: off, the default): every step renders the depth moments of "
                         "the Gaussians next to the colour")
    ap.add_argument("--dist-reg-from", type=int, default=0, help="no distortion loss before this step")
    ap.add_argument("--dist-space", choices=("ndc", "linear", "disparity"), default="ndc",
                    help="what the distortion term measures depth in (ndc: the mapping of 2DGS)")
    ap.add_argument("--target-jitter", type=float, default=0.0,
                    help="S > 0: a seeded per-channel affine on every target view, gain in [1 - S, 1 + S], offset in [-S / 4, S / 4] (default 0: none)")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.views < 1:
        sys.exit("fit_ply needs at least one step and one view")
    if a.normal_reg < 0.0 or a.flatten_reg < 0.0 or not a.normal_alpha_min > 0.0:
        sys.exit("--normal-reg and --flatten-reg must not be negative and --normal-alpha-min must be positive")
    if a.normal_reg > 0.0 and a.absgrad:
        sys.exit("--normal-reg with --absgrad: colour and normals are six payload channels, the absolute gradient takes at most four")
    if a.dist_reg < 0.0:
        sys.exit("--dist-reg must not be negative")
    if a.dist_reg > 0.0 and a.absgrad:
        sys.exit("--dist-reg with --absgrad: colour and depth moments are five payload channels, the absolute gradient takes at most four")
    if not 0.0 <= a.lambda_dssim <= 1.0:
        sys.exit("--lambda-dssim must be in [0, 1]")
    if not 0.0 <= a.drop < 1.0 or a.densify_interval < 0 or a.opacity_reset_interval < 0 or a.sh_degree_interval < 0:
        sys.exit("--drop must be in [0, 1); the intervals must not be negative")
    if a.lr_position_final is not None and (a.lr_position_final < 0.0 or (a.lr_position_max_steps or a.steps) < 1):
        sys.exit("--lr-position-final must not be negative and --lr-position-max-steps must be positive")
    if a.filter_3d_interval < 1:
        sys.exit("--filter-3d-interval must be positive")
    if a.cap_max is not None and a.cap_max < 1:
        sys.exit("--cap-max must be positive")
    if a.target_jitter < 0.0 or a.tv_weight < 0.0 or a.bilateral_grid_lr <= 0.0:
        sys.exit("--target-jitter and --tv-weight must not be negative, --bilateral-grid-lr must be positive")
    if a.bilateral_grid is not None and not (1 <= a.bilateral_grid[0] <= 64 and 1 <= a.bilateral_grid[1] <= 64 and 1 <= a.bilateral_grid[2] <= 16):
        sys.exit("--bilateral-grid X Y L takes 1..64 nodes in x and y and 1..16 in luminance")
    if not torch.cuda.is_available():
        sys.exit("fit_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.rasterizer import build_view_table
    from latentsplat_amd.losses import photometric_loss
    from latentsplat_amd.normals import flatten_loss, normal_consistency_loss
    from latentsplat_amd.optim import SceneAdam, expon_lr, visible_from_radii
    from latentsplat_amd.scene_model import GaussianScene
    dev = torch.device("cuda:0")
    scene = GaussianScene.from_ply(a.ply, dev)
    gaussians_file = scene.num_gaussians
    with torch.no_grad():
        centre, extent = scene_extent(scene._xyz)
        ext, intr, near, far = circle_cameras(centre, extent, a.views, a.distance)
        views = build_view_table(ext, intr, near, far, torch.zeros(3, device=dev))
        target = scene.render(views, a.size, a.size, antialiasing=a.antialiasing)[0]
        if a.dist_reg > 0.0:            # near / far where space="ndc" reads them (the NATIVE render does not), and the pivot
            from latentsplat_amd.distortion import depth_pivot, distortion_loss, with_near_far
            dist_views = with_near_far(views, near, far)
            dist_pivot = depth_pivot(dist_views, scene._xyz.mean(dim=0), a.dist_space)
        if a.target_jitter > 0.0:       # a generator of its own: the perturbation below draws what it always drew
            gen_jitter = torch.Generator().manual_seed(a.seed + 0x5eed)
            gain = 1.0 + a.target_jitter * (2.0 * torch.rand(a.views, 3, generator=gen_jitter) - 1.0)
            offset = 0.25 * a.target_jitter * (2.0 * torch.rand(a.views, 3, generator=gen_jitter) - 1.0)
            target = target * gain.to(dev)[:, :, None, None] + offset.to(dev)[:, :, None, None]
        gen = torch.Generator().manual_seed(a.seed)
        noise = dict(UNIT_NOISE, _xyz=POSITION_NOISE * float(extent))
        if a.from_points:
            colors = (0.5 + 0.2820948 * scene._features_dc.detach()[:, 0, :]).clamp(0.0, 1.0)
            scene = GaussianScene.from_point_cloud(scene._xyz.detach(), colors, sh_degree=scene.max_sh_degree)
        for name, p in scene.named_parameters():
            if name in noise and a.noise and not a.from_points:
                p.add_((torch.randn(p.shape, generator=gen) * (a.noise * noise[name])).to(dev))
        if a.drop > 0.0 and not a.from_points:
            keep = (torch.rand(scene.num_gaussians, generator=gen) >= a.drop).to(dev)
            scene.replace_parameters_(**{name[1:]: p.detach()[keep] for name, p in scene.named_parameters()})
    rates = dict(_xyz=a.lr_position * float(extent), _features_dc=a.lr_dc,
                 _features_rest=a.lr_dc / 20 if a.lr_rest is None else a.lr_rest, _opacity=a.lr_opacity,
                 _scaling=a.lr_scaling, _rotation=a.lr_rotation)
    groups = [dict(params=[p], lr=rates[name], name=name) for name, p in scene.named_parameters() if p.numel()]
    if a.optimizer == "torch":
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    else:
        opt = SceneAdam(groups, lr=0.0, eps=1e-15, bias_correction=a.optimizer == "fused")
    sparse = a.optimizer == "sparse"
    xyz_group = next(g for g in opt.param_groups if g["name"] == "_xyz")
    gen_dev = torch.Generator(device=dev).manual_seed(a.seed)      # the children's offsets at a split
    mcmc = None
    if a.strategy == "mcmc":
        from latentsplat_amd.mcmc import MCMCControl
        cap_max = gaussians_file if a.cap_max is None else a.cap_max
        mcmc = MCMCControl(scene, cap_max, a.min_opacity)
        mcmc_until = a.steps if a.densify_until is None else a.densify_until
    densify = a.densify_interval > 0 and mcmc is None
    control = None
    if densify:
        from latentsplat_amd.density import DensityControl
        control = DensityControl(scene)
        until = a.steps if a.densify_until is None else a.densify_until
        # (8e-4: the value gsplat documents next to absgrad; like 2e-4 a default, not a measurement)
        threshold = (8e-4 if a.absgrad else 2e-4) / a.views if a.densify_grad_threshold is None else a.densify_grad_threshold
    grids, tv = None, None
    if a.bilateral_grid is not None:
        from latentsplat_amd.bilagrid import BilateralGrid
        grids = BilateralGrid(a.views, *a.bilateral_grid).to(dev)
        grid_opt = torch.optim.Adam(grids.parameters(), lr=a.bilateral_grid_lr, eps=1e-15)
        view_idx = torch.arange(a.views, dtype=torch.int32, device=dev)
    gaussians_first, events = scene.num_gaussians, []
    filter_3d, filter_events = None, []

    def refresh_filter(step, reason):
        nonlocal filter_3d
        if a.filter_3d:
            filter_3d = scene.compute_filter_3d(views, a.size)
            filter_events.append(dict(step=step, reason=reason, gaussians=scene.num_gaussians))

    refresh_filter(0, "start")
    warm = min(WARMUP_STEPS, a.steps // 2)
    losses, normal_losses, dist_losses = [], [], []
    t0 = None
    for step in range(a.steps):
        if step == warm:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        with_normals = a.normal_reg > 0.0 and step >= a.normal_reg_from
        render_scene = scene.render_with_normals if with_normals else scene.render      # (without --normal-reg: the call it was)
        with_dist = a.dist_reg > 0.0 and step >= a.dist_reg_from
        if with_dist:                   # (--absgrad is refused above: no means2D_abs reaches these)
            dist_kw = dict(space=a.dist_space, pivot=dist_pivot, check_near_far=False)
            if with_normals:
                def render_scene(v, h, w, **kw):
                    color, nmap, moment_map, m, d, r = scene.render_surface(dist_views, h, w, **dist_kw, **kw)
                    return color, (nmap, moment_map), m, d, r
            else:
                def render_scene(v, h, w, **kw):
                    color, moment_map, m, d, r = scene.render_with_distortion(dist_views, h, w, **dist_kw, **kw)
                    return color, (None, moment_map), m, d, r
        if densify and step < until:
            means2D = torch.zeros((a.views, scene.num_gaussians, 3), device=dev, requires_grad=True)
            stat = dict(means2D_abs=torch.zeros_like(means2D, requires_grad=True)) if a.absgrad else {}
            render, normal_map, mask, depth, radii = render_scene(views, a.size, a.size, filter_3d=filter_3d, means2D=means2D,
                                                                  antialiasing=a.antialiasing, **stat)
        else:
            means2D = None
            render, normal_map, mask, depth, radii = render_scene(views, a.size, a.size, filter_3d=filter_3d,
                                                                  antialiasing=a.antialiasing)
        if with_dist:
            normal_map, moment_map = normal_map
        if grids is not None:
            grid_opt.zero_grad(set_to_none=True)
            render = grids(render, view_idx)
        loss = photometric_loss(render, target, a.lambda_dssim) if a.lambda_dssim > 0 else (render - target).abs().mean()
        if mcmc is not None:
            loss = loss + mcmc.regularizer(a.opacity_reg, a.scale_reg)
        if with_normals:
            normal_loss = normal_consistency_loss(normal_map, depth, mask, views, a.normal_alpha_min)
            normal_losses.append(normal_loss.detach())
            loss = loss + a.normal_reg * normal_loss
        if with_dist:
            dist_loss = distortion_loss(moment_map, mask)
            dist_losses.append(dist_loss.detach())
            loss = loss + a.dist_reg * dist_loss
        if a.flatten_reg > 0.0:
            loss = loss + a.flatten_reg * flatten_loss(scene._scaling)
        if grids is not None:
            tv = grids.tv_loss()
            loss = loss + a.tv_weight * tv
        loss.backward()
        if grids is not None:
            grid_opt.step()
        if a.lr_position_final is not None:
            xyz_group["lr"] = expon_lr(step, a.lr_position * float(extent), a.lr_position_final * float(extent),
                                       a.lr_position_max_steps or a.steps)
        if sparse:
            opt.step(visibility=visible_from_radii(radii))
        else:
            opt.step()
        losses.append(loss.detach())
        if means2D is not None:
            done = step + 1
            control.update(stat["means2D_abs"].grad if a.absgrad else means2D.grad, radii)
            if done > a.densify_from and done % a.densify_interval == 0:
                size = 20.0 if a.opacity_reset_interval and done > a.opacity_reset_interval else 0.0
                counts = control.densify_and_prune(opt, threshold, a.min_opacity, float(extent), size, generator=gen_dev)
                events.append(dict(step=done, **counts))
                refresh_filter(done, "densify")
        if mcmc is not None:
            done = step + 1
            if a.densify_interval > 0 and a.densify_from < done <= mcmc_until and done % a.densify_interval == 0:
                events.append(dict(step=done, **mcmc.step(opt, gen_dev)))
                refresh_filter(done, "mcmc")
            mcmc.inject_noise(xyz_group["lr"], a.noise_lr, gen_dev)
        if control is not None and a.opacity_reset_interval and (step + 1) % a.opacity_reset_interval == 0:
            control.reset_opacity(opt)
        if a.sh_degree_interval and (step + 1) % a.sh_degree_interval == 0:
            scene.oneup_sh_degree()
        if (step + 1) % a.filter_3d_interval == 0 and not (filter_events and filter_events[-1]["step"] == step + 1):
            refresh_filter(step + 1, "interval")
    torch.cuda.synchronize(dev)
    per_step = (time.perf_counter() - t0) / (a.steps - warm)
    os.makedirs(a.out, exist_ok=True)
    scene.save_ply(os.path.join(a.out, "point_cloud.ply"))
    res = dict(loss_first=float(losses[0]), loss_last=float(losses[-1]), steps=a.steps, ms_per_step=1e3 * per_step,
               timed_steps=a.steps - warm, gaussians=scene.num_gaussians, sh_degree=scene.max_sh_degree, views=a.views,
               size=a.size, noise=a.noise, seed=a.seed, extent=float(extent), lambda_dssim=a.lambda_dssim, optimizer=a.optimizer,
               from_points=bool(a.from_points), active_sh_degree_last=scene.active_sh_degree,
               antialiasing=bool(a.antialiasing), absgrad=bool(a.absgrad))
    if a.normal_reg > 0.0 or a.flatten_reg > 0.0:
        res.update(normal_reg=a.normal_reg, normal_reg_from=a.normal_reg_from, normal_alpha_min=a.normal_alpha_min,
                   flatten_reg=a.flatten_reg)
        if normal_losses:
            res.update(normal_loss_first=float(normal_losses[0]), normal_loss_last=float(normal_losses[-1]))
    if a.dist_reg > 0.0:
        res.update(dist_reg=a.dist_reg, dist_reg_from=a.dist_reg_from, dist_space=a.dist_space)
        if dist_losses:
            res.update(dist_loss_first=float(dist_losses[0]), dist_loss_last=float(dist_losses[-1]))
    if densify:
        res.update(gaussians_first=gaussians_first, gaussians_last=scene.num_gaussians, densify_events=events)
    if mcmc is not None:
        res.update(strategy="mcmc", cap_max=cap_max, gaussians_first=gaussians_first, gaussians_last=scene.num_gaussians,
                   mcmc_events=events)
    if a.filter_3d:
        scene.save_ply(os.path.join(a.out, "point_cloud_fused.ply"), filter_3d=filter_3d)
        res.update(filter_3d=True, filter_3d_interval=a.filter_3d_interval, filter_3d_events=filter_events,
                   fused_ply="point_cloud_fused.ply")
    if grids is not None:
        torch.save(grids.state_dict(), os.path.join(a.out, "bilateral_grids.pt"))
        res.update(bilateral_grid=list(a.bilateral_grid), tv_weight=a.tv_weight, tv_last=float(tv.detach()))
    if a.target_jitter > 0.0:
        res.update(target_jitter=a.target_jitter)
    with open(os.path.join(a.out, "fit.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
