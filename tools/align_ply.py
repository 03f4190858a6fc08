#!/usr/bin/env python
"""Register one 3DGS scene file to another photometrically: fit the pose of `moving.ply` so that its renders match the
renders of `fixed.ply`.

  1. both files are loaded as `GaussianScene`s; cameras on a circle around `fixed.ply` (the ring of tools/render_ply.py)
     render it once: the targets;
  2. one `PartPoses(1)` (a quaternion, a translation and, with `--learn-scale`, a log-scale) poses `moving.ply` inside
     `scene.render(..., poses=...)`; Adam minimises `photometric_loss` (L1 + D-SSIM) between its renders and the targets.
     Only the pose is trained: its gradient comes from `lsr_scene_pose_grad`, one pass over the scene per step;
  3. the moving scene is moved in place by the fitted similarity (`transform_`) and written to `DIR/aligned.ply`;
     `DIR/align.json` holds the recovered 4x4 matrix (row-major, float64, built from the fitted parameters) and the loss
     curve.

The fit is local: it follows the image gradient from the identity, so the two scenes must overlap in the renders to begin
with (a few degrees, a few percent of the extent).  Optimizer moments are the pose's own and start at zero.

usage: python tools/align_ply.py moving.ply --to fixed.ply --out DIR [--views 8] [--size 128] [--steps 200] [--learn-scale]
                                 [--lambda-dssim 0.2] [--lr 0.003] [--distance 2.5]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def fit(moving, views, targets, height: int, width: int, steps: int, learn_scale: bool, lambda_dssim: float, lr: float,
        translation_lr: float):
    """Adam on one `PartPoses(1)`: (poses, loss curve).  The rotation and the log-scale step by `lr`, the translation by
    `translation_lr` (scene units)."""
    from latentsplat_amd.losses import photometric_loss
    from latentsplat_amd.pose import PartPoses
    poses = PartPoses(1, learn_scale=learn_scale).to(targets.device)
    groups = [dict(params=[poses.rotation], lr=lr), dict(params=[poses.translation], lr=translation_lr)]
    if learn_scale:
        groups.append(dict(params=[poses.log_scale], lr=lr))
    opt = torch.optim.Adam(groups)
    curve = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = photometric_loss(moving.render(views, height, width, poses=poses)[0], targets, lambda_dssim)
        loss.backward()
        opt.step()
        curve.append(loss.detach())
    return poses, [float(v) for v in torch.stack(curve).cpu()] if curve else []


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("moving")
    ap.add_argument("--to", required=True, dest="fixed")
    ap.add_argument("--out", required=True)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--learn-scale", action="store_true")
    ap.add_argument("--lambda-dssim", type=float, default=0.2)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--distance", type=float, default=2.5, help="circle radius in scene extents")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("align_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.rasterizer import build_view_table
    from render_ply import circle_cameras, scene_extent
    dev = torch.device("cuda:0")
    fixed, moving = GaussianScene.from_ply(a.fixed, dev), GaussianScene.from_ply(a.moving, dev)
    for p in moving.parameters():
        p.requires_grad_(False)                     # only the pose is fitted
    with torch.no_grad():
        centre, extent = scene_extent(fixed._xyz.detach())
        ext, intr, near, far = circle_cameras(centre, extent, a.views, a.distance)
        views = build_view_table(ext, intr, near, far, torch.zeros(3, device=dev))
        targets = fixed.render(views, a.size, a.size)[0]
    poses, curve = fit(moving, views, targets, a.size, a.size, a.steps, a.learn_scale, a.lambda_dssim, a.lr,
                       a.lr * float(extent))
    M = poses.as_matrices()[0]
    moving.transform_(M.to(dev))
    os.makedirs(a.out, exist_ok=True)
    moving.save_ply(os.path.join(a.out, "aligned.ply"))
    result = dict(matrix=[float(v) for v in M.reshape(-1)], loss=curve, gaussians=int(moving.num_gaussians), views=a.views,
                  size=a.size, steps=a.steps, learn_scale=bool(a.learn_scale), lambda_dssim=a.lambda_dssim)
    with open(os.path.join(a.out, "align.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(matrix=result["matrix"], first_loss=curve[0] if curve else None, last_loss=curve[-1] if curve else None)))
    return result


if __name__ == "__main__":
    main()
