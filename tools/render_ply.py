#!/usr/bin/env python
"""Render a trained 3DGS scene file: the recipe of INTEGRATION.md §9, as a tool.

  1. `load_ply(path, device)`: the library's host reader + one HIP kernel -> means, covariances, opacities, colour SH;
  2. cameras on a circle around the median of the means, in the x-z plane, looking at it; the circle's radius is
     `--distance` times the scene's extent (the 0.95-quantile of |mean - median| over the Gaussians, largest axis);
  3. `build_view_table` (scale-invariant: the scene is rescaled so that near == 1, and with it the near cull) ->
     `rasterize_views` (colour SH in the "3dgs" basis, what such files hold);
  4. `color.npy (V,3,H,W)`, `mask.npy (V,H,W)`, `depth.npy (V,H,W)` (scene units) and `status.json` (the pair counts of
     `last_forward_status()` and the scene's size) in `--out`.

Files written by this project's own `export_ply` store the opacity as it is: pass `--opacity raw` for those.
`--antialiasing` renders with the rasterizer's opacity compensation for its 0.3 screen-space low-pass;
`status.json` holds `antialiasing`.
`--normals OUT.npy` also writes `(2, V, 3, H, W)`: the rendered normal map (the Gaussians' shortest axes, turned toward the
camera, blended as a payload and divided by the mask where it exceeds `--normal-alpha-min`) and the normals of the rendered
depth (`depth_to_normals`, 0 where invalid) of the same views, both in camera space.
`--distortion OUT.npy` also writes `(V, H, W)`: the depth distortion map `A M2 - M1^2` of the same views,
from a render with the depth moments of the Gaussians as the payload: depths in `--dist-space` (default ndc, with the
cameras' near / far), taken about `depth_pivot` at the scene's centre.

usage: python tools/render_ply.py scene.ply --out renders [--views 8] [--size 256] [--distance 2.5] [--opacity logit]
                                  [--antialiasing] [--normals OUT.npy] [--normal-alpha-min 0.5]
                                  [--distortion OUT.npy] [--dist-space ndc|linear|disparity]"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FOCAL = 0.8     # normalised focal length of the cameras (tan(fov / 2) = 0.625)


def scene_extent(means: torch.Tensor):
    """(median (3,), 0.95-quantile extent) of the means; at most ~4 M of them are looked at (torch.quantile's limit)."""
    sample = means[:: max(1, means.shape[0] // 4_000_000)]
    centre = sample.median(dim=0).values
    extent = (sample - centre).abs().quantile(0.95, dim=0).max()
    return centre, extent


def circle_cameras(centre: torch.Tensor, extent: torch.Tensor, views: int, distance: float):
    """Camera-to-world matrices (V,4,4) (x right, y down, z forward), normalised intrinsics (V,3,3), near / far (V,)."""
    dev = centre.device
    radius = float(extent) * distance
    ang = torch.arange(views, device=dev, dtype=torch.float32) * (2 * math.pi / views)
    zero, one = torch.zeros_like(ang), torch.ones_like(ang)
    offset = torch.stack([torch.cos(ang), zero, torch.sin(ang)], -1)
    forward = -offset                                              # towards the centre
    down = torch.stack([zero, one, zero], -1)
    right = torch.linalg.cross(down, forward)
    ext = torch.zeros((views, 4, 4), device=dev)
    ext[:, :3, 0], ext[:, :3, 1], ext[:, :3, 2] = right, down, forward
    ext[:, :3, 3] = centre + radius * offset
    ext[:, 3, 3] = 1
    intr = torch.tensor([[FOCAL, 0, 0.5], [0, FOCAL, 0.5], [0, 0, 1.0]], device=dev).repeat(views, 1, 1)
    near = torch.full((views,), 0.05 * radius, device=dev)
    far = torch.full((views,), 4.0 * radius, device=dev)
    return ext, intr, near, far


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("ply")
    ap.add_argument("--out", required=True)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--distance", type=float, default=2.5, help="circle radius in scene extents")
    ap.add_argument("--opacity", choices=("logit", "raw"), default="logit")
    ap.add_argument("--background", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--antialiasing", action="store_true",
                    help="opacity compensation for the 0.3 screen-space low-pass (default: the classic mode)")
    ap.add_argument("--normals", default=None, metavar="OUT.npy",
                    help="also write the rendered normal map and the normals of the rendered depth, (2, V, 3, H, W)")
    ap.add_argument("--normal-alpha-min", type=float, default=0.5, help="(a default, not a measurement)")
    ap.add_argument("--distortion", default=None, metavar="OUT.npy", help="also write the depth distortion map, (V, H, W)")
    ap.add_argument("--dist-space", choices=("ndc", "linear", "disparity"), default="ndc")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("render_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.ply_import import load_ply
    from latentsplat_amd.rasterizer import (build_view_table, get_color_sh_convention, last_forward_status,
                                            rasterize_views, set_color_sh_convention)
    dev = torch.device("cuda:0")
    convention = get_color_sh_convention()
    set_color_sh_convention("3dgs")
    try:
        with torch.no_grad():
            s = load_ply(a.ply, dev, opacity=a.opacity)
            centre, extent = scene_extent(s.means)
            ext, intr, near, far = circle_cameras(centre, extent, a.views, a.distance)
            views = build_view_table(ext, intr, near, far, torch.tensor(a.background, device=dev))
            color, _, mask, depth, radii = rasterize_views(views, a.size, a.size, s.sh_degree, s.means, s.covariances,
                                                           s.opacities, shs=s.shs, antialiasing=a.antialiasing)
            status = last_forward_status()
            if a.normals:       # a second render with the normals as the payload (depth and mask are the first one's)
                from latentsplat_amd.normals import depth_to_normals, gaussian_normals
                payload = gaussian_normals(views, s.means, s.scales, s.rotations)
                normal_map = rasterize_views(views, a.size, a.size, s.sh_degree, s.means, s.covariances, s.opacities, shs=s.shs,
                                             features=payload, antialiasing=a.antialiasing)[1]
                covered = (mask > a.normal_alpha_min)[:, None]
                normal_map = torch.where(covered, normal_map / mask[:, None].clamp_min(1e-12), torch.zeros_like(normal_map))
                from_depth, _ = depth_to_normals(depth, mask, views, a.normal_alpha_min)
                both = torch.stack([normal_map, from_depth])
            if a.distortion:    # a render with the depth moments as the payload, and its own mask
                from latentsplat_amd.distortion import depth_pivot, distortion_map, gaussian_depth_moments, with_near_far
                dist_views = with_near_far(views, near, far)
                moments = gaussian_depth_moments(dist_views, s.means, a.dist_space, depth_pivot(dist_views, centre, a.dist_space))
                _, moment_map, dist_mask, _, _ = rasterize_views(views, a.size, a.size, s.sh_degree, s.means, s.covariances,
                                                                 s.opacities, shs=s.shs, features=moments,
                                                                 antialiasing=a.antialiasing)
                distortion = distortion_map(moment_map, dist_mask)
            depth = depth * near[:, None, None]        # (the table rescales the scene so that near == 1)
    finally:
        set_color_sh_convention(convention)
    os.makedirs(a.out, exist_ok=True)
    np.save(os.path.join(a.out, "color.npy"), color.cpu().numpy())
    np.save(os.path.join(a.out, "mask.npy"), mask.cpu().numpy())
    np.save(os.path.join(a.out, "depth.npy"), depth.cpu().numpy())
    if a.normals:
        np.save(a.normals, both.cpu().numpy())
    if a.distortion:
        np.save(a.distortion, distortion.cpu().numpy())
    status = dict(status, gaussians=int(s.means.shape[0]), sh_degree=int(s.sh_degree), views=a.views, size=a.size,
                  visible=[int(v) for v in (radii > 0).sum(dim=1).tolist()], centre=[float(c) for c in centre.tolist()],
                  extent=float(extent), antialiasing=bool(a.antialiasing))
    with open(os.path.join(a.out, "status.json"), "w") as f:
        json.dump(status, f, indent=1)
    print(json.dumps(status))
    return status


if __name__ == "__main__":
    main()
