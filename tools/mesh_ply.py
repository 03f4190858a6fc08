#!/usr/bin/env python
"""Extract a triangle mesh from a trained 3DGS scene file: the recipe of INTEGRATION.md §24, as a tool.

  1. `GaussianScene.from_ply(path, device)`: the scene with its raw parameters;
  2. the cameras of tools/render_ply.py: on a circle around the median of the means, in the x-z plane, looking at it;
  3. `scene.extract_mesh`: the views are rendered in batches (colour, depth of depth mode NATIVE, mask), fused into a
     truncated signed distance volume in one pass over the volume per batch, and the zero level set is extracted by marching
     tetrahedra on the Kuhn subdivision, all in HIP;
  4. `--out mesh.ply`: a binary little-endian triangle mesh with per-vertex colour (`save_mesh_ply`), and one JSON line with
     its size.

`--voxel-size` is in scene units (default: 1/128 of the scene's extent); `--trunc` defaults to 4 voxel sizes (a default,
not a measurement).  `--filter-3d` renders with the 3D smoothing filter of the same cameras and
`--antialiasing` with the rasterizer's opacity compensation, as a scene trained with them expects.
`--keep-largest K` keeps the K connected components with the most faces and `--min-faces F` those of at least F faces
(`clean_mesh`, INTEGRATION.md §25: the floaters every TSDF of rendered depth contains); both are off by default and the
output is unchanged without them.
A scene trained with `tools/fit_ply.py --normal-reg` has the depth this step needs.

usage: python tools/mesh_ply.py scene.ply --out mesh.ply [--views 32] [--size 512] [--voxel-size v] [--trunc t] [--distance 2.5]
                                [--filter-3d] [--antialiasing] [--keep-largest K] [--min-faces F]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from render_ply import circle_cameras, scene_extent  # noqa: E402


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("ply")
    ap.add_argument("--out", required=True)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--voxel-size", type=float, default=None, help="scene units (default: extent / 128)")
    ap.add_argument("--trunc", type=float, default=None, help="scene units (default: 4 voxel sizes; a default, not a measurement)")
    ap.add_argument("--distance", type=float, default=2.5, help="circle radius in scene extents")
    ap.add_argument("--filter-3d", action="store_true", help="render with the 3D smoothing filter of these cameras")
    ap.add_argument("--antialiasing", action="store_true", help="opacity compensation for the 0.3 screen-space low-pass")
    ap.add_argument("--keep-largest", type=int, default=None, help="keep the K connected components with the most faces")
    ap.add_argument("--min-faces", type=int, default=None, help="keep the connected components of at least F faces")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("mesh_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.mesh import clean_mesh, save_mesh_ply
    from latentsplat_amd.rasterizer import build_view_table, get_color_sh_convention, set_color_sh_convention
    dev = torch.device("cuda:0")
    convention = get_color_sh_convention()
    set_color_sh_convention("3dgs")
    try:
        with torch.no_grad():
            scene = GaussianScene.from_ply(a.ply, dev)
            centre, extent = scene_extent(scene._xyz)
            ext, intr, near, far = circle_cameras(centre, extent, a.views, a.distance)
            views = build_view_table(ext, intr, near, far, torch.zeros(3, device=dev))
            voxel = a.voxel_size if a.voxel_size is not None else float(extent) / 128
            kw = dict(antialiasing=True) if a.antialiasing else {}
            if a.filter_3d:
                kw["filter_3d"] = scene.compute_filter_3d(views, a.size)
            vertices, faces, colors = scene.extract_mesh(views, a.size, a.size, voxel, trunc=a.trunc, **kw)
            cleanup = None
            if a.keep_largest is not None or a.min_faces is not None:
                vertices, faces, colors, cleanup = clean_mesh(vertices, faces, colors, keep_largest=a.keep_largest, min_faces=a.min_faces)
    finally:
        set_color_sh_convention(convention)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    save_mesh_ply(a.out, vertices, faces, colors)
    status = dict(gaussians=scene.num_gaussians, views=a.views, size=a.size, voxel_size=voxel, vertices=int(vertices.shape[0]),
                  faces=int(faces.shape[0]), filter_3d=bool(a.filter_3d), antialiasing=bool(a.antialiasing), out=a.out)
    if cleanup is not None:
        status["cleanup"] = dict(keep_largest=a.keep_largest, min_faces=a.min_faces, **cleanup)
    print(json.dumps(status))
    return status


if __name__ == "__main__":
    main()
