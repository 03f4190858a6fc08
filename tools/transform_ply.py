#!/usr/bin/env python
"""Move a 3DGS scene file: rotate, rescale, translate, centre, normalise, merge.

  1. `GaussianScene.from_ply(in.ply)`: the raw parameters, bit for bit;
  2. the similarity `M = T . S . R` from `--translate`, `--scale` and `--axis-angle` (or `--matrix`, 16 numbers row-major,
     which must be a similarity: rotation, uniform scale, translation); `--center` then moves the median of the moved
     means to the origin and `--unit-extent` rescales about the origin so that `render_ply.scene_extent` of the result is
     1; `--inverse` applies the inverse of all that instead;
  3. `transform_(M)`: one HIP launch over positions, log-scales, quaternions and every SH band of the view-dependent colour
     (a tool that leaves `f_rest` alone keeps the highlights glued to the old axes); opacities and `f_dc` stay;
  4. `--merge other.ply` (may repeat): the other files' Gaussians are appended as they are (the transform applies to the
     first file only; `f_rest` is zero-padded to the highest degree among the files);
  5. `save_ply(out.ply)` and one JSON line: the matrix applied (row-major, float64) and the row count.

usage: python tools/transform_ply.py in.ply out.ply [--axis-angle x y z deg] [--scale s] [--translate x y z] [--matrix 16 numbers]
                                                    [--center] [--unit-extent] [--inverse] [--merge other.ply ...]"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("ply")
    ap.add_argument("out")
    ap.add_argument("--matrix", type=float, nargs=16, default=None, help="a similarity, 16 numbers row-major")
    ap.add_argument("--axis-angle", type=float, nargs=4, default=None, metavar=("X", "Y", "Z", "DEG"))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--translate", type=float, nargs=3, default=None)
    ap.add_argument("--center", action="store_true", help="move the median of the means to the origin")
    ap.add_argument("--unit-extent", action="store_true", help="rescale so that the scene's extent is 1")
    ap.add_argument("--inverse", action="store_true", help="apply the inverse")
    ap.add_argument("--merge", action="append", default=[], metavar="OTHER.ply")
    a = ap.parse_args(argv)
    if a.matrix is not None and (a.axis_angle is not None or a.translate is not None or a.scale != 1.0):
        sys.exit("transform_ply: --matrix excludes --axis-angle, --scale and --translate")
    if not a.scale > 0:
        sys.exit("transform_ply: --scale must be positive")
    if not torch.cuda.is_available():
        sys.exit("transform_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.scene_model import GaussianScene
    from latentsplat_amd.transform import check_similarity, invert_similarity, similarity_matrix
    from render_ply import scene_extent
    dev = torch.device("cuda:0")
    if a.matrix is not None:
        M = torch.tensor(a.matrix, dtype=torch.float64).reshape(4, 4)
    else:
        rotation = None
        if a.axis_angle is not None:
            axis = torch.tensor(a.axis_angle[:3], dtype=torch.float64)
            if not float(axis.norm()) > 0:
                sys.exit("transform_ply: --axis-angle needs a non-zero axis")
            half = math.radians(a.axis_angle[3]) / 2
            rotation = torch.cat([torch.tensor([math.cos(half)], dtype=torch.float64), math.sin(half) * axis / axis.norm()])
        M = similarity_matrix(rotation, a.translate, a.scale)
    check_similarity(M[None])
    scene = GaussianScene.from_ply(a.ply, dev)
    with torch.no_grad():
        if a.center or a.unit_extent:
            moved = scene._xyz.double() @ M[:3, :3].to(dev).T + M[:3, 3].to(dev)
            centre, extent = scene_extent(moved)
            if a.center:
                M = similarity_matrix(None, -centre.cpu()) @ M
            if a.unit_extent:
                M = similarity_matrix(None, None, 1.0 / float(extent)) @ M
        if a.inverse:
            M = invert_similarity(M)
        scene.transform_(M)
        if a.merge:
            scene = GaussianScene.merge([scene] + [GaussianScene.from_ply(path, dev) for path in a.merge])
        scene.save_ply(a.out)
    result = dict(matrix=[float(v) for v in M.reshape(-1).tolist()], gaussians=int(scene.num_gaussians))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
