#!/usr/bin/env python
"""Score an extracted mesh against a ground-truth cloud or mesh: the recipe of INTEGRATION.md §25, as a tool.

  1. `load_mesh_ply(MESH.ply)`: the mesh `tools/mesh_ply.py` (or `save_mesh_ply`) wrote;
  2. with `--keep-largest K` / `--min-faces F`: `clean_mesh` first (connected components in HIP; the published
     `post_process_mesh`);
  3. `sample_mesh`: `--samples` points uniform by area (seeded: `--seed`);
  4. the ground truth `--gt`: a points file (`load_points_ply`) taken as it is, or a mesh file (`load_mesh_ply`), sampled
     the same way with seed + 1;
  5. `cloud_metrics`: accuracy, completeness, Chamfer (DTU), precision / recall / F-score at every `--thresholds` value
     (Tanks and Temples); `--max-dist` clips the distances before the means (DTU's 20 mm rule).  The nearest-neighbour
     queries are HIP and exact;
  6. `--out metrics.json`: the metrics and the counts; the same dict is printed as one JSON line and returned.

Dataset plumbing (DTU's observation masks, the alignment files of Tanks and Temples) is not here: both inputs are taken in
one frame.

usage: python tools/eval_mesh.py MESH.ply --gt GT.ply [--samples 1000000] [--thresholds t ...] [--max-dist D]
                                 [--keep-largest K] [--min-faces F] [--seed S] --out metrics.json"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _has_faces(path) -> bool:
    with open(path, "rb") as f:
        head = f.read(4096)
    end = head.find(b"end_header")
    return any(line.split()[:2] == [b"element", b"face"] for line in head[:end if end >= 0 else len(head)].split(b"\n"))


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh")
    ap.add_argument("--gt", required=True, help="a points .ply, or a mesh .ply (sampled)")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[])
    ap.add_argument("--max-dist", type=float, default=None)
    ap.add_argument("--keep-largest", type=int, default=None)
    ap.add_argument("--min-faces", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("eval_mesh needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import clean_mesh, cloud_metrics, load_mesh_ply, load_points_ply, sample_mesh
    dev = torch.device("cuda:0")
    vertices, faces, _ = load_mesh_ply(a.mesh)
    vertices, faces = torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev)
    out = dict(mesh=a.mesh, gt=a.gt, samples=a.samples, seed=a.seed, vertices_in=int(vertices.shape[0]), faces_in=int(faces.shape[0]))
    if a.keep_largest is not None or a.min_faces is not None:
        vertices, faces, _, info = clean_mesh(vertices, faces, None, keep_largest=a.keep_largest, min_faces=a.min_faces)
        out["cleanup"] = dict(keep_largest=a.keep_largest, min_faces=a.min_faces, **info)
    out["vertices"], out["faces"] = int(vertices.shape[0]), int(faces.shape[0])
    pred, _ = sample_mesh(vertices, faces, a.samples, torch.Generator().manual_seed(a.seed))
    if _has_faces(a.gt):
        gv, gf, _ = load_mesh_ply(a.gt)
        gt, _ = sample_mesh(torch.from_numpy(gv).to(dev), torch.from_numpy(gf).to(dev), a.samples, torch.Generator().manual_seed(a.seed + 1))
        out["gt_kind"] = "mesh"
    else:
        gt, _ = load_points_ply(a.gt, dev)
        out["gt_kind"] = "points"
    out.update(cloud_metrics(pred, gt, thresholds=a.thresholds, max_dist=a.max_dist))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
