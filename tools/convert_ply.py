#!/usr/bin/env python
"""Load a 3DGS scene file and save it again: `load_ply` then `save_ply`.

What that is good for:
  --max-degree D            keep SH bands 0..D only (viewers commonly stop at degree 3; a degree-4 scene becomes readable)
  --from-convention reference   the file's colour SH are in the "reference" axis convention (coefficients taken from this
                            pipeline as they are): re-base them to the "3dgs" basis the format means
  --opacity raw             the input stores opacities as they are (files of `export_ply`); the output stores logits

Positions and (without --from-convention) the kept SH coefficients are copied bit for bit; scales and rotations go through
exp / normalise on the way in and log on the way out (2e-5 relative).  The output's quaternions have w >= 0.

usage: python tools/convert_ply.py in.ply out.ply [--max-degree D] [--from-convention reference] [--opacity raw]"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--max-degree", type=int, default=None)
    ap.add_argument("--from-convention", choices=("3dgs", "reference"), default="3dgs")
    ap.add_argument("--opacity", choices=("logit", "raw"), default="logit")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("convert_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd.ply_export import save_ply
    from latentsplat_amd.ply_import import load_ply
    s = load_ply(a.src, torch.device("cuda:0"), opacity=a.opacity)
    save_ply(a.dst, s.means, s.opacities, s.shs, scales=s.scales, rotations=s.rotations, convention=a.from_convention,
             channel_major=False, max_sh_degree=a.max_degree)
    degree = s.sh_degree if a.max_degree is None else min(s.sh_degree, a.max_degree)
    status = dict(gaussians=int(s.means.shape[0]), sh_degree_in=s.sh_degree, sh_degree_out=degree, bytes=os.path.getsize(a.dst))
    print(status)
    return status


if __name__ == "__main__":
    main()
