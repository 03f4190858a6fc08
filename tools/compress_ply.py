#!/usr/bin/env python
"""Compress a 3DGS scene file with codebooks: `GaussianScene.from_ply`, `quantize_scene`, `QuantizedScene.save`
(INTEGRATION.md §19).

The view-dependent colour rows (f_rest) and the shape rows (scale + rotation) become 16-bit indices into two codebooks
found by weighted k-means in HIP; positions, f_dc and opacities are stored as they are.  The output is one
numpy.savez_compressed file that `QuantizedScene.load` reads back bit for bit.

  --rest-codes / --shape-codes   codebook sizes (default 4096 each, at most 65536, never more than the scene has rows)
  --iters                        Lloyd iterations (default 10)
  --seed                         the initial codes are rows drawn with this seed (default 0): the same seed, the same file
  --decode out.ply               also write the dequantised scene as a standard 3DGS file

usage: python tools/compress_ply.py in.ply out.npz [--rest-codes K] [--shape-codes K] [--iters N] [--seed S] [--decode out.ply]"""
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
    ap.add_argument("--rest-codes", type=int, default=4096)
    ap.add_argument("--shape-codes", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--decode", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("compress_ply needs an MI355X: no ROCm device is visible (there is no CPU fallback)")
    from latentsplat_amd import GaussianScene, quantize_scene
    scene = GaussianScene.from_ply(a.src, torch.device("cuda:0"))
    n = scene.num_gaussians
    q = quantize_scene(scene, rest_codes=max(1, min(a.rest_codes, n)), shape_codes=max(1, min(a.shape_codes, n)), iters=a.iters,
                       generator=torch.Generator().manual_seed(a.seed))
    q.save(a.dst)
    if a.decode:
        q.dequantize().save_ply(a.decode)
    size_in, size_out = os.path.getsize(a.src), os.path.getsize(a.dst)
    status = dict(gaussians=n, sh_degree=scene.max_sh_degree, bytes_in=size_in, bytes_out=size_out, bytes_before_deflate=q.nbytes,
                  ratio=size_in / size_out, rest_codes=0 if q.rest_codebook is None else int(q.rest_codebook.shape[0]),
                  shape_codes=int(q.shape_codebook.shape[0]))
    print(f"{a.src}: {size_in} bytes -> {a.dst}: {size_out} bytes, {status['ratio']:.2f} x smaller ({n} Gaussians, degree {scene.max_sh_degree})")
    return status


if __name__ == "__main__":
    main()
