#!/usr/bin/env python
"""Generate tests/golden/depth_modes.npz: the reference wrapper's depth modes, by IMPORTING the reference's own Python
(this container only, like make_golden.py, whose stubs and scene builder this script uses).

For one seeded batch (b = 2 scenes x v = 2 views, G = 400, 48 x 48) and the oracle-served ``diff_gaussian_rasterization``:
  * ``render_depth_cuda`` through the reference's ``DecoderSplattingCUDA.render_depth`` for all four
    ``DepthRenderingMode``s: the fake colour every call handed to the rasterizer (the per-Gaussian value the mode
    computes, ``shs[:, 0, 0]``) and the returned depth images;
  * ``DecoderSplattingCUDA.forward(depth_mode=m)`` for m = "relative_disparity" and "log": the whole DecoderOutput
    (colour, mask and posterior once: asserted here to be the same for both modes; the depth images are asserted to be
    those of ``render_depth`` above and not stored again).
Arrays only; nothing from the reference is copied."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

MODES = ("depth", "disparity", "relative_disparity", "log")
SCENE = dict(G=400, image_size=48, views=2, color_sh_degree=1, feature_channels=4, feature_sh_degree=0)
FAKE: list = []


def _recording_oracle_module():
    """The oracle rasterizer, noting the degree-0 colour coefficient of every call it serves."""
    m = types.ModuleType("diff_gaussian_rasterization")
    m.GaussianRasterizationSettings = mg.orc.GaussianRasterizationSettings

    def make(raster_settings):
        inner = mg.orc.GaussianRasterizer(raster_settings)

        class _Rec(torch.nn.Module):
            def forward(self, **kw):
                FAKE.append(None if kw.get("shs") is None else kw["shs"].detach().clone())
                return inner(**kw)

        return _Rec()

    m.GaussianRasterizer = make
    return m


def main():
    batch = mg._scene_batch(SCENE)
    bg = [0.1, 0.3, 0.7]
    mg._install_stubs(_recording_oracle_module())
    dec, cs, tm = mg._import_reference()
    decoder = dec.DecoderSplattingCUDA(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), bg, False)
    gauss = tm.Gaussians(batch["means"], batch["covariances"], batch["opacities"],
                         batch["color_harmonics"], batch["feature_harmonics"])
    cams = (batch["extrinsics"], batch["intrinsics"], batch["near"], batch["far"], batch["image_shape"])
    b, v = batch["extrinsics"].shape[:2]
    rec = {f"in_{k}": mg._np(t) for k, t in batch.items() if torch.is_tensor(t)}
    rec["in_image_shape"] = np.array(batch["image_shape"], np.int32)
    rec["in_bg"] = np.array(bg, np.float32)
    for mode in MODES:
        FAKE.clear()
        depth = decoder.render_depth(gauss, *cams, mode)
        assert len(FAKE) == b * v and all(f.shape[1:] == (1, 3) for f in FAKE)
        fake = torch.stack(FAKE)                                  # (b v, G, 1, 3): one grey coefficient per Gaussian
        assert torch.equal(fake[..., 0], fake[..., 1]) and torch.equal(fake[..., 0], fake[..., 2])
        rec[f"fake_{mode}"] = mg._np(fake[:, :, 0, 0])            # (b v, G)
        rec[f"depth_{mode}"] = mg._np(depth)                      # (b, v, h, w)
    outs = {}
    for mode in ("relative_disparity", "log"):
        FAKE.clear()
        out = decoder.forward(gauss, *cams, depth_mode=mode)
        assert len(FAKE) == 2 * b * v                             # the payload render and the depth render, per view
        outs[mode] = out
        np.testing.assert_array_equal(mg._np(out.depth), rec[f"depth_{mode}"])     # (stored once: depth_<mode>)
    a, c = outs["relative_disparity"], outs["log"]
    for x, y in ((a.color, c.color), (a.mask, c.mask), (a.feature_posterior.mean, c.feature_posterior.mean),
                 (a.feature_posterior.logvar, c.feature_posterior.logvar)):
        assert torch.equal(x, y)
    rec.update(decoder_color=mg._np(a.color), decoder_mask=mg._np(a.mask),
               decoder_posterior_mean=mg._np(a.feature_posterior.mean),
               decoder_posterior_logvar=mg._np(a.feature_posterior.logvar))
    path = os.path.join(mg.ROOT, "tests", "golden", "depth_modes.npz")
    np.savez_compressed(path, **rec)
    print("depth_modes.npz", os.path.getsize(path), "bytes;", {k: val.shape for k, val in rec.items()})


if __name__ == "__main__":
    if not os.path.isdir(mg.REF):
        raise SystemExit("the reference is only available in the build container")
    sys.path.insert(0, mg.REF)
    main()
