"""Helpers shared by tests/test_depth_modes_{cpu,gpu}.py: the camera-space depth a view table implies, the per-Gaussian
depth payload from the public PyTorch helper, and a slot-aware CPU stand-in for ``rasterize_views``."""
from __future__ import annotations

import os

import numpy as np
import torch

from latentsplat_amd import rasterizer as R
from tests import util

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = ("depth", "disparity", "relative_disparity", "log")


def camera_depth(views, v, means):
    """(G,) camera-space depth of the UNSCALED scene in view v: the view-space z of the scaled means (row 2 of the
    table's view matrix, memory = transposed matrix) divided by the scene scale.  Any dtype, differentiable."""
    vw = views[v]
    p = means * vw[40]
    return (vw[2] * p[:, 0] + vw[6] * p[:, 1] + vw[10] * p[:, 2] + vw[14]) / vw[40]


def payload(views, v, means):
    """(G,) what the depth image of view v blends per Gaussian: ``depth_mode_payload`` at the table's mode / near / far."""
    vw = views[v]
    z = camera_depth(views, v, means)
    mode = int(vw[41])
    return z * vw[40] if mode == 0 else R.depth_mode_payload(z, vw[42], vw[43], mode)


def scene_slice(t, v, V, base):
    """Slice of view v of a shared (base dims), per-view or per-scene (leading dim dividing V) tensor."""
    return t if t.dim() == base else t[v * t.shape[0] // V]


CALLS: list = []   # one entry (the views table) per call of the stand-in


def slot_aware_oracle_rasterize_views(views, image_height, image_width, sh_degree, means3D, cov3D_precomp, opacities,
                                      shs=None, colors_precomp=None, features=None, means2D=None, debug=False,
                                      feature_sh=None, shs_channel_major=False):
    """``tests.util.oracle_rasterize_views`` for tables that carry a depth mode.  The oracle knows nothing of slots 41-43:
    one oracle render gives colour / feature / mask / radii (and the native depth); for the views with a mode a second
    render with ``colors_precomp = d`` (the public helper, one grey value per (view, Gaussian)) gives the depth image."""
    CALLS.append(views.detach().clone())
    kw = dict(shs=shs, colors_precomp=colors_precomp, features=features, feature_sh=feature_sh, shs_channel_major=shs_channel_major)
    color, feat, mask, depth, radii = util.oracle_rasterize_views(views, image_height, image_width, sh_degree, means3D,
                                                                  cov3D_precomp, opacities, **kw)
    vd = views.detach().cpu()
    if not bool((vd[:, 41] != 0).any()):
        return color, feat, mask, depth, radii
    V = vd.shape[0]
    m = means3D.detach().cpu()
    d = torch.stack([payload(vd, v, scene_slice(m, v, V, 2)) for v in range(V)])            # (V, G)
    per_view = lambda t, base: torch.stack([scene_slice(t.detach().cpu(), v, V, base) for v in range(V)])
    full = cov3D_precomp.shape[-2:] == (3, 3)
    black = vd.clone()
    black[:, 37:40] = 0.0                                                                    # no background term
    grey = util.oracle_rasterize_views(black, image_height, image_width, 0, per_view(m, 2),
                                       per_view(cov3D_precomp, 3 if full else 2), per_view(opacities, 2),
                                       colors_precomp=d[:, :, None].expand(-1, -1, 3).contiguous())[0]
    depth = depth.clone()
    moded = vd[:, 41] != 0
    depth[moded] = grey[moded].mean(dim=1)
    return color, feat, mask, depth, radii


def load_fixture():
    return np.load(os.path.join(GOLD, "depth_modes.npz"))
