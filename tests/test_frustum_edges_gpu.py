"""GPU parity at the frustum edges (tests/util.py make_edge_scene): the HIP path against the CPU oracle where the
projection is discontinuous — the EWA Jacobian clamp at |t.x / t.z| = 1.3 tanfov, down to single ulps on both sides,
the near cull t.z <= 0.2, means outside the cone with footprints reaching the image, rectangles that reach one edge tile,
and wide-baseline targets.  Same checks and bars as tests/test_parity_gpu.py; decisions (radii, rectangles, the clamp)
bit for bit, float sums at the usual tolerances."""
import numpy as np
import pytest

from tests import test_parity_gpu as tp
from tests import util

pytestmark = pytest.mark.gpu

# payload widths that select the compositing kernels' 4-, 8-, 12- and 36-float record instances
PAYLOADS = {4: dict(color_sh_degree=None, feature_channels=4), 8: dict(color_sh_degree=1, feature_channels=4),
            12: dict(color_sh_degree=2, feature_channels=8, feature_sh_degree=1), 36: dict(color_sh_degree=0, feature_channels=32)}
FWD_CASES = [("band", 8, 64, 64), ("band", 36, 48, 80), ("outside", 4, 64, 64), ("outside", 12, 50, 70), ("near", 12, 64, 64),
             ("near", 4, 33, 47), ("border", 8, 48, 64), ("border", 36, 64, 64), ("wide", 8, 64, 64), ("wide_encoder", 12, 64, 64)]


def _edge_scene(pop, width, H, W, views=3, seed=1):
    return util.make_edge_scene(pop, H=H, W=W, views=views, seed=seed, **PAYLOADS[width])


@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("pop,width,H,W", FWD_CASES)
def test_forward_parity_at_frustum_edges(hip_device, pop, width, H, W, contracted):
    from latentsplat_amd import _lib
    from oracle import oracle as orc
    lib = _lib.load()
    sc, lab = _edge_scene(pop, width, H, W)
    bi = util.boundary_inputs(sc, H, W, bg=(0.2, 0.4, 0.6))
    try:
        lib.lsr_set_projection_contraction(int(contracted))
        orc.set_fma_contraction(contracted)
        run = util.HipRun(bi, hip_device)
        tp._check_forward(bi, run)   # radii (the cull band among them), rectangles, depth bits, conics, lists: bit exact
    finally:
        lib.lsr_set_projection_contraction(0)
        orc.set_fma_contraction(False)
    if not contracted:   # the replica's cull is the kernel's
        assert not (run.radii.cpu().numpy()[lab["culled"]] > 0).any()


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("pop,width", [("band", 8), ("near", 4), ("outside", 12), ("wide", 36)])
def test_fused_scene_inputs_at_frustum_edges(hip_device, pop, width, shared):
    """The scene-level path (in-kernel scene scale, 3x3 covariances, stored-layout colour SH, latent SH; shared inputs run
    the fused projection + SH kernel k_preprocess_sh): images, radii and every input gradient.  Scene scale 1 in every
    view, so that the band Gaussians keep their exact ratios."""
    cfg = dict(PAYLOADS[width])
    cfg["feature_sh_degree"] = 1 if cfg["feature_channels"] * 4 <= 120 else 0
    sc, _ = util.make_edge_scene(pop, H=64, W=64, views=3, seed=3, **cfg)
    tp._fused_scene_check(hip_device, sc, 64, shared, near_spread=(1.0, 1.0))


BAND_ROW_TOL = {"means": 2e-4, "cov": 2e-3}   # the per-row bars of tests/test_headline_gpu.py


@pytest.mark.parametrize("contracted", [False, True])
def test_backward_parity_clamp_band(hip_device, contracted):
    """dL/dmeans3D switches a whole term on the clamp decision: the band rows (ratio = limit + k ulps, k = -4..4, both
    signs, both axes, an identity and a turned view) are held to the suite's bars and, each on its own, to a per-row bar.
    Three views: the band Gaussians of one view are clamped or not in the others independently, so the per-view rows and
    the opacity / SH rows summed over views mix both decisions."""
    from latentsplat_amd import _lib
    from oracle import oracle as orc
    lib = _lib.load()
    sc, lab = _edge_scene("band", 8, 64, 64, views=3, seed=4)
    vis = ~lab["culled"]
    cl = lab["clamped"].any(-1)
    assert ((cl[0] & vis[0]) & (~cl[1] & vis[1])).any() or ((cl[1] & vis[1]) & (~cl[0] & vis[0])).any()
    band = lab["kind"] == 1
    rows = {v: (np.flatnonzero(band & (lab["band_view"] == v)), BAND_ROW_TOL) for v in (0, 1)}
    try:
        lib.lsr_set_projection_contraction(int(contracted))
        orc.set_fma_contraction(contracted)
        tp._grad_scene(hip_device, sc, 64, 64, True, row_checks=rows)
    finally:
        lib.lsr_set_projection_contraction(0)
        orc.set_fma_contraction(False)


@pytest.mark.parametrize("pop,width,H,W", [("outside", 8, 64, 64), ("near", 4, 64, 64), ("near", 12, 40, 56),
                                           ("border", 4, 48, 64), ("wide", 8, 64, 64), ("wide_encoder", 4, 40, 40)])
def test_backward_parity_at_frustum_edges(hip_device, pop, width, H, W):
    sc, lab = _edge_scene(pop, width, H, W, views=2, seed=6)
    rows = None
    if pop == "near":   # the Gaussians at the cull band, each on its own
        rows = {0: (np.flatnonzero(lab["kind"] == 3), BAND_ROW_TOL)}
    tp._grad_scene(hip_device, sc, H, W, True, row_checks=rows)
