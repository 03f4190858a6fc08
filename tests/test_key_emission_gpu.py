"""The key emission, histogram flush / segment reservation and folded tile scan that k_preprocess and the fused projection +
SH kernel k_preprocess_sh share (csrc/lsr_key_emit.h), bit for bit against the two-phase binning (LSR_SEGMENTS = 0: the
projection kernel only counts, k_scatter writes the keys), which runs none of the emission code.  Compared per run: pair
count, longest list, tile offsets, canonical lists, half-list lengths, the half lists inside their counted prefixes,
n_contrib, radii and every image."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


class _Run(util.HipRun):
    """util.HipRun for inputs SHARED by the views of a scene (or by each of b view groups): what lets k_preprocess take
    several views per workgroup and what the fused kernel needs.  Payload: colour harmonics (G,3,K) channel-major and / or
    latent features, either harmonics (G,C,Kf) or direct (G,C)."""

    def __init__(self, scenes, H, W, dev, direct, forward_flags=0):
        from latentsplat_amd import _lib
        from latentsplat_amd.decoder import cuda_splatting as cs
        from latentsplat_amd.rasterizer import make_view_table
        b, v, G = len(scenes), scenes[0].extrinsics.shape[0], scenes[0].means.shape[0]
        tables = []
        for sc in scenes:
            cams, scale = cs._scaled_cameras(sc.extrinsics, sc.intrinsics, sc.near * torch.linspace(1.0, 1.2, v), sc.far, True)
            tables.append(make_view_table(cams.view_matrix, cams.full_projection, cams.campos, cams.tan_fov_x, cams.tan_fov_y,
                                          torch.tensor([[0.3, 0.2, 0.1]]).expand(v, 3), scale))
        self.views = torch.cat(tables).to(dev).contiguous()
        stack = lambda name: None if getattr(scenes[0], name) is None else torch.stack([getattr(s, name) for s in scenes]).to(dev).contiguous()
        self.means, self.cov6, self.opac, self.color, self.features = (stack(n) for n in ("means", "covariances", "opacities", "color_sh", "feature_sh"))
        Cf, Kf = self.features.shape[-2:]
        if direct:
            assert Kf == 1
            self.features = self.features[..., 0].contiguous()
        K = 0 if self.color is None else self.color.shape[-1]
        per = (lambda n: n * G) if b > 1 else (lambda n: 0)        # elements per scene slice; 0 = one shared scene
        d = _lib.Dims(b * v, G, H, W, Cf, _lib.COLOR_SH if K else _lib.COLOR_NONE, int(round(K ** 0.5)) - 1 if K else 0, K,
                      per(3), per(9), per(1), per(3 * K), per(Cf * Kf), 9, _lib.FEAT_DIRECT if direct else _lib.FEAT_SH,
                      0 if direct else int(round(Kf ** 0.5)) - 1, 0 if direct else Kf, 1 if K else 0, v if b > 1 else 0,
                      _lib.SH_AXES_3DGS, forward_flags, 0)
        self._forward(d, dev)

    def snapshot(self):
        return dict(P=self.P, maxtile=self.maxtile, ts=self.tile_start(), pl=self.point_list(), hc=self.half_count(), hl=self.half_list(),
                    img=[None if t is None else t.clone() for t in (self.color_out, self.feat_out, self.mask_out, self.depth_out)],
                    nc=self.n_contrib(), radii=self.radii.clone())


def _assert_same(a, b, name):
    assert (a["P"], a["maxtile"]) == (b["P"], b["maxtile"]), name + ": pair count / longest list"
    np.testing.assert_array_equal(a["ts"], b["ts"], err_msg=name + ": tile offsets")
    np.testing.assert_array_equal(a["pl"], b["pl"], err_msg=name + ": canonical lists")
    np.testing.assert_array_equal(a["hc"], b["hc"], err_msg=name + ": half-list lengths")
    for vt in range(a["hc"].shape[0]):       # (the half-list area is only defined inside the counted prefixes)
        s0, n = a["ts"][vt], a["ts"][vt + 1] - a["ts"][vt]
        for h in range(2):
            sl = slice(2 * s0 + h * n, 2 * s0 + h * n + a["hc"][vt, h])
            np.testing.assert_array_equal(a["hl"][sl], b["hl"][sl], err_msg=f"{name}: half list {h} of (view, tile) {vt}")
    np.testing.assert_array_equal(a["nc"], b["nc"], err_msg=name + ": n_contrib")
    assert torch.equal(a["radii"], b["radii"]), name + ": radii"
    for x, y in zip(a["img"], b["img"]):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), name + ": images"


def _launches(run):
    """run() with the stage profile on: {stage: launches}."""
    from latentsplat_amd import _lib
    _lib.profile_read()
    _lib.profile_enable(True)
    try:
        out = run()
        prof = {k: n for k, (ms, n) in _lib.profile_read().items()}
    finally:
        _lib.profile_enable(False)
    return out, prof


def _segments_equal_two_phase(make_run, fused, overflow_leg=True):
    """Two-phase, single-pass and (overflow_leg) single-pass with a capacity at the median non-empty list length — some tiles
    then overflow into the fallback scatter, some do not.  Returns the two-phase snapshot."""
    from latentsplat_amd import _lib
    try:
        _lib.set_knob("LSR_SEGMENTS", 0)
        _lib.set_knob("LSR_SEG_CAP", 0)
        r, prof = _launches(make_run)
        a = r.snapshot()
        assert prof["scatter"] == 1 and (not fused or prof["sh_forward"] == 0), prof
        lens = np.diff(a["ts"])
        small = int(-(-int(np.median(lens[lens > 0])) // 64) * 64)
        for name, cap in (("segments", 0),) + ((("overflow_fallback", small),) if overflow_leg else ()):
            _lib.set_knob("LSR_SEGMENTS", 1)
            _lib.set_knob("LSR_SEG_CAP", cap)
            r, prof = _launches(make_run)
            # the single-pass path was taken: no scatter unless a segment overflowed; the fused kernel: no separate SH pass
            assert prof["scatter"] == (1 if cap else 0), (name, prof)
            assert not fused or prof["sh_forward"] == 0, (name, prof)
            _assert_same(a, r.snapshot(), name)
        if overflow_leg:
            assert (lens > small).any() and ((lens > 0) & (lens <= small)).any(), "the fallback leg needs overfull AND fitting tiles"
        if fused:      # and the fused kernel computes what k_preprocess + k_sh_fwd compute
            _lib.set_knob("LSR_FUSE_SH", 0)
            r, prof = _launches(make_run)
            assert prof["sh_forward"] == 1, prof
            _assert_same(a, r.snapshot(), "two-kernel path")
        return a
    finally:
        _lib.set_knob("LSR_FUSE_SH", 1)
        _lib.set_knob("LSR_SEGMENTS", 1)
        _lib.set_knob("LSR_SEG_CAP", 0)


@pytest.mark.parametrize("b,v", [(1, 6), (2, 3)])
def test_fused_kernel_lists_equal_two_phase(hip_device, b, v):
    """k_preprocess_sh's emission, compared through its lists (the existing fused-kernel test compares images only).
    G = 1100: 17 full 64-Gaussian chunks and a 12-row tail, no multiple of a 512-Gaussian workgroup; 40 x 72: 15 tiles with
    ragged edges; six views of a shared scene: a wave takes two views; two groups of three: the segment index carries the
    group's first view, a term only the fused kernel has."""
    from latentsplat_amd import _lib
    scenes = [util.make_scene(1100, image_size=72, views=v, seed=70 + s, color_sh_degree=2, feature_channels=4,
                              feature_sh_degree=1, sigma_px=(0.5, 8.0)) for s in range(b)]
    _segments_equal_two_phase(lambda: _Run(scenes, 40, 72, hip_device, direct=False, forward_flags=_lib.FWD_REACHED_ONLY), fused=True)


# Slots of the emission's LDS bucket array: 12 bytes each in at most 16 640 bytes — k_preprocess' record staging array
# (4 x 260 float4) and, for payloads whose coefficient rows are smaller than that (here: 27 + 16 floats per Gaussian), the
# 16 384 bytes the fused kernel's launcher pads its coefficient area to.  16 640 / 12 = 1386 (less the tile deltas in front).
_MOST_BUCKET_SLOTS = 1386


@pytest.mark.parametrize("direct", [True, False])
def test_more_pairs_than_bucket_slots_take_the_direct_store(hip_device, direct):
    """A workgroup with more pairs in one view than its bucket array holds stores the surplus keys straight into the
    segments (both kernels).  Few, very wide, opaque splats with the published pairs: nearly every Gaussian covers all 36
    tiles of both views.  An aligned block of 64 consecutive Gaussians always lies inside one workgroup of either kernel."""
    G, S, V = 256, 96, 2
    cfg = dict(color_sh_degree=None, feature_sh_degree=0) if direct else dict(color_sh_degree=2, feature_sh_degree=1)
    scenes = [util.make_scene(G, image_size=S, views=V, seed=91, feature_channels=4, sigma_px=(60.0, 90.0), opacity_scale=1.0, **cfg)]
    a = _segments_equal_two_phase(lambda: _Run(scenes, S, S, hip_device, direct=direct), fused=not direct, overflow_leg=False)
    T = (S // 16) ** 2
    most = max(int(np.bincount(a["pl"][a["ts"][v * T]:a["ts"][(v + 1) * T]] // 64).max()) for v in range(V))
    assert most > _MOST_BUCKET_SLOTS, f"the fullest (64-Gaussian block, view) has {most} pairs: the direct store was not reached"


def test_reserve_pass_skips_views_beyond_the_last(hip_device):
    """Five views of a shared scene with direct features: k_preprocess runs four views per workgroup, so its second
    workgroup row holds one view and three beyond num_views, whose counters (they would be the NEXT words of the workspace)
    must not be touched: the tile offsets of all V * T entries are compared."""
    from latentsplat_amd import _lib
    scenes = [util.make_scene(700, image_size=48, views=5, seed=33, color_sh_degree=None, feature_channels=4, feature_sh_degree=0,
                              sigma_px=(0.5, 8.0))]
    a = _segments_equal_two_phase(lambda: _Run(scenes, 48, 48, hip_device, direct=True, forward_flags=_lib.FWD_REACHED_ONLY), fused=False)
    assert a["ts"].shape[0] == 5 * 9 + 1 and (np.diff(a["ts"])[4 * 9:] > 0).any(), "the fifth view must have lists"
