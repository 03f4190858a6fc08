"""The frustum-edge scenes (tests/util.py make_edge_scene) and the oracles on them, without a GPU.

The projection has two geometric discontinuities: the clamp of the EWA Jacobian at |t.x / t.z| = 1.3 tanfov and the near
cull t.z <= 0.2.  These tests check that the builder places Gaussians on both sides of both, that the two oracles agree
there (the C backward against autograd through the torch oracle: an independent check of the clamped-Jacobian rule, which
treats the clamped t.x as a constant — finite differences would not), and that a backward deciding the clamp differently
from the forward moves gradient rows by far more than the GPU tests' bar."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from oracle import torch_oracle as to
from tests import util

GPU_BAR = 1e-4   # tests/test_parity_gpu.py ABS_TOL: gradient rows within 1e-4 of the tensor's scale


def _torch_f32_ratio(bi, v):
    """The forward's t and ratio once more, through torch float32 elementwise operations (not the builder's numpy)."""
    vm = bi["cams"].view_matrix[v].contiguous().reshape(16)
    p = bi["means"][v]
    t = torch.stack([((vm[k] * p[:, 0] + vm[4 + k] * p[:, 1]) + vm[8 + k] * p[:, 2]) + vm[12 + k] for k in range(3)], -1)
    return t, t[:, :2] / t[:, 2:3]


@pytest.mark.parametrize("pop", util.EDGE_POPS)
def test_edge_scene_labels(pop):
    H, W = (48, 64) if pop == "border" else (64, 64)
    sc, lab = util.make_edge_scene(pop, H=H, W=W, views=3, seed=5, color_sh_degree=1, feature_channels=4)
    bi = util.boundary_inputs(sc, H, W)
    V = bi["V"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    for v in range(V):
        t, ratio = _torch_f32_ratio(bi, v)
        np.testing.assert_array_equal(t.numpy().view(np.uint32), lab["t"][v].view(np.uint32))
        ok = np.isfinite(lab["ratio"][v])
        np.testing.assert_array_equal(ratio.numpy()[ok].view(np.uint32), lab["ratio"][v][ok].view(np.uint32))
        o = util.oracle_forward(bi, v)
        # the near cull of the C forward is the replica's, and nothing the cull keeps is lost to it
        assert not (o["radii"][lab["culled"][v]] > 0).any()
        np.testing.assert_array_equal(o["gdepth"][o["radii"] > 0].view(np.uint32), lab["t"][v][o["radii"] > 0, 2].view(np.uint32))
        if pop == "band" and v < 2:
            b = (lab["kind"] == 1) & (lab["band_view"] == v)
            assert (o["radii"][b] > 0).all(), "band Gaussians reach the image of their view"
            assert np.median(o["radii"][b]) >= 0.25 * W, "band footprints are tens of pixels"
        if pop == "outside" and v < 2:
            b = (lab["kind"] == 2) & lab["clamped"][v].any(-1)
            if b.any():
                assert (o["radii"][b] > 0).mean() >= 0.8, "clamped Gaussians outside the cone reach the image"
        if pop == "near" and v == 0:
            b = lab["kind"] == 3
            z = lab["t"][0, :, 2]
            assert (o["radii"][b & (z == np.nextafter(util.NEAR_CULL, np.float32(1)))] > 0).any()
            assert (o["radii"][b & (z == util.NEAR_CULL)] == 0).all()
            assert (o["radii"][b] > 3 * max(H, W)).any(), "near footprints several times the image"
        if pop == "border" and v == 0:
            e, c = lab["kind"] == 4, lab["kind"] == 5
            r = o["rect"]
            assert ((r[e, 2] - r[e, 0] == 1) | (r[e, 3] - r[e, 1] == 1)).all()
            assert (r[c] == np.array([0, 0, gx, gy])).all()
            for side, hit in (("left", r[e, 2] == 1), ("right", r[e, 0] == gx - 1), ("top", r[e, 3] == 1), ("bottom", r[e, 1] == gy - 1)):
                assert hit.any(), f"border: no rectangle on the {side} edge tiles"
    if pop == "band":
        # both sides of the boundary, in both views, on every side: k <= 0 kept, k > 0 clamped
        b = lab["kind"] == 1
        for v in (0, 1):
            sel = b & (lab["band_view"] == v)
            cl = lab["clamped"][v, sel, lab["band_axis"][sel]]
            assert cl.any() and (~cl).any()
            np.testing.assert_array_equal(cl, lab["band_k"][sel] > 0)
        # the band is narrow enough that a reciprocal formulation or a double decision would decide some rows differently
        bv, bax = lab["band_view"][b], lab["band_axis"][b]
        assert (lab["clamped_rcp"][bv, np.flatnonzero(b), bax] != lab["clamped"][bv, np.flatnonzero(b), bax]).any()
        assert (lab["clamped_f64"][bv, np.flatnonzero(b), bax] != lab["clamped"][bv, np.flatnonzero(b), bax]).any()


def _autograd_vs_c(bi, v):
    """C oracle backward against autograd through the torch oracle, view v (the bar of test_oracle_cpu.py)."""
    fwd = util.oracle_forward(bi, v)
    c = bi["cams"]
    H, W = bi["H"], bi["W"]
    req = lambda x: None if x is None else x.clone().requires_grad_(True)
    means, cov6, opac, shs, feats = req(bi["means"][v]), req(bi["cov6"][v]), req(bi["opac"]), req(bi["shs"]), req(bi["features"][v])
    color, feat, mask, depth, radii = to.rasterize(H, W, float(c.tan_fov_x[v]), float(c.tan_fov_y[v]), bi["bg"][v],
                                                   c.view_matrix[v], c.full_projection[v], c.campos[v], bi["sh_degree"],
                                                   means, cov6, opac, shs, None, feats)
    np.testing.assert_array_equal(radii.numpy(), fwd["radii"])
    gen = torch.Generator().manual_seed(11 + v)
    loss, grads = 0, {}
    for name, t in (("color", color), ("feature", feat), ("mask", mask), ("depth", depth)):
        if t is None:
            grads[name] = None
            continue
        grads[name] = torch.randn(t.shape, generator=gen)
        loss = loss + (t * grads[name]).sum()
    loss.backward()
    n = lambda g: None if g is None else g.numpy()
    bw = util.oracle_backward(bi, v, fwd, n(grads["color"]), n(grads["feature"]), n(grads["mask"])[0], n(grads["depth"])[0])
    for name, a, b in (("means", means.grad, bw["means3D"]), ("cov", cov6.grad, bw["cov3D"]), ("opac", opac.grad, bw["opacities"]),
                       ("shs", None if shs is None else shs.grad, bw["shs"]), ("feat", feats.grad, bw["features"])):
        if a is None:
            continue
        a = a.numpy()
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(a).max()), f"{name}[view {v}]"
    return fwd, grads


@pytest.mark.parametrize("pop", ["band", "outside", "near"])
def test_c_oracle_backward_matches_autograd_on_edges(pop):
    """(The plain projection convention: the torch oracle's clamp decision replicates the C forward's without
    contraction; the contracted one is held against the kernel in tests/test_frustum_edges_gpu.py.)"""
    sc, lab = util.make_edge_scene(pop, H=48, W=48, views=2, seed=2, color_sh_degree=1, feature_channels=4, filler=60)
    bi = util.boundary_inputs(sc, 48, 48, bg=(0.1, 0.2, 0.3))
    for v in range(bi["V"]):
        _autograd_vs_c(bi, v)


def test_old_double_clamp_mask_would_be_caught():
    """The C backward once decided the clamp in double (ratio and 1.3 * (double)tanfov).  On the band scene, the rows
    where that decision differs from the forward's move by more than 100x the GPU tests' gradient bar: a kernel that
    took the wrong decision cannot pass them."""
    sc, lab = util.make_edge_scene("band", H=64, W=64, views=2, seed=0, color_sh_degree=None, feature_channels=4)
    bi = util.boundary_inputs(sc, 64, 64, bg=(0.3, 0.1, 0.5))
    flipped_total = 0
    for v in range(bi["V"]):
        fwd = util.oracle_forward(bi, v)
        gen = torch.Generator().manual_seed(7)
        g_feat = torch.randn(fwd["feature"].shape, generator=gen).numpy()
        g_mask = torch.randn(fwd["mask"].shape, generator=gen).numpy()
        fixed = util.oracle_backward(bi, v, fwd, None, g_feat, g_mask)
        try:
            orc.set_legacy_clamp_mask(True)
            legacy = util.oracle_backward(bi, v, fwd, None, g_feat, g_mask)
        finally:
            orc.set_legacy_clamp_mask(False)
        flipped = np.flatnonzero((lab["clamped"][v] != lab["clamped_f64"][v]).any(-1) & (fwd["radii"] > 0))
        same = np.setdiff1d(np.arange(len(fwd["radii"])), flipped)
        # (the mask gates dL/dt.x, i.e. the mean's gradient; the covariance's sees only the rounding of the clamped t.x)
        for name in ("means3D", "cov3D"):
            scale = max(1.0, np.abs(fixed[name]).max())
            diff = np.abs(fixed[name] - legacy[name]).max(1)
            assert (diff[same if name == "means3D" else slice(None)] <= 1e-6 * scale).all(), \
                f"{name}: rows moved by more than a rounding"
            if name == "means3D":
                assert (diff[flipped] > 100 * GPU_BAR * scale).all(), \
                    f"{name}[view {v}]: a flipped clamp moves a row by only {diff[flipped].min():.3e} (scale {scale:.3e})"
        flipped_total += len(flipped)
    assert flipped_total >= 2
