"""Depth modes, host side (no GPU): the public PyTorch statement ``depth_mode_payload`` against the fake colours the
reference's ``render_depth_cuda`` hands to its rasterizer (tests/golden/depth_modes.npz, made by
tests/golden/make_golden_depth_modes.py), slots 41-43 of the view table and their gradient, and ``render_scenes`` /
``render_cuda`` / ``DecoderSplattingCUDA.forward`` with a mode over a slot-aware oracle stand-in for the rasterizer."""
import numpy as np
import pytest
import torch

from latentsplat_amd import decoder as dec
from latentsplat_amd import rasterizer as R
from latentsplat_amd.decoder import cuda_splatting as cs
from tests import depth_modes_util as du

MODES = du.MODES
BOUNDARY = dict(rtol=2e-5, atol=2e-5)     # tests/test_golden_cpu.py: boundary tensors
DEPTH = dict(rtol=1e-5, atol=1e-4)        # tests/test_golden_cpu.py: decoder depth


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def gold():
    return du.load_fixture()


def _flat(g):
    """inputs of the fixture flattened over (b v), Gaussians per view"""
    b, v = g["in_extrinsics"].shape[:2]
    f = lambda k: _t(g[k]).flatten(0, 1)
    rep = lambda k: _t(g[k]).repeat_interleave(v, dim=0)
    return f("in_extrinsics"), f("in_intrinsics"), f("in_near"), f("in_far"), rep("in_means"), rep("in_covariances"), rep("in_opacities")


@pytest.mark.parametrize("mode", MODES)
def test_helper_reproduces_reference_fake_colours(gold, mode):
    ext, intr, near, far, means, _, _ = _flat(gold)
    # camera-space depth two ways: the reference's (inverse extrinsics) and the one the kernels use (table: tz / scale)
    z_ref = torch.einsum("bij,bgj->bgi", torch.linalg.inv(ext), torch.nn.functional.pad(means, (0, 1), value=1.0))[..., 2]
    views = cs._view_table(ext, intr, near, far, torch.zeros(3), True, mode)
    z_tab = torch.stack([du.camera_depth(views, v, means[v]) for v in range(views.shape[0])])
    fake = gold[f"fake_{mode}"]
    for z in (z_ref, z_tab):
        u = R.depth_mode_value(z, near[:, None], far[:, None], mode)
        np.testing.assert_allclose(u.numpy(), fake, **BOUNDARY)
        d = R.depth_mode_payload(z, near[:, None], far[:, None], mode)
        np.testing.assert_allclose(d.numpy(), np.maximum(R.SH_C0 * fake + 0.5, 0.0), **BOUNDARY)
    if mode == "log":     # the reference's expression as it stands: log(far) for every Gaussian
        np.testing.assert_allclose(fake, np.broadcast_to(np.log(far.numpy())[:, None], fake.shape), **BOUNDARY)


def test_view_table_slots(gold):
    ext, intr, near, far, *_ = _flat(gold)
    bg = torch.tensor([0.1, 0.3, 0.7])
    plain = cs._view_table(ext, intr, near, far, bg, True)
    assert torch.equal(plain[:, 41:44], torch.zeros(plain.shape[0], 3))
    for mode in MODES:
        t = cs._view_table(ext, intr, near, far, bg, True, mode)
        assert torch.equal(t[:, :41], plain[:, :41])
        assert torch.equal(t[:, 41], torch.full((t.shape[0],), float(R.DEPTH_MODES[mode])))
        assert torch.equal(t[:, 42], near) and torch.equal(t[:, 43], far)
    t0 = cs._view_table(ext, intr, near, far, bg, True, "native")
    assert torch.equal(t0, plain)
    assert R.depth_mode_id(None) == 0 and R.depth_mode_id("log") == 4 and R.depth_mode_id(3) == 3
    with pytest.raises(R.LsrError):
        R.depth_mode_id("median")
    with pytest.raises(R.LsrError):
        cams, scale = cs._scaled_cameras(ext, intr, near, far, True)
        R.make_view_table(cams.view_matrix, cams.full_projection, cams.campos, cams.tan_fov_x, cams.tan_fov_y, bg, scale,
                          depth_mode="disparity")


@pytest.mark.parametrize("mode", ["relative_disparity", "log"])
def test_table_gradient_in_near_far_matches_helper(gold, mode):
    """float64: a loss on the payload computed from the table's slots differentiates into near / far like the helper fed
    near / far directly; near also keeps its path through the scene scale (slot 40)."""
    ext, intr, near, far, means, _, _ = (t.double() for t in _flat(gold))
    if mode == "log":     # every branch of min / max: far inside the scene, near further inside (z < far: far, z > near: near)
        z = torch.einsum("bij,bgj->bgi", torch.linalg.inv(ext), torch.nn.functional.pad(means, (0, 1), value=1.0))[..., 2]
        q = z.sort(dim=1).values
        near, far = q[:, 300] * 1.0001, q[:, 100] * 1.0001     # (off every z: no min / max tie)
    w = torch.randn(means.shape[:2], generator=torch.Generator().manual_seed(0), dtype=torch.float64)

    def table_loss(n, f):
        cams, scale = cs._scaled_cameras(ext, intr, n, f, True)
        t = R.make_view_table(cams.view_matrix, cams.full_projection, cams.campos, cams.tan_fov_x, cams.tan_fov_y,
                              torch.zeros(3, dtype=torch.float64), scale, dtype=torch.float64, depth_mode=mode, near=n, far=f)
        d = torch.stack([du.payload(t, v, means[v]) for v in range(t.shape[0])])
        return (d * w).sum() + (t[:, 40] * 0.3).sum()

    def helper_loss(n, f):
        z = torch.einsum("bij,bgj->bgi", torch.linalg.inv(ext), torch.nn.functional.pad(means, (0, 1), value=1.0))[..., 2]
        return (R.depth_mode_payload(z, n[:, None], f[:, None], mode) * w).sum() + (0.3 / n).sum()

    grads = []
    for fn in (table_loss, helper_loss):
        n, f = near.clone().requires_grad_(True), far.clone().requires_grad_(True)
        fn(n, f).backward()
        grads.append((n.grad, f.grad))
    for a, b in zip(*grads):
        assert float(b.abs().max()) > 0
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-9, atol=1e-12 * float(b.abs().max()))


@pytest.mark.parametrize("mode", MODES)
def test_render_scenes_and_render_cuda_with_a_mode(monkeypatch, gold, mode):
    monkeypatch.setattr(cs, "rasterize_views", du.slot_aware_oracle_rasterize_views)
    g = gold
    want = g[f"depth_{mode}"]
    shape = tuple(int(x) for x in g["in_image_shape"])
    bg = _t(g["in_bg"])
    kw = dict(gaussian_color_sh_coefficients=_t(g["in_color_harmonics"]), gaussian_feature_sh_coefficients=_t(g["in_feature_harmonics"]))
    plain = cs.render_scenes(_t(g["in_extrinsics"]), _t(g["in_intrinsics"]), _t(g["in_near"]), _t(g["in_far"]), shape, bg,
                             _t(g["in_means"]), _t(g["in_covariances"]), _t(g["in_opacities"]), **kw)
    out = cs.render_scenes(_t(g["in_extrinsics"]), _t(g["in_intrinsics"]), _t(g["in_near"]), _t(g["in_far"]), shape, bg,
                           _t(g["in_means"]), _t(g["in_covariances"]), _t(g["in_opacities"]), depth_mode=mode, **kw)
    np.testing.assert_allclose(out.depth.numpy(), want.reshape(out.depth.shape), **DEPTH)
    for k in ("color", "feature", "mask"):
        assert torch.equal(getattr(out, k), getattr(plain, k))
    assert not np.allclose(plain.depth.numpy(), want.reshape(out.depth.shape), **DEPTH)
    ext, intr, near, far, means, cov, opac = _flat(g)
    v = g["in_extrinsics"].shape[1]
    rep = lambda k: _t(g[k]).repeat_interleave(v, dim=0)
    out = cs.render_cuda(ext, intr, near, far, shape, bg.expand(ext.shape[0], 3), means, cov, opac,
                         rep("in_color_harmonics"), rep("in_feature_harmonics"), depth_mode=mode)
    np.testing.assert_allclose(out.depth.numpy(), want.reshape(out.depth.shape), **DEPTH)


def _decoder(g):
    gauss = dec.Gaussians(_t(g["in_means"]), _t(g["in_covariances"]), _t(g["in_opacities"]), _t(g["in_color_harmonics"]),
                          _t(g["in_feature_harmonics"]))
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), [float(x) for x in g["in_bg"]], False)
    args = (gauss, _t(g["in_extrinsics"]), _t(g["in_intrinsics"]), _t(g["in_near"]), _t(g["in_far"]),
            tuple(int(x) for x in g["in_image_shape"]))
    return d, args


@pytest.mark.parametrize("mode", ["relative_disparity", "log"])
def test_decoder_switch_on_is_one_rasterizer_call(monkeypatch, gold, mode):
    monkeypatch.setattr(cs, "rasterize_views", du.slot_aware_oracle_rasterize_views)
    d, args = _decoder(gold)
    assert dec.get_fused_depth_modes() is False          # the default
    dec.set_fused_depth_modes(True)
    try:
        du.CALLS.clear()
        out = d.forward(*args, depth_mode=mode)
        assert len(du.CALLS) == 1 and args[1].shape[0] == 2           # b = 2 scenes, one call
        assert bool((du.CALLS[0][:, 41] == R.DEPTH_MODES[mode]).all())
        du.CALLS.clear()
        native = d.forward(*args, depth_mode="depth")                 # None and "depth" keep the native depth
        assert len(du.CALLS) == 1 and bool((du.CALLS[0][:, 41:44] == 0).all())
    finally:
        dec.set_fused_depth_modes(False)
    g = gold
    np.testing.assert_allclose(out.depth.numpy(), g[f"depth_{mode}"], **DEPTH)
    tol = dict(rtol=0, atol=2e-5)
    np.testing.assert_allclose(out.mask.numpy(), g["decoder_mask"], **tol)
    np.testing.assert_allclose(out.color.numpy(), g["decoder_color"], **tol)
    np.testing.assert_allclose(out.feature_posterior.mean.numpy(), g["decoder_posterior_mean"], **tol)
    np.testing.assert_allclose(out.feature_posterior.logvar.numpy(), g["decoder_posterior_logvar"], rtol=1e-4, atol=2e-3)
    assert torch.equal(native.mask, out.mask) and not torch.equal(native.depth, out.depth)


def test_decoder_switch_off_keeps_the_reference_call_pattern(monkeypatch, gold):
    """One payload call plus one depth call per scene: what DecoderSplattingCUDA.forward made before the switch existed."""
    monkeypatch.setattr(cs, "rasterize_views", du.slot_aware_oracle_rasterize_views)
    d, args = _decoder(gold)
    b = args[1].shape[0]
    du.CALLS.clear()
    out = d.forward(*args, depth_mode="relative_disparity")
    assert len(du.CALLS) == 1 + b
    assert all(bool((c[:, 41:44] == 0).all()) for c in du.CALLS)       # no table carries a mode
    np.testing.assert_allclose(out.depth.numpy(), gold["depth_relative_disparity"], **DEPTH)
    du.CALLS.clear()
    d.forward(*args)
    assert len(du.CALLS) == 1
