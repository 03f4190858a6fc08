"""Fused depth head on the MI355X (lsr_depth_head_forward / _backward through latentsplat_amd.depth_head):
parity with the vectors the reference's DepthPredictorMonocular generated, with the float64 restatement at
ragged, edge, peaked and encoder sizes, reproducibility, the module mirror, and the head feeding the adapter.

Tolerances are the adapter tests' (tests/test_adapter_gpu.py): forward rtol 2e-5 / atol 2e-6; gradients: largest
absolute error at most 1e-4 of the reference tensor's largest magnitude.  Indices are exact: every case's
uniforms keep 1e-5 from the cumulative-sum edges (golden maker / depth_head_ref.random_case), far more than
float32 summation order can move an edge."""
import numpy as np
import pytest
import torch

from tests import depth_head_ref as ref
from tests.test_depth_head_cpu import GOLDEN, case_id, flat_case, rel_err

pytestmark = pytest.mark.gpu

PAD = 5     # the strided runs embed the row in a matrix PAD floats wider, 2 floats in (odd stride, odd offset)


def run_op(c, F, dev, wide=False, backward=True, **kw):
    """depth_head on the device.  c: numpy arrays logits (cams, rays, W), near, far (cams,), uniforms,
    g_depth, g_opacity (cams, rays, F, k).  `wide`: hand the op a strided view of a wider zero matrix and check
    that the gradient outside the row is exactly 0."""
    from latentsplat_amd.depth_head import depth_head
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    W = c["logits"].shape[-1]
    if wide:
        full = torch.zeros(c["logits"].shape[:-1] + (W + PAD,), device=dev)
        full[..., 2:2 + W] = t(c["logits"])
        full.requires_grad_()
        logits = full[..., 2:2 + W]
    else:
        full = t(c["logits"]).requires_grad_()
        logits = full
    if not kw.get("deterministic"):
        kw["uniforms"] = t(c["uniforms"])
    depth, opacity, index = depth_head(logits, t(c["near"]), t(c["far"]), num_surfaces=F, **kw)
    assert index.dtype == torch.int32 and not index.requires_grad
    grad = None
    if backward:
        ((depth * t(c["g_depth"])).sum() + (opacity * t(c["g_opacity"])).sum()).backward()
        grad = full.grad
        if wide:
            assert float(grad[..., :2].abs().max()) == 0 and float(grad[..., 2 + W:].abs().max()) == 0
            grad = grad[..., 2:2 + W]
        grad = grad.cpu().numpy()
    return depth.detach().cpu().numpy(), opacity.detach().cpu().numpy(), index.cpu().numpy(), grad


def op_kwargs(kw):
    """keyword arguments of the restatement -> those of the op"""
    out = dict(deterministic=kw.get("deterministic", False), use_transmittance=kw.get("transmittance", False),
               opacity_exponent=kw.get("exponent", 1.0), opacity_scale=kw.get("scale", 1.0))
    if out["deterministic"]:
        out["num_samples"] = kw["samples"]
    return out


def assert_matches(got, want, rows=None):
    """(depth, opacity, index, d_logits) of the op against the reference's; `rows`: boolean (cams, rays) mask of
    the rows the gradient is compared on."""
    depth, opacity, index, grad = got
    wdepth, wopacity, windex, wgrad = want
    assert np.array_equal(index, windex)
    assert np.isfinite(depth).all() and np.isfinite(opacity).all()
    np.testing.assert_allclose(depth, wdepth, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(opacity, wopacity, rtol=2e-5, atol=2e-6)
    if grad is not None:
        assert np.isfinite(grad).all()
        if rows is not None:
            grad, wgrad = grad[rows], wgrad[rows]
        assert rel_err(grad, wgrad) <= 1e-4


def against_restatement(c, F, dev, wide=False, **kw):
    want = ref.forward_backward(c["logits"], c["near"], c["far"], F, c["g_depth"], c["g_opacity"],
                                uniforms=None if kw.get("deterministic") else c["uniforms"], **kw)
    got = run_op(c, F, dev, wide=wide, **op_kwargs(kw))
    assert_matches(got, want)
    return got, want


@pytest.mark.parametrize("path", GOLDEN, ids=case_id)
def test_matches_reference_vectors(path, hip_device):
    """Forward and backward of every golden case, through a strided view (row stride 2 S F + 5)."""
    z, c, F, kw = flat_case(path)
    got = run_op(c, F, hip_device, wide=True, **op_kwargs(kw))
    assert_matches(got, (c["depth"], c["opacity"], c["index"], c["d_logits"]))


def test_mirror_module_end_to_end(hip_device):
    """DepthPredictorMonocular with the recorded Linear weights on the first golden case.  The recorded uniforms are
    the reference's draws from the CPU generator; a ROCm generator gives other numbers under the same seed, so the
    golden outputs are reproduced with those uniforms passed in, and the draw itself is pinned separately: without
    `uniforms` the module consumes the device generator exactly as the reference's one torch.rand((b, v, r, srf, spp),
    device=...) call does."""
    from latentsplat_amd import DepthPredictorMonocular
    dev = hip_device
    z = np.load([p for p in GOLDEN if case_id(p) == "stochastic"][0])
    b, v, rays, F, k = z["depth"].shape
    t = lambda a: torch.tensor(a, device=dev)
    m = DepthPredictorMonocular(z["features"].shape[-1], z["logits"].shape[-1] // (2 * F), F, bool(z["transmittance"]))
    m.load_state_dict({"projection.1.weight": torch.tensor(z["weight"]), "projection.1.bias": torch.tensor(z["bias"])})
    m.to(dev)
    features = t(z["features"]).requires_grad_()
    depth, opacity = m(features, t(z["near"]), t(z["far"]), False, k, uniforms=t(z["uniforms"]))
    assert depth.shape == opacity.shape == (b, v, rays, F, k)
    # (the logits come from a device matmul here: float32 summation order moves them by ~1e-6, which moves a
    # depth by the offset's sigmoid only; an index would need 1e-5)
    np.testing.assert_allclose(depth.detach().cpu().numpy(), z["depth"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(opacity.detach().cpu().numpy(), z["opacity"], rtol=2e-5, atol=2e-6)
    ((depth * t(z["g_depth"])).sum() + (opacity * t(z["g_opacity"])).sum()).backward()
    assert torch.isfinite(features.grad).all() and float(features.grad.abs().max()) > 0
    assert torch.isfinite(m.projection[1].weight.grad).all() and float(m.projection[1].weight.grad.abs().max()) > 0

    seed = int(z["forward_seed"])
    torch.manual_seed(seed)
    drawn = torch.rand((b, v, rays, F, k), device=dev)
    after_reference_call = torch.cuda.get_rng_state(dev)
    torch.manual_seed(seed)
    with torch.no_grad():
        d0, o0 = m(features, t(z["near"]), t(z["far"]), False, k)
        assert torch.equal(torch.cuda.get_rng_state(dev), after_reference_call)
        d1, o1 = m(features, t(z["near"]), t(z["far"]), False, k, uniforms=drawn)
    assert torch.equal(d0, d1) and torch.equal(o0, o1)
    # deterministic: no draw at all
    with torch.no_grad():
        m(features, t(z["near"]), t(z["far"]), True, 1)
    assert torch.equal(torch.cuda.get_rng_state(dev), after_reference_call)


@pytest.mark.parametrize("rows", [1, 63, 65, 257])
def test_ragged_row_counts(rows, hip_device):
    """The reference's S = 32, F = 1, k = 3 at row counts around the two-rows-per-wave and eight-waves-per-block
    boundaries, contiguous rows (the 8-byte load path)."""
    c = ref.random_case(1, rows, 32, 1, 3, seed=rows)
    against_restatement(c, 1, hip_device)


@pytest.mark.parametrize("S,F,k,kw", [
    (1, 1, 1, {}),
    (12, 3, 2, dict(exponent=2 ** 0.5, scale=0.5)),
    (64, 1, 8, dict(exponent=0.5, scale=1 / 3)),
    (33, 2, 3, dict(deterministic=True, samples=3)),
    (16, 2, 3, {}),                                  # 2 S F = 64 with two surfaces side by side in a wave
], ids=lambda v: str(v) if isinstance(v, int) else "")
def test_other_bucket_and_surface_counts(S, F, k, kw, hip_device):
    c = ref.random_case(1, 65, S, F, k, seed=100 * S + F, deterministic=bool(kw.get("deterministic")))
    against_restatement(c, F, hip_device, **kw)
    against_restatement(c, F, hip_device, wide=True, **kw)


def test_edge_uniforms(hip_device):
    """u = 0 picks the first bucket, u = 1 - 2^-24 and u = 1.0 clip to the last; k equal uniforms repeat an index and
    its gradient is the sum."""
    S, k = 32, 3
    c = ref.random_case(2, 8, S, 1, k, seed=7)
    u = c["uniforms"]
    u[:, 0], u[:, 1], u[:, 2] = 0.0, np.float32(1 - 2.0 ** -24), 1.0
    u[:, 3] = u[:, 3, :, :1]                       # all k equal
    u[:, 4, :, 0], u[:, 4, :, 1] = 0.0, 1.0        # mixed with a random one
    cdf = ref.distribution(torch.tensor(c["logits"]).double(), 1)[3]
    assert float(ref.edge_gap(cdf, torch.tensor(u).double())[:, 3:].min()) >= 1e-5
    assert float(cdf[..., 0].min()) >= 1e-5 and float((1 - cdf[..., -2]).min()) >= 1e-5   # first / last bucket are not empty
    (depth, opacity, index, grad), _ = against_restatement(c, 1, hip_device)
    assert (index[:, 0] == 0).all() and (index[:, 1] == S - 1).all() and (index[:, 2] == S - 1).all()
    assert (index[:, 3] == index[:, 3, :, :1]).all()
    assert (index[:, 4, :, 0] == 0).all() and (index[:, 4, :, 1] == S - 1).all()
    # the repeated index: the gradient of the three samples is the sum of the gradients of each alone
    one = {n: a[:, 3:4].copy() for n, a in c.items() if a.ndim > 1}
    one.update(near=c["near"], far=c["far"])
    total = 0
    for j in range(k):
        single = dict(one)
        single["g_depth"], single["g_opacity"] = np.zeros_like(one["g_depth"]), np.zeros_like(one["g_opacity"])
        single["g_depth"][..., j], single["g_opacity"][..., j] = one["g_depth"][..., j], one["g_opacity"][..., j]
        total = total + run_op(single, 1, hip_device)[3].astype(np.float64)
    assert rel_err(grad[:, 3:4], total) <= 1e-5


@pytest.mark.parametrize("transmittance", [False, True], ids=["plain", "transmittance"])
def test_peaked_rows(transmittance, hip_device):
    """One logit at +40 and the rest at 0; every logit at -40: finite outputs and gradients that match the restatement."""
    S, k = 32, 3
    c = ref.random_case(1, 4, S, 1, k, seed=21, min_gap=None)
    c["logits"][0, 0] = 0.0
    c["logits"][0, 0, 2 * 5] = 40.0                # the pdf logit of bucket 5
    c["logits"][0, 1] = -40.0
    c["logits"][0, 2] = 0.0
    c["logits"][0, 2, 2 * (S - 1)] = 40.0          # the peak on the last bucket
    cdf = ref.distribution(torch.tensor(c["logits"]).double(), 1)[3]
    assert float(ref.edge_gap(cdf, torch.tensor(c["uniforms"]).double()).min()) >= 1e-5
    (depth, opacity, index, grad), _ = against_restatement(c, 1, hip_device, transmittance=transmittance)
    assert (index[0, 0] == 5).all() and (index[0, 2] == S - 1).all()
    assert len(np.unique(index[0, 1])) > 1


def test_encoder_size(hip_device):
    """2 cameras x 65 536 rays, S = 32, k = 3 against the float64 restatement.  Samples whose float64 gap to the nearest
    cumulative-sum edge is below 1e-6 (float32 cumulative-sum rounding) are left out of the index and value comparison;
    their share is capped at 5e-4 (expected 6.4e-5).  Gradients are compared on the rows with no such sample."""
    c, close = ref.encoder_case()
    F = ref.ENCODER_SHAPE[3]
    assert close.mean() <= ref.ENCODER_MAX_SHARE
    depth, opacity, index, grad = run_op(c, F, hip_device)
    wdepth, wopacity, windex, _ = ref.forward_backward(c["logits"], c["near"], c["far"], F, c["g_depth"], c["g_opacity"],
                                                       uniforms=c["uniforms"])
    keep = ~close
    assert np.array_equal(index[keep], windex[keep])
    assert np.abs(index - windex)[close].max(initial=0) <= 1          # a left-out sample lands on a neighbour at most
    np.testing.assert_allclose(depth[keep], wdepth[keep], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(opacity[keep], wopacity[keep], rtol=2e-5, atol=2e-6)
    # the gradient for the indices the kernel chose (identical on the compared rows)
    wgrad = ref.forward_backward(c["logits"], c["near"], c["far"], F, c["g_depth"], c["g_opacity"], index=index)[3]
    rows = ~close.any(axis=(2, 3))
    assert np.isfinite(grad).all() and rel_err(grad[rows], wgrad[rows]) <= 1e-4


def test_backward_is_bitwise_reproducible(hip_device):
    c = ref.random_case(2, 4099, 32, 1, 3, seed=3, min_gap=None)
    c["uniforms"][:, ::2] = c["uniforms"][:, ::2, :, :1]          # every other row repeats one index
    for kw in (dict(use_transmittance=True), dict(opacity_exponent=1.5)):
        first, second = run_op(c, 1, hip_device, **kw), run_op(c, 1, hip_device, **kw)
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
        assert np.isfinite(first[3]).all() and float(np.abs(first[3]).max()) > 0


def test_head_feeds_the_adapter_and_the_renderer(hip_device):
    """depth and opacity from the op go into adapter_geometry and a small render_scenes call; backward() reaches the
    logits with a finite, non-zero gradient."""
    from latentsplat_amd.decoder.cuda_splatting import render_scenes
    from latentsplat_amd.depth_head import depth_head
    from latentsplat_amd.gaussian_adapter import adapter_geometry
    dev = hip_device
    v, h, w, S, k = 2, 8, 8, 32, 3
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn(1, v, h * w, 2 * S, generator=gen).to(dev).requires_grad_()
    near, far = torch.full((1, v), 1.0, device=dev), torch.full((1, v), 6.0, device=dev)
    uniforms = torch.rand(1, v, h * w, 1, k, generator=gen).to(dev)
    depth, opacity, index = depth_head(logits, near, far, num_surfaces=1, uniforms=uniforms,
                                       opacity_exponent=2 ** 0.5, opacity_scale=1 / k)
    ext = torch.eye(4, device=dev).repeat(v, 1, 1)
    ext[1, 0, 3] = 0.2
    intr = torch.tensor([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1]], device=dev).repeat(v, 1, 1)
    ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij")
    coords = torch.stack([xs, ys], -1).reshape(1, h * w, 2).repeat(v, 1, 1).to(dev)
    raw = torch.randn(v, h * w, 7, generator=gen).to(dev)
    means, cov, _, _ = adapter_geometry(ext, intr, coords, depth.reshape(v, h * w, k), raw, (h, w), 0.5, 15.0)
    g = v * h * w * k
    color = torch.rand(1, g, 3, 1, generator=gen).to(dev)
    out = render_scenes(ext[None], intr[None], near, far, (32, 32), torch.zeros(3, device=dev), means.reshape(1, g, 3),
                        cov.reshape(1, g, 3, 3), opacity.reshape(1, g), color)
    weight = torch.rand(out.color.shape, generator=gen).to(dev)
    (out.color * weight).sum().backward()
    assert float(out.color.detach().abs().max()) > 0
    grad = logits.grad
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    # both channels are reached: the pdf logits through the opacity, the offset logits through the depth
    assert float(grad[..., 0::2].abs().max()) > 0 and float(grad[..., 1::2].abs().max()) > 0
