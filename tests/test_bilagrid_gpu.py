"""Bilateral-grid appearance compensation on the MI355X: lsr_bilagrid_slice_* and lsr_bilagrid_tv_* against the float64
restatement (tests/bilagrid_ref.py), held to the stock float32 composition's own error on the same inputs; determinism, views
without a grid, non-finite pixels, luminance on a node, the autograd surface, a fit through the operator and the fitting tool.

The bar (tests/bilagrid_ref.py `held`): every element of out, grad_image, grad_grids, tv and tv's gradient within
max(4 x the stock float32 composition's largest error, 2^-20 x max |want|) of float64.

Kernel paths (csrc/bilagrid.hip) and the cases of tests/bilagrid_ref.py CASES that reach them, asserted per case through
lsr_bilagrid_slice_path:
  * 32 x 32 pixel tiles, footprint in LDS: affine_1x1, affine_5x7, tiny_grid, shared_grid (three tiles wide, two high, the
    last ones partial), default_256 (the published grid; eight tiles wide, two high);
  * 16 x 16 pixel tiles, footprint in LDS: default_64 (a 32-tile would reach 800 nodes), default_33x65 (partial tiles both ways);
  * no tile's footprint fits, the parameter read and its gradient added in global memory: grid_wider_than_image, largest_8,
    largest_40 (nine 16-tiles, the outer ones partial)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import bilagrid_ref as ref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu


def _on(dev, c):
    return {k: v.to(dev) for k, v in c.items()}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_matches_float64_within_the_stock_compositions_error(hip_device, name):
    """Every case of the table on its kernel path (module docstring); grad_grids arrives full of NaN: the call zeroes it."""
    from latentsplat_amd import bilagrid as bg
    want, yard = ref.reference(name)
    c = _on(hip_device, ref.make_case(name))
    assert bg.slice_path(c["grids"], c["image"]) == ref.CASES[name][5]
    out = bg.slice_forward(c["grids"], c["image"], c["grid_idx"])
    filled = torch.full_like(c["grids"], float("nan"))
    grad_image, grad_grids = bg.slice_backward(c["grids"], c["image"], c["grid_idx"], c["grad_out"], grad_grids=filled)
    assert grad_grids.data_ptr() == filled.data_ptr()
    tv = bg.tv_forward(c["grids"])
    grad_tv = bg.tv_backward(c["grids"], c["grad_tv"].reshape(1))
    got = dict(out=out, grad_image=grad_image, grad_grids=grad_grids, tv=tv, grad_tv=grad_tv)
    for k, v in got.items():
        ref.held(k, v.cpu().numpy(), want[k], yard[k], f"{name}:")
    # grids no view indexes receive exactly nothing
    idx = set(ref.CASES[name][4])
    for n in range(ref.CASES[name][3]):
        if n not in idx:
            assert not grad_grids[n].any(), (name, n)


TV_BLOCK_ELEMS, TV_MAX_BLOCKS = 256 * 8, 1024       # kBgThreads * kTvPerThread, kTvMaxBlocks of csrc/bilagrid.hip
TV_PAST_THE_GRID = (3, 12, 16, 64, 64)              # no image goes with it: a case of its own, beside ref.CASES


@functools.lru_cache(maxsize=None)
def _tv_past_the_grid():
    """Seeded grids past the capped grid of the two total-variation kernels, the float64 restatement and the stock float32
    loop: computed once, shared, never modified."""
    g = torch.Generator().manual_seed(4242 + len(ref.CASES))
    grids = torch.eye(3, 4).reshape(1, 12, 1, 1, 1) + 0.3 * torch.randn(*TV_PAST_THE_GRID, generator=g)
    up = 1.7
    want, yard = ref.restate_tv(grids, up), ref.stock_tv(grids, up, dtype=torch.float32)
    return grids, up, {k: v.numpy() for k, v in want.items()}, {k: v.numpy() for k, v in yard.items()}


def test_total_variation_past_the_grid_cap(hip_device):
    """Both kernels launch one workgroup per 2048 elements, at most 1024, and a lane strides over all the launch's lanes: up
    to the cap a lane takes at most eight elements whatever the size (786 432 floats, the largest grid of ref.CASES, are 384
    workgroups); 2 359 296 floats would be 1152 workgroups, run on 1024, and every lane takes a ninth element."""
    from latentsplat_amd import bilagrid as bg
    grids, up, want, yard = _tv_past_the_grid()
    assert grids.numel() == 2_359_296 > TV_BLOCK_ELEMS * TV_MAX_BLOCKS
    assert max(int(np.prod(c[0])) * 12 * c[3] for c in ref.CASES.values()) == 786_432 < TV_BLOCK_ELEMS * TV_MAX_BLOCKS
    d = grids.to(hip_device)
    grad_tv = torch.full((1,), up, device=hip_device)
    tv, grad = bg.tv_forward(d), bg.tv_backward(d, grad_tv)
    ref.held("tv", tv.cpu().numpy(), want["tv"], yard["tv"], "tv past the grid:")
    ref.held("grad_tv", grad.cpu().numpy(), want["grad"], yard["grad"], "tv past the grid:")
    assert torch.equal(_bits(tv), _bits(bg.tv_forward(d))) and torch.equal(_bits(grad), _bits(bg.tv_backward(d, grad_tv)))


def test_forward_gives_the_same_bits_every_call_and_on_a_side_stream(hip_device):
    from latentsplat_amd import bilagrid as bg
    for name in ("default_33x65", "default_256", "largest_40"):
        c = _on(hip_device, ref.make_case(name))
        first = bg.slice_forward(c["grids"], c["image"], c["grid_idx"])
        again = bg.slice_forward(c["grids"], c["image"], c["grid_idx"])
        side = torch.cuda.Stream(hip_device)
        side.wait_stream(torch.cuda.current_stream(hip_device))
        with torch.cuda.stream(side):
            aside = bg.slice_forward(c["grids"], c["image"], c["grid_idx"])
            tv_aside = bg.tv_forward(c["grids"])
        side.synchronize()
        assert torch.equal(_bits(first), _bits(again)) and torch.equal(_bits(first), _bits(aside)), name
        # the image gradient and both total-variation calls are deterministic too
        a, b = (bg.slice_backward(c["grids"], c["image"], c["grid_idx"], c["grad_out"])[0] for _ in range(2))
        assert torch.equal(_bits(a), _bits(b)), name
        assert torch.equal(_bits(bg.tv_forward(c["grids"])), _bits(tv_aside))
        up = c["grad_tv"].reshape(1)
        assert torch.equal(_bits(bg.tv_backward(c["grids"], up)), _bits(bg.tv_backward(c["grids"], up)))


@pytest.mark.parametrize("name", ["default_64", "default_33x65"])
def test_a_view_without_a_grid_passes_through_bit_for_bit(hip_device, name):
    from latentsplat_amd import bilagrid as bg
    c = _on(hip_device, ref.make_case(name))
    assert int(c["grid_idx"][1]) == -1
    out = bg.slice_forward(c["grids"], c["image"], c["grid_idx"])
    grad_image, grad_grids = bg.slice_backward(c["grids"], c["image"], c["grid_idx"], c["grad_out"])
    assert torch.equal(_bits(out[1]), _bits(c["image"][1])) and torch.equal(_bits(grad_image[1]), _bits(c["grad_out"][1]))
    assert not torch.equal(out[0], c["image"][0]) and not grad_grids[1].any() and grad_grids[0].any() and grad_grids[2].any()
    # an index past the last grid is no grid either
    idx = c["grid_idx"].clone()
    idx[0] = 3
    out = bg.slice_forward(c["grids"], c["image"], idx)
    grad_image, grad_grids = bg.slice_backward(c["grids"], c["image"], idx, c["grad_out"])
    assert torch.equal(_bits(out[:2]), _bits(c["image"][:2])) and torch.equal(_bits(grad_image[:2]), _bits(c["grad_out"][:2]))
    assert not grad_grids[1:].any() and grad_grids[0].any()


@pytest.mark.parametrize("name", ["default_256", "default_33x65", "largest_40"])
def test_non_finite_pixels_reach_nothing_else(hip_device, name):
    """A few NaN / +-Inf pixels: every other pixel of out and grad_image keeps its bits, and grad_grids, a slice of a larger
    buffer at an odd offset, leaves the sentinels around it untouched."""
    from latentsplat_amd import bilagrid as bg
    c = _on(hip_device, ref.make_case(name))
    clean_out = bg.slice_forward(c["grids"], c["image"], c["grid_idx"])
    clean_grad = bg.slice_backward(c["grids"], c["image"], c["grid_idx"], c["grad_out"])[0]
    image = c["image"].clone()
    V, _, H, W = image.shape
    bad = torch.zeros((V, H, W), dtype=torch.bool, device=hip_device)
    v = 0 if int(c["grid_idx"][0]) >= 0 else 1
    for k, (value, ch) in enumerate(((float("nan"), 0), (float("inf"), 1), (float("-inf"), 2), (float("nan"), 2), (float("inf"), 0))):
        y, x = (7 * k + 3) % H, (11 * k + 5) % W
        image[v, ch, y, x] = value
        bad[v, y, x] = True
    image[v, :, H - 1, W - 1] = torch.tensor([float("inf"), float("-inf"), float("nan")], device=hip_device)
    bad[v, H - 1, W - 1] = True
    keep = ~bad[:, None].expand_as(image)
    n, pad, sentinel = c["grids"].numel(), 3, -12345.0
    buffer = torch.full((n + 2 * pad,), sentinel, device=hip_device)
    out = bg.slice_forward(c["grids"], image, c["grid_idx"])
    grad_image, grad_grids = bg.slice_backward(c["grids"], image, c["grid_idx"], c["grad_out"],
                                               grad_grids=buffer[pad:pad + n].view(c["grids"].shape))
    torch.cuda.synchronize(hip_device)
    assert torch.equal(_bits(out[keep]), _bits(clean_out[keep])) and torch.equal(_bits(grad_image[keep]), _bits(clean_grad[keep]))
    assert (buffer[:pad] == sentinel).all() and (buffer[pad + n:] == sentinel).all()
    assert (grad_grids != sentinel).all()


def test_luminance_exactly_on_a_node_or_a_clamp(hip_device):
    """Grey pixels k / 4 under five luminance levels, 0 and 1 among them: the value is continuous there, so the forward is on
    the bar; the gradients pick one side and are finite."""
    from latentsplat_amd import bilagrid as bg
    g = torch.Generator().manual_seed(77)
    grids = torch.eye(3, 4).reshape(1, 12, 1, 1, 1) + 0.3 * torch.randn(2, 12, 5, 3, 4, generator=g)
    levels = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, -0.2, 1.2])
    image = levels[torch.randint(0, len(levels), (2, 1, 9, 13), generator=g)].expand(2, 3, 9, 13).contiguous()
    idx, up = torch.tensor([1, 0], dtype=torch.int32), torch.randn(2, 3, 9, 13, generator=g)
    want = ref.restate(grids, image, idx)["out"].numpy()
    yard = ref.stock(grids, image, idx, dtype=torch.float32)["out"].numpy()
    d = lambda t: t.to(hip_device)
    ref.held("out", bg.slice_forward(d(grids), d(image), d(idx)).cpu().numpy(), want, yard, "on a node:")
    grad_image, grad_grids = bg.slice_backward(d(grids), d(image), d(idx), d(up))
    assert torch.isfinite(grad_image).all() and torch.isfinite(grad_grids).all() and grad_grids.any()


def test_autograd_surface(hip_device):
    from latentsplat_amd import BilateralGrid, bilagrid_slice, bilagrid_tv
    from latentsplat_amd import bilagrid as bg
    c = _on(hip_device, ref.make_case("default_33x65"))
    want, yard = ref.reference("default_33x65")
    grids, image = c["grids"].clone().requires_grad_(True), c["image"].clone().requires_grad_(True)
    out = bilagrid_slice(grids, image, c["grid_idx"])
    tv = bilagrid_tv(grids)
    assert out.shape == image.shape and tv.shape == ()
    ((out * c["grad_out"]).sum() + c["grad_tv"] * tv).backward()
    ref.held("grad_image", image.grad.cpu().numpy(), want["grad_image"], yard["grad_image"], "autograd:")
    ref.held("grad_grids", grids.grad.cpu().numpy(), want["grad_grids"] + want["grad_tv"], yard["grad_grids"] + yard["grad_tv"], "autograd:")
    # only the image needs a gradient: the rasterizer's side of a frozen grid
    image2 = c["image"].clone().requires_grad_(True)
    (bilagrid_slice(c["grids"], image2, c["grid_idx"]) * c["grad_out"]).sum().backward()
    assert torch.equal(_bits(image2.grad), _bits(image.grad))
    alone, none = bg.slice_backward(c["grids"], c["image"], c["grid_idx"], c["grad_out"], want_grids=False)
    assert none is None and torch.equal(_bits(alone), _bits(image.grad))
    # a non-contiguous image is taken as it is
    wide = torch.zeros((3, 3, 33, 70), device=hip_device)
    wide[..., :65] = c["image"]
    assert torch.equal(_bits(bg.slice_forward(c["grids"], wide[..., :65], c["grid_idx"])), _bits(out))
    module = BilateralGrid(3).to(hip_device)
    same = module(c["image"], c["grid_idx"])
    ident = ref.restate(module.grids.detach().cpu(), c["image"].cpu(), c["grid_idx"].cpu())["out"].numpy()
    assert np.abs(same.detach().cpu().numpy() - ident).max() <= 2.0 ** -20 * 1.2 and float(module.tv_loss().detach()) == 0.0
    with pytest.raises(_lib.LsrError, match=r"\(V, 3, H, W\)"):
        bilagrid_slice(c["grids"], c["image"][:, :2], c["grid_idx"])
    with pytest.raises(_lib.LsrError, match="int32"):
        bilagrid_slice(c["grids"], c["image"], c["grid_idx"].long())
    with pytest.raises(_lib.LsrError, match=r"\(N, 12, L, Y, X\)"):
        bilagrid_tv(c["grids"][:, :11])


def test_fit_through_the_operator(hip_device):
    """4 views of 32 x 32, each target the view under a 3 x 4 affine of its own; a 1 x 1 x 1 BilateralGrid,
    torch.optim.Adam(lr=0.02), 200 steps through photometric_loss(., ., 0.0); the final loss below 1 % of the first.

    The affines lie 0.75 to 1.25 from the identity in every one of the 12 entries (first loss near 2.5), so that all of them
    have to be learnt through the operator's gradient and the 1 % bound is far above where constant-rate Adam hovers on an
    exactly fittable L1 objective (about 0.005 at this rate, whatever the target): DESIGN.md 2.17 has the reasoning."""
    from latentsplat_amd import BilateralGrid, photometric_loss
    g = torch.Generator().manual_seed(5)
    V = 4
    image = torch.rand(V, 3, 32, 32, generator=g)
    A = torch.eye(3, 4) + 1.0 + 0.25 * (2.0 * torch.rand(V, 3, 4, generator=g) - 1.0)
    target = (torch.einsum("vrk,vkhw->vrhw", A[:, :, :3], image) + A[:, :, 3, None, None]).to(hip_device)
    image = image.to(hip_device)
    module = BilateralGrid(V, 1, 1, 1).to(hip_device)
    opt = torch.optim.Adam(module.parameters(), lr=0.02)
    idx = torch.arange(V, dtype=torch.int32, device=hip_device)
    losses = []
    for _ in range(200):
        opt.zero_grad(set_to_none=True)
        loss = photometric_loss(module(image, idx), target, 0.0)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    first, last = float(losses[0]), float(losses[-1])
    print(f"fit through the operator: first {first:.5f} last {last:.5f} ratio {last / first:.4f}")
    assert np.isfinite(last) and last < 0.01 * first, (first, last)
    # and it arrived where it was sent: no entry further from its target than Adam moves it in two and a half steps
    assert float((module.affine().detach().cpu() - A).abs().max()) < 0.05


def test_fit_tool_with_and_without_the_grid(hip_device, tmp_path):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    from latentsplat_amd import BilateralGrid
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, 2000, 64, 2)            # the scene file of tests/test_scene_params_gpu.py
    common = [str(path), "--noise", "0", "--target-jitter", "0.3", "--views", "3", "--size", "48", "--steps", "40", "--seed", "0"]
    plain = fit_ply.main(common + ["--out", str(tmp_path / "plain")])
    res = fit_ply.main(common + ["--out", str(tmp_path / "grid"), "--bilateral-grid", "1", "1", "1", "--bilateral-grid-lr", "0.02"])
    print("fit without the grid:", plain)
    print("fit with the grid:   ", res)
    assert res["loss_last"] < plain["loss_last"] and res["loss_last"] < res["loss_first"]
    assert json.load(open(tmp_path / "grid" / "fit.json")) == res and json.load(open(tmp_path / "plain" / "fit.json")) == plain
    assert res["bilateral_grid"] == [1, 1, 1] and res["tv_weight"] == 10.0 and res["tv_last"] == 0.0 and res["target_jitter"] == 0.3
    assert plain["target_jitter"] == 0.3 and not {"bilateral_grid", "tv_weight", "tv_last"} & set(plain)
    assert not os.path.exists(tmp_path / "plain" / "bilateral_grids.pt")
    module = BilateralGrid(3, 1, 1, 1)
    module.load_state_dict(torch.load(tmp_path / "grid" / "bilateral_grids.pt", map_location="cpu"))
    assert torch.isfinite(module.grids).all() and not torch.equal(module.affine()[0].detach(), torch.eye(3, 4))
