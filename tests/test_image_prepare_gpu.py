"""lsr_image_prepare (csrc/image_prepare.hip; latentsplat_amd.images) against the float64 restatement of tests/colmap_ref.py.

Exact path: a pinhole photograph, a power-of-two reduction and a principal point offset by (+-3, +-2.5) from the centre put
every sub-sample on a pixel centre or half way between two, so every operation is exact: the image is
``float32(block sum) / float32(255 n)`` bit for bit and the coverage the exact fraction.

General path: the distortion models, fractional reductions, RGBA, batches, output widths around a wave, many workgroups,
uncovered pixels.  The bar per output is the project's usual one: at most 4 x the error the stock float32 composition
(``grid_sample`` on the sub-sample grid, ``avg_pool2d``; colmap_ref.stock_prepare) makes against the same float64 values.
Coverage is a threshold: an output pixel that owns a sub-sample within 1e-3 source pixels of the source border may count it
either way and is left out; at most 1 % of a case's pixels may be (asserted on the float64 positions alone, and checked on
the CPU when the cases were fixed: the largest share is 0.033 %)."""
import functools

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd.images import SourceCamera, prepare_images, subsamples
from tests import colmap_ref as cr

pytestmark = pytest.mark.gpu


def _photos(B, Hs, Ws, C, seed):
    """Smooth structure plus noise, so that a misplaced tap changes the value; alpha (C = 4) spans 0..255."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    base = 127.5 + 100.0 * np.sin(xx[None, :, :, None] * 0.21 + np.arange(C)[None, None, None, :] + np.arange(B)[:, None, None, None]) \
        * np.cos(yy[None, :, :, None] * 0.17)
    return np.clip(np.rint(base + rng.uniform(-27, 27, (B, Hs, Ws, C))), 0, 255).astype(np.uint8)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- exact path ----

@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("Ws,Hs", [(37, 29), (64, 48)])
def test_exact_path_is_the_block_mean_bit_for_bit(hip_device, Ws, Hs, model, r):
    from latentsplat_amd.capture import target_size
    W, H = target_size(Ws, Hs, r)
    src = _photos(2, Hs, Ws, 3, seed=Ws + r)
    dev_src = torch.from_numpy(src).to(hip_device)
    f = 40.0
    for sx in (3.0, -3.0):
        for sy in (2.5, -2.5):
            cx, cy = Ws / 2.0 + sx, Hs / 2.0 + sy
            params = [f, cx, cy] if model == 0 else [f, f, cx, cy]
            cam = cr.camera_numbers(model, params)
            assert subsamples(SourceCamera.from_colmap(model, params), f / r, f / r) == r
            total, count = cr.block_sums(src, cam, H, W, f / r, f / r)
            assert np.array_equal(total, total.astype(np.float32)) and np.array_equal(total * 4, np.rint(total * 4))   # halves at most: exact
            want = np.where(count[None, :, :, None] > 0, total.astype(np.float32) / np.maximum(np.float32(255.0) * count.astype(np.float32), 1)[None, :, :, None],
                            np.float32(0)).astype(np.float32).transpose(0, 3, 1, 2)
            image, coverage = prepare_images(dev_src, SourceCamera.from_colmap(model, params), H, W, f / r, f / r)
            assert image.shape == (2, 3, H, W) and coverage.shape == (2, H, W)
            assert np.array_equal(_bits(image), np.ascontiguousarray(want).view(np.uint32))
            assert np.array_equal(coverage.cpu().numpy(), np.broadcast_to((count / (r * r)).astype(np.float32), (2, H, W)))
            assert count.max() == r * r and (count < r * r).any()      # the shift exposes a border


@pytest.mark.parametrize("model", [0, 1])
def test_identity_returns_the_pixels_and_even_blocks_their_mean(hip_device, model):
    Hs, Ws = 48, 64
    src = _photos(1, Hs, Ws, 3, seed=5)
    dev_src = torch.from_numpy(src).to(hip_device)
    params = [50.0, Ws / 2.0, Hs / 2.0] if model == 0 else [50.0, 50.0, Ws / 2.0, Hs / 2.0]
    image, coverage = prepare_images(dev_src, SourceCamera.from_colmap(model, params), Hs, Ws, 50.0, 50.0)
    want = (src.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    assert np.array_equal(_bits(image), np.ascontiguousarray(want).view(np.uint32)) and bool((coverage == 1).all())
    for r in (2, 4):                                        # plain numpy blocks, nothing of the restatement
        image, coverage = prepare_images(dev_src, SourceCamera.from_colmap(model, params), Hs // r, Ws // r, 50.0 / r, 50.0 / r)
        sums = src.astype(np.float32).reshape(1, Hs // r, r, Ws // r, r, 3).sum(axis=(2, 4))
        want = (sums / np.float32(255.0 * r * r)).transpose(0, 3, 1, 2)
        assert np.array_equal(_bits(image), np.ascontiguousarray(want).view(np.uint32)) and bool((coverage == 1).all())


# ---- general path ----

# label: model, parameters (COLMAP order), Hs, Ws, C, B, H, W, r
CASES = {
    "simple_radial_plus_w64": (2, [52.0, 33.3, 23.3, 0.2], 48, 64, 3, 1, 48, 64, 1),
    "simple_radial_minus_w63_rgba_b3": (2, [50.0, 30.2, 20.7, -0.2], 40, 63, 4, 3, 40, 63, 1),
    "radial_w65": (3, [55.0, 33.8, 24.3, 0.1, -0.05], 50, 65, 3, 1, 50, 65, 1),
    "opencv_r2.5_rgba": (4, [130.0, 128.0, 81.3, 59.3, 0.08, -0.02, 0.004, -0.003], 120, 160, 4, 1, 48, 64, 2.5),
    "opencv_r3_w63_b3": (4, [150.0, 151.0, 95.8, 47.1, -0.1, 0.03, -0.002, 0.005], 96, 189, 3, 3, 32, 63, 3),
    "simple_radial_r3_w1": (2, [8.0, 1.4, 4.6, 0.2], 9, 3, 3, 1, 3, 1, 3),
    "radial_r2.5_w65_rgba": (3, [135.0, 80.2, 50.9, -0.12, 0.04], 100, 162, 4, 1, 40, 65, 2.5),
    "opencv_1024x768_r4": (4, [820.0, 818.0, 515.3, 380.6, 0.06, -0.015, 0.002, -0.001], 768, 1024, 3, 1, 192, 256, 4),
    "pinhole_fractional_shift_uncovered": (1, [60.0, 61.0, 42.3, 17.6], 48, 64, 3, 1, 48, 64, 1),
    "simple_pinhole_r2.5_rgba_b3": (0, [70.0, 31.7, 25.2], 50, 64, 4, 3, 20, 26, 2.5),
}
BACKGROUND = (0.25, 0.5, 0.875)
UNCOVERED = ("simple_radial_plus_w64", "pinhole_fractional_shift_uncovered")


@functools.lru_cache(maxsize=None)
def _reference(label):
    model, params, Hs, Ws, C, B, H, W, r = CASES[label]
    src = _photos(B, Hs, Ws, C, seed=len(label))
    cam = cr.camera_numbers(model, params)
    fxo, fyo = cam["fx"] / r, cam["fy"] / r
    image, coverage, fragile = cr.prepare_ref(src, cam, H, W, fxo, fyo, BACKGROUND)
    for a in (src, image, coverage, fragile):
        a.setflags(write=False)
    return src, cam, fxo, fyo, image, coverage, fragile


@pytest.mark.parametrize("label", list(CASES))
def test_general_path_against_float64(hip_device, label):
    model, params, Hs, Ws, C, B, H, W, r = CASES[label]
    src, cam, fxo, fyo, want_image, want_cov, fragile = _reference(label)
    dev = hip_device
    assert fragile.mean() <= 0.01, f"{label}: {100 * fragile.mean():.2f} % of the pixels own a sub-sample at the border"
    bg = torch.tensor(BACKGROUND, device=dev)
    dev_src = torch.from_numpy(src.copy()).to(dev)
    camera = SourceCamera.from_colmap(model, params)
    image, coverage = prepare_images(dev_src, camera, H, W, fxo, fyo, bg)
    again = prepare_images(dev_src, camera, H, W, fxo, fyo, bg)
    assert image.shape == (B, 3, H, W) and coverage.shape == (B, H, W)
    assert np.array_equal(_bits(image), _bits(again[0])) and np.array_equal(_bits(coverage), _bits(again[1]))     # the same bits
    assert bool(torch.isfinite(image).all()) and bool(torch.isfinite(coverage).all())
    assert float(coverage.min()) >= 0.0 and float(coverage.max()) <= 1.0
    assert float(image.min()) >= 0.0 and float(image.max()) <= 1.0 + 1e-6
    stock_image, stock_cov = cr.stock_prepare(dev_src, cam, H, W, fxo, fyo, bg)
    keep = ~fragile
    err = lambda got, want: float(np.abs(got.double().cpu().numpy() - want)[..., keep].max()) if keep.any() else 0.0
    mine_i, stock_i = err(image, want_image), err(stock_image, want_image)
    mine_c, stock_c = err(coverage, want_cov), err(stock_cov, want_cov)
    S = cr.subsamples(cam, fxo, fyo)
    print(f"{label}: S={S} fragile {100 * fragile.mean():.3f} %  image err {mine_i:.3e} (stock {stock_i:.3e}, ratio "
          f"{mine_i / stock_i if stock_i else float('nan'):.3f})  coverage err {mine_c:.3e} (stock {stock_c:.3e})")
    assert stock_i < 1e-4                                      # the yardstick itself is sane
    assert mine_i <= 4.0 * stock_i
    assert mine_c <= 4.0 * stock_c
    zero = torch.from_numpy((want_cov[0] == 0) & keep).to(dev)          # where the photograph has nothing to say: exactly 0
    assert bool((coverage[:, zero] == 0).all()) and bool((image[:, :, zero] == 0).all())
    if label in UNCOVERED:
        assert int(zero.sum()) > 100


def test_seventeen_subsamples_are_refused_before_any_launch(hip_device):
    src = torch.zeros((1, 40, 40, 3), dtype=torch.uint8, device=hip_device)
    cam = SourceCamera(1, 170.0, 170.0, 20.0, 20.0)
    with pytest.raises(_lib.LsrError, match="unsupported"):
        prepare_images(src, cam, 2, 2, 10.0, 10.0)
    with pytest.raises(_lib.LsrError, match="unsupported"):
        subsamples(cam, 10.0, 10.0)
    assert subsamples(cam, 170.0 / 16, 170.0 / 16) == 16
    image, coverage = prepare_images(src + 255, cam, 2, 2, 170.0 / 16, 170.0 / 16)       # S = 16 runs
    assert bool((image == 1).all()) and bool((coverage == 1).all())
    assert _lib.load().lsr_last_hip_error() == 0
    for bad in (src.float(), src[0], src[..., :2]):
        with pytest.raises(_lib.LsrError):
            prepare_images(bad, cam, 2, 2, 170.0, 170.0)
    with pytest.raises(_lib.LsrError):
        prepare_images(src, cam, 2, 2, 170.0, 170.0, background=torch.zeros(4, device=hip_device))
    empty, cover = prepare_images(src[:0], cam, 2, 2, 170.0, 170.0)
    assert empty.shape == (0, 3, 2, 2) and cover.shape == (0, 2, 2)


def test_a_captured_graph_replays_the_launch(hip_device):
    label = "opencv_r2.5_rgba"
    model, params, Hs, Ws, C, B, H, W, r = CASES[label]
    src, cam, fxo, fyo, *_ = _reference(label)
    dev = hip_device
    bg = torch.tensor(BACKGROUND, device=dev)
    camera = SourceCamera.from_colmap(model, params)
    static = torch.from_numpy(src.copy()).to(dev)
    want = prepare_images(static, camera, H, W, fxo, fyo, bg)
    other = torch.from_numpy(_photos(B, Hs, Ws, C, seed=99)).to(dev)
    want_other = prepare_images(other, camera, H, W, fxo, fyo, bg)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        prepare_images(static, camera, H, W, fxo, fyo, bg)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = prepare_images(static, camera, H, W, fxo, fyo, bg)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(_bits(got[0]), _bits(want_other[0])) and np.array_equal(_bits(got[1]), _bits(want_other[1]))
