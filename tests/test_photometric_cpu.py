"""The photometric loss without a GPU: the float64 restatement (tests/photometric_ref.py) against torch's float64 conv2d
composition and autograd, its metric mode against the scipy filter skimage calls, and the host-only behaviour of the C ABI
(include/lsr_loss.h)."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import photometric_ref as ref

SHAPES = [(1, 1, 1, 1), (1, 3, 7, 5), (2, 3, 11, 11), (2, 3, 20, 23), (1, 2, 37, 53)]


def _f64(a):
    return torch.from_numpy(a.astype(np.float64))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_restatement_matches_the_float64_composition(shape, kind):
    x, y = ref.make_pair(shape, kind, seed=sum(shape))
    for lam in (0.0, 0.2, 1.0):
        got, want = ref.results(x, y, lam), ref.stock_results(_f64(x), _f64(y), lam, grad=False)
        for k in ("loss", "l1", "ssim", "map"):
            assert np.abs(got[k] - want[k]).max() <= 1e-12, (k, lam)
    # the metric's constants
    if min(shape[2:]) >= 11:
        got, want = ref.results(x, y, 1.0, 121 / 120, 5), ref.stock_results(_f64(x), _f64(y), 1.0, 121 / 120, 5, grad=False)
        assert np.abs(got["ssim"] - want["ssim"]).max() <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_analytic_gradient_matches_float64_autograd(shape, kind):
    x, y = ref.make_pair(shape, kind, seed=1 + sum(shape))
    for lam in (0.0, 0.2, 1.0):
        want = ref.stock_results(_f64(x), _f64(y), lam)["grad"]
        got = ref.gradient(x, y, lam)
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), lam


def test_metric_mode_matches_the_scipy_filter():
    """skimage's structural_similarity(win_size=11, gaussian_weights=True, data_range=1) filters with
    scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5, mode="reflect"), takes sample covariances and averages the map
    without its 5-pixel border: the pin is to that formula (skimage itself is not a dependency)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    x, y = ref.make_pair((2, 3, 24, 31), "noise", seed=5)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    f = lambda a: ndimage.gaussian_filter(a, 1.5, truncate=3.5, mode="reflect")
    cn = 121 / 120
    want = np.zeros(2)
    for v in range(2):
        for c in range(3):
            X, Y = x64[v, c], y64[v, c]
            ux, uy = f(X), f(Y)
            vx, vy, vxy = cn * (f(X * X) - ux * ux), cn * (f(Y * Y) - uy * uy), cn * (f(X * Y) - ux * uy)
            S = ((2 * ux * uy + ref.C1) * (2 * vxy + ref.C2)) / ((ux ** 2 + uy ** 2 + ref.C1) * (vx + vy + ref.C2))
            want[v] += S[5:-5, 5:-5].mean() / 3
    got = ref.results(x, y, 1.0, cn, 5)["ssim"]
    assert np.abs(got - want).max() <= 1e-12


# ---- what the GPU test's shapes reach ----

# shape of tests/test_photometric_gpu.py SHAPES -> (photo_shift, slots per image, (tiles_y, tiles_x)), worked out by hand from
# csrc/photometric.hip: share = H W / ((H + 10)(W + 10)), shift = floor(4 share + 0.5) / 8, one slot per 32 x 32 tile of every
# plane.  A shape that is dropped or "simplified" has to be taken out of this table too, and the coverage below then says
# what is lost.
REACHED = {
    (1, 1, 1, 1): (0.0, 1, (1, 1)),
    (1, 3, 7, 5): (0.125, 3, (1, 1)),
    (2, 3, 11, 11): (0.125, 3, (1, 1)),
    (1, 3, 10, 12): (0.125, 3, (1, 1)),
    (2, 3, 37, 53): (0.375, 12, (2, 2)),
    (3, 1, 64, 64): (0.375, 4, (2, 2)),
    (1, 4, 33, 17): (0.25, 8, (2, 1)),
    (1, 2, 31, 32): (0.25, 2, (1, 1)),
    (1, 2, 32, 33): (0.25, 4, (1, 2)),
    (1, 2, 33, 31): (0.25, 4, (2, 1)),
    (1, 3, 160, 160): (0.5, 75, (5, 5)),
    (2, 3, 96, 352): (0.5, 99, (3, 11)),
    (1, 1, 33, 2081): (0.375, 132, (2, 66)),
    (17, 1, 7, 5): (0.125, 1, (1, 1)),
    (33, 2, 11, 11): (0.125, 2, (1, 1)),
}


def test_the_gpu_shapes_reach_every_trip_count_of_a_full_size_fit():
    from tests.test_photometric_gpu import FULL_SIZE, SHAPES
    assert ref.TILE == 32 and ref.WAVE == 64 and ref.FINISH_WAVES == 16
    assert sorted(SHAPES) == sorted(REACHED) and len(set(SHAPES)) == len(SHAPES)
    for shape in SHAPES:
        shift, slots, tiles = REACHED[shape]
        assert ref.photo_shift(*shape[2:]) == shift, shape
        assert ref.slots_per_image(shape) == slots, shape
        assert ref.tile_grid(*shape[2:]) == tiles, shape
    # the shift: every value it takes; 0.5 from 145 px a side, and at every larger square image
    assert {ref.photo_shift(*s[2:]) for s in SHAPES} == {0.0, 0.125, 0.25, 0.375, 0.5}
    assert ref.photo_shift(144, 144) == 0.375 and all(ref.photo_shift(s, s) == 0.5 for s in (145, 256, 800, 4000))
    assert ref.photo_shift(64, 64) == 0.375 and REACHED[FULL_SIZE][0] == 0.5
    # k_photo_finish: lanes that take a second slot of an image, and a third; waves that take a second image, and a third
    slots = [ref.slots_per_image(s) for s in SHAPES]
    assert any(ref.WAVE < n <= 2 * ref.WAVE for n in slots) and any(n > 2 * ref.WAVE for n in slots)
    assert any(ref.FINISH_WAVES < s[0] <= 2 * ref.FINISH_WAVES for s in SHAPES) and any(s[0] > 2 * ref.FINISH_WAVES for s in SHAPES)
    # an interior tile, whose 42 x 42 halo lies wholly inside the image: tile 1 covers 32..63 and reads 27..68, each way
    assert any(min(ref.tile_grid(*s[2:])) >= 3 and min(s[2:]) >= 2 * ref.TILE + ref.R for s in SHAPES)
    # partial tiles both ways next to the long row of tiles
    assert any(ref.slots_per_image(s) > 2 * ref.WAVE and s[2] % ref.TILE and s[3] % ref.TILE for s in SHAPES)


# ---- host-only ABI ----

def _dims(**kw):
    base = dict(num_images=2, channels=3, height=37, width=53, lambda_dssim=0.2, cov_norm=1.0, crop=0, reserved0=0)
    base.update(kw)
    return _lib.PhotometricDims(**base)


INVALID = [dict(num_images=0), dict(channels=0), dict(height=0), dict(width=-1), dict(lambda_dssim=-0.1), dict(lambda_dssim=1.5),
           dict(lambda_dssim=float("nan")), dict(cov_norm=0.0), dict(cov_norm=-1.0), dict(cov_norm=float("inf")),
           dict(cov_norm=float("nan")), dict(crop=1), dict(crop=-5), dict(crop=5, height=10), dict(crop=5, width=10),
           dict(reserved0=1)]


@pytest.mark.parametrize("bad", INVALID)
def test_invalid_dims_are_refused_before_any_gpu_work(bad):
    lib = _lib.load()
    d = _dims(**bad)
    assert lib.lsr_photometric_workspace_bytes(C.byref(d)) == 0
    host = (C.c_float * 16)()          # never touched: the calls return before any GPU work
    p = C.cast(host, C.c_void_p)
    assert lib.lsr_photometric_forward(C.byref(d), p, p, p, p, None, None, None, None, None) == -1
    assert lib.lsr_photometric_backward(C.byref(d), p, p, p, p, p, None) == -1


def test_saved_maps_need_the_loss_mode():
    lib = _lib.load()
    host = (C.c_float * 16)()
    p = C.cast(host, C.c_void_p)
    for d in (_dims(crop=5), _dims(cov_norm=121 / 120)):
        assert lib.lsr_photometric_workspace_bytes(C.byref(d)) > 0                  # fine as a metric ...
        assert lib.lsr_photometric_forward(C.byref(d), p, p, p, p, None, None, None, p, None) == -1   # ... not with `saved`
        assert lib.lsr_photometric_backward(C.byref(d), p, p, p, p, p, None) == -1


def test_null_pointers_are_refused_before_any_gpu_work():
    lib = _lib.load()
    d = _dims()
    host = (C.c_float * 16)()
    p = C.cast(host, C.c_void_p)
    assert lib.lsr_photometric_workspace_bytes(None) == 0
    assert lib.lsr_photometric_forward(None, p, p, p, p, None, None, None, None, None) == -2
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.lsr_photometric_forward(C.byref(d), *args, p, None, None, None, None, None) == -2
    assert lib.lsr_photometric_backward(None, p, p, p, p, p, None) == -2
    for i in range(5):
        args = [p] * 5
        args[i] = None
        assert lib.lsr_photometric_backward(C.byref(d), *args, None) == -2


def test_too_many_values_are_unsupported():
    lib = _lib.load()
    d = _dims(num_images=8, channels=4, height=8192, width=8192)       # 2^31 values
    host = (C.c_float * 16)()
    p = C.cast(host, C.c_void_p)
    assert lib.lsr_photometric_workspace_bytes(C.byref(d)) == 0
    assert lib.lsr_photometric_forward(C.byref(d), p, p, p, p, None, None, None, None, None) == -5
    assert lib.lsr_photometric_backward(C.byref(d), p, p, p, p, p, None) == -5


def test_workspace_bytes_are_positive_and_monotone():
    lib = _lib.load()
    size = lambda **kw: lib.lsr_photometric_workspace_bytes(C.byref(_dims(**kw)))
    assert size() == size() > 0
    assert size(num_images=1, channels=1, height=1, width=1) > 0
    for key, values in (("num_images", (1, 2, 3, 16, 200)), ("height", (1, 31, 32, 33, 64, 65, 1024, 4000)),
                        ("width", (1, 31, 32, 33, 64, 65, 1024, 4000))):
        sizes = [size(**{key: v}) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], (key, sizes)
    # one pair of doubles per 32 x 32 tile of every plane
    assert size(num_images=16, channels=3, height=256, width=256) >= 16 * 3 * 8 * 8 * 16
    # lambda, and the metric's constants, do not change it
    assert size(lambda_dssim=1.0) == size(cov_norm=121 / 120, crop=5) == size()


def test_product_path_refuses_cpu_tensors():
    from latentsplat_amd import compute_ssim, l1, photometric_loss, ssim
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    for fn in (photometric_loss, ssim, l1, compute_ssim):
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            fn(a, b)
