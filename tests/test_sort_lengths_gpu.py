"""k_sort_tiles at every list length and key range at which its per-tile work changes shape.

The sort stops its per-thread key loops at the end of the list (`nq = ceil(n / 512)` live slots per thread), fixes the
bucket shift from the depth words alone (with the exact 64-bit range behind a branch when the depth words span fewer
values than there are buckets) and reads the sub-block masks of the half-tile render lists from a table.  What can go
wrong is therefore tied to the list length around multiples of the workgroup size, to the tier edges and to the key
range — not to scale: every case is ONE 16x16 view (one tile) holding a few thousand Gaussians.

References that do not run the code under test: the oracle's canonical list, and a numpy restatement of span_code /
code_mask (lsr_blend.h) applied to the span bytes the projection kernel left in the binning records."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

LENGTHS = [2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1536, 2047, 2048, 2049, 3000, 4095, 4096, 4097, 8192, 8193]
RANGES = [("equal", 1500), ("ulps", 1500), ("outlier", 1500), ("outlier", 3000)]


def _one_tile_scene(G, depths=None, seed=11):
    """G Gaussians on the one tile of a 16x16 view, footprints of about a pixel (the recipe of
    test_every_sort_tier_in_one_call; the centres are spread over the middle of the tile rather than over one pixel, so
    that the entries differ in the sub-blocks and halves they reach).  `depths` replaces the depths; the covariances are
    rescaled with them so that the footprints keep their size in pixels."""
    gen = torch.Generator().manual_seed(seed)
    sc = util.make_scene(G, image_size=16, views=1, color_sh_degree=None, feature_channels=4, seed=seed,
                         sigma_px=(0.3, 0.6), opacity_scale=0.02)
    z_old = sc.means[:, 2].clone()
    z = z_old if depths is None else depths.float()
    sc.means[:, 0] = (torch.rand(G, generator=gen) * 0.6 - 0.3) / 0.8 * z
    sc.means[:, 1] = (torch.rand(G, generator=gen) * 0.6 - 0.3) / 0.8 * z
    sc.means[:, 2] = z
    sc.covariances = sc.covariances * ((z / z_old) ** 2)[:, None, None]
    return sc


def _range_depths(kind, G):
    rng = np.random.default_rng(5)
    if kind == "equal":        # one depth word: only the index words tell the keys apart
        z = np.full(G, 5.0, np.float32)
    elif kind == "ulps":       # eight neighbouring floats: the depth words span far fewer values than the sort has buckets
        z = (np.full(G, 5.0, np.float32).view(np.uint32) + rng.integers(0, 8, G).astype(np.uint32)).view(np.float32)
    else:                      # a cluster 2^13 ulps wide and one Gaussian at ten times the depth: the cluster shares a bucket
        z = (5.0 + 0.0039 * rng.random(G)).astype(np.float32)
        z[G // 3] = 50.0
    return torch.from_numpy(z.copy())


def _code_masks(span):
    """(n, 4) span bytes x0, x1, y0, y1 of a pair whose tile is the first of its rectangle -> 16-bit sub-block masks
    (span_code with dx = dy = 0, then code_mask)."""
    x0, x1, y0, y1 = (span[:, k].astype(np.int64) for k in range(4))
    c0, c1 = np.maximum(0, x0), np.where(x1 == 255, 3, np.minimum(3, x1))
    r0, r1 = np.maximum(0, y0), np.where(y1 == 255, 3, np.minimum(3, y1))
    some = (x0 <= x1) & (c0 <= c1) & (r0 <= r1)
    code = np.where(some, c0 | (c1 << 2) | (r0 << 4) | (r1 << 6), 0x11)
    c0, c1, r0, r1 = code & 3, (code >> 2) & 3, (code >> 4) & 3, (code >> 6) & 3
    cols = np.where(c0 <= c1, (2 << c1) - (1 << c0), 0)
    rows = np.where(r0 <= r1, (2 << r1) - (1 << r0), 0)
    spread = (rows & 1) | ((rows & 2) << 3) | ((rows & 4) << 6) | ((rows & 8) << 9)     # row r -> bit 4r
    return cols * spread


def _check(hip_device, G, depths=None):
    sc = _one_tile_scene(G, depths)
    bi = util.boundary_inputs(sc, 16, 16)
    run = util.HipRun(bi, hip_device)
    ts = run.tile_start()
    assert np.diff(ts)[0] == G and run.T == 1, "the scene does not put every Gaussian on the tile"
    o = util.oracle_forward(bi, 0)
    canon = run.point_list()[:G]
    np.testing.assert_array_equal(canon, o["point_list"])
    # half lists: the canonical list restricted to the entries whose half mask is not zero, in order, with those bits
    assert run.layout.geom_bin_stride == 12
    rec = run._view(run.geom, run.layout.geom_bin, G * 12, torch.uint8).cpu().numpy().reshape(G, 12)
    assert (rec[canon, 0:2] == 0).all()                      # the tile is the first of every rectangle
    m16 = _code_masks(rec[canon, 8:12])
    hc, hl = run.half_count(), run.half_list()
    for h in range(2):
        bits = (m16 >> (8 * h)) & 0xFF
        want = (canon[bits != 0] | (bits[bits != 0] << 24)).astype(np.uint32)
        assert hc[0, h] == len(want), (h, int(hc[0, h]), len(want))
        np.testing.assert_array_equal(hl[h * G: h * G + len(want)], want)
    if G >= 64:   # the scene exercises what the lists can hold: entries of one half only, of both, and of neither
        assert ((m16 & 0xFF) == 0).any() and ((m16 >> 8) == 0).any() and ((m16 & 0xFF != 0) & (m16 >> 8 != 0)).any() and (m16 == 0).any()
    np.testing.assert_allclose(run.feat_out[0].cpu().numpy(), o["feature"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(run.mask_out[0].cpu().numpy(), o["mask"], atol=1e-4, rtol=0)
    return o


@pytest.mark.parametrize("G", LENGTHS)
def test_sort_list_lengths(hip_device, G):
    """Every first-tier instance (1024 / 2048 / 4096 keys), every number of live key slots per thread, one key more and
    one fewer than a multiple of the workgroup, and the hand-over to both persistent tiers (4097, 8192, 8193)."""
    _check(hip_device, G)


@pytest.mark.parametrize("kind,G", RANGES)
def test_sort_key_ranges(hip_device, kind, G):
    """Depth words that are all equal or a few ulps apart (the exact 64-bit key range has to run, or the keys share one
    bucket), and a cluster plus a far outlier (a bucket beyond the in-bucket pass: the bitonic network; at 3000 keys its
    padded list is longer than 2048)."""
    o = _check(hip_device, G, _range_depths(kind, G))
    words = np.unique(o["gdepth"].view(np.uint32))
    if kind == "equal":
        assert len(words) == 1
    elif kind == "ulps":
        assert 1 < len(words) < 1024
    else:
        lo, hi = int(words[0]), int(words[-1])
        assert hi - lo >= 2048        # the coarse range is the one in use, and the cluster fits one bucket of it:
        width = 1 << max(0, (hi - lo).bit_length() - 11)     # (2048 buckets: a bucket is this many depth words wide)
        assert int(words[-2]) - lo < width
