"""The half-tile compositing kernel's inner loop takes two sub-block-list entries per trip (the plain 4- and 8-channel
instances, latentsplat_amd/csrc/render_forward.hip): scenes of hand-placed Gaussians whose list structure is known, against the CPU
oracle with the helpers and bars of tests/test_parity_gpu.py (images 1e-4 abs, n_contrib exact outside fragile pixels,
final_T = 1 - mask).

View 0 looks down the z axis, so a Gaussian's pixel position and footprint are what the scene builder asked for and the
tests assert the list structure they were built for (list lengths, sub-block bits, where pixels stop) before they
compare anything.  View 1 is a perturbed camera: the same Gaussians in lists nobody planned.
"""
import functools

import numpy as np
import pytest
import torch

from latentsplat_amd.synthetic import FAR, NEAR, Scene, make_scene
from tests import util
from tests.test_parity_gpu import _check_forward

pytestmark = pytest.mark.gpu

S = 64            # image: 4 x 4 tiles, 32 half-tile items per view
FX = 0.8          # normalised focal length of the synthetic cameras


class _Builder:
    """Gaussians by pixel position of view 0, in the order they are added = depth order."""

    def __init__(self, seed, channels):
        self.rows = []
        self.channels = channels
        self.gen = torch.Generator().manual_seed(seed)
        self.z = 2.0

    def add(self, px, py, sigma_px, opacity, feat=None):
        z = self.z
        self.z += 0.004          # every Gaussian its own depth: the sort order is the order of the calls
        x, y = ((px + 0.5) / S - 0.5) / FX * z, ((py + 0.5) / S - 0.5) / FX * z
        s = sigma_px * z / (FX * S)
        f = torch.randn(self.channels, generator=self.gen) * 0.5 if feat is None else torch.full((self.channels,), float(feat))
        self.rows.append((x, y, z, s, opacity, f))

    def scene(self):
        r = self.rows
        means = torch.tensor([[a[0], a[1], a[2]] for a in r], dtype=torch.float32)
        cov = torch.stack([torch.eye(3) * (a[3] * a[3]) for a in r]).float()
        opac = torch.tensor([a[4] for a in r], dtype=torch.float32)
        feat = torch.stack([a[5] for a in r])[:, :, None].float()
        cam = make_scene(1, image_size=S, views=2, color_sh_degree=None, feature_channels=None, seed=7)
        return Scene(means, cov, opac, None, feat, cam.extrinsics, cam.intrinsics, torch.full((2,), NEAR), torch.full((2,), FAR))


def _half_origin(tx, ty, h):
    return 16 * tx, 16 * ty + 8 * h


def _narrow(b, tx, ty, h, g, n, opacity=0.02):
    """n Gaussians that reach only sub-block g (bit 4 * row + col) of half h of tile (tx, ty): centred between its four middle
    pixels, alpha >= 1/255 within 1.4 px."""
    x0, y0 = _half_origin(tx, ty, h)
    for _ in range(n):
        b.add(x0 + 4 * (g & 3) + 1.5, y0 + 4 * (g >> 2) + 1.5, 0.5, opacity)


# half lists of ONE sub-block: every batch length nk the loop has to get right (1, 2, 3, 63, 64: odd ones are rounded up to
# the null record or the pad word) and every hn around the batch edges
SINGLE = [(1, 0), (2, 5), (3, 7), (63, 2), (64, 3), (65, 4), (66, 1), (67, 6), (127, 0), (128, 7), (129, 3)]   # (hn, sub-block)
# the eight sub-blocks of a half with different counts of both parities, the longest list odd; one batch and three batches
MIXED = [[5, 2, 7, 0, 3, 8, 1, 9], [33, 20, 11, 6, 17, 8, 2, 41]]


def _place(k):
    """k-th designated half tile: the upper half of the k-th tile."""
    return (k % 4, (k // 4) % 4, (k // 16) % 2)


CHANNELS = [4, 8]      # the two instances with the two-entry loop


@functools.lru_cache(maxsize=None)
def _lengths_scene(channels):
    b = _Builder(1, channels)
    plan = {}
    for k, (hn, g) in enumerate(SINGLE):
        tx, ty, h = _place(k)
        _narrow(b, tx, ty, h, g, hn)
        counts = [0] * 8
        counts[g] = hn
        plan[(tx, ty, h)] = counts
    for k, counts in enumerate(MIXED):
        tx, ty, h = _place(len(SINGLE) + k)
        left = list(counts)
        while any(left):                    # round robin over the sub-blocks: every batch holds entries of all of them
            for g in range(8):
                if left[g]:
                    _narrow(b, tx, ty, h, g, 1)
                    left[g] -= 1
        plan[(tx, ty, h)] = list(counts)
    sc = b.scene()
    return sc, util.boundary_inputs(sc, S, S, bg=(0.0, 0.0, 0.0)), plan


def _half_entries(run, tx, ty, h):
    """The words of view 0's render list of half h of tile (tx, ty)."""
    t = ty * 4 + tx
    ts, hc, hl = run.tile_start(), run.half_count(), run.half_list()
    s0, n = ts[t], ts[t + 1] - ts[t]
    return hl[2 * s0 + h * n: 2 * s0 + h * n + hc[t, h]]


def _forward_checked(hip_device, bi):
    from latentsplat_amd import _lib
    try:
        _lib.set_knob("LSR_FWD_ROWS", 0)      # the half-tile kernel, however few items the call has
        run = util.HipRun(bi, hip_device)
    finally:
        _lib.set_knob("LSR_FWD_ROWS", -1)
    _check_forward(bi, run)
    assert np.allclose(1.0 - run.mask_out.cpu().numpy(), run.final_T(), atol=1e-6)
    return run


@pytest.mark.parametrize("channels", CHANNELS)
def test_list_lengths_of_both_parities_and_batch_edges(hip_device, channels):
    sc, bi, plan = _lengths_scene(channels)
    run = _forward_checked(hip_device, bi)
    seen_nk = set()
    for (tx, ty, h), counts in plan.items():
        bits = (_half_entries(run, tx, ty, h) >> 24) & 0xFF
        assert len(bits) == sum(counts), (tx, ty, h, len(bits))
        per_block = np.stack([(bits >> g) & 1 for g in range(8)])                 # (8, hn)
        np.testing.assert_array_equal(per_block.sum(1), counts, err_msg=f"sub-block list lengths of half {(tx, ty, h)}")
        assert (per_block.sum(0) == 1).all(), "every entry was placed on one sub-block"
        for base in range(0, len(bits), 64):
            seen_nk.add(int(per_block[:, base:base + 64].sum(1).max()))
    assert {1, 2, 3, 63, 64} <= seen_nk, seen_nk
    assert any(max(c) % 2 == 1 and len({x % 2 for x in c if x}) == 2 for c in MIXED)
    # every pixel of a designated sub-block saw all of its half's entries (nothing stops in this scene)
    nc = run.n_contrib()[0]
    for (tx, ty, h), counts in plan.items():
        x0, y0 = _half_origin(tx, ty, h)
        assert (nc[y0:y0 + 8, x0:x0 + 16] == sum(counts)).all()


def _wide(b, cx, cy, sigma_px, opacity, n, jitter=0.0, feat=None):
    for i in range(n):
        # (centres on a small circle: neighbouring pixels get different alphas from entry to entry, so they stop at different entries)
        b.add(cx + jitter * np.cos(2.4 * i), cy + jitter * np.sin(2.4 * i), sigma_px, opacity, feat)


# the three designated halves of the stop scene: (tile x, tile y, half)
STACK, EDGE, EARLY = (0, 0, 0), (3, 0, 0), (1, 3, 1)


@functools.lru_cache(maxsize=None)
def _stops_scene(channels):
    b = _Builder(2, channels)
    # opaque stack: pixels run out at entries 5 ... 15 of the list, of both parities; behind it loud entries (feature 30) that
    # would show at once were one of them blended, or took the stop, after the pixel had stopped
    x0, y0 = _half_origin(*STACK)
    _wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.99, 10, jitter=4.0)
    _wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.5, 6, feat=30.0)
    # 57 faint entries, then the stack: stops on both sides of the batch edge (entries 63 and 64)
    x0, y0 = _half_origin(*EDGE)
    _wide(b, x0 + 7.5, y0 + 7.5, 7.0, 0.012, 57)
    _wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.99, 10, jitter=4.0)
    _wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.5, 6, feat=30.0)
    # the earliest stop there is: two entries at the alpha clamp on a pixel centre leave T = 1e-4 within rounding (the second
    # entry of the list may stop that pixel: either way is right and the oracle marks the pixel fragile), the pixels around
    # it stop at the third entry
    x0, y0 = _half_origin(*EARLY)
    _wide(b, x0 + 5.0, y0 + 3.0, 8.0, 0.99, 3)
    _wide(b, x0 + 5.0, y0 + 3.0, 8.0, 0.99, 3, jitter=2.0)
    _wide(b, x0 + 5.0, y0 + 3.0, 8.0, 0.5, 4, feat=30.0)
    sc = b.scene()
    return sc, util.boundary_inputs(sc, S, S, bg=(0.0, 0.0, 0.0))


def _stop_index(run, where):
    """(8, 16) index in the half's list of the entry that stopped each pixel of view 0, or -1 where none did; the list length."""
    tx, ty, h = where
    x0, y0 = _half_origin(tx, ty, h)
    hn = len(_half_entries(run, tx, ty, h))
    s = run.n_contrib()[0][y0:y0 + 8, x0:x0 + 16].astype(np.int64)
    return np.where(s < hn, s, -1), hn


@pytest.mark.parametrize("channels", CHANNELS)
def test_stops_at_either_entry_of_a_trip(hip_device, channels):
    sc, bi = _stops_scene(channels)
    run = _forward_checked(hip_device, bi)
    for where, hn in ((STACK, 16), (EDGE, 73), (EARLY, 10)):
        words = _half_entries(run, *where)
        assert len(words) == hn, (where, len(words))
        # every entry is on every sub-block's list: the position in a sub-block list is the position in the half's list, and
        # the entries at even positions of a batch are the first of their trip, those at odd positions the second
        assert (((words >> 24) & 0xFF) == 0xFF).all(), where
    # the two pixels of a lane, over the three halves (64 is even: the trips of a batch pair the positions (2k, 2k + 1) of the list)
    stops = {where: _stop_index(run, where)[0] for where in (STACK, EDGE, EARLY)}
    a = np.concatenate([s[:, 0::2].ravel() for s in stops.values()])
    b = np.concatenate([s[:, 1::2].ravel() for s in stops.values()])
    both = (a >= 0) & (b >= 0)
    assert (both & (a // 2 == b // 2) & (a != b)).any(), "no lane whose pixels stop at the two entries of one trip"
    assert (both & (a == b) & (a % 2 == 0)).any() and (both & (a == b) & (a % 2 == 1)).any(), "no lane whose pixels stop at the same entry"
    assert (both & (a // 2 != b // 2)).any(), "no lane whose pixels stop in different trips"
    s = stops[EDGE]
    assert (s == 63).any() and (s == 64).any(), ("no stop at the last entry of a batch and the first of the next", np.unique(s))
    s = stops[EARLY]
    assert (s == 2).any() and s[s >= 0].min() >= 1, np.unique(s)
