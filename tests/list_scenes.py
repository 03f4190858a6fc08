"""Scenes of hand-placed Gaussians whose half-tile render lists are known (tests/test_fwd_two_entries_gpu.py,
tests/test_record_forward_gpu.py).

View 0 looks down the z axis, so a Gaussian's pixel position and footprint are what the builder was asked for; view 1 is a
perturbed camera: the same Gaussians in lists nobody planned.  Every Gaussian has its own depth, so the order of the calls
is the order of the lists.
"""
import functools

import numpy as np
import torch

from latentsplat_amd.synthetic import FAR, NEAR, Scene, make_scene
from tests import util

S = 64            # default image: 4 x 4 tiles, 32 half-tile items per view
FX = 0.8          # normalised focal length of the synthetic cameras


class Builder:
    """Gaussians by pixel position of view 0, in the order they are added = depth order."""

    def __init__(self, seed, channels, size=S, dz=0.004):
        self.rows = []
        self.channels = channels
        self.gen = torch.Generator().manual_seed(seed)
        self.z = 2.0
        self.size = size
        self.dz = dz

    def add(self, px, py, sigma_px, opacity, feat=None):
        z = self.z
        self.z += self.dz        # every Gaussian its own depth: the sort order is the order of the calls
        n = self.size
        x, y = ((px + 0.5) / n - 0.5) / FX * z, ((py + 0.5) / n - 0.5) / FX * z
        s = sigma_px * z / (FX * n)
        f = torch.randn(self.channels, generator=self.gen) * 0.5 if feat is None else torch.full((self.channels,), float(feat))
        self.rows.append((x, y, z, s, opacity, f))
        return len(self.rows) - 1

    def scene(self, views=2):
        r = self.rows
        means = torch.tensor([[a[0], a[1], a[2]] for a in r], dtype=torch.float32)
        cov = torch.stack([torch.eye(3) * (a[3] * a[3]) for a in r]).float()
        opac = torch.tensor([a[4] for a in r], dtype=torch.float32)
        feat = torch.stack([a[5] for a in r])[:, :, None].float()
        cam = make_scene(1, image_size=self.size, views=2, color_sh_degree=None, feature_channels=None, seed=7)
        reps = -(-views // 2)
        ext, intr = cam.extrinsics.repeat(reps, 1, 1)[:views], cam.intrinsics.repeat(reps, 1, 1)[:views]    # copies of the two cameras
        return Scene(means, cov, opac, None, feat, ext, intr, torch.full((views,), NEAR), torch.full((views,), FAR))


def half_origin(tx, ty, h):
    return 16 * tx, 16 * ty + 8 * h


def narrow(b, tx, ty, h, g, n, opacity=0.02):
    """n Gaussians that reach only sub-block g (bit 4 * row + col) of half h of tile (tx, ty): centred between its four middle
    pixels, alpha >= 1/255 within 1.4 px.  Returns their indices."""
    x0, y0 = half_origin(tx, ty, h)
    return [b.add(x0 + 4 * (g & 3) + 1.5, y0 + 4 * (g >> 2) + 1.5, 0.5, opacity) for _ in range(n)]


def wide(b, cx, cy, sigma_px, opacity, n, jitter=0.0, feat=None):
    for i in range(n):
        # (centres on a small circle: neighbouring pixels get different alphas from entry to entry, so they stop at different entries)
        b.add(cx + jitter * np.cos(2.4 * i), cy + jitter * np.sin(2.4 * i), sigma_px, opacity, feat)


# half lists of ONE sub-block: every batch length nk the loop has to get right (1, 2, 3, 63, 64: odd ones are rounded up to
# the null record or the pad word) and every hn around the batch edges
SINGLE = [(1, 0), (2, 5), (3, 7), (63, 2), (64, 3), (65, 4), (66, 1), (67, 6), (127, 0), (128, 7), (129, 3)]   # (hn, sub-block)
# the eight sub-blocks of a half with different counts of both parities, the longest list odd; one batch and three batches
MIXED = [[5, 2, 7, 0, 3, 8, 1, 9], [33, 20, 11, 6, 17, 8, 2, 41]]


def place(k):
    """k-th designated half tile of a 64 x 64 image: the upper halves of the 16 tiles, then the lower ones."""
    return (k % 4, (k // 4) % 4, (k // 16) % 2)


@functools.lru_cache(maxsize=None)
def lengths_scene(channels):
    """(scene, boundary inputs, {(tx, ty, h): the eight sub-block list lengths}): nothing stops in this scene."""
    b = Builder(1, channels)
    plan = {}
    for k, (hn, g) in enumerate(SINGLE):
        tx, ty, h = place(k)
        narrow(b, tx, ty, h, g, hn)
        counts = [0] * 8
        counts[g] = hn
        plan[(tx, ty, h)] = counts
    for k, counts in enumerate(MIXED):
        tx, ty, h = place(len(SINGLE) + k)
        left = list(counts)
        while any(left):                    # round robin over the sub-blocks: every batch holds entries of all of them
            for g in range(8):
                if left[g]:
                    narrow(b, tx, ty, h, g, 1)
                    left[g] -= 1
        plan[(tx, ty, h)] = list(counts)
    sc = b.scene()
    return sc, util.boundary_inputs(sc, S, S, bg=(0.0, 0.0, 0.0)), plan


# the three designated halves of the stop scene: (tile x, tile y, half)
STACK, EDGE, EARLY = (0, 0, 0), (3, 0, 0), (1, 3, 1)


def add_stops(b, faint=0.012, early=5.0):
    """The three halves of the stop scene on builder ``b``; ``faint``: opacity of the 57 entries in front of the second stack,
    ``early``: x offset of the third half's centre (5.0: a pixel centre)."""
    # opaque stack: pixels run out at entries 5 ... 15 of the list, of both parities; behind it loud entries (feature 30) that
    # would show at once were one of them blended, or took the stop, after the pixel had stopped
    x0, y0 = half_origin(*STACK)
    wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.99, 10, jitter=4.0)
    wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.5, 6, feat=30.0)
    # 57 faint entries, then the stack: stops on both sides of the batch edge (entries 63 and 64)
    x0, y0 = half_origin(*EDGE)
    wide(b, x0 + 7.5, y0 + 7.5, 7.0, faint, 57)
    wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.99, 10, jitter=4.0)
    wide(b, x0 + 7.5, y0 + 7.5, 5.0, 0.5, 6, feat=30.0)
    # the earliest stop there is: two entries at the alpha clamp on a pixel centre leave T = 1e-4 within rounding (the second
    # entry of the list may stop that pixel: either way is right and the oracle marks the pixel fragile), the pixels around
    # it stop at the third entry
    x0, y0 = half_origin(*EARLY)
    wide(b, x0 + early, y0 + 3.0, 8.0, 0.99, 3)
    wide(b, x0 + early, y0 + 3.0, 8.0, 0.99, 3, jitter=2.0)
    wide(b, x0 + early, y0 + 3.0, 8.0, 0.5, 4, feat=30.0)


@functools.lru_cache(maxsize=None)
def stops_scene(channels):
    b = Builder(2, channels)
    add_stops(b)
    sc = b.scene()
    return sc, util.boundary_inputs(sc, S, S, bg=(0.0, 0.0, 0.0))


def half_entries(run, tx, ty, h, gx=4):
    """The words of view 0's render list of half h of tile (tx, ty)."""
    t = ty * gx + tx
    ts, hc, hl = run.tile_start(), run.half_count(), run.half_list()
    s0, n = ts[t], ts[t + 1] - ts[t]
    return hl[2 * s0 + h * n: 2 * s0 + h * n + hc[t, h]]


def stop_index(run, where, lists=None):
    """(8, 16) index in the half's list of the entry that stopped each pixel of view 0, or -1 where none did; the list length.
    ``lists``: the run to take the list structure from (default: ``run`` itself)."""
    tx, ty, h = where
    x0, y0 = half_origin(tx, ty, h)
    hn = len(half_entries(run if lists is None else lists, tx, ty, h))
    s = run.n_contrib()[0][y0:y0 + 8, x0:x0 + 16].astype(np.int64)
    return np.where(s < hn, s, -1), hn


# ---- lists whose entries contribute or not in chosen patterns (tests/test_record_forward_gpu.py) ----------------------------
# A CONTRIBUTING entry: sigma 0.5 px, opacity 0.02, centred between four pixels.  With the projection's low-pass the screen
# variance is 0.55 px^2 on the optical axis and up to 0.73 px^2 along the diagonal of a corner tile (perspective), so the
# four nearest pixels (d^2 = 0.5) see alpha = 0.02 exp(-0.25 / 0.55 ... 0.73) = 3.2 ... 3.6 / 255.
# A HIT-FREE entry: the same placement with an opacity that leaves those four pixels below 1/255 while the entry is still
# listed: its opacity is >= 1/255 and its footprint box (half width sqrt(2 ln(255 o) 0.55) + 0.05 px >= 0.5 from o = 0.0047)
# contains their centres.  0.008 would put 1.3 ... 1.45 / 255 on the four pixels — a faint contribution, not a hit-free
# entry; at 0.0048 they see 0.78 ... 0.87 / 255, and every alpha of the designated halves is more than 10 % away from 1/255
# (tests/test_record_ref_cpu.py checks it).
CONTRIBUTING, HIT_FREE = 0.02, 0.0048
LENGTHS = [1, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 129]      # per sub-block: both marking rounds of a lane (8 / 16 lanes to a group),
                                                              # the 32-iteration history register's edge, the batch edges
ALL_DIFFERENT = [33, 20, 11, 6, 17, 8, 2, 41]                 # one half, eight sub-block lists
# position j of a sub-block list of n entries contributes?
PATTERNS = {
    "all": lambda j, n: True,
    "none": lambda j, n: False,
    "first_of_chunk": lambda j, n: j % 32 == 0,
    "last_of_chunk": lambda j, n: j % 32 == 31 or j == n - 1,
    "alternating": lambda j, n: j % 2 == 0,
}
FINISHER = (3, 2, 0)       # the half of the stops scene that finishes in its first batch while its list has three
NARROWING_SCENES = list(PATTERNS) + ["stops"]


@functools.lru_cache(maxsize=None)
def narrowing_scene(name, channels):
    """(scene, boundary inputs, plan): plan = {(tx, ty, h): [(Gaussian, sub-block, contributes)] in list order} for the halves
    of view 0 whose lists are known entry by entry."""
    plan = {}
    if name == "stops":
        b = Builder(2, channels)
        # (faint = 0.012 leaves 0.98 / 255 on the corner pixels of the half.  early = 5.0 puts two entries AT the alpha clamp on a
        # pixel centre: T = 1e-4 within rounding behind them, a stop either way is right — and with 1 / (1 - alpha) = 100 the two
        # choices are gradients apart.  Half a pixel off, alpha is 0.9885 there, T = 1.3e-4 behind two entries, and the third stops it.)
        add_stops(b, faint=0.014, early=5.5)
        # 20 opaque entries over the whole half (alpha >= 0.38 on its farthest pixel: every pixel stops by entry 19), 150 loud ones behind
        x0, y0 = half_origin(*FINISHER)
        wide(b, x0 + 7.5, y0 + 3.5, 6.0, 0.99, 20)
        wide(b, x0 + 7.5, y0 + 3.5, 6.0, 0.5, 150, feat=30.0)
    else:
        b = Builder(3, channels)
        contributes = PATTERNS[name]
        for k, n in enumerate(LENGTHS):
            tx, ty, h = place(k)
            g = (3 * k) % 8
            plan[(tx, ty, h)] = [(narrow(b, tx, ty, h, g, 1, CONTRIBUTING if contributes(j, n) else HIT_FREE)[0], g, contributes(j, n))
                                 for j in range(n)]
        tx, ty, h = place(len(LENGTHS))
        at, entries = [0] * 8, []
        while any(at[g] < ALL_DIFFERENT[g] for g in range(8)):      # round robin: every batch holds entries of all sub-blocks
            for g in range(8):
                if at[g] < ALL_DIFFERENT[g]:
                    c = contributes(at[g], ALL_DIFFERENT[g])
                    entries.append((narrow(b, tx, ty, h, g, 1, CONTRIBUTING if c else HIT_FREE)[0], g, c))
                    at[g] += 1
        plan[(tx, ty, h)] = entries
    sc = b.scene()
    return sc, util.boundary_inputs(sc, S, S, bg=(0.0, 0.0, 0.0)), plan


def designated(name, plan):
    return list(plan) if name != "stops" else [STACK, EDGE, EARLY, FINISHER]


def alpha_margin(bi, halves):
    """Smallest |255 alpha - 1| over every (entry of the tile's list, pixel) of the given halves of view 0, in float64 from the
    oracle's projection — on the CPU, before anything runs on the GPU."""
    o = util.oracle_forward(bi, 0)
    xy, co = o["xy"].astype(np.float64), o["conic_opacity"].astype(np.float64)
    worst = np.inf
    for tx, ty, h in halves:
        s0, s1 = o["ranges"][ty * (S // 16) + tx]
        lst = o["point_list"][s0:s1].astype(np.int64)
        x0, y0 = half_origin(tx, ty, h)
        dx = xy[lst, 0][:, None, None] - (x0 + np.arange(16.0))[None, None, :]
        dy = xy[lst, 1][:, None, None] - (y0 + np.arange(8.0))[None, :, None]
        A, B, C, op = (co[lst, k][:, None, None] for k in range(4))
        alpha = op * np.exp(-0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy)
        worst = min(worst, float(np.abs(255.0 * alpha - 1.0).min(initial=np.inf)))
    return worst


# ---- random scenes whose narrowed bits are checked exactly: the cases of test_forward_for_backward_narrows_the_render_lists_losslessly
# (tests/test_parity_gpu.py), at their sizes and seeds ------------------------------------------------------------------------
RANDOM_CASES = {
    "feat4_v4": dict(G=30_000, size=96, views=4, color_sh_degree=None, feature_channels=4),
    "rgb_feat4_ragged_v3": dict(G=14_000, size=(80, 112), views=3, color_sh_degree=2, feature_channels=4),
    "long_lists_v4": dict(G=4_000, size=64, views=4, color_sh_degree=None, feature_channels=4, sigma_px=(3.0, 25.0), opacity_scale=1.0),
}


def random_inputs(case):
    case = dict(case)
    size = case.pop("size")
    H, W = size if isinstance(size, tuple) else (size, size)
    sc = make_scene(case.pop("G"), image_size=max(H, W), **case)
    return util.boundary_inputs(sc, H, W, bg=(0.3, 0.2, 0.1))
