"""tests/record_ref.py (the reference of tests/test_record_forward_gpu.py) on hand-written arrays, and against a scalar
pixel-by-pixel restatement of the RECORD / REC bookkeeping of latentsplat_amd/csrc/render_forward.hip on a one-tile scene."""
import numpy as np
import pytest

from tests import record_ref as rr
from tests import util
from tests.list_scenes import NARROWING_SCENES, RANDOM_CASES, alpha_margin, designated, narrowing_scene, random_inputs

H = W = 16      # one tile, one view


def _records(rows):
    """rows of (x, y, sigma2, opacity) -> HipRun.q()-shaped records of one view (isotropic conics)."""
    r = np.asarray(rows, np.float64)
    q0 = np.stack([r[:, 0], r[:, 1], 1.0 / r[:, 2], np.zeros(len(r))], 1).astype(np.float32)[None]
    q1 = np.stack([1.0 / r[:, 2], r[:, 3], np.full(len(r), 2.0), np.zeros(len(r))], 1).astype(np.float32)[None]
    return q0, q1


def _lists(upper, lower=()):
    """One tile whose canonical list has max(len) entries; upper / lower: (index, footprint bits) per entry of the half list."""
    n = max(len(upper), len(lower))
    hl = np.zeros(2 * n, np.uint32)
    for h, ent in enumerate((upper, lower)):
        for i, (g, bits) in enumerate(ent):
            hl[h * n + i] = g | (bits << 24)
    return np.array([0, n], np.int64), np.array([[len(upper), len(lower)]], np.int64), hl


def test_bits_follow_the_pixels_that_keep_the_entry():
    # a 0.74 px Gaussian between pixels (1, 1) ... (2, 2): sub-block 0 only, whatever the footprint bits claim
    q = _records([(1.5, 1.5, 0.55, 0.02), (5.5, 5.5, 0.55, 0.02)])
    lists = _lists([(0, 0xFF), (1, 0x33), (0, 0x01)])
    nc = np.full((1, H, W), 3)
    must, may = rr.expected_bits(lists, nc, q, H, W)
    np.testing.assert_array_equal(must[:3], [0x01, 0x20, 0x01])      # (5.5, 5.5) is in sub-block (1, 1) = bit 5, which 0x33 covers
    np.testing.assert_array_equal(may, must)
    # the pixels of sub-block 0 stopped AT entry 2: they blended entries 0 and 1 only
    nc[0, :4, :4] = 2
    must, may = rr.expected_bits(lists, nc, q, H, W)
    np.testing.assert_array_equal(must[:3], [0x01, 0x20, 0x00])
    np.testing.assert_array_equal(may, must)
    # a footprint bit that is not set is never expected, even where a pixel would keep the entry
    must, may = rr.expected_bits(_lists([(0, 0xFE)]), np.ones((1, H, W), np.int64), q, H, W)
    assert must[0] == 0 and may[0] == 0


def test_alpha_window_separates_must_and_may():
    # centred on pixel (1, 1): alpha there is the opacity itself; the other pixels see 0.16 of it
    lo, mid, hi = (np.float32(rr.ALPHA_MIN * (1 + k)) for k in (-3e-5, 2e-6, 3e-5))
    q = _records([(1.0, 1.0, 0.55, lo), (1.0, 1.0, 0.55, mid), (1.0, 1.0, 0.55, hi)])
    must, may = rr.expected_bits(_lists([(0, 1), (1, 1), (2, 1)]), np.full((1, H, W), 3), q, H, W)
    np.testing.assert_array_equal(must[:3], [0, 0, 1])
    np.testing.assert_array_equal(may[:3], [0, 1, 1])


def test_unprocessed_batches_keep_or_lose_their_bits():
    q = _records([(1.5, 1.5, 0.55, 0.02)])
    lists = _lists([(0, 0x13)] * 130, [(0, 0x01)] * 3)
    nc = np.zeros((1, H, W), np.int64)
    nc[0, :8] = 40           # every pixel of the upper half stopped in the first batch
    nc[0, 0, 0] = 63         # ... the last one at its last entry
    nc[0, 8:] = 3            # the lower half: nothing stopped
    np.testing.assert_array_equal(rr.processed_batches(lists, nc, H, W), [[1, 1]])
    np.testing.assert_array_equal(rr.processed_batches(lists, nc, H, W, rows=True), [[[1, 1], [1, 1]]])
    r = rr.walk(lists, nc, q, H, W)
    np.testing.assert_array_equal(r["must"][:130], [0x01] * 40 + [0x00] * 24 + [0x13] * 66)      # footprint bits behind batch 0
    np.testing.assert_array_equal(r["may"], r["must"])
    np.testing.assert_array_equal(r["staged"][:130], [0x13] * 64 + [0] * 66)
    r = rr.walk(lists, nc, q, H, W, rows=True)
    np.testing.assert_array_equal(r["must"][:130], [0x01] * 40 + [0x00] * 90)                    # row items: cleared
    # one pixel of rows 4-7 never stops: that row is walked to the end (and blends nothing: the Gaussian is far away), rows 0-3 stop
    nc[0, 5, 1] = 130
    np.testing.assert_array_equal(rr.processed_batches(lists, nc, H, W), [[3, 1]])
    np.testing.assert_array_equal(rr.processed_batches(lists, nc, H, W, rows=True), [[[1, 3], [1, 1]]])
    r = rr.walk(lists, nc, q, H, W, rows=True)
    np.testing.assert_array_equal(r["must"][:130], [0x01] * 40 + [0x00] * 90)
    np.testing.assert_array_equal(r["staged"][:130], [0x13] * 64 + [0x10] * 66)   # later batches staged for the live sub-block (0, 1) only
    r = rr.walk(lists, nc, q, H, W)
    np.testing.assert_array_equal(r["must"][:130], [0x01] * 40 + [0x00] * 90)     # the half-tile kernel processed all three batches


def test_a_ragged_image_counts_inside_pixels_only():
    q = _records([(1.5, 1.5, 0.55, 0.02)])
    lists = _lists([(0, 0x01)] * 70, [(0, 0x01)] * 70)
    nc = np.full((1, 6, W), 5)          # image of 6 rows: rows 0-3 whole, 4-7 half, the lower half outside
    np.testing.assert_array_equal(rr.processed_batches(lists, nc, 6, W), [[1, 0]])
    np.testing.assert_array_equal(rr.processed_batches(lists, nc, 6, W, rows=True), [[[1, 1], [0, 0]]])


def test_expected_cost_is_the_longest_narrowed_sub_block_list_per_batch():
    upper = [(0, 0x01)] * 10 + [(0, 0x03)] * 5 + [(0, 0x00)] * 49 + [(0, 0x80)] * 7      # batch 0: 15 on sub-block 0; batch 1: 7
    lower = [(0, 0x10)] * 64 + [(0, 0x10)] * 64 + [(0, 0x30)] * 2
    lists = _lists(upper, lower)
    np.testing.assert_array_equal(rr.expected_cost(lists, np.array([[2, 3]])), [[22, 130]])
    np.testing.assert_array_equal(rr.expected_cost(lists, np.array([[1, 2]])), [[15, 128]])
    np.testing.assert_array_equal(rr.expected_cost(lists, np.array([[0, 0]])), [[0, 0]])


def _order_case():
    cost = np.array([[0, 7], [2100, 6], [3000, 1], [64, 65]])
    # classes: 0 3 / 1023 3 / 1023 0 / 32 32 -> costliest first; equal classes in any order
    order = np.array([2, 1, 3 | 1 << 28, 3, 1 | 1 << 28, 0 | 1 << 28, 2 | 1 << 28, 0])
    return order, cost


def test_check_order_accepts_the_sorted_permutation():
    order, cost = _order_case()
    rr.check_order(order, cost, 8)
    rr.check_order(order[[1, 0, 2, 3, 5, 4, 7, 6]], cost, 8)      # within a class the order is free


def test_check_order_rejects_wrong_orders():
    order, cost = _order_case()
    dup = order.copy()
    dup[4] = dup[5]                                  # one item twice, one missing: gradients of a half tile lost
    with pytest.raises(AssertionError, match="no permutation"):
        rr.check_order(dup, cost, 8)
    with pytest.raises(AssertionError):
        rr.check_order(order[:-1], cost, 8)          # an item dropped
    with pytest.raises(AssertionError, match="no work item"):
        rr.check_order(np.where(order == 3, 4, order), cost, 8)
    with pytest.raises(AssertionError, match="cost class rises"):
        rr.check_order(order[[0, 1, 2, 4, 3, 5, 6, 7]], cost, 8)
    # the saturated class: 2046 and 2047 and everything above are one class, 2045 is not
    rr.check_order(np.array([0, 0 | 1 << 28]), np.array([[2046, 5000]]), 2)
    with pytest.raises(AssertionError, match="cost class rises"):
        rr.check_order(np.array([0, 0 | 1 << 28]), np.array([[2045, 2046]]), 2)


# ---- a scalar restatement of the kernels' bookkeeping, pixel by pixel -----------------------------------------------------
def _simulate(lists, q, rows):
    """What k_render_fwd<RECORD> (rows=False) / render_row_item<REC> leave for ONE tile of a 16 x 16 image: narrowed bits per
    word, n_contrib, item_cost (half-tile kernel), staged bits — entry by entry, pixel by pixel, in float64."""
    ts, hc, hl = lists
    n = int(ts[1])
    q0, q1 = (a[0].astype(np.float64) for a in q)
    out = np.zeros(len(hl), np.uint8)
    staged = np.zeros(len(hl), np.uint8)
    nc = np.zeros((1, H, W), np.int64)
    cost = np.zeros((1, 2), np.int64)
    for h in range(2):
        cnt = int(hc[0, h])
        words = hl[h * n: h * n + cnt]
        groups = [range(0, 4), range(4, 8)] if rows else [range(8)]       # sub-blocks that stop and clear together
        for grp in groups:
            pix = [(8 * h + 4 * (g >> 2) + ly, 4 * (g & 3) + lx, g) for g in grp for ly in range(4) for lx in range(4)]
            T = {p[:2]: 1.0 for p in pix}
            stop = {}
            base = 0
            while base < cnt:
                if len(stop) == len(pix):
                    break
                live = {g for (y, x, g) in pix if (y, x) not in stop}
                per_block = {g: 0 for g in grp}
                for i in range(base, min(base + 64, cnt)):
                    g_idx, foot = int(words[i]) & 0xFFFFFF, int(words[i]) >> 24
                    X, Y, A, B = q0[g_idx]
                    Cc, o = q1[g_idx][:2]
                    hits = 0
                    for (y, x, g) in pix:
                        if not (foot >> g) & 1 or g not in live:
                            continue
                        staged[h * n + i] |= 1 << g
                        if (y, x) in stop:
                            continue
                        dx, dy = X - x, Y - y
                        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
                        alpha = min(0.99, o * np.exp(power))
                        if power > 0 or alpha < rr.ALPHA_MIN:
                            continue
                        if T[(y, x)] * (1 - alpha) < 1e-4:
                            stop[(y, x)] = i
                            continue
                        T[(y, x)] *= 1 - alpha
                        hits |= 1 << g
                    out[h * n + i] |= hits
                    for g in grp:
                        per_block[g] += (hits >> g) & 1
                cost[0, h] += max(per_block.values())
                base += 64
            mask = sum(1 << g for g in grp)
            for i in range(base, cnt):               # not processed
                out[h * n + i] |= 0 if rows else (int(words[i]) >> 24) & mask
            for (y, x, g) in pix:
                nc[0, y, x] = stop.get((y, x), cnt)
    return out, nc, cost, staged


def _one_tile_scene(seed):
    rng = np.random.default_rng(seed)
    G = 300
    rows = [(rng.uniform(-1, 17), rng.uniform(-1, 17), rng.uniform(0.4, 6.0) ** 2 + 0.3,
             rng.choice([0.02, 0.3, 0.9, 0.99]) if k % 3 else 0.005) for k in range(G)]
    q = _records(rows)
    # footprint bits: generous boxes (3.4 sigma), as the sort would give them; entries without a bit are not listed
    lists_ent = [[], []]
    for k, (x, y, s2, o) in enumerate(rows):
        r = 3.4 * np.sqrt(s2)
        for h in range(2):
            bits = 0
            for g in range(8):
                cx0, cy0 = 4 * (g & 3), 8 * h + 4 * (g >> 2)
                if x - r <= cx0 + 3 and x + r >= cx0 and y - r <= cy0 + 3 and y + r >= cy0:
                    bits |= 1 << g
            if bits:
                lists_ent[h].append((k, bits))
    return _lists(*lists_ent), q


@pytest.fixture(scope="module", params=[False, True], ids=["half_tile", "row_items"])
def simulated(request):
    lists, q = _one_tile_scene(3)
    rows = request.param
    bits, nc, cost, staged = _simulate(lists, q, rows)
    return lists, q, rows, bits, nc, cost, staged


def test_reference_agrees_with_the_scalar_restatement(simulated):
    lists, q, rows, bits, nc, cost, staged = simulated
    ts, hc, hl = lists
    assert hc.min() > 130, "the scene should have three batches per half"
    assert (nc < hc.max()).any() and len(np.unique(nc)) > 5, "pixels should stop at different entries"
    r = rr.walk(lists, nc, q, H, W, rows)
    assert not (r["must"] & ~bits).any() and not (bits & ~r["may"]).any()
    assert not (r["may"] & ~r["must"]).any(), "no alpha of this scene is within 5e-6 of the threshold"
    np.testing.assert_array_equal(r["staged"], staged)
    foot = (hl >> 24).astype(np.uint8)
    assert (bits != foot).mean() > 0.3 and (bits != 0).any(), "the narrowing should change many entries"
    if not rows:
        narrowed = (ts, hc, (hl & 0xFFFFFF) | (bits.astype(np.uint32) << 24))
        np.testing.assert_array_equal(rr.expected_cost(narrowed, r["batches"]), cost)
    flags = rr.expected_flags(lists, r["staged"], q, 1)
    assert flags.shape == (1, 2) and flags.all()


def test_a_reference_shifted_by_one_iteration_fails(simulated):
    """The check  must <= bits <= may  is not vacuous: the same reference moved by one list position is rejected."""
    lists, q, rows, bits, nc, cost, staged = simulated
    must, may = rr.expected_bits(lists, nc, q, H, W, rows)
    for shift in (1, -1):
        m, y = np.roll(must, shift), np.roll(may, shift)
        assert (m & ~bits).any() or (bits & ~y).any()
    # ... and so is a single dropped bit of a faint contribution, or a single bit too many
    i = int(np.flatnonzero(bits)[-1])
    low = bits.copy()
    low[i] &= low[i] - 1
    assert (must & ~low).any()
    foot = (lists[2] >> 24).astype(np.uint8)
    j = int(np.flatnonzero(foot & ~may)[0])
    high = bits.copy()
    high[j] |= foot[j] & ~may[j]
    assert (high & ~may).any()


@pytest.mark.parametrize("name", NARROWING_SCENES)
def test_hand_built_scenes_keep_every_alpha_away_from_the_threshold(name):
    """The scenes tests/test_record_forward_gpu.py expects exact bits of: every alpha of the designated halves of view 0 is at
    least 10 % away from 1/255, in float64 from the oracle's projection."""
    sc, bi, plan = narrowing_scene(name, 4)
    margin = alpha_margin(bi, designated(name, plan))
    assert margin >= 0.1, margin


@pytest.mark.parametrize("name", list(RANDOM_CASES))
def test_random_scenes_leave_few_pairs_undecided(name):
    """The share of (entry, sub-block) pairs the float64 reference cannot decide (an alpha within the window of 1/255 and none
    above it) stays far below the 1 % tests/test_record_forward_gpu.py allows — from the oracle's projection alone, over every
    entry of the canonical tile lists on every sub-block, with no pixel stopped (a superset of what the GPU test can meet)."""
    bi = random_inputs(RANDOM_CASES[name])
    Hh, Ww = bi["H"], bi["W"]
    undecided = pairs = 0
    for v in range(bi["V"]):
        o = util.oracle_forward(bi, v)
        ranges = o["ranges"].astype(np.int64)
        n = ranges[:, 1] - ranges[:, 0]
        ts = np.concatenate([[0], np.cumsum(n)])
        pl = np.concatenate([o["point_list"][a:b] for a, b in ranges]).astype(np.uint32) if n.sum() else np.zeros(0, np.uint32)
        hl = np.zeros(2 * len(pl), np.uint32)
        for t in range(len(n)):               # both halves list every entry of the tile on all of their sub-blocks
            hl[2 * ts[t]: 2 * ts[t] + 2 * n[t]] = np.tile(pl[ts[t]:ts[t + 1]] | np.uint32(0xFF << 24), 2)
        lists = (ts, np.stack([n, n], 1), hl)
        nc = np.repeat(np.repeat(n.reshape((Hh + 15) // 16, (Ww + 15) // 16), 16, 0), 16, 1)[None, :Hh, :Ww]
        co = o["conic_opacity"]
        q = (np.concatenate([o["xy"], co[:, :2]], 1)[None], np.concatenate([co[:, 2:], np.zeros_like(co[:, :2])], 1)[None])
        must, may = rr.expected_bits(lists, nc, q, Hh, Ww)
        undecided += int(np.unpackbits(may & ~must).sum())
        pairs += int(np.unpackbits(may).sum())
    assert pairs > 10_000 and undecided <= 1e-3 * pairs, (undecided, pairs)
