"""Plain numpy statement of what a forward that a backward follows (lsr_dims.forward_flags FOR_BACKWARD) hands the compositing
backward besides the images (latentsplat_amd/csrc/render_forward.hip, RECORD / REC):

* the narrowed sub-block bits of every half-list entry: expected_bits;
* the per-item cost: expected_cost;
* the work order derived from it: check_order;
* and, on the way, which entries the kernels staged at all (item_flags): walk()["staged"].

``lists`` is always the triple (tile_start (V T + 1,), half_count (V T, 2), half_list words (2 P,)) of tests/util.py HipRun;
per-entry results are arrays parallel to half_list (only the counted prefixes of the lists are defined, 0 elsewhere).
Half h of the tile whose canonical list is [s, s + n) owns the words [2 s + h n, 2 s + h n + half_count).
"""
import numpy as np

BATCH = 64                  # list entries the kernels stage at a time
ALPHA_MIN = 1.0 / 255.0
ALPHA_WINDOW = 5e-6         # relative: the band in which the oracle calls an alpha >= 1/255 decision fragile (oracle/raster_oracle.c)
POWER_WINDOW = 1e-6         # power <= 0, as tests/util.py fragile_gaussians allows it
STEEP_OPACITY = 0.75        # lsr_internal.h kSteepOpacity
COST_CLASSES = 1024         # lsr_internal.h kCostClasses
HALF_SHIFT = 28             # work item = view T + tile | half << 28


def half_slices(lists):
    """(vt, half, first word, entries) of every half-tile list."""
    ts, hc, _ = lists
    for vt in range(hc.shape[0]):
        s0, n = int(ts[vt]), int(ts[vt + 1] - ts[vt])
        for h in range(2):
            yield vt, h, 2 * s0 + h * n, int(hc[vt, h])


def counted(lists):
    """Which words of half_list belong to a list (the rest of the area is not defined)."""
    mask = np.zeros(len(lists[2]), bool)
    for _, _, w0, cnt in half_slices(lists):
        mask[w0:w0 + cnt] = True
    return mask


def _padded(n_contrib, H, W):
    """n_contrib on whole tiles, and which of those pixels are inside the image."""
    V = n_contrib.shape[0]
    gy, gx = (H + 15) // 16, (W + 15) // 16
    nc = np.zeros((V, 16 * gy, 16 * gx), np.int64)
    nc[:, :H, :W] = n_contrib
    inside = np.zeros((16 * gy, 16 * gx), bool)
    inside[:H, :W] = True
    return nc, inside, gy, gx


def processed_batches(lists, n_contrib, H, W, rows=False):
    """(V T, 2) batches of 64 entries the half-tile kernel staged per item, or (V T, 2, 2) per row of four sub-blocks for the
    row items: all of the list, unless every inside pixel of the half (row) stopped — then up to the batch of the last stop.
    A half (row) without a pixel inside the image stages nothing."""
    ts, hc, _ = lists
    nc, inside, gy, gx = _padded(n_contrib, H, W)
    V = nc.shape[0]
    # (V, gy, half, row, 4, gx, 16) -> pixels of one (view, tile, half, row) last
    grp = lambda a: a.reshape(a.shape[0], gy, 2, 2, 4, gx, 16).transpose(0, 1, 5, 2, 3, 4, 6).reshape(a.shape[0] * gy * gx, 2, 2, 64)
    nc_g, in_g = grp(nc), np.tile(grp(inside[None]), (V, 1, 1, 1))
    if not rows:
        nc_g, in_g = nc_g.reshape(-1, 2, 128), in_g.reshape(-1, 2, 128)
    cnt = hc.reshape(-1, 2, *([1] * (nc_g.ndim - 2)))
    stopped = nc_g < cnt
    all_stopped = (stopped | ~in_g).all(-1)
    any_inside = in_g.any(-1)
    last_stop = np.where(in_g, nc_g, -1).max(-1)
    full = -(-cnt[..., 0] // BATCH)
    return np.where(any_inside, np.where(all_stopped, last_stop // BATCH + 1, full), 0)


def walk(lists, n_contrib, records, H, W, rows=False):
    """Per list entry (arrays parallel to half_list, uint8 sub-block bits): ``must`` / ``may`` — the narrowed bits the kernel
    must at least / may at most leave (see expected_bits), ``staged`` — the sub-blocks the entry was staged for (its footprint
    bits on the sub-blocks that still had a pixel to blend when its batch began, 0 in batches that were not processed)."""
    ts, hc, hl = lists
    q0, q1 = records
    nc, inside, gy, gx = _padded(n_contrib, H, W)
    T = gy * gx
    done = processed_batches(lists, n_contrib, H, W, rows)
    must, may, staged = (np.zeros(len(hl), np.uint8) for _ in range(3))
    weights = (1 << np.arange(8)).reshape(2, 4)                          # bit 4 r + c of sub-block (c, r)
    blocks = lambda a: a.reshape(a.shape[0], 2, 4, 4, 4).any((2, 4))     # (n, 8, 16) pixels -> (n, 2, 4) sub-blocks
    for vt, h, w0, cnt in half_slices(lists):
        if cnt == 0:
            continue
        v, t = divmod(vt, T)
        ty, tx = divmod(t, gx)
        y0, x0 = 16 * ty + 8 * h, 16 * tx
        words = hl[w0:w0 + cnt]
        idx, foot = (words & 0x00FFFFFF).astype(np.int64), (words >> 24).astype(np.int64)
        x, y, A, B = (q0[v, idx, k].astype(np.float64)[:, None, None] for k in range(4))
        C, o = (q1[v, idx, k].astype(np.float64)[:, None, None] for k in range(2))
        dx = x - (x0 + np.arange(16, dtype=np.float64))[None, None, :]
        dy = y - (y0 + np.arange(8, dtype=np.float64))[None, :, None]
        power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        with np.errstate(over="ignore", invalid="ignore"):
            alpha = o * np.exp(np.minimum(power, 1.0))
        pos = np.arange(cnt)[:, None, None]
        px_nc, px_in = nc[v, y0:y0 + 8, x0:x0 + 16][None], inside[y0:y0 + 8, x0:x0 + 16][None]
        reached = px_in & (px_nc > pos)                                  # the pixel got as far as the entry and did not stop at it
        keep_must = reached & (power <= 0.0) & (alpha >= ALPHA_MIN * (1.0 + ALPHA_WINDOW))
        keep_may = reached & (power <= POWER_WINDOW) & (alpha >= ALPHA_MIN * (1.0 - ALPHA_WINDOW))
        b_must, b_may = blocks(keep_must), blocks(keep_may)              # (cnt, 2, 4)
        # sub-blocks with a pixel left to blend when the entry's batch begins: never stopped, or stopped in that batch or later
        alive = px_in & ((px_nc == cnt) | (px_nc // BATCH >= pos // BATCH))
        b_alive = blocks(alive)
        batch = np.arange(cnt) // BATCH
        if rows:
            proc = batch[:, None] < done[vt, h][None, :]                 # (cnt, 2): per row of sub-blocks
            proc = np.repeat(proc[:, :, None], 4, 2)
        else:
            proc = np.broadcast_to((batch < done[vt, h])[:, None, None], (cnt, 2, 4))
        foot_b = ((foot[:, None, None] >> np.arange(8).reshape(1, 2, 4)) & 1).astype(bool)
        # a batch that was not processed keeps its footprint bits (half-tile kernel) or has the row's nibble cleared (row items)
        keep_foot = foot_b & ~proc & (not rows)
        bits = lambda b: ((b * weights[None]).sum((1, 2))).astype(np.uint8)
        must[w0:w0 + cnt] = bits((b_must & foot_b & proc) | keep_foot)
        may[w0:w0 + cnt] = bits((b_may & foot_b & proc) | keep_foot)
        staged[w0:w0 + cnt] = bits(foot_b & proc & b_alive)
    return dict(must=must, may=may, staged=staged, batches=done)


def expected_bits(lists, n_contrib, records, H, W, rows=False):
    """(must, may): the sub-block bits a RECORD / REC forward leaves on every entry of the half lists ``lists`` (the footprint
    lists of a plain run of the same inputs), given the kernel's own ``n_contrib`` (V, H, W) and screen records ``records`` =
    HipRun.q().  For an entry at position i of a processed batch, bit g is set iff some inside pixel of sub-block g has
    n_contrib > i and keeps the entry (power <= 0 and alpha >= 1/255, evaluated in float64): ``must`` where a pixel clears
    the alpha threshold by more than ALPHA_WINDOW, ``may`` where a pixel is within the window or above.  The kernel's bits b
    must satisfy  must <= b <= may  (as sets; may is already intersected with the footprint bits).  ``rows``: the row items'
    rule (per row of four sub-blocks) instead of the half-tile kernel's."""
    r = walk(lists, n_contrib, records, H, W, rows)
    return r["must"], r["may"]


def expected_flags(lists, staged, records, T):
    """(V T, 2) item_flags: 1 where the item's list holds a staged entry of opacity >= kSteepOpacity."""
    ts, hc, hl = lists
    out = np.zeros(hc.shape, np.int64)
    for vt, h, w0, cnt in half_slices(lists):
        idx = (hl[w0:w0 + cnt] & 0x00FFFFFF).astype(np.int64)
        out[vt, h] = int(((staged[w0:w0 + cnt] != 0) & (records[1][vt // T, idx, 1] >= np.float32(STEEP_OPACITY))).any())
    return out


def expected_cost(narrowed_lists, processed):
    """(V T, 2) item_cost of the half-tile RECORD kernel: over the batches it processed ((V T, 2), processed_batches), the sum of
    the longest per-sub-block count of set bits among the batch's entries in the NARROWED lists.  Exact."""
    ts, hc, hl = narrowed_lists
    counts = hc.reshape(-1).astype(np.int64)
    n_items = len(counts)
    n = (ts[1:] - ts[:-1]).astype(np.int64)
    first = np.stack([2 * ts[:-1], 2 * ts[:-1] + n], 1).reshape(-1).astype(np.int64)      # first word of every item's list
    item = np.repeat(np.arange(n_items), counts)
    pos = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    bits = (hl[np.repeat(first, counts) + pos] >> 24).astype(np.int64)
    batch = pos // BATCH
    ok = batch < np.asarray(processed).reshape(-1)[item]
    nb = int(batch.max(initial=0)) + 1
    longest = np.zeros(n_items * nb, np.int64)
    for g in range(8):
        sel = ok & (((bits >> g) & 1) != 0)
        longest = np.maximum(longest, np.bincount(item[sel] * nb + batch[sel], minlength=n_items * nb))
    return longest.reshape(n_items, nb).sum(1).reshape(-1, 2)


def cost_class(cost):
    """The counting sort's class of a cost, as a number that falls along the order: min(1023, cost >> 1)."""
    return np.minimum(COST_CLASSES - 1, np.asarray(cost, np.int64) >> 1)


def check_order(order2, cost, num_items):
    """tile_order2 of k_order_items: a permutation of all ``num_items`` work items `vt | half << 28`, costliest class first.
    ``cost``: (V T, 2)."""
    order2 = np.asarray(order2, np.int64)
    assert order2.shape == (num_items,), (order2.shape, num_items)
    vt, half = order2 & ((1 << HALF_SHIFT) - 1), order2 >> HALF_SHIFT
    assert ((half == 0) | (half == 1)).all() and (vt < num_items // 2).all(), "tile_order2 holds a word that is no work item"
    flat = 2 * vt + half
    seen = np.bincount(flat, minlength=num_items)
    assert (seen == 1).all(), (f"tile_order2 is no permutation: {int((seen == 0).sum())} items missing "
                               f"(first {int(np.argmax(seen == 0))}), {int((seen > 1).sum())} more than once")
    cls = cost_class(np.asarray(cost).reshape(-1)[flat])
    assert (np.diff(cls) <= 0).all(), f"cost class rises along tile_order2 at position {int(np.argmax(np.diff(cls) > 0)) + 1}"
