"""What a forward that a backward follows (lsr_dims.forward_flags FOR_BACKWARD: the RECORD instances of k_render_fwd, the REC
row items of k_render_fwd_small; latentsplat_amd/csrc/render_forward.hip) hands the compositing backward besides the images,
against the plain numpy statement of tests/record_ref.py:

* the narrowed sub-block bits of every list entry, bit for bit — on hand-built lists whose entries contribute or not in
  chosen patterns (a), and on random scenes (b);
* entries whose bits became 0, through the backward (c);
* the instances that must leave lists and header alone (d);
* item_cost, tile_order2 and header word kHdrOrder2Valid around the item counts at which k_order_items runs (e).
"""
import functools

import numpy as np
import pytest
import torch

from tests import record_ref as rr
from tests import util
from tests.list_scenes import (CONTRIBUTING, EARLY, EDGE, FINISHER, HIT_FREE, NARROWING_SCENES, RANDOM_CASES, S, SINGLE, STACK, Builder, add_stops,
                               half_entries, half_origin, narrow, narrowing_scene, random_inputs, wide)
from tests.test_parity_gpu import _grad_scene

pytestmark = pytest.mark.gpu

HDR_FLAGS_VALID, HDR_ORDER2_VALID = 6, 9        # lsr_internal.h kHdrFlagsValid, kHdrOrder2Valid


# ---- (a) hand-built lists (tests/list_scenes.py narrowing_scene) -----------------------------------------------------------
def _knobs(**kw):
    from latentsplat_amd import _lib
    for k, v in kw.items():
        _lib.set_knob(k, v)


def _plain_and_record(bi, dev, rows):
    """The plain and the FOR_BACKWARD run of the half-tile kernel (rows = 0) or the row items (rows = 1) on the same inputs."""
    from latentsplat_amd import _lib
    try:
        _knobs(LSR_FWD_ROWS=rows, LSR_FWD_QUAD=0)
        return util.HipRun(bi, dev), util.HipRun(bi, dev, forward_flags=_lib.FWD_FOR_BACKWARD)
    finally:
        _knobs(LSR_FWD_ROWS=-1, LSR_FWD_QUAD=-1)


def _check_record_run(bi, plain, rec, rows, max_undecided):
    """Everything a RECORD / REC run must leave, against the reference; returns (narrowed bits, reference walk, lists)."""
    H, W = bi["H"], bi["W"]
    for a, b in ((plain.color_out, rec.color_out), (plain.feat_out, rec.feat_out), (plain.mask_out, rec.mask_out), (plain.depth_out, rec.depth_out)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), "the images of the RECORD run differ from the plain run's"
    np.testing.assert_array_equal(plain.n_contrib(), rec.n_contrib())
    np.testing.assert_array_equal(plain.final_T().view(np.uint32), rec.final_T().view(np.uint32))
    lists = (plain.tile_start(), plain.half_count(), plain.half_list())
    np.testing.assert_array_equal(lists[0], rec.tile_start())
    np.testing.assert_array_equal(lists[1], rec.half_count())
    valid = rr.counted(lists)
    words = rec.half_list()
    np.testing.assert_array_equal(words[valid] & 0x00FFFFFF, lists[2][valid] & 0x00FFFFFF, err_msg="the entries of the lists changed")
    got = np.where(valid, words >> 24, 0).astype(np.uint8)
    foot = np.where(valid, lists[2] >> 24, 0).astype(np.uint8)
    r = rr.walk(lists, rec.n_contrib(), rec.q(), H, W, rows=bool(rows))
    undecided = int(np.unpackbits(r["may"] & ~r["must"]).sum())
    pairs = int(np.unpackbits(foot).sum())
    print(f"rows={rows}: {pairs} (entry, sub-block) pairs, {int(np.unpackbits(got).sum())} after narrowing, {undecided} undecided")
    assert undecided <= max_undecided * pairs, f"{undecided} of {pairs} (entry, sub-block) pairs within the alpha window"
    lost, extra = r["must"] & ~got, got & ~r["may"]
    assert not lost.any(), (f"{int(np.unpackbits(lost).sum())} (entry, sub-block) pairs with a contributing pixel lost their bit; first at word "
                            f"{int(np.flatnonzero(lost)[0])}: bits {int(got[np.flatnonzero(lost)[0]]):#04x}, must {int(r['must'][np.flatnonzero(lost)[0]]):#04x}")
    assert not extra.any(), (f"{int(np.unpackbits(extra).sum())} (entry, sub-block) pairs without a contributing pixel kept their bit; first at word "
                             f"{int(np.flatnonzero(extra)[0])}: bits {int(got[np.flatnonzero(extra)[0]]):#04x}, may {int(r['may'][np.flatnonzero(extra)[0]]):#04x}")
    flags, valid_word = rec.item_flags()
    assert valid_word == 1 and rec.header()[HDR_FLAGS_VALID] == 1
    np.testing.assert_array_equal(flags, rr.expected_flags(lists, r["staged"], rec.q(), plain.T), err_msg="item_flags")
    return got, r, lists


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("channels", [4, 8])
@pytest.mark.parametrize("name", NARROWING_SCENES)
def test_hand_built_narrowing(hip_device, name, channels, rows):
    sc, bi, plan = narrowing_scene(name, channels)
    plain, rec = _plain_and_record(bi, hip_device, rows)
    # the lists are the planned ones: the hit-free entries are listed, on their sub-block
    for where, entries in plan.items():
        words = half_entries(plain, *where)
        np.testing.assert_array_equal(words & 0x00FFFFFF, [e[0] for e in entries], err_msg=f"list of half {where}")
        np.testing.assert_array_equal(words >> 24, [1 << e[1] for e in entries], err_msg=f"footprint bits of half {where}")
    got, r, lists = _check_record_run(bi, plain, rec, rows, max_undecided=0.0)      # nothing undecided: bits == must == may
    # ... and what the plan says they are
    for where, entries in plan.items():
        np.testing.assert_array_equal(half_entries(rec, *where) >> 24, [(1 << e[1]) if e[2] else 0 for e in entries],
                                      err_msg=f"narrowed bits of half {where}")
    if name == "stops":
        nc = rec.n_contrib()[0]
        for where, hn in ((STACK, 16), (EDGE, 73), (EARLY, 10)):
            # the planned entries reach every pixel of the half: entry i keeps bit g iff a pixel of g got past it
            x0, y0 = half_origin(*where)
            blk = nc[y0:y0 + 8, x0:x0 + 16].reshape(2, 4, 4, 4).transpose(0, 2, 1, 3).reshape(8, 16)      # [sub-block 4 r + c][pixel]
            want = ((blk.max(1)[None, :] > np.arange(hn)[:, None]) * (1 << np.arange(8))[None, :]).sum(1)
            np.testing.assert_array_equal((half_entries(rec, *where) >> 24)[:hn], want, err_msg=f"half {where}")
        x0, y0 = half_origin(*FINISHER)
        before, after = half_entries(plain, *FINISHER) >> 24, half_entries(rec, *FINISHER) >> 24
        assert len(before) > 128 and nc[y0:y0 + 8, x0:x0 + 16].max() < 64, "the half should finish in the first of its three batches"
        assert (before[64:] == 0xFF).all()
        np.testing.assert_array_equal(after[64:], 0 if rows else before[64:])      # footprint bits kept / nibbles cleared


# ---- (b) random scenes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("case", list(RANDOM_CASES.values()), ids=list(RANDOM_CASES))
def test_random_scenes_narrow_to_exactly_the_contributing_sub_blocks(hip_device, case, rows):
    bi = random_inputs(case)
    plain, rec = _plain_and_record(bi, hip_device, rows)
    got, r, lists = _check_record_run(bi, plain, rec, rows, max_undecided=0.01)
    assert (got != np.where(rr.counted(lists), lists[2] >> 24, 0)).any()


# ---- (c) entries without a bit, through the backward ------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("with_aux", [False, True])
@pytest.mark.parametrize("name", NARROWING_SCENES)
def test_backward_of_hand_built_lists(hip_device, name, with_aux, rows):
    """The scenes of (a) through the autograd op and the compositing backward (unsplit and split lists; forward order, back to
    front, and by the forward's flags) against the oracle at the suite's bars (_grad_scene: 1e-4, clean rows CLEAN_TOL); a
    Gaussian that reaches no pixel of view 0 has no gradient there."""
    sc, bi, plan = narrowing_scene(name, 4)
    hit_free = np.array([e[0] for entries in plan.values() for e in entries if not e[2]], np.int64)
    try:
        _knobs(LSR_FWD_ROWS=rows, LSR_FWD_QUAD=0)
        for parts in (-1, 0):
            for rev in (0, 1, 2):
                _knobs(LSR_BWD_PARTS=parts, LSR_BWD_REV=rev)
                g = _grad_scene(hip_device, sc, S, S, with_aux)
                for k in ("means", "cov", "m2d", "feat"):
                    rows_of_view0 = g[k][0].detach().cpu().numpy()[hit_free]
                    assert not rows_of_view0.any(), f"dL/d{k} of a hit-free Gaussian (parts {parts}, rev {rev}): {np.abs(rows_of_view0).max()}"
    finally:
        _knobs(LSR_FWD_ROWS=-1, LSR_FWD_QUAD=-1, LSR_BWD_PARTS=-1, LSR_BWD_REV=2)


# ---- (d), (e): calls of more than 16 x CUs items ----------------------------------------------------------------------------
BIG = 128                  # image: 64 tiles, 128 items per view
PILE = (6, 6, 1, 5)        # (tx, ty, h, sub-block) of the 2100-entry list
PILE_N, PILE_OPACITY = 2100, 0.0063     # alpha = 1.02 ... 1.06 / 255 on four pixels; (1 - alpha)^2100 = 1.6e-4: nothing stops, cost 2100


@functools.lru_cache(maxsize=None)
def _big_scene(channels, views):
    """About 600 random Gaussians on the left half of a 128 x 128 image (with the opaque stacks of the stop scene among them),
    hand-built single-sub-block lists on the right half, one list of 2100 narrow entries, and tiles nobody reaches."""
    b = Builder(5, channels, size=BIG, dz=0.001)
    x0, y0 = half_origin(1, 6, 1)              # in front of everything: a half that finishes in its first batch, more behind
    wide(b, x0 + 7.5, y0 + 3.5, 6.0, 0.99, 20)
    wide(b, x0 + 7.5, y0 + 3.5, 6.0, 0.5, 150, feat=30.0)
    rng = np.random.default_rng(11)
    for _ in range(600):
        b.add(rng.uniform(0, 64), rng.uniform(0, 128), float(np.exp(rng.uniform(np.log(0.5), np.log(3.0)))), rng.uniform(0.05, 0.6))
    add_stops(b)
    for k, (hn, g) in enumerate(SINGLE):
        narrow(b, 4 + k % 4, k // 4, k % 2, g, hn, CONTRIBUTING if k % 3 else HIT_FREE)
    narrow(b, *PILE, PILE_N, PILE_OPACITY)
    sc = b.scene(views)
    return util.boundary_inputs(sc, BIG, BIG, bg=(0.0, 0.0, 0.0))


def _v_on(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    v_on = 16 * cus // 128 + 1          # the smallest V with 128 V > 16 CUs
    assert 2 <= v_on <= 128, f"{cus} compute units: the view counts of this test do not bracket k_order_items' range"
    return cus, v_on


def _gradients(bi, dev):
    from latentsplat_amd.rasterizer import rasterize_views
    views = util.view_table(bi, dev)
    leaves = {k: bi[k].to(dev).clone().requires_grad_(True) for k in ("means", "cov6", "opac", "features")}
    out = rasterize_views(views, bi["H"], bi["W"], bi["sh_degree"], leaves["means"], leaves["cov6"], leaves["opac"], features=leaves["features"])
    gen = torch.Generator().manual_seed(13)
    torch.autograd.backward([out[1]], [torch.randn(out[1].shape, generator=gen).to(dev)])
    return {k: v.grad.clone() for k, v in leaves.items()}


@pytest.mark.parametrize("which", ["below", "on", "upper_edge", "above"])
def test_item_cost_and_work_order(hip_device, which):
    from latentsplat_amd import _lib
    cus, v_on = _v_on(hip_device)
    V = {"below": v_on - 1, "on": v_on, "upper_edge": 128, "above": 129}[which]
    items = 2 * V * (BIG // 16) ** 2
    applies = 16 * cus < items <= 16384
    assert applies == (which in ("on", "upper_edge"))
    bi = _big_scene(4, V)
    rec = util.HipRun(bi, hip_device, forward_flags=_lib.FWD_FOR_BACKWARD)
    hdr = rec.header()
    assert hdr[HDR_FLAGS_VALID] == 1, "a call of this size runs the RECORD instance of the half-tile kernel"
    assert hdr[HDR_ORDER2_VALID] == int(applies), (which, V, items, int(hdr[HDR_ORDER2_VALID]))
    if not applies:
        return
    narrowed = (rec.tile_start(), rec.half_count(), rec.half_list())
    nc = rec.n_contrib()
    done = rr.processed_batches(narrowed, nc, BIG, BIG)
    assert (done < -(-narrowed[1] // 64)).any(), "no item that finished before the end of its list"
    want = rr.expected_cost(narrowed, done)
    tx, ty, h, g = PILE
    x0, y0 = half_origin(tx, ty, h)
    assert (nc[0, y0:y0 + 8, x0:x0 + 16] == PILE_N).all() and want[ty * (BIG // 16) + tx, h] == PILE_N       # nothing stops in the pile
    cls = rr.cost_class(want)
    assert (cls == 1023).any() and (want == 0).sum() >= items // 8 and len(np.unique(cls)) > 8, "saturated class, empty items, a spread between"
    np.testing.assert_array_equal(rec.item_cost(), want, err_msg="item_cost")
    rr.check_order(rec.tile_order2(), want, items)
    try:
        _knobs(LSR_REORDER=0)
        off = util.HipRun(bi, hip_device, forward_flags=_lib.FWD_FOR_BACKWARD)
        assert off.header()[HDR_ORDER2_VALID] == 0 and off.header()[HDR_FLAGS_VALID] == 1
        np.testing.assert_array_equal(off.half_list(), narrowed[2])
        g_off = _gradients(bi, hip_device)
        _knobs(LSR_REORDER=1)
        g_on = _gradients(bi, hip_device)
    finally:
        _knobs(LSR_REORDER=1)
    for k in g_on:
        scale = max(1.0, float(g_off[k].abs().max()))
        assert float(g_off[k].abs().max()) > 0
        assert float((g_on[k] - g_off[k]).abs().max()) <= 2e-5 * scale, k


@pytest.mark.parametrize("channels", [12, 32])
def test_instances_without_record_leave_lists_and_header_alone(hip_device, channels):
    """12 and 32 payload channels (the 12- and 36-channel instances) have no RECORD instance: a FOR_BACKWARD forward of a call
    whose item count would otherwise be re-ordered leaves the lists as the sort wrote them and raises neither header word."""
    from latentsplat_amd import _lib
    cus, v_on = _v_on(hip_device)
    bi = _big_scene(channels, v_on)
    plain = util.HipRun(bi, hip_device)
    rec = util.HipRun(bi, hip_device, forward_flags=_lib.FWD_FOR_BACKWARD)
    lists = (plain.tile_start(), plain.half_count(), plain.half_list())
    valid = rr.counted(lists)
    assert valid.sum() > PILE_N
    np.testing.assert_array_equal(rec.half_count(), lists[1])
    np.testing.assert_array_equal(rec.half_list()[valid], lists[2][valid])
    assert torch.equal(plain.feat_out, rec.feat_out)
    np.testing.assert_array_equal(plain.n_contrib(), rec.n_contrib())
    for run in (plain, rec):
        hdr = run.header()
        assert hdr[HDR_FLAGS_VALID] == 0 and hdr[HDR_ORDER2_VALID] == 0, (int(hdr[HDR_FLAGS_VALID]), int(hdr[HDR_ORDER2_VALID]))
