"""The half-tile compositing kernel's inner loop takes two sub-block-list entries per trip (the plain 4- and 8-channel
instances, latentsplat_amd/csrc/render_forward.hip): scenes of hand-placed Gaussians whose list structure is known
(tests/list_scenes.py), against the CPU oracle with the helpers and bars of tests/test_parity_gpu.py (images 1e-4 abs,
n_contrib exact outside fragile pixels, final_T = 1 - mask) — through every compositing instance: the instances with the
one-entry loop (RECORD, 12 and 36 channels), the row items (plain and REC) and the sub-block items walk the same lists.

View 0 looks down the z axis, so a Gaussian's pixel position and footprint are what the scene builder asked for and the
tests assert the list structure they were built for (list lengths, sub-block bits, where pixels stop) before they
compare anything.  View 1 is a perturbed camera: the same Gaussians in lists nobody planned.
"""
import numpy as np
import pytest

from tests import util
from tests.list_scenes import EARLY, EDGE, MIXED, STACK, half_entries, half_origin, lengths_scene, stop_index, stops_scene
from tests.test_parity_gpu import _check_forward

pytestmark = pytest.mark.gpu

# The compositing instances: (payload channels, kernel).  "half": the half-tile kernel k_render_fwd, "rows" / "quad": the row
# and the sub-block items of k_render_fwd_small (4 and 8 padded channels only); "_rec": the instance a forward runs that a
# backward follows (RECORD / REC).  12 and 32 channels have the plain half-tile instance only.
KERNELS = {"half": dict(LSR_FWD_ROWS=0), "half_rec": dict(LSR_FWD_ROWS=0), "rows": dict(LSR_FWD_ROWS=1, LSR_FWD_QUAD=0),
           "rows_rec": dict(LSR_FWD_ROWS=1, LSR_FWD_QUAD=0), "quad": dict(LSR_FWD_QUAD=1)}
INSTANCES = [(c, k) for c in (4, 8) for k in KERNELS] + [(12, "half"), (32, "half")]
instances = pytest.mark.parametrize("channels,kernel", INSTANCES, ids=[str(c) if k == "half" else f"{c}-{k}" for c, k in INSTANCES])


def _forward_checked(hip_device, bi, kernel="half"):
    """(run of the instance, held to the oracle; the run to read the list structure from: a RECORD / REC run narrows its own
    lists, so theirs comes from the plain instance of the same kernel on the same inputs)."""
    from latentsplat_amd import _lib
    try:
        for knob, value in KERNELS[kernel].items():
            _lib.set_knob(knob, value)
        run = util.HipRun(bi, hip_device, forward_flags=_lib.FWD_FOR_BACKWARD if kernel.endswith("_rec") else 0)
        lists = util.HipRun(bi, hip_device) if kernel.endswith("_rec") else run
    finally:
        _lib.set_knob("LSR_FWD_ROWS", -1)
        _lib.set_knob("LSR_FWD_QUAD", -1)
    _check_forward(bi, run)
    assert np.allclose(1.0 - run.mask_out.cpu().numpy(), run.final_T(), atol=1e-6)
    if lists is not run:
        np.testing.assert_array_equal(run.half_count(), lists.half_count())
    return run, lists


@instances
def test_list_lengths_of_both_parities_and_batch_edges(hip_device, channels, kernel):
    sc, bi, plan = lengths_scene(channels)
    run, lists = _forward_checked(hip_device, bi, kernel)
    seen_nk = set()
    for (tx, ty, h), counts in plan.items():
        bits = (half_entries(lists, tx, ty, h) >> 24) & 0xFF
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
        x0, y0 = half_origin(tx, ty, h)
        assert (nc[y0:y0 + 8, x0:x0 + 16] == sum(counts)).all()


@instances
def test_stops_at_either_entry_of_a_trip(hip_device, channels, kernel):
    sc, bi = stops_scene(channels)
    run, lists = _forward_checked(hip_device, bi, kernel)
    for where, hn in ((STACK, 16), (EDGE, 73), (EARLY, 10)):
        words = half_entries(lists, *where)
        assert len(words) == hn, (where, len(words))
        # every entry is on every sub-block's list: the position in a sub-block list is the position in the half's list, and
        # the entries at even positions of a batch are the first of their trip, those at odd positions the second
        assert (((words >> 24) & 0xFF) == 0xFF).all(), where
    # the two pixels of a lane, over the three halves (64 is even: the trips of a batch pair the positions (2k, 2k + 1) of the list)
    stops = {where: stop_index(run, where, lists)[0] for where in (STACK, EDGE, EARLY)}
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
