"""The MCMC strategy on the MI355X: lsr_mcmc_sample, lsr_mcmc_classify, lsr_mcmc_apply and lsr_mcmc_noise against the
references of tests/mcmc_ref.py, MCMCControl end to end, and the fitting tool with ``--strategy mcmc``.

Exact: the draws, their counts and the total; the dead list, the counts and the zero pattern of the weights; every copied
column, every zeroed or untouched moment, the rows a relocation does not name, and a destination's opacity / scaling
against its source's.  On a bar: the live weights, the new opacity / scaling of the sources (in the stored domain: logits
and log-scales) and the noise increment.  The bar is that of tests/test_density_gpu.py: the kernel's largest error against
float64 must be within 4 x the largest error of the float32 torch-CPU composition (the published sequence,
tests/mcmc_ref.py) on the same inputs, with a floor of 2^-20 of the quantity's scale (its largest magnitude).  Every
element is on the bar.

Sizes: the constants of csrc/mcmc.hip are kMcmcChunk = 256 rows per workgroup of the chunked kernels (sums, prefix sums,
classification, sources), kMcmcScanThreads = 256 lanes of the one workgroup that scans the chunk sums, kMcmcThreads = 256
per draw / noise / destination workgroup and kMcmcApplyElems = 2048 destination floats per workgroup.  70 001 rows are 274
chunks: more than one workgroup in every kernel, and more chunk sums than scan lanes, so that lanes walk two sums each
(the scan's second level); its n / 20 = 3500 draws are 14 draw workgroups and, three floats wide, 6 destination
workgroups.  524 291 rows (PAST_THE_GRID: sampling, classification and noise, one case each) are 2049 chunks, nine sums
per scan lane, and past the noise grid's cap of 2048 workgroups: the trips a scene of half a million Gaussians takes."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import mcmc_ref as ref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu

CHUNK, SCAN_THREADS, THREADS, APPLY_ELEMS = 256, 256, 256, 2048
BIG = 70_001
assert BIG > CHUNK * SCAN_THREADS and BIG // 20 > THREADS and 3 * (BIG // 20) > APPLY_ELEMS
SIZES = [0, 1, 63, 64, 65, 255, 257, 1000, BIG]
# The noise grid is capped at kMcmcMaxBlocks = 2048 workgroups of 256 lanes; past that, lanes take a second row.  The same
# size is 2049 chunks: each lane of the two scans walks ceil(2049 / 256) = 9 chunk sums.  One case each, outside the
# cross-products.
GRID_ROWS = 2048 * 256
PAST_THE_GRID = GRID_ROWS + 3
FLOOR = 2.0 ** -20
MARGIN = 4.0
LAST_UNIFORM = 1.0 - 2.0 ** -53


def _held(name, got, want, stock, show):
    got, want, stock = (np.asarray(a, np.float64) for a in (got, want, stock))
    if want.size == 0:
        assert got.size == 0
        return
    assert np.isfinite(stock).all(), (show, name)
    scale = float(np.abs(want).max())
    err, err_stock = float(np.abs(got - want).max()), float(np.abs(stock - want).max())
    bar = max(MARGIN * err_stock, FLOOR * scale)
    print(f"{show} {name:10s} kernel {err:.3e}  composition {err_stock:.3e}  bar {bar:.3e}  ({want.size} elements)")
    assert err <= bar, (show, name, err, err_stock, bar)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- sampling ----

def _weights(kind, n, rng):
    w = rng.random(n).astype(np.float32)
    if kind == "zeros30":
        w[rng.random(n) < 0.3] = 0.0
    elif kind == "one_row":
        w[:] = 0.0
        if n:
            w[(2 * n) // 3] = 0.37
    elif kind == "nasty":                                    # NaN, negatives, values above 1, sub-quantum weights
        r = rng.random(n)
        w[r < 0.15] = np.nan
        w[(r >= 0.15) & (r < 0.3)] *= -1.0
        w[(r >= 0.3) & (r < 0.45)] += 1.0
        w[(r >= 0.45) & (r < 0.5)] = 2.0 ** -31
    elif kind == "few":                                      # m far larger than the number of non-zero rows
        keep = rng.choice(n, size=min(3, n), replace=False)
        kept = w[keep]
        w[:] = 0.0
        w[keep] = kept
    return w


def _uniforms(m, rng):
    u = rng.random(m)
    if m >= 2:
        u[0], u[-1] = 0.0, LAST_UNIFORM
    if m >= 64:
        u[5], u[6], u[7] = np.nan, -0.25, 1.5
    return u


def _sample(dev, w, u):
    from latentsplat_amd import sample_by_weight
    idx, count, total = sample_by_weight(torch.from_numpy(w).to(dev), torch.from_numpy(u).to(dev), return_total=True)
    return idx.cpu().numpy(), count.cpu().numpy().view(np.uint32), int(total.cpu().numpy().view(np.uint64)[0])


@pytest.mark.parametrize("kind", ["zeros30", "one_row", "nasty", "few", "all_zero"])
@pytest.mark.parametrize("n", SIZES)
def test_sampling_is_exact(hip_device, n, kind):
    draws = [0] if n == 0 else sorted({0, 1, 64, 65, n // 20} | ({5000} if kind == "few" else set()))
    _check_sampling(hip_device, n, kind, draws)


@pytest.mark.parametrize("kind", ["zeros30", "nasty"])
def test_sampling_is_exact_past_the_grid_cap(hip_device, kind):
    """2049 chunks: k_mcmc_scan's lanes walk nine chunk sums each, and a draw searches 2049 bases (twelve halvings)."""
    chunks = -(-PAST_THE_GRID // CHUNK)
    assert chunks == 2049 and -(-chunks // SCAN_THREADS) == 9
    _check_sampling(hip_device, PAST_THE_GRID, kind, [65, PAST_THE_GRID // 20])


def _check_sampling(hip_device, n, kind, draws):
    rng = np.random.default_rng(100 * n + len(kind))
    w = np.zeros(n, np.float32) if kind == "all_zero" else _weights(kind, n, rng)
    for m in draws:
        u = _uniforms(m, rng)
        want_idx, want_count, want_total = ref.sample(w, u)
        idx, count, total = _sample(hip_device, w, u)
        show = f"n={n} {kind} m={m}:"
        assert total == want_total, (show, total, want_total)
        assert np.array_equal(idx, want_idx), show
        assert np.array_equal(count, want_count), show
        again = _sample(hip_device, w, u)                    # a second call gives the same bits
        assert np.array_equal(idx, again[0]) and np.array_equal(count, again[1]) and total == again[2]
        if want_total:
            assert (ref.quanta(w)[idx] > 0).all()
        else:
            assert (idx == -1).all() and not count.any()
    print(f"n={n} {kind}: draws {draws}, total {want_total}")


# ---- classification ----

@pytest.mark.parametrize("n", SIZES)
def test_classification_is_exact(hip_device, n):
    _check_classification(hip_device, n)


def test_classification_is_exact_past_the_grid_cap(hip_device):
    """2049 chunks: k_mcmc_classify_scan's lanes walk nine chunk sums each."""
    _check_classification(hip_device, PAST_THE_GRID)


def _check_classification(hip_device, n):
    from latentsplat_amd.mcmc import classify_dead, dead_logit
    rng = np.random.default_rng(n)
    thr = np.float32(dead_logit(0.005))
    assert thr == ref.dead_logit(0.005)
    o = rng.uniform(-9.0, 5.0, (n, 1)).astype(np.float32)
    if n >= 63:
        o[3::16, 0] = thr                                    # at the threshold: dead
        o[7::16, 0] = np.nextafter(thr, np.float32(np.inf))  # its float neighbour above: alive
    if n >= 1000:
        o[100:612, 0] = -9.0                                 # two whole chunks' worth of consecutive dead rows
        o[1], o[2] = np.nan, -np.inf
    want_w, want_dead, want_counts = ref.classify(o, thr)
    weights, dead, counts = classify_dead(torch.from_numpy(o).to(hip_device), float(thr))
    got_counts = counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_counts, want_counts), (got_counts, want_counts)
    assert np.array_equal(dead.cpu().numpy()[:int(want_counts[0])], want_dead)
    w = weights.cpu().numpy()
    is_dead = np.zeros(n, bool)
    is_dead[want_dead] = True
    assert not _bits(w[is_dead]).any()                       # exactly +0
    ok = ~is_dead & ~np.isnan(o[:, 0])
    assert (w[ok] > 0).all() and np.isnan(w[~is_dead & ~ok]).all()
    _held("weights", w[ok], want_w[ok], torch.sigmoid(torch.from_numpy(o[ok, 0])).numpy(), f"n={n}:")
    if n >= 63:
        assert is_dead[3] and not is_dead[7]
    # the weights alone (a growth: nothing is dead)
    only, none_dead, none_counts = classify_dead(torch.from_numpy(o).to(hip_device), -math.inf, want_dead=False)
    assert none_dead is None and none_counts is None
    live = ~np.isnan(o[:, 0]) & ~np.isinf(o[:, 0])
    assert _same(only.cpu().numpy()[ok], w[ok]) and (only.cpu().numpy()[live] > 0).all()


# ---- relocation values ----

COUNTS = (0, 1, 49, 50, 500, 2, 7, 0, 20)


@functools.lru_cache(maxsize=None)
def _values_case(n):
    rng = np.random.default_rng(n + 17)
    lo, hi = math.log(0.006 / 0.994), math.log((1 - 1e-7) / 1e-7)
    opacity = rng.uniform(lo, hi, (n, 1)).astype(np.float32)
    if n >= 63:
        opacity[:9, 0], opacity[9:18, 0] = np.float32(lo), np.float32(hi)   # both ends meet every count
    scaling = rng.uniform(np.log(1e-3), np.log(10.0), (n, 3)).astype(np.float32)
    count = np.array([COUNTS[i % len(COUNTS)] for i in range(n)], np.int32)
    return opacity, scaling, count, ref.relocation_values(opacity, scaling, count), ref.relocation_values_stock(opacity, scaling, count)


@pytest.mark.parametrize("n", SIZES)
def test_relocation_values_match(hip_device, n):
    from latentsplat_amd import relocation_values
    opacity, scaling, count, want, stock = _values_case(n)
    dev = hip_device
    args = (torch.from_numpy(opacity).to(dev), torch.from_numpy(scaling).to(dev), torch.from_numpy(count).to(dev))
    got_o, got_s = (t.cpu().numpy() for t in relocation_values(*args))
    again = relocation_values(*args)
    assert _same(got_o, again[0]) and _same(got_s, again[1])
    assert _same(args[0], opacity) and _same(args[1], scaling)              # the inputs are not touched
    assert got_o.shape == opacity.shape and got_s.shape == scaling.shape
    keep = count == 0
    assert _same(got_o[keep], opacity[keep]) and _same(got_s[keep], scaling[keep])
    show = f"n={n}:"
    _held("opacity", got_o[~keep], want[0][~keep], stock[0][~keep], show)
    _held("scaling", got_s[~keep], want[1][~keep], stock[1][~keep], show)
    # (n,) opacities are taken as well
    flat = relocation_values(args[0].reshape(-1), args[1], args[2])[0]
    assert flat.shape == (n,) and _same(flat, got_o.reshape(-1))


# ---- relocation and growth over whole tables ----

def _tables(dev, inp, moments, rows=None):
    """Device copies (optionally grown to ``rows`` rows, the new ones poisoned with NaN) and the (tensor, role) list."""
    def up(a):
        t = torch.from_numpy(a).to(dev)
        if rows is not None:
            grown = torch.full((rows,) + tuple(t.shape[1:]), float("nan"), dtype=torch.float32, device=dev)
            grown[:t.shape[0]] = t
            t = grown
        return t
    params = {k: up(inp[k]) for k in ref.PARAMS}
    moms = {(k, m): up(moments[k][m]) for k in ref.PARAMS for m in ref.MOMENTS} if moments is not None else {}
    tables = [(params[k], ref.ROLES[k]) for k in ref.PARAMS] + [(t, "moment") for t in moms.values()]
    return params, moms, tables


def _check_apply(n, inp, moments, params, moms, idx, count, dest, growth, show):
    src_rows = count > 0
    valid = idx >= 0
    dst = (n + np.arange(idx.shape[0]))[valid] if growth else dest[valid]
    src = idx[valid]
    assert src_rows[src].all() and not src_rows[dst[dst < n]].any()
    want = ref.relocation_values(inp["opacity"], inp["scaling"], count)
    stock = ref.relocation_values_stock(inp["opacity"], inp["scaling"], count)
    untouched = np.ones(n, bool)
    untouched[src_rows] = False
    untouched[dst[dst < n]] = False
    after = {k: t.cpu().numpy() for k, t in params.items()}
    for k in ref.PARAMS:
        a, b = after[k], inp[k]
        assert _same(a[:n][untouched], b[untouched]), (show, k)              # rows no draw names
        if ref.ROLES[k] == "copy":
            assert _same(a[:n][src_rows], b[src_rows]), (show, k)            # a source keeps its copied columns
            assert _same(a[dst], b[src]), (show, k)                          # a destination is its source
        else:
            _held(k, a[:n][src_rows], want[0 if k == "opacity" else 1][src_rows], stock[0 if k == "opacity" else 1][src_rows], show)
            assert _same(a[dst], a[src]), (show, k)                          # ... with the bits of the source's new values
    for (k, m), t in moms.items():
        a, b = t.cpu().numpy(), moments[k][m]
        assert _same(a[:n][untouched], b[untouched]), (show, k, m)
        assert not _bits(a[:n][src_rows]).any(), (show, k, m)                # source moments: exactly +0
        if growth:
            assert not _bits(a[n:]).any(), (show, k, m)                      # a new row starts at 0
        else:
            assert _same(a[dst], b[dst]), (show, k, m)                       # a relocated row keeps its own


@pytest.mark.parametrize("with_moments", [False, True])
@pytest.mark.parametrize("n", SIZES[1:])
def test_relocation_matches(hip_device, n, with_moments):
    from latentsplat_amd.mcmc import apply_relocation, classify_dead, dead_logit, sample_by_weight
    dev = hip_device
    K = (1, 4, 16)[(SIZES.index(n) + with_moments) % 3]
    inp, moments = ref.scene_inputs(n, seed=n, sh_rest=K - 1)
    moments = moments if with_moments else None
    params, moms, tables = _tables(dev, inp, moments)
    weights, dead, counts = classify_dead(params["opacity"], dead_logit(0.005))
    n_dead, n_alive = counts.cpu().numpy().view(np.uint32).tolist()
    want_w, want_dead, want_counts = ref.classify(inp["opacity"], ref.dead_logit(0.005))
    assert [n_dead, n_alive] == want_counts.tolist()
    show = f"n={n} K={K} moments={with_moments} dead={n_dead}:"
    print(show)
    if n_dead == 0 or n_alive == 0:
        return
    u = torch.rand(n_dead, dtype=torch.float64, generator=torch.Generator().manual_seed(n)).to(dev)
    idx, count = sample_by_weight(weights, u)
    apply_relocation(tables, n, idx, count, dead[:n_dead], 0.005)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(idx, ref.sample(weights.cpu().numpy(), u.cpu().numpy())[0])
    if n >= 1000:
        assert count.max() >= 2                              # some source is drawn more than once
    _check_apply(n, inp, moments, params, moms, idx, count, want_dead, False, show)


@pytest.mark.parametrize("with_moments", [False, True])
@pytest.mark.parametrize("n", SIZES[1:])
def test_growth_matches(hip_device, n, with_moments):
    from latentsplat_amd.mcmc import apply_relocation, classify_dead, sample_by_weight
    dev = hip_device
    K = (1, 4, 16)[(SIZES.index(n) + with_moments + 1) % 3]
    inp, moments = ref.scene_inputs(n, seed=n + 1, sh_rest=K - 1, dead_fraction=0.0)
    moments = moments if with_moments else None
    m = n // 20 + 1
    params, moms, tables = _tables(dev, inp, moments, rows=n + m)
    weights, _, _ = classify_dead(params["opacity"][:n], -math.inf, want_dead=False)
    u = torch.rand(m, dtype=torch.float64, generator=torch.Generator().manual_seed(n)).to(dev)
    idx, count = sample_by_weight(weights, u)
    apply_relocation(tables, n, idx, count, None, 0.005)
    show = f"n={n} m={m} K={K} moments={with_moments}:"
    print(show)
    _check_apply(n, inp, moments, params, moms, idx.cpu().numpy(), count.cpu().numpy(), None, True, show)
    assert all(torch.isfinite(t).all() for t in params.values())             # every new row was written


def test_skipped_draws_touch_nothing(hip_device):
    """idx = -1 (a scene whose weights are all 0): nothing is relocated, nothing grows, nothing changes."""
    from latentsplat_amd.mcmc import apply_relocation
    dev = hip_device
    n, m = 300, 40
    inp, moments = ref.scene_inputs(n, seed=5, sh_rest=3)
    idx = torch.full((m,), -1, dtype=torch.int32, device=dev)
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    params, moms, tables = _tables(dev, inp, moments)
    apply_relocation(tables, n, idx, count, torch.arange(m, dtype=torch.int32, device=dev), 0.005)
    for k in ref.PARAMS:
        assert _same(params[k], inp[k])
    for (k, mm), t in moms.items():
        assert _same(t, moments[k][mm])


def test_relocation_is_repeatable_and_stream_independent(hip_device):
    from latentsplat_amd.mcmc import apply_relocation, classify_dead, dead_logit, sample_by_weight
    dev = hip_device
    inp, moments = ref.scene_inputs(BIG, seed=3, sh_rest=15)
    u = torch.rand(BIG, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)

    def run():
        params, moms, tables = _tables(dev, inp, moments)
        weights, dead, counts = classify_dead(params["opacity"], dead_logit(0.005))
        n_dead = int(counts[0])
        idx, count = sample_by_weight(weights, u[:n_dead])
        apply_relocation(tables, BIG, idx, count, dead[:n_dead], 0.005)
        return [t.cpu().numpy() for t, _ in tables] + [idx.cpu().numpy(), count.cpu().numpy()]

    first, second = run(), run()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for other in (second, third):
        for a, b in zip(first, other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- noise ----

STEP_SCALE = 5e5 * 1.6e-4


@functools.lru_cache(maxsize=None)
def _noise_case(n):
    inp = ref.noise_inputs(n, seed=n)
    args = (inp["opacity"], inp["scaling"], inp["rotation"], inp["eps"], STEP_SCALE)
    return inp, ref.noise_increment(*args), ref.noise_increment_stock(*args).numpy()


def _noise(dev, inp, xyz):
    from latentsplat_amd import inject_noise
    x = torch.from_numpy(xyz).to(dev)
    inject_noise(x, *(torch.from_numpy(inp[k]).to(dev) for k in ("opacity", "scaling", "rotation", "eps")), STEP_SCALE)
    return x


@pytest.mark.parametrize("n", SIZES)
def test_noise_matches(hip_device, n):
    _check_noise(hip_device, n)


def test_noise_matches_past_the_grid_cap(hip_device):
    """2049 workgroups' worth of rows on a grid capped at 2048: the first three lanes take a second row, and it moves."""
    inp, want, stock = _noise_case(PAST_THE_GRID)
    bar = max(MARGIN * np.abs(stock - want).max(), FLOOR * np.abs(want).max())
    assert np.abs(want[GRID_ROWS:]).max() > 10 * bar         # a row left where it was would be far off the bar
    _check_noise(hip_device, PAST_THE_GRID)


def _check_noise(hip_device, n):
    inp, want, stock = _noise_case(n)
    show = f"n={n}:"
    inc = _noise(hip_device, inp, np.zeros((n, 3), np.float32)).cpu().numpy()
    _held("increment", inc, want, stock, show)
    if n >= 1000:                                            # the factor's whole transition is in the data
        f = 1.0 / (1.0 + np.exp(-100.0 * (1.0 / (1.0 + np.exp(inp["opacity"].astype(np.float64))) - 0.995)))
        assert (f < 1e-6).any() and (f > 0.5).any() and ((f > 0.05) & (f < 0.5)).any()
    # with real positions: the float32 sum of the position and that increment, one rounding
    moved = _noise(hip_device, inp, inp["xyz"]).cpu().numpy()
    assert _same(moved, inp["xyz"] + inc), show
    assert _same(moved, _noise(hip_device, inp, inp["xyz"])), show            # a second call gives the same bits


def test_noise_leaves_a_row_with_a_bad_scale_alone(hip_device):
    inp = {k: v.copy() for k, v in ref.noise_inputs(300, seed=1).items()}
    inp["opacity"][:] = -10.0                                # f = step_scale: every row moves
    inp["scaling"][5, 1] = np.inf
    inp["scaling"][6, 0] = np.nan
    inp["scaling"][7, 2] = 60.0                              # exp(120) overflows float32
    inp["rotation"][8] = 0.0                                 # 0 / 0
    moved = _noise(hip_device, inp, inp["xyz"]).cpu().numpy()
    bad = np.zeros(300, bool)
    bad[5:9] = True
    assert _same(moved[bad], inp["xyz"][bad])
    assert np.isfinite(moved).all() and (moved[~bad] != inp["xyz"][~bad]).any(1).all()


def test_noise_on_a_side_stream_and_captured(hip_device):
    from latentsplat_amd import inject_noise
    dev = hip_device
    inp, _, _ = _noise_case(BIG)
    rest = [torch.from_numpy(inp[k]).to(dev) for k in ("opacity", "scaling", "rotation", "eps")]
    fresh = lambda: torch.from_numpy(inp["xyz"]).to(dev)
    eager = fresh()
    inject_noise(eager, *rest, STEP_SCALE)
    once = _bits(eager)
    inject_noise(eager, *rest, STEP_SCALE)                   # two eager calls
    side_xyz = fresh()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        inject_noise(side_xyz, *rest, STEP_SCALE)
    side.synchronize()
    assert np.array_equal(once, _bits(side_xyz))
    # captured once, replayed twice = two eager calls
    static, warm = fresh(), fresh()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        inject_noise(warm, *rest, STEP_SCALE)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inject_noise(static, *rest, STEP_SCALE)
    with torch.no_grad():
        static.copy_(torch.from_numpy(inp["xyz"]).to(dev))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(_bits(eager), _bits(static))


# ---- MCMCControl ----

G, W, VIEWS = 2000, 64, 2
RATES = dict(_xyz=1.6e-4, _features_dc=2.5e-3, _features_rest=2.5e-3 / 20, _opacity=5e-2, _scaling=5e-3, _rotation=1e-3)


def _views(sc, dev):
    from latentsplat_amd.rasterizer import build_view_table
    return build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                            torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False).detach()


def _optimizer(scene, which):
    from latentsplat_amd import SceneAdam
    groups = [dict(params=[p], lr=RATES[name], name=name) for name, p in scene.named_parameters() if p.numel()]
    return torch.optim.Adam(groups, lr=0.0, eps=1e-15) if which == "torch" else SceneAdam(groups, lr=0.0, eps=1e-15)


def _step(scene, control, opt, views, target):
    opt.zero_grad(set_to_none=True)
    color = scene.render(views, W, W)[0]
    loss = (color - target).abs().mean() + control.regularizer()
    loss.backward()
    opt.step()
    control.inject_noise(RATES["_xyz"], generator=None)
    return float(loss.detach())


def _clear_of(values, target, margin=1e-3):
    """``target`` moved to the middle of the widest gap among the values around it, so that no value lies within
    ``margin`` (relative) of it: a decision that float32 rounding of the sigmoid cannot flip."""
    v = np.unique(np.asarray(values, np.float64))
    at = int(np.searchsorted(v, target))
    lo, hi = max(at - 20, 0), min(at + 20, len(v) - 1)
    gaps = v[lo + 1:hi + 1] - v[lo:hi]
    j = lo + int(np.argmax(gaps))
    mid = 0.5 * (v[j] + v[j + 1])
    assert (np.abs(v - mid) > margin * abs(mid)).all()
    return float(mid)


@pytest.mark.parametrize("which", ["torch", "fused"])
def test_mcmc_control_end_to_end(hip_device, tmp_path, which):
    from latentsplat_amd import GaussianScene, MCMCControl
    dev = hip_device
    path = tmp_path / "scene.ply"
    sc, _, _ = sref.write_scene_file(path, G, W, VIEWS)
    scene = GaussianScene.from_ply(path, dev)
    views = _views(sc, dev)
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        target = scene.render(views, W, W)[0]
        faint = (torch.rand(G, generator=gen) < 0.2).to(dev)
        scene._opacity[faint] = -7.0 - torch.rand(int(faint.sum()), 1, generator=gen).to(dev)     # about 20 % below the threshold
    opt = _optimizer(scene, which)
    plain = MCMCControl(scene, cap_max=10 * G)
    for _ in range(3):
        _step(scene, plain, opt, views, target)

    o = 1 / (1 + np.exp(-scene._opacity.detach().cpu().numpy().astype(np.float64).reshape(-1)))
    min_opacity = _clear_of(o, 0.005)
    want_dead = int((o <= min_opacity).sum())
    assert 0.1 * G < want_dead < 0.3 * G
    control = MCMCControl(scene, cap_max=int(1.05 * G) + 50, min_opacity=min_opacity)
    before = {name: p for name, p in scene.named_parameters()}
    rows = scene.rows().clone()
    dead_rows = torch.from_numpy(o <= min_opacity).to(dev)
    moments = {name: {m: opt.state[p][m].clone() for m in ("exp_avg", "exp_avg_sq")} for name, p in before.items()}

    # relocate: the size and the parameter objects stay; dead is the float64 count
    res = control.relocate(opt, generator=torch.Generator(device=dev).manual_seed(7))
    print("relocate:", res)
    assert res == dict(dead=want_dead, alive=G - want_dead, relocated=want_dead)
    assert scene.num_gaussians == G and all(getattr(scene, name) is p for name, p in before.items())
    after = scene.rows()
    changed = (_bits(after) != _bits(rows)).any(1)
    assert changed[dead_rows.cpu().numpy()].all()
    for name, p in before.items():
        state = opt.state[p]
        assert float(state["step"]) == 3.0
        for m in ("exp_avg", "exp_avg_sq"):
            same = (state[m] == moments[name][m]).reshape(G, -1).all(1)
            assert same[dead_rows].all()                     # a relocated row keeps its own moments
            zeroed = ~same
            assert not state[m][zeroed].any() and zeroed.any()               # the sources lost theirs
    # ... every relocated row is now a copy of a live one
    live_xyz = {tuple(r) for r in rows[~dead_rows][:, :3].cpu().numpy().tolist()}
    assert all(tuple(r) in live_xyz for r in after[dead_rows][:, :3].cpu().numpy().tolist())

    # add_new: exactly min(cap_max, int(1.05 n)) rows; the optimizer is re-keyed and keeps its step
    res = control.add_new(opt, generator=torch.Generator(device=dev).manual_seed(8))
    n1 = min(control.cap_max, int(1.05 * G))
    print("add_new:", res)
    assert res == dict(added=n1 - G, n_in=G, n_out=n1) and scene.num_gaussians == n1 and n1 > G
    for name, p in scene.named_parameters():
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == n1 and p is not before[name]
        group = next(g for g in opt.param_groups if g["name"] == name)
        assert len(group["params"]) == 1 and group["params"][0] is p
        state = opt.state[p]
        assert float(state["step"]) == 3.0
        for m in ("exp_avg", "exp_avg_sq"):
            assert state[m].shape == p.shape and not state[m][G:].any() and state[m][:G].any()
    assert len(opt.state) == 6
    assert _same(scene.rows()[:G, :3], after[:, :3])         # the old rows keep their place
    loss = _step(scene, control, opt, views, target)
    assert np.isfinite(loss) and float(opt.state[scene._xyz]["step"]) == 4.0

    # up to the cap, then a no-op that leaves the scene bit-identical
    res = control.add_new(opt)
    assert res["n_out"] == control.cap_max == scene.num_gaussians
    held, rows = {name: p for name, p in scene.named_parameters()}, scene.rows().clone()
    res = control.add_new(opt)
    assert res == dict(added=0, n_in=control.cap_max, n_out=control.cap_max)
    assert _same(rows, scene.rows()) and all(getattr(scene, name) is p for name, p in held.items())

    # with no dead rows a relocation changes nothing
    nothing = MCMCControl(scene, cap_max=control.cap_max, min_opacity=0.0)
    res = nothing.relocate(opt)
    assert res == dict(dead=0, alive=control.cap_max, relocated=0) and _same(rows, scene.rows())

    # step = relocate + add_new; training goes on
    res = control.step(opt)
    assert res["n_in"] == res["n_out"] == control.cap_max and res["added"] == 0 and res["relocated"] == res["dead"]
    for _ in range(2):
        loss = _step(scene, control, opt, views, target)
    assert np.isfinite(loss) and all(torch.isfinite(p).all() for p in scene.parameters())


def test_mcmc_control_refuses_what_it_cannot_take(hip_device):
    from latentsplat_amd import GaussianScene, MCMCControl
    dev = hip_device
    inp, _ = ref.scene_inputs(50, seed=0, sh_rest=0)
    scene = GaussianScene.from_tensors(**{k: torch.from_numpy(inp[k]) for k in ref.PARAMS}).to(dev)
    control = MCMCControl(scene, cap_max=60)
    sgd = torch.optim.SGD(scene.parameters(), lr=0.1, momentum=0.9)
    assert control.step(sgd)["n_out"] == 52                  # no state yet: allowed, and re-keyed
    assert sgd.param_groups[0]["params"][0] is scene._xyz
    scene._xyz.sum().backward()
    sgd.step()
    with pytest.raises(_lib.LsrError, match="Adam"):
        control.relocate(sgd)
    with pytest.raises(_lib.LsrError, match="Adam"):
        control.add_new(sgd)
    with pytest.raises(_lib.LsrError, match="cap_max"):
        MCMCControl(scene, cap_max=0)


def test_fit_tool_with_the_mcmc_strategy(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, G, W, VIEWS)
    out = tmp_path / "fit"
    K = 1100
    res = fit_ply.main([str(path), "--out", str(out), "--views", "3", "--size", "48", "--steps", "20", "--drop", "0.5",
                        "--strategy", "mcmc", "--cap-max", str(K), "--densify-interval", "5"])
    print("fit:", {k: v for k, v in res.items() if k != "mcmc_events"})
    for e in res["mcmc_events"]:
        print("  event:", e)
    assert json.load(open(out / "fit.json")) == res
    assert [e["step"] for e in res["mcmc_events"]] == [5, 10, 15, 20] and res["strategy"] == "mcmc" and res["cap_max"] == K
    n_in = res["gaussians_first"]
    assert 0 < n_in < G
    for e in res["mcmc_events"]:
        assert set(e) >= {"step", "dead", "relocated", "added", "n_out"}
        assert e["n_in"] == n_in and e["n_out"] == min(K, int(1.05 * n_in)) <= int(1.05 * n_in) and e["added"] == e["n_out"] - n_in
        n_in = e["n_out"]
    assert res["gaussians_last"] == res["gaussians"] == n_in <= K and res["gaussians_last"] > res["gaussians_first"]
    assert "densify_events" not in res
    fitted = GaussianScene.from_ply(out / "point_cloud.ply", hip_device)
    assert fitted.num_gaussians == res["gaussians_last"]
    assert all(torch.isfinite(p).all() for p in fitted.parameters())
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
