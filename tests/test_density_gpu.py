"""Adaptive density control on the MI355X: lsr_density_accumulate, lsr_densify_plan and lsr_densify_apply against the
references of tests/density_ref.py, DensityControl end to end, and the fitting tool with densification on.

Exact: the map and the counts, every COPY table, the kept and clone rows of the XYZ / SCALING tables (a gather, bit for
bit), the zeros of ZERO_NEW tables on new rows, denom and max_radii.  On a bar: grad_accum and the children's xyz and
scaling.  The bar is that of tests/test_photometric_gpu.py: the kernel's largest error against float64 must be within
4 x the largest error of the float32 torch-CPU composition (the published sequence, tests/density_ref.py) on the same
inputs, with a floor of 2^-20 of the quantity's scale (its largest magnitude).  Every element is on the bar.

Sizes: the constants of csrc/density.hip are kPlanChunk = 256 Gaussians per classify / emit workgroup, kPlanScanThreads =
256 lanes of the one workgroup that scans the chunk sums, kApplyElems = 4096 destination floats per gather workgroup and
kDensityThreads = 256 per accumulate workgroup.  70 001 Gaussians are 274 chunks: more than one workgroup in every
kernel, and more chunk sums than scan lanes, so that lanes walk two sums each (the scan's second level).  524 291
Gaussians (PAST_THE_GRID, one accumulate and one plan-and-apply case) are past the accumulate grid's cap of 2048
workgroups and are 2049 chunks, nine sums per scan lane: the trips a scene of half a million Gaussians takes."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import density_ref as ref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu

PLAN_CHUNK, SCAN_THREADS, APPLY_ELEMS = 256, 256, 4096
BIG = 70_001
assert BIG > PLAN_CHUNK * SCAN_THREADS and 3 * BIG > APPLY_ELEMS
SIZES = [0, 1, 63, 64, 65, 255, 257, 1000, BIG]
# The accumulate grid is capped at kDensityMaxBlocks = 2048 workgroups of 256 lanes; past that, lanes take a second row.
# The same size is 2049 chunks of the plan: each lane of the scan walks ceil(2049 / 256) = 9 chunk sums, the last lanes
# none.  One case each, outside the cross-products, on the narrowest tables (K = 1).
GRID_ROWS = 2048 * 256
PAST_THE_GRID = GRID_ROWS + 3
SH_COEFFS = (1, 4, 16)
FLOOR = 2.0 ** -20
MARGIN = 4.0
FLT_MAX = 3.4028234663852886e38
PARENT = (1 << ref.KIND_SHIFT) - 1


def _held(name, got, want, stock, show):
    got, want, stock = (np.asarray(a, np.float64) for a in (got, want, stock))
    if want.size == 0:
        assert got.size == 0
        return
    scale = float(np.abs(want).max())
    err, err_stock = float(np.abs(got - want).max()), float(np.abs(stock - want).max())
    bar = max(MARGIN * err_stock, FLOOR * scale)
    print(f"{show} {name:10s} kernel {err:.3e}  composition {err_stock:.3e}  bar {bar:.3e}  ({want.size} elements)")
    assert err <= bar, (show, name, err, err_stock, bar)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(inp, dev, keys):
    return {k: torch.from_numpy(inp[k]).to(dev) for k in keys}


# ---- the statistics ----

@functools.lru_cache(maxsize=None)
def _stats_case(n, V):
    rng = np.random.default_rng(1000 * V + n)
    grad = (rng.normal(size=(V, n, 3)) * np.exp(rng.uniform(-8, 0, (V, n, 1)))).astype(np.float32)
    radii = np.where(rng.uniform(size=(V, n)) < 0.3, 0, rng.integers(-2, 60, (V, n))).astype(np.int32)
    start = (rng.uniform(0, 2, n).astype(np.float32), rng.integers(0, 9, n).astype(np.float32), rng.integers(0, 30, n).astype(np.float32))
    return grad, radii, start, ref.accumulate_direct(grad, radii, *start), ref.accumulate_literal(grad, radii, *start)


@pytest.mark.parametrize("V", [1, 4, 16])
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_matches(hip_device, n, V):
    _check_accumulate(hip_device, n, V)


def test_accumulate_past_the_grid_cap(hip_device):
    """2049 workgroups' worth of rows on a grid capped at 2048: the first three lanes take a second row."""
    _, _, start, want, _ = _stats_case(PAST_THE_GRID, 2)
    assert (want[1][GRID_ROWS:] != start[1][GRID_ROWS:]).any()             # ... and those rows have something to add
    _check_accumulate(hip_device, PAST_THE_GRID, 2)


def _check_accumulate(hip_device, n, V):
    from latentsplat_amd import accumulate_density_stats
    grad, radii, start, want, stock = _stats_case(n, V)
    runs = []
    for shape in ((n, 1), (n,)):
        acc, den, mr = (torch.from_numpy(s).to(hip_device).reshape(shape).contiguous() for s in start)
        accumulate_density_stats(torch.from_numpy(grad).to(hip_device), torch.from_numpy(radii).to(hip_device), acc, den, mr)
        runs.append((acc, den, mr))
    acc, den, mr = (t.cpu().numpy().reshape(-1) for t in runs[0])
    assert np.array_equal(den, want[1]) and np.array_equal(mr, want[2])
    _held("grad_accum", acc, want[0], stock[0], f"n={n} V={V}:")
    for a, b in zip(*runs):                                  # a second call gives the same bits
        assert np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def test_accumulate_on_a_side_stream_and_captured(hip_device):
    from latentsplat_amd import accumulate_density_stats
    dev = hip_device
    n, V = BIG, 4
    grad, radii, start, _, _ = _stats_case(n, V)
    g, r = torch.from_numpy(grad).to(dev), torch.from_numpy(radii).to(dev)
    fresh = lambda: [torch.from_numpy(s).to(dev) for s in start]
    eager = fresh()
    accumulate_density_stats(g, r, *eager)
    once = [_bits(t) for t in eager]
    accumulate_density_stats(g, r, *eager)                   # two eager calls
    side_stats = fresh()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        accumulate_density_stats(g, r, *side_stats)
    side.synchronize()
    for a, b in zip(once, side_stats):
        assert np.array_equal(a, _bits(b))
    # captured once, replayed twice = two eager calls
    static = fresh()
    warm = fresh()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        accumulate_density_stats(g, r, *warm)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        accumulate_density_stats(g, r, *static)
    with torch.no_grad():
        for t, s in zip(static, start):
            t.copy_(torch.from_numpy(s).to(dev))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize(dev)
    for a, b in zip(eager, static):
        assert np.array_equal(_bits(a), _bits(b))


def test_wrappers_refuse_what_they_cannot_take(hip_device):
    from latentsplat_amd import DensityControl, GaussianScene, accumulate_density_stats
    dev = hip_device
    inp = ref.make_inputs(10, 0, sh_rest=0)
    scene = GaussianScene.from_tensors(**{k: torch.from_numpy(inp[k]) for k in ref.PARAMS}).to(dev)
    control = DensityControl(scene)
    radii = torch.ones((2, 10), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.LsrError, match="already summed"):
        control.update(torch.zeros((10, 3), device=dev), radii)
    with pytest.raises(_lib.LsrError, match="int32"):
        accumulate_density_stats(torch.zeros((2, 10, 3), device=dev), radii.float(), control.xyz_gradient_accum, control.denom, control.max_radii2D)
    sgd = torch.optim.SGD(scene.parameters(), lr=0.1, momentum=0.9)
    control.densify_and_prune(sgd, 1.0, 0.0, 1.0, 0)         # no state yet: allowed
    assert sgd.param_groups[0]["params"][0] is scene._xyz
    scene._xyz.sum().backward()
    sgd.step()
    with pytest.raises(_lib.LsrError, match="Adam"):
        control.densify_and_prune(sgd, 1.0, 0.0, 1.0, 0)


# ---- plan and apply ----

@functools.lru_cache(maxsize=None)
def _case(n, N, size_pruning, K):
    """Inputs, eps, moments and the references: computed once, shared, never modified."""
    inp = ref.make_inputs(n, seed=7 * n + K, sh_rest=K - 1)
    thr = ref.thresholds(size_pruning)
    map_, counts = ref.direct_map(inp, thr, N)
    rng = np.random.default_rng(n + N)
    eps = rng.normal(size=(N * int(counts[2]), 3)).astype(np.float32)
    moments = {k: dict(exp_avg=rng.normal(size=inp[k].shape).astype(np.float32),
                       exp_avg_sq=rng.uniform(size=inp[k].shape).astype(np.float32)) for k in ref.PARAMS}
    rows = ref.direct_rows(inp, map_, counts, N, eps)
    stock, _, stock_map, _ = ref.literal_sequence(inp, thr, N, eps, torch.float32, "cpu")
    assert np.array_equal(stock_map, map_)                   # (the composition's float32 decisions are the float64 ones)
    return inp, thr, map_, counts, eps, moments, rows, {k: v.numpy() for k, v in stock.items()}


def _run(dev, inp, thr, N, eps, moments):
    from latentsplat_amd import apply_densify, plan_densify
    d = _dev(inp, dev, ref.PARAMS + ("grad_accum", "denom", "max_radii"))
    map_, counts = plan_densify(d["opacity"], d["scaling"], d["grad_accum"], d["denom"], d["max_radii"], n_split=N, **thr)
    c = counts.cpu().numpy().view(np.uint32)                 # the one host read
    n_out = int(c[3])
    rules = dict(xyz="xyz", scaling="scaling")
    tables = [(d[k], rules.get(k, "copy")) for k in ref.PARAMS]
    if moments is not None:
        tables += [(torch.from_numpy(moments[k][m]).to(dev), "zero_new") for k in ref.PARAMS for m in ("exp_avg", "exp_avg_sq")]
    out = apply_densify(map_, counts, n_out, tables, n_split=N, scaling=d["scaling"], rotation=d["rotation"],
                        eps=torch.from_numpy(eps).to(dev))
    return map_[:n_out].cpu().numpy().view(np.uint32), c, [t.cpu().numpy() for t in out]


def _check(n, N, got, inp, map_, counts, moments, rows, stock, show):
    got_map, got_counts, out = got
    assert np.array_equal(got_counts, counts), (show, got_counts, counts)
    assert np.array_equal(got_map, map_), show
    parent, kind = (map_ & PARENT).astype(np.int64), map_ >> ref.KIND_SHIFT
    new = kind >= 2
    for k, t in zip(ref.PARAMS, out):
        gathered = inp[k][parent]
        assert t.shape == gathered.shape and t.dtype == np.float32
        if k in ("xyz", "scaling"):
            assert np.array_equal(_bits(t[~new]), _bits(gathered[~new])), (show, k)
            _held(k + " children", t[new], rows[k][new], stock[k][new], show)
        else:
            assert np.array_equal(_bits(t), _bits(gathered)), (show, k)
    if moments is not None:
        names = [(k, m) for k in ref.PARAMS for m in ("exp_avg", "exp_avg_sq")]
        for (k, m), t in zip(names, out[len(ref.PARAMS):]):
            assert np.array_equal(_bits(t[kind == 0]), _bits(moments[k][m][parent[kind == 0]])), (show, k, m)
            assert not _bits(t[kind != 0]).any(), (show, k, m)               # exactly +0


@pytest.mark.parametrize("size_pruning", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_plan_and_apply_match(hip_device, n, N, size_pruning):
    i = SIZES.index(n)
    K = SH_COEFFS[(i + N) % 3]                               # 70 001 meets K = 1, 4 and 16 (N = 1, 2, 3)
    with_moments = (i + N + size_pruning) % 2 == 0
    inp, thr, map_, counts, eps, moments, rows, stock = _case(n, N, size_pruning, K)
    show = f"n={n} N={N} size={size_pruning} K={K} moments={with_moments}:"
    got = _run(hip_device, inp, thr, N, eps, moments if with_moments else None)
    print(show, "counts", got[1].tolist(), ref.outcomes(map_, n))
    if n >= 1000:
        assert min(ref.outcomes(map_, n).values()) > 0
    _check(n, N, got, inp, map_, counts, moments if with_moments else None, rows, stock, show)


def test_both_moment_settings_and_every_width_meet_the_large_size(hip_device):
    """(the parametrisation above rotates K and the moments over the cases; this pins the two combinations it leaves out
    at the size with more than one workgroup per table: degree 3 with moments, degree 0 with moments)"""
    for N, K in ((2, 16), (3, 1)):
        inp, thr, map_, counts, eps, moments, rows, stock = _case(BIG, N, True, K)
        show = f"n={BIG} N={N} K={K} with moments:"
        _check(BIG, N, _run(hip_device, inp, thr, N, eps, moments), inp, map_, counts, moments, rows, stock, show)


def test_plan_and_apply_past_256_chunks_per_scan_lane(hip_device):
    """PAST_THE_GRID rows are 2049 chunks: k_densify_scan's first 228 lanes walk nine sums each (the last of them six) and the rest none.  K = 1
    (no f_rest), N = 2, size pruning on, with the moments: the map and the counts exact, the children on the bar."""
    n, N, K = PAST_THE_GRID, 2, 1
    chunks = -(-n // PLAN_CHUNK)
    assert chunks == 2049 and -(-chunks // SCAN_THREADS) == 9
    inp, thr, map_, counts, eps, moments, rows, stock = _case(n, N, True, K)
    show = f"n={n} N={N} size=True K={K} moments=True:"
    got = _run(hip_device, inp, thr, N, eps, moments)
    print(show, "counts", got[1].tolist(), ref.outcomes(map_, n))
    assert min(ref.outcomes(map_, n).values()) > 0
    _check(n, N, got, inp, map_, counts, moments, rows, stock, show)


SPECIAL = dict(
    nothing=dict(grad_threshold=FLT_MAX, dense_extent=1.0, min_opacity=0.0, max_screen_size=0.0, world_limit=0.0),
    all_pruned=dict(grad_threshold=FLT_MAX, dense_extent=1.0, min_opacity=2.0, max_screen_size=0.0, world_limit=0.0),
    all_cloned=dict(grad_threshold=0.0, dense_extent=1e30, min_opacity=0.0, max_screen_size=0.0, world_limit=0.0),
    all_split=dict(grad_threshold=0.0, dense_extent=0.0, min_opacity=0.0, max_screen_size=0.0, world_limit=0.0))


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("which", list(SPECIAL))
def test_special_scenes(hip_device, which, N):
    n = 1000
    inp = ref.make_inputs(n, seed=3, sh_rest=3)
    thr = SPECIAL[which]
    map_, counts = ref.direct_map(inp, thr, N)
    rng = np.random.default_rng(N)
    eps = rng.normal(size=(N * int(counts[2]), 3)).astype(np.float32)
    moments = {k: dict(exp_avg=rng.normal(size=inp[k].shape).astype(np.float32),
                       exp_avg_sq=rng.uniform(size=inp[k].shape).astype(np.float32)) for k in ref.PARAMS}
    got_map, got_counts, out = got = _run(hip_device, inp, thr, N, eps, moments)
    want = dict(nothing=[n, 0, 0, n], all_pruned=[0, 0, 0, 0], all_cloned=[n, n, 0, 2 * n], all_split=[0, 0, n, N * n])[which]
    assert got_counts.tolist() == want == counts.tolist()
    if which == "nothing":
        assert np.array_equal(got_map, np.arange(n, dtype=np.uint32))
        for t, src in zip(out, [inp[k] for k in ref.PARAMS] + [moments[k][m] for k in ref.PARAMS for m in ("exp_avg", "exp_avg_sq")]):
            assert np.array_equal(_bits(t), _bits(src))
    elif which == "all_pruned":
        assert all(t.shape[0] == 0 for t in out)
    else:
        rows = ref.direct_rows(inp, map_, counts, N, eps)
        stock = ref.literal_sequence(inp, thr, N, eps, torch.float32, "cpu")[0]
        _check(n, N, got, inp, map_, counts, moments, rows, {k: v.numpy() for k, v in stock.items()}, f"{which} N={N}:")


def test_repeatable_and_stream_independent(hip_device):
    dev = hip_device
    inp, thr, map_, counts, eps, moments, _, _ = _case(BIG, 2, True, 4)
    first = _run(dev, inp, thr, 2, eps, moments)
    second = _run(dev, inp, thr, 2, eps, moments)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = _run(dev, inp, thr, 2, eps, moments)
    side.synchronize()
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])
        for a, b in zip(first[2], other[2]):
            assert np.array_equal(_bits(a), _bits(b))


# ---- DensityControl ----

G, W, VIEWS = 2000, 64, 2


def _views(sc, dev):
    from latentsplat_amd.rasterizer import build_view_table
    return build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                            torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False).detach()


def _optimizer(scene):
    rates = dict(_xyz=1.6e-4, _features_dc=2.5e-3, _features_rest=2.5e-3 / 20, _opacity=5e-2, _scaling=5e-3, _rotation=1e-3)
    groups = [dict(params=[p], lr=rates[name], name=name) for name, p in scene.named_parameters() if p.numel()]
    return torch.optim.Adam(groups, lr=0.0, eps=1e-15)


def _step(scene, control, opt, views, target, dev):
    opt.zero_grad(set_to_none=True)
    means2D = torch.zeros((VIEWS, scene.num_gaussians, 3), device=dev, requires_grad=True)
    color, _, _, _, radii = scene.render(views, W, W, means2D=means2D)
    loss = (color - target).abs().mean()
    loss.backward()
    opt.step()
    control.update(means2D.grad, radii)
    return float(loss.detach())


def _clear_of(values, target, margin=1e-3):
    """``target`` moved to the middle of the widest gap among the values around it, so that no value lies within
    ``margin`` (relative) of it: a decision that float32 rounding of exp / sigmoid cannot flip."""
    v = np.unique(np.asarray(values, np.float64))
    at = int(np.searchsorted(v, target))
    lo, hi = max(at - 20, 0), min(at + 20, len(v) - 1)
    gaps = v[lo + 1:hi + 1] - v[lo:hi]
    j = lo + int(np.argmax(gaps))
    mid = 0.5 * (v[j] + v[j + 1])
    assert (np.abs(v - mid) > margin * abs(mid)).all()
    return float(mid)


def test_density_control_end_to_end(hip_device, tmp_path):
    from latentsplat_amd import DensityControl, GaussianScene
    dev = hip_device
    path = tmp_path / "scene.ply"
    sc, _, _ = sref.write_scene_file(path, G, W, VIEWS)
    scene = GaussianScene.from_ply(path, dev)
    views = _views(sc, dev)
    with torch.no_grad():
        target = scene.render(views, W, W)[0]
        gen = torch.Generator().manual_seed(0)
        for name, p in scene.named_parameters():
            p.add_((torch.randn(p.shape, generator=gen) * dict(_xyz=0.01, _opacity=0.5).get(name, 0.05)).to(dev))
    opt = _optimizer(scene)
    control = DensityControl(scene)
    for _ in range(3):
        _step(scene, control, opt, views, target, dev)
    assert control.xyz_gradient_accum.shape == (G, 1) and control.denom.shape == (G, 1) and control.max_radii2D.shape == (G,)
    assert float(control.denom.max()) == 3 * VIEWS and float(control.max_radii2D.max()) > 0

    # thresholds in the data's own range, each clear of every value it is compared with
    N = 2
    stats = dict(grad_accum=control.xyz_gradient_accum.cpu().numpy(), denom=control.denom.cpu().numpy(),
                 max_radii=control.max_radii2D.cpu().numpy())
    before = {k: getattr(scene, "_" + k).detach().cpu().numpy().copy() for k in ref.PARAMS}
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(stats["grad_accum"].astype(np.float64) / stats["denom"], nan=0.0).reshape(-1)
    smax = np.exp(before["scaling"].astype(np.float64)).max(1)
    o = 1 / (1 + np.exp(-before["opacity"].astype(np.float64).reshape(-1)))
    max_grad = _clear_of(avg, np.quantile(avg, 0.7))
    min_opacity = _clear_of(o, np.quantile(o, 0.1))
    extent = None
    for q in np.linspace(0.4, 0.6, 21):                      # dense_extent = 0.01 extent near the median size ...
        dense = _clear_of(smax, np.quantile(smax, q))
        world = 10.0 * dense                                 # ... and world_limit = 0.1 extent clear of what it is compared with
        if all((np.abs(x - world) > 1e-3 * world).all() for x in (smax, smax / (0.8 * N))) and (smax > world).any():
            extent = dense / 0.01
            break
    assert extent is not None
    size = float(np.median(stats["max_radii"][stats["max_radii"] > 0])) + 0.5      # radii are integers
    thr = dict(grad_threshold=max_grad, dense_extent=0.01 * extent, min_opacity=min_opacity, max_screen_size=size,
               world_limit=0.1 * extent)
    moments = {k: {m: opt.state[getattr(scene, "_" + k)][m].cpu().numpy().copy() for m in ("exp_avg", "exp_avg_sq")} for k in ref.PARAMS}
    steps = {k: float(opt.state[getattr(scene, "_" + k)]["step"]) for k in ref.PARAMS}
    inp = dict(before, **stats)
    want_map, want_counts = ref.direct_map(inp, thr, N)

    counts = control.densify_and_prune(opt, max_grad, min_opacity, extent, size, n_split=N,
                                       generator=torch.Generator(device=dev).manual_seed(7))
    print("densify_and_prune:", counts, ref.outcomes(want_map, G))
    assert min(ref.outcomes(want_map, G).values()) > 0
    eps = torch.randn((N * counts["split_parents"], 3), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    lit, lit_moments, lit_map, _ = ref.literal_sequence(inp, thr, N, eps.cpu().numpy(), torch.float32, dev, moments)
    n_out = counts["n_out"]
    assert [counts[k] for k in ("kept", "clones", "split_parents", "n_out")] == want_counts.tolist() and counts["n_in"] == G
    got_map = control.last_map.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_map, want_map) and np.array_equal(got_map, lit_map)
    kind = want_map >> ref.KIND_SHIFT
    assert scene.num_gaussians == n_out and scene.active_sh_degree == 1
    for k in ref.PARAMS:
        p = getattr(scene, "_" + k)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == n_out
        group = next(g for g in opt.param_groups if g["name"] == "_" + k)
        assert len(group["params"]) == 1 and group["params"][0] is p
        state = opt.state[p]
        assert float(state["step"]) == steps[k] == 3.0
        got, want = p.detach().cpu().numpy(), lit[k].cpu().numpy()
        if k in ("xyz", "scaling"):
            assert np.array_equal(_bits(got[kind < 2]), _bits(want[kind < 2])), k
            # the children: float32 on both sides, a few roundings apart
            assert np.allclose(got[kind >= 2], want[kind >= 2], rtol=1e-5, atol=1e-5 * np.abs(want).max()), k
        else:
            assert np.array_equal(_bits(got), _bits(want)), k
        for m in ("exp_avg", "exp_avg_sq"):
            t = state[m].cpu().numpy()
            assert t.shape == got.shape
            assert np.array_equal(_bits(t), _bits(lit_moments[k][m].cpu().numpy())), (k, m)
            assert not _bits(t[kind != 0]).any() and np.abs(t[kind == 0]).max() > 0
    assert len(opt.state) == 6
    for t, shape in ((control.xyz_gradient_accum, (n_out, 1)), (control.denom, (n_out, 1)), (control.max_radii2D, (n_out,))):
        assert tuple(t.shape) == shape and not t.any()

    # training goes on
    for _ in range(2):
        loss = _step(scene, control, opt, views, target, dev)
    assert np.isfinite(loss) and float(control.denom.max()) == 2 * VIEWS

    # a densification that selects and prunes nothing changes nothing
    with torch.no_grad():
        image = scene.render(views, W, W)[0]
    rows = scene.rows()
    n_now = scene.num_gaussians
    counts = control.densify_and_prune(opt, float("inf"), 0.0, extent, 0)
    assert counts == dict(kept=n_now, clones=0, split_parents=0, n_out=n_now, n_in=n_now)
    with torch.no_grad():
        again = scene.render(views, W, W)[0]
    assert np.array_equal(_bits(rows), _bits(scene.rows())) and np.array_equal(_bits(image), _bits(again))
    loss = _step(scene, control, opt, views, target, dev)
    assert np.isfinite(loss) and float(opt.state[scene._xyz]["step"]) == 6.0

    # reset_opacity clamps the logits and zeroes exactly the opacity's moments
    limit = float(np.log(0.01 / 0.99))
    old = scene._opacity.detach().clone()
    assert (old > limit).any()
    control.reset_opacity(opt)
    assert torch.equal(scene._opacity.detach(), old.clamp(max=limit)) and float(scene._opacity.max()) <= limit
    for k in ref.PARAMS:
        state = opt.state[getattr(scene, "_" + k)]
        for m in ("exp_avg", "exp_avg_sq"):
            assert bool(state[m].any()) == (k != "opacity"), (k, m)
    assert float(opt.state[scene._opacity]["step"]) == 6.0


def test_fit_tool_with_densification(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, G, W, VIEWS)
    out = tmp_path / "fit"
    res = fit_ply.main([str(path), "--out", str(out), "--views", "3", "--size", "48", "--steps", "20", "--drop", "0.5",
                        "--densify-interval", "5", "--densify-until", "6"])
    print("fit:", {k: v for k, v in res.items() if k != "densify_events"})
    for e in res["densify_events"]:
        print("  event:", e)
    assert json.load(open(out / "fit.json")) == res
    assert [e["step"] for e in res["densify_events"]] == [5] and res["densify_events"][0]["n_out"] > res["gaussians_first"]
    assert 0 < res["gaussians_first"] < G and res["gaussians_last"] == res["gaussians"] == res["densify_events"][-1]["n_out"]
    fitted = GaussianScene.from_ply(out / "point_cloud.ply", hip_device)
    assert fitted.num_gaussians == res["gaussians_last"]
    assert all(torch.isfinite(p).all() for p in fitted.parameters())
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
