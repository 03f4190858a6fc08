"""The fused Adam step on the MI355X: lsr_adam_step against the float64 reference of tests/adam_ref.py on the bounds
written there, the bit-for-bit properties of include/lsr_optim.h (invisible rows, dense == all-visible, one launch ==
one launch per table, repeatable, stream-independent, alignment-independent), SceneAdam's behaviour as a
torch.optim.Adam, with DensityControl, under graph capture, and the fitting tool with --optimizer.

Sizes: csrc/optim.hip gives a workgroup 4096 consecutive floats of one table and a lane groups of four; rows 1, 63, 64,
65, 1000, 4097 and 100 003 with the scene's widths 3, 3, 45, 1, 3, 4 put table ends inside a group (n = 1, 63, 65,
100 003 are odd: 3 n and 45 n are no multiples of 4), inside a wave and inside a workgroup, make the next table start at
a misaligned address of a shared buffer only where the test says so, and give f_rest 1 to 1099 workgroups.  The bounds
are asserted on every element; stock torch.optim.Adam's error against the same reference is printed beside the
kernel's."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import adam_ref as ref
from tests import density_ref as dref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 1000, 4097, 100_003]
PARENT = (1 << 28) - 1


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=2)
def _case(n, T, rest=15, extra=None):
    """float32 inputs, computed once and never modified: shapes, hyperparameters, p0 and T gradients per table."""
    rng = np.random.default_rng(100 * n + 10 * T + rest)
    shapes = ref.SHAPES(n, rest) + ([extra] if extra else [])
    hyper = list(ref.HYPER) + ([ref.HYPER[0]] if extra else [])
    p0 = [rng.normal(size=s).astype(np.float32) for s in shapes]
    grads = [[ref.draw_grad(rng, s) for s in shapes] for _ in range(T)]
    return shapes, hyper, p0, grads


def _state(dev, p0, moments=None):
    P = [torch.from_numpy(a).to(dev) for a in p0]
    if moments is None:
        return P, [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    return P, [m.clone() for m in moments[0]], [v.clone() for v in moments[1]]


def _step(P, G, M, V, hyper, step, bc, vis=None, one_by_one=False):
    from latentsplat_amd import adam_step
    tables = [dict(param=p, grad=g, exp_avg=m, exp_avg_sq=v, step=step, bias_correction=bc, **h) for p, g, m, v, h in zip(P, G, M, V, hyper)]
    if one_by_one:
        for t in tables:
            adam_step([t], vis)
    else:
        adam_step(tables, vis)


def _run(dev, p0, grads, hyper, bc, masks=None, one_by_one=False):
    P, M, V = _state(dev, p0)
    for t, gs in enumerate(grads):
        G = [torch.from_numpy(g).to(dev) for g in gs]
        vis = None if masks is None else torch.from_numpy(masks[t]).to(dev)
        _step(P, G, M, V, hyper, t + 1, bc, vis, one_by_one)
    return P, M, V


def _stock(dev, p0, grads, hyper):
    P = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in p0 if a.size]
    opt = torch.optim.Adam([dict(params=[p], **h) for p, h in zip(P, [h for a, h in zip(p0, hyper) if a.size])], lr=0.0)
    for gs in grads:
        for p, g in zip(P, [g for g in gs if g.size]):
            p.grad = torch.from_numpy(g).to(dev)
        opt.step()
    return P, [opt.state[p]["exp_avg"] for p in P], [opt.state[p]["exp_avg_sq"] for p in P]


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _hold(got, p0, grads, hyper, bc, show, masks=None, stock=None):
    """Every table of ``got = (P, M, V)`` on the three bounds of tests/adam_ref.py."""
    P, M, V = (_np(x) for x in got)
    k = 0
    for i, (a, h) in enumerate(zip(p0, hyper)):
        if a.size == 0:
            assert P[i].size == 0
            continue
        r = ref.run(a, [gs[i] for gs in grads], h, bc, masks)
        where = f"{show} table {i} {a.shape}:"
        if stock is not None:
            ref.within("stock", dict(p=_np(stock[0])[k], m=_np(stock[1])[k], v=_np(stock[2])[k]), r, where)
        worst = ref.within("kernel", dict(p=P[i], m=M[i], v=V[i]), r, where)
        assert max(worst.values()) <= 1.0, (where, worst)
        k += 1


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n", ROWS)
def test_dense_step_matches_the_reference(hip_device, n, T, bias_correction):
    shapes, hyper, p0, grads = _case(n, T)
    got = _run(hip_device, p0, grads, hyper, bias_correction)
    stock = _stock(hip_device, p0, grads, hyper) if bias_correction else None     # (stock Adam always corrects the bias)
    _hold(got, p0, grads, hyper, bias_correction, f"n={n} T={T} bc={bias_correction}", stock=stock)


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("n", [65, 4097])
def test_sparse_step_matches_the_reference(hip_device, n, bias_correction):
    T = 5
    shapes, hyper, p0, grads = _case(n, T)
    rng = np.random.default_rng(n)
    masks = [(rng.uniform(size=n) < 0.5).astype(np.uint8) for _ in range(T)]
    got = _run(hip_device, p0, grads, hyper, bias_correction, masks)
    _hold(got, p0, grads, hyper, bias_correction, f"sparse n={n} bc={bias_correction}", masks)


def test_degree_zero_scene_and_the_widest_table(hip_device):
    """features_rest of a degree-0 scene has no columns and is skipped; a table of LSR_ADAM_MAX_WIDTH floats per row."""
    n, T = 37, 2
    shapes, hyper, p0, grads = _case(n, T, rest=0, extra=(n, 4096))
    assert p0[2].size == 0 and p0[6].shape == (n, 4096)
    got = _run(hip_device, p0, grads, hyper, True)
    _hold(got, p0, grads, hyper, True, "degree 0 + width 4096", stock=_stock(hip_device, p0, grads, hyper))
    rng = np.random.default_rng(0)
    masks = [(rng.uniform(size=n) < 0.5).astype(np.uint8) for _ in range(T)]
    sparse = _run(hip_device, p0, grads, hyper, True, masks)
    _hold(sparse, p0, grads, hyper, True, "degree 0 + width 4096, sparse", masks)
    # a wider row: dense mode takes it (rows mean nothing there), sparse mode refuses it
    from latentsplat_amd import adam_step
    wide = torch.zeros((3, 5000), device=hip_device)
    table = dict(param=wide, grad=torch.ones_like(wide), exp_avg=torch.zeros_like(wide), exp_avg_sq=torch.zeros_like(wide), lr=0.5,
                 betas=(0.5, 0.5), eps=0.0, step=1, bias_correction=True)
    adam_step([table])
    assert float((wide + 0.5).abs().max()) <= 1e-6       # lr / (1 - 0.5) * 0.5 / (sqrt(0.5) / sqrt(0.5)), to rounding
    with pytest.raises(_lib.LsrError, match="4096"):
        adam_step([table], torch.ones(3, dtype=torch.bool, device=hip_device))
    with pytest.raises(_lib.LsrError, match="contiguous"):
        adam_step([dict(table, param=torch.zeros((5000, 3), device=hip_device).t())])
    with pytest.raises(_lib.LsrError, match="rows"):
        adam_step([table], torch.ones(4, dtype=torch.bool, device=hip_device))


def _masks(n, seed):
    rng = np.random.default_rng(seed)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[n - 1] = 1, 1
    runs = (np.arange(n) // 37 % 3 == 0).astype(np.uint8)             # contiguous runs of 37 rows, one in three
    return dict(none=np.zeros(n, np.uint8), all=np.ones(n, np.uint8), random=(rng.uniform(size=n) < 0.3).astype(np.uint8),
                first=first, last=last, runs=runs, other_bytes=((rng.uniform(size=n) < 0.5) * rng.integers(1, 256, n)).astype(np.uint8))


@pytest.mark.parametrize("n", ROWS)
def test_invisible_rows_keep_their_bits(hip_device, n):
    """After one dense step (moments that are not 0), a second step: the visible rows get the dense step's bits, the
    others keep theirs, in p, m and v of every table; an all-ones mask is the dense step."""
    dev = hip_device
    shapes, hyper, p0, grads = _case(n, 5)
    start = _run(dev, p0, grads[:1], hyper, True)
    G = [torch.from_numpy(g).to(dev) for g in grads[1]]
    clone = lambda: tuple([t.clone() for t in ts] for ts in start)
    dense = clone()
    _step(*dense[:1], G, *dense[1:], hyper, 2, True)
    for name, mask in _masks(n, n).items():
        got = clone()
        vis = torch.from_numpy(mask).to(dev)
        _step(*got[:1], G, *got[1:], hyper, 2, True, vis if name != "random" else vis.bool())     # (a bool mask too)
        on = mask != 0
        for which, (gs, ds, ss) in enumerate(zip(got, dense, start)):
            for i, (g, d, s) in enumerate(zip(gs, ds, ss)):
                g, d, s = _bits(g), _bits(d), _bits(s)
                assert np.array_equal(g[on], d[on]), (n, name, "pmv"[which], i)
                assert np.array_equal(g[~on], s[~on]), (n, name, "pmv"[which], i)
        if name == "all":
            assert all(np.array_equal(_bits(a), _bits(b)) for gs, ds in zip(got, dense) for a, b in zip(gs, ds))


@pytest.mark.parametrize("n", [65, 4097])
def test_poisoned_invisible_rows_reach_nothing(hip_device, n):
    dev = hip_device
    shapes, hyper, p0, grads = _case(n, 5)
    for name in ("random", "runs", "first", "none"):
        mask = _masks(n, 3)[name]
        P, M, V = _state(dev, p0)
        for t in range(2):
            G = []
            for g in grads[t]:
                g = g.copy()
                g[mask == 0] = np.nan
                G.append(torch.from_numpy(g).to(dev))
            _step(P, G, M, V, hyper, t + 1, True, torch.from_numpy(mask).to(dev))
        for ts in (P, M, V):
            assert all(bool(torch.isfinite(t).all()) for t in ts), (n, name)
        if mask.any():
            assert all(bool(m[torch.from_numpy(mask != 0).to(dev)].any()) for m in M)         # ... and the visible rows did move


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for xs, ys in zip(a, b) for x, y in zip(xs, ys))


def test_one_launch_is_six_launches_is_any_stream(hip_device):
    dev = hip_device
    n, T = 4097, 2
    shapes, hyper, p0, grads = _case(n, 5)
    grads = grads[:T]
    rng = np.random.default_rng(1)
    masks = [(rng.uniform(size=n) < 0.5).astype(np.uint8) for _ in range(T)]
    for m in (None, masks):
        first = _run(dev, p0, grads, hyper, True, m)
        assert _same(first, _run(dev, p0, grads, hyper, True, m))                      # two runs
        assert _same(first, _run(dev, p0, grads, hyper, True, m, one_by_one=True))     # one launch per table
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            third = _run(dev, p0, grads, hyper, True, m)
        side.synchronize()
        assert _same(first, third)


@pytest.mark.parametrize("n", [65, 4097])
def test_a_misaligned_pointer_gives_the_same_bits(hip_device, n):
    """A contiguous slice that starts 4 bytes into a larger buffer is not 16-byte aligned: the table moves as single
    floats.  Every one of the four arrays in turn, and all four."""
    dev = hip_device
    shapes, hyper, p0, grads = _case(n, 5)
    mask = torch.from_numpy(_masks(n, 5)["random"]).to(dev)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=dev)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        return out

    for vis in (None, mask):
        want = _run(dev, p0, grads[:2], hyper, True, None if vis is None else [mask.cpu().numpy()] * 2)
        for which in ("p", "g", "m", "v", "pgmv"):
            P, M, V = _state(dev, p0)
            assert all(t.data_ptr() % 16 == 0 for ts in (P, M, V) for t in ts if t.numel())
            if "p" in which: P = [shifted(t) for t in P]
            if "m" in which: M = [shifted(t) for t in M]
            if "v" in which: V = [shifted(t) for t in V]
            for t in range(2):
                G = [torch.from_numpy(g).to(dev) for g in grads[t]]
                if "g" in which: G = [shifted(g) for g in G]
                _step(P, G, M, V, hyper, t + 1, True, vis)
            assert _same(want, (P, M, V)), (n, which, vis is not None)


# ---- SceneAdam ----

def _scene(dev, n, seed=0, sh_rest=15):
    from latentsplat_amd import GaussianScene
    inp = dref.make_inputs(n, seed, sh_rest=sh_rest)
    return GaussianScene.from_tensors(**{k: torch.from_numpy(inp[k]) for k in dref.PARAMS}).to(dev)


def _scene_grads(scene, T, seed):
    rng = np.random.default_rng(seed)
    return [{name: ref.draw_grad(rng, tuple(p.shape)) for name, p in scene.named_parameters()} for _ in range(T)]


def _give(scene, grads, dev):
    for name, p in scene.named_parameters():
        p.grad = torch.from_numpy(grads[name]).to(dev)


def _hold_scene(scene, opt, p0, grads, show, first=0):
    """The scene's parameters and opt's state after the steps ``grads`` from ``p0`` (stock or fused) on the bounds."""
    for group in opt.param_groups:
        name, p = group["name"], group["params"][0]
        r = ref.run(p0[name], [g[name] for g in grads], group, group.get("bias_correction", True))
        s = opt.state[p]
        worst = ref.within(type(opt).__name__, dict(p=_np([p])[0], m=_np([s["exp_avg"]])[0], v=_np([s["exp_avg_sq"]])[0]), r, f"{show} {name}:")
        assert max(worst.values()) <= 1.0, (show, name, worst)
        assert float(s["step"]) == len(grads)


def test_scene_adam_behaves_like_adam(hip_device):
    from latentsplat_amd import SceneAdam
    dev = hip_device
    scene = _scene(dev, 1000, sh_rest=0)                     # degree 0: _features_rest is empty and left out
    opt = SceneAdam.for_scene(scene, extent=2.0)
    assert [g["name"] for g in opt.param_groups] == ["_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"]
    assert [g["lr"] for g in opt.param_groups] == [1.6e-4 * 2.0, 2.5e-3, 5e-2, 5e-3, 1e-3]
    assert all(g["eps"] == 1e-15 and g["bias_correction"] for g in opt.param_groups)
    scene = _scene(dev, 1000)
    opt = SceneAdam.for_scene(scene, extent=2.0, lr_rest=1e-3)
    assert len(opt.param_groups) == 6 and opt.param_groups[2]["lr"] == 1e-3 and len(opt.state) == 0      # lazily created
    p0 = {name: p.detach().cpu().numpy().copy() for name, p in scene.named_parameters()}
    grads = _scene_grads(scene, 4, 1)
    # a parameter without a gradient is untouched, has no state, and its step does not advance
    _give(scene, grads[0], dev)
    scene._opacity.grad = None
    opt.step()
    assert scene._opacity not in opt.state and len(opt.state) == 5 and np.array_equal(_bits(scene._opacity), _bits(p0["_opacity"]))
    state = opt.state[scene._xyz]
    assert set(state) == {"step", "exp_avg", "exp_avg_sq"} and not state["step"].is_cuda and float(state["step"]) == 1.0
    assert state["exp_avg"].shape == scene._xyz.shape and bool(state["exp_avg"].any())
    _give(scene, grads[1], dev)
    opt.step()
    assert float(opt.state[scene._opacity]["step"]) == 1.0 and float(opt.state[scene._xyz]["step"]) == 2.0
    # set_lr takes effect: at rate 0 the moments move and the parameter does not
    opt.set_lr("_scaling", 0.0)
    before, m_before = scene._scaling.detach().clone(), opt.state[scene._scaling]["exp_avg"].clone()
    _give(scene, grads[2], dev)
    opt.step(visibility=None)
    assert torch.equal(scene._scaling.detach(), before) and not torch.equal(opt.state[scene._scaling]["exp_avg"], m_before)
    assert not torch.equal(scene._xyz.detach(), torch.from_numpy(p0["_xyz"]).to(dev))
    # a masked step advances the count of every parameter that had a gradient
    opt.step(visibility=torch.zeros(1000, dtype=torch.bool, device=dev))
    assert float(opt.state[scene._xyz]["step"]) == 4.0 and torch.equal(scene._scaling.detach(), before)
    # step(closure)
    assert opt.step(lambda: torch.tensor(7.0)) == 7.0


@pytest.mark.parametrize("direction", ["fused_to_stock", "stock_to_fused"])
def test_state_dict_moves_between_the_classes(hip_device, direction):
    """Two steps with one class, the state_dict into the other, two more steps: four steps of the reference."""
    from latentsplat_amd import SceneAdam
    dev = hip_device
    scenes = [_scene(dev, 1000, seed=2), _scene(dev, 1000, seed=2)]
    p0 = {name: p.detach().cpu().numpy().copy() for name, p in scenes[0].named_parameters()}
    grads = _scene_grads(scenes[0], 4, 3)
    make = dict(fused=lambda s: SceneAdam.for_scene(s, extent=3.0),
                stock=lambda s: torch.optim.Adam([dict(params=[p], lr=g["lr"], name=g["name"]) for g in SceneAdam.for_scene(s, extent=3.0).param_groups
                                                  for p in g["params"]], lr=0.0, eps=1e-15))
    a, b = direction.split("_to_")
    first, second = make[a](scenes[0]), make[b](scenes[1])
    for g in grads[:2]:
        _give(scenes[0], g, dev)
        first.step()
    _hold_scene(scenes[0], first, p0, grads[:2], f"{a}, two steps")
    second.load_state_dict(first.state_dict())
    with torch.no_grad():
        for (_, p), (_, q) in zip(scenes[1].named_parameters(), scenes[0].named_parameters()):
            p.copy_(q)
    assert type(second) is (SceneAdam if b == "fused" else torch.optim.Adam)
    for g in grads[2:]:
        _give(scenes[1], g, dev)
        second.step()
    _hold_scene(scenes[1], second, p0, grads, f"{a} then {b}")


def _graph_shape(graph):
    """(node types, number of edges) of a captured graph kept with ``keep_graph=True``, from the HIP runtime the
    library is linked to (the process's one)."""
    import ctypes as C
    hip = _lib.load()
    handle = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, C.byref(n)) == 0
    nodes = (C.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(handle, nodes, C.byref(n)) == 0
    types = []
    for i in range(n.value):
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
        types.append(t.value)
    e = C.c_size_t(0)
    assert hip.hipGraphGetEdges(handle, None, None, C.byref(e)) == 0
    return types, e.value


HIP_GRAPH_NODE_KERNEL = 0      # hipGraphNodeTypeKernel


def test_captured_step_replays_bit_for_bit(hip_device):
    """bias_correction=False and constant rates: three replays of one captured step are three eager steps.  The graph
    holds one kernel node and nothing beside it."""
    from latentsplat_amd import SceneAdam
    dev = hip_device
    n = 4097
    grads = None
    results = []
    for captured in (False, True):
        scene = _scene(dev, n, seed=4)
        opt = SceneAdam.for_scene(scene, extent=1.5, bias_correction=False)
        grads = grads or _scene_grads(scene, 1, 5)[0]
        _give(scene, grads, dev)
        start = [p.detach().clone() for p in scene.parameters()]
        if not captured:
            for _ in range(3):
                opt.step()
        else:
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                opt.step()                                   # the state now exists, outside the graph's pool
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(graph):
                opt.step()
            types, edges = _graph_shape(graph)
            print(f"captured graph: node types {types}, {edges} edge(s)")
            assert types == [HIP_GRAPH_NODE_KERNEL] and edges == 0          # one kernel, nothing beside or behind it
            graph.instantiate()
            with torch.no_grad():                            # back to the start
                for p, s in zip(scene.parameters(), start):
                    p.copy_(s)
                    opt.state[p]["exp_avg"].zero_()
                    opt.state[p]["exp_avg_sq"].zero_()
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize(dev)
        results.append([_bits(p) for p in scene.parameters()] + [_bits(opt.state[p][k]) for p in scene.parameters() for k in ("exp_avg", "exp_avg_sq")])
    assert all(np.array_equal(a, b) for a, b in zip(*results))


# ---- with DensityControl, and the tool ----

G, W, VIEWS = 2000, 32, 2


def test_with_density_control(hip_device, tmp_path):
    from latentsplat_amd import DensityControl, GaussianScene, SceneAdam, visible_from_radii
    from latentsplat_amd.rasterizer import build_view_table
    dev = hip_device
    path = tmp_path / "scene.ply"
    sc, _, _ = sref.write_scene_file(path, G, W, VIEWS)
    scene = GaussianScene.from_ply(path, dev)
    views = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                             torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False).detach()
    with torch.no_grad():
        target = scene.render(views, W, W)[0]
        gen = torch.Generator().manual_seed(0)
        for name, p in scene.named_parameters():
            p.add_((torch.randn(p.shape, generator=gen) * dict(_xyz=0.01, _opacity=0.5).get(name, 0.05)).to(dev))
    opt = SceneAdam.for_scene(scene, extent=1.0)
    control = DensityControl(scene)

    def step(sparse=False):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((VIEWS, scene.num_gaussians, 3), device=dev, requires_grad=True)
        color, _, _, _, radii = scene.render(views, W, W, means2D=means2D)
        loss = (color - target).abs().mean()
        loss.backward()
        opt.step(visibility=visible_from_radii(radii) if sparse else None)
        control.update(means2D.grad, radii)
        return float(loss.detach())

    for _ in range(3):
        step()
    names = [g["name"] for g in opt.param_groups]
    old = {k: {m: opt.state[getattr(scene, k)][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k in names}
    assert all(bool(old[k]["exp_avg"].any()) for k in names)
    avg = (control.xyz_gradient_accum / control.denom).nan_to_num(0.0).reshape(-1)
    smax = scene._scaling.detach().exp().amax(1)
    counts = control.densify_and_prune(opt, float(avg.quantile(0.7)), 0.005, float(smax.median()) / 0.01, 0, n_split=2,
                                       generator=torch.Generator(device=dev).manual_seed(7))
    print("densify_and_prune with SceneAdam:", counts)
    n_out = counts["n_out"]
    assert counts["clones"] > 0 and counts["split_parents"] > 0 and 0 < counts["kept"] < G and scene.num_gaussians == n_out
    map_ = control.last_map.cpu().numpy().view(np.uint32)
    parent, kind = (map_ & PARENT).astype(np.int64), map_ >> 28
    assert len(opt.state) == 6
    for group in opt.param_groups:
        k = group["name"]
        p = getattr(scene, k)
        assert len(group["params"]) == 1 and group["params"][0] is p and p.shape[0] == n_out
        state = opt.state[p]
        assert float(state["step"]) == 3.0
        for m in ("exp_avg", "exp_avg_sq"):
            t, was = _bits(state[m]), _bits(old[k][m])
            assert t.shape[0] == n_out
            assert np.array_equal(t[kind == 0], was[parent[kind == 0]]), (k, m)          # the moments travel with their rows
            assert not t[kind != 0].any(), (k, m)                                        # new rows start at exactly +0
    # the next steps run, dense and masked, on the new parameters
    before = scene._xyz.detach().clone()
    assert np.isfinite(step()) and np.isfinite(step(sparse=True))
    assert float(opt.state[scene._xyz]["step"]) == 5.0 and not torch.equal(before, scene._xyz.detach())
    assert all(bool(torch.isfinite(p).all()) for p in scene.parameters())
    # reset_opacity zeroes exactly the opacity's moments
    control.reset_opacity(opt)
    for group in opt.param_groups:
        state = opt.state[group["params"][0]]
        for m in ("exp_avg", "exp_avg_sq"):
            assert bool(state[m].any()) == (group["name"] != "_opacity"), (group["name"], m)


TODAY = {"loss_first", "loss_last", "steps", "ms_per_step", "timed_steps", "gaussians", "sh_degree", "views", "size", "noise", "seed",
         "extent", "lambda_dssim"}


@pytest.mark.parametrize("optimizer", ["fused", "sparse", "torch"])
def test_fit_tool_with_each_optimizer(hip_device, tmp_path, optimizer):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, 2000, 64, 4)
    out = tmp_path / "fit"
    extra = ["--lr-position-final", "1.6e-6", "--lr-position-max-steps", "30"] if optimizer == "fused" else []
    res = fit_ply.main([str(path), "--out", str(out), "--views", "4", "--size", "64", "--steps", "30", "--optimizer", optimizer] + extra)
    print("fit:", res)
    assert json.load(open(out / "fit.json")) == res
    assert TODAY <= set(res) and res["optimizer"] == optimizer and res["steps"] == 30
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
