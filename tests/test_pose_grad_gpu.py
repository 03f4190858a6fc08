"""Pose gradients of a GaussianScene's rigid parts on the MI355X (latentsplat_amd.pose, csrc/scene_pose.hip) against
autograd of the float64 restatement of tests/pose_grad_ref.py, within the bound C u sum|terms| counted there; the
reduction's corner cases (64 ids in a wave, nothing in range, a second chunk per workgroup); what the call promises about
bits (optional upstream gradients, repeats, the workspace's contents, guard words); the op against transform_scene; the
posed render inside a scene; the recovery of a known similarity; the tool.

Measured worst error / bound of the gradient cases (MI355X): see DESIGN.md section 2.20."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import pose_grad_ref as pref
from tests import transform_ref as tref
from tests import util

pytestmark = pytest.mark.gpu

NAMES = tref.NAMES
MAXT = _lib.POSE_MAX_TRANSFORMS
H = W = 64
# the grid is capped at 2048 workgroups of 128 Gaussians (K = 4): one n just past it, where a workgroup takes a second chunk
PAST_THE_GRID = 2048 * 128 + 1
# (n, K, T, with log-scales); T == 0: no index
CASES = ([(n, K, 0, (n + K) % 2 == 0) for n in (1, 63, 64, 65, 127, 129, 1031) for K in (1, 4, 9, 16, 25)] +
         [(1031, K, T, (T + K) % 2 == 1) for T in (1, 3, 64, MAXT) for K in (1, 4, 9, 16, 25)] +
         [(1031, 16, T, s) for T in (1, 3, 64, MAXT) for s in (False, True)] +
         [(n, 16, 3, True) for n in (1, 63, 64, 65, 127, 129)] +
         [(PAST_THE_GRID, 4, 0, True), (PAST_THE_GRID, 4, 3, False)])
CASES = list(dict.fromkeys(CASES))


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _index(n, T, seed):
    """idx drawn from [-1, T] (both out-of-range sides), and with T > 1 one transform (T // 2) that owns no row."""
    idx = np.random.default_rng(seed).integers(-1, T + 1, size=n)
    if T > 1:
        idx[idx == T // 2] = -1
    if n >= 3:
        idx[0], idx[1] = -1, T
    return torch.from_numpy(idx.astype(np.int32))


def _case(n, K, T, with_scale, seed, dev):
    scene = tref.random_scene(n, K, seed)
    p, t, ls = pref.random_poses(max(T, 1), seed + 1, with_scale=with_scale)
    idx = _index(n, T, seed + 2) if T else None
    gen = torch.Generator().manual_seed(seed + 3)
    grads = [torch.randn(scene[k].shape, generator=gen) for k in NAMES]
    return scene, (p, t, ls), idx, grads


def _gpu_grads(scene, poses, idx, grads, dev):
    from latentsplat_amd.pose import pose_scene
    leaves = [v.to(dev).requires_grad_(True) for v in poses if v is not None]
    outs = pose_scene(*(scene[k].to(dev) for k in NAMES), *leaves, *([None] if len(leaves) == 2 else []),
                      None if idx is None else idx.to(dev))
    given = [(o, g.to(dev)) for o, g in zip(outs, grads) if g is not None]
    got = torch.autograd.grad([o for o, _ in given], leaves, [g for _, g in given])
    return outs, got


def _reference(scene, poses, idx, grads, outs):
    s64 = tref.f64(scene)
    p, t, ls = (None if v is None else v.double() for v in poses)
    g64 = [None if g is None else g.double() for g in grads]
    signs = pref.quaternion_signs(s64[3], outs[3], p, idx)
    return pref.pose_grads(s64, p, t, ls, idx, g64, signs), pref.abs_terms(s64, p, t, ls, idx, g64)


def _hold(got, want, terms, what):
    worst = {}
    for name, g, w, a, c in zip(("quaternion", "translation", "log_scale"), got, want, terms,
                                (pref.C_QUATERNION, pref.C_TWIST, pref.C_TWIST)):
        if w is None:
            continue
        g = g.detach().cpu().double()
        assert torch.isfinite(g).all(), (what, name)
        err, bound = (g - w).abs(), c * pref.U * a
        ratio = err / bound.clamp_min(1e-300)
        worst[name] = float(ratio.max())
        assert bool((err <= bound).all()), f"{what}: {name} misses its bound, worst error / bound {worst[name]:.3f}"
    print(f"[pose] {what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("n,K,T,with_scale", CASES)
def test_pose_gradients_within_the_bound(hip_device, n, K, T, with_scale):
    scene, poses, idx, grads = _case(n, K, T, with_scale, 1000 + n % 997 + 7 * K + T, hip_device)
    outs, got = _gpu_grads(scene, poses, idx, grads, hip_device)
    want, terms = _reference(scene, poses, idx, grads, outs)
    _hold(got, want, terms, f"n={n} K={K} T={T} scale={with_scale}")
    if T > 1:                                        # the transform that owns no row: exact zeros
        for g in got:
            assert not g[T // 2].any()


@pytest.mark.parametrize("distinct", [3, 4, 5, 6, 64])
def test_one_wave_of_distinct_ids(hip_device, distinct):
    """A wave reduces up to four ids by a wave sum each and walks the lanes that are left one by one: at, one past and two
    past that threshold, and 64 distinct ids in one wave."""
    n, K, T = 64, 16, distinct
    scene, poses, _, grads = _case(n, K, T, True, 77, hip_device)
    idx = torch.from_numpy((np.random.default_rng(5).permutation(64) % distinct).astype(np.int32))
    outs, got = _gpu_grads(scene, poses, idx, grads, hip_device)
    want, terms = _reference(scene, poses, idx, grads, outs)
    _hold(got, want, terms, f"{distinct} distinct ids in one wave")
    assert all(bool(g.abs().reshape(T, -1).max(dim=1).values.gt(0).all()) for g in got)


def test_all_rows_out_of_range_give_exact_zeros(hip_device):
    scene, poses, _, grads = _case(300, 9, 3, True, 5, hip_device)
    idx = torch.from_numpy(np.where(np.arange(300) % 2 == 0, -1, 3).astype(np.int32))
    _, got = _gpu_grads(scene, poses, idx, grads, hip_device)
    for g in got:
        assert not g.any() and bool(torch.isfinite(g).all())


# ---- the C ABI as it is: optional gradients, repeats, the workspace, guard words ----

GUARD, MARK = 64, -7.25


class _Raw:
    """One forward through the public pieces, then lsr_scene_pose_grad on flat guarded buffers."""

    def __init__(self, n, K, T, seed, dev):
        from latentsplat_amd.pose import pose_matrices
        from latentsplat_amd.transform import apply_records, transform_records
        self.n, self.K, self.T, self.dev = n, K, T, dev
        scene, poses, idx, grads = _case(n, K, T, True, seed, dev)
        self.idx = None if idx is None else idx.to(dev)
        self.q, t, ls = (v.to(dev) for v in poses)
        self.records = transform_records(pose_matrices(self.q, t, ls), tref.degree_of(K), check=False)
        self.ins = {k: scene[k].to(dev) for k in NAMES}
        self.outs = {k: torch.empty_like(v) for k, v in self.ins.items()}
        apply_records(self.records, self.idx, self.ins, self.outs, n, K)
        self.grads = [g.to(dev) for g in grads]
        self.ws_bytes = int(_lib.load().lsr_pose_grad_workspace_bytes(n, K, max(T, 1)))

    def __call__(self, grads=None, ws_fill=None, wanted=(True, True, True)):
        T = max(self.T, 1)
        grads = self.grads if grads is None else grads
        ptr = lambda v: C.c_void_p(None if v is None or v.numel() == 0 else v.data_ptr())
        flat = [torch.full((T * w + GUARD,), MARK, device=self.dev) for w in (4, 3, 1)]
        ws = torch.empty(self.ws_bytes + 8 * GUARD, dtype=torch.uint8, device=self.dev)
        ws.view(torch.float64)[:] = float("nan") if ws_fill is None else ws_fill
        ws.view(torch.float64)[self.ws_bytes // 8:] = MARK
        dims = _lib.TransformDims(n=self.n, sh_coeffs=self.K, num_transforms=T, reserved0=0, reserved1=0)
        gin = _lib.PoseGradIn(xyz=ptr(self.ins["xyz"]), rotation=ptr(self.outs["rotation"]), features_rest=ptr(self.outs["features_rest"]),
                              g_xyz=ptr(grads[0]), g_features_rest=ptr(grads[1]), g_scaling=ptr(grads[2]), g_rotation=ptr(grads[3]))
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        _lib.check(_lib.load().lsr_scene_pose_grad(C.byref(dims), ptr(self.records), ptr(self.idx), ptr(self.q), C.byref(gin), ptr(ws),
                                                   self.ws_bytes, *(ptr(f) if w else None for f, w in zip(flat, wanted)), stream),
                   "lsr_scene_pose_grad")
        torch.cuda.synchronize(self.dev)
        assert bool((ws.view(torch.float64)[self.ws_bytes // 8:] == MARK).all()), "words behind the workspace written"
        for f, w, width in zip(flat, wanted, (4, 3, 1)):
            assert bool((f[T * width:] == MARK).all()), "guard words written"
            if not w:
                assert bool((f == MARK).all()), "an unwanted output was written"
        return [_bits(f[:T * width]) for f, width in zip(flat, (4, 3, 1))]


@pytest.mark.parametrize("n,K,T", [(1031, 16, 3), (300, 25, 0), (257, 1, 64), (129, 4, MAXT)])
def test_bits_repeats_workspace_and_guard_words(hip_device, n, K, T):
    raw = _Raw(n, K, T, 40 + K, hip_device)
    base = raw()
    assert all(torch.equal(a, b) for a, b in zip(base, raw())), "a repeated call gave other bits"
    assert all(torch.equal(a, b) for a, b in zip(base, raw(ws_fill=0.0))), "the result depends on the workspace's contents"
    assert all(torch.equal(a, b) for a, b in zip(base, raw(ws_fill=1e300)))
    # any subset of the outputs: the wanted ones have the bits of the full call
    for wanted in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        for a, b, w in zip(base, raw(wanted=wanted), wanted):
            assert not w or torch.equal(a, b), wanted
    # each upstream gradient None: the bits of passing zeros
    for k in range(4):
        if K == 1 and k == 1:
            continue
        none = [None if j == k else g for j, g in enumerate(raw.grads)]
        zeros = [torch.zeros_like(g) if j == k else g for j, g in enumerate(raw.grads)]
        assert all(torch.equal(a, b) for a, b in zip(raw(grads=none), raw(grads=zeros))), NAMES[k]
    assert not any(bool(b.view(torch.float32).any()) for b in raw(grads=[None] * 4))


def test_rows_permuted_with_their_index(hip_device):
    n, K, T = 1031, 16, 3
    scene, poses, idx, grads = _case(n, K, T, True, 91, hip_device)
    outs, got = _gpu_grads(scene, poses, idx, grads, hip_device)
    want, terms = _reference(scene, poses, idx, grads, outs)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n))
    _, got_perm = _gpu_grads({k: v[perm] for k, v in scene.items()}, poses, idx[perm], [g[perm] for g in grads], hip_device)
    _hold(got_perm, want, terms, "rows permuted with idx")
    _hold(got, want, terms, "rows in order")


def test_forward_and_scene_gradients_are_transform_scenes(hip_device):
    from latentsplat_amd.pose import pose_matrices, pose_scene
    from latentsplat_amd.transform import transform_scene
    dev = hip_device
    for n, K, T in ((1031, 16, 3), (300, 25, 0), (65, 1, 1)):
        scene, poses, idx, grads = _case(n, K, T, True, 60 + K, dev)
        idx = None if idx is None else idx.to(dev)
        p, t, ls = (v.to(dev).requires_grad_(True) for v in poses)
        a = [scene[k].to(dev).requires_grad_(True) for k in NAMES]
        b = [scene[k].to(dev).requires_grad_(True) for k in NAMES]
        outs = pose_scene(*a, p, t, ls, idx)
        M = pose_matrices(p, t, ls)
        assert not M.requires_grad and tuple(M.shape) == (max(T, 1), 4, 4)
        plain = transform_scene(*b, M, idx)
        for k, x, y in zip(NAMES, outs, plain):
            assert torch.equal(_bits(x), _bits(y)), (k, "forward")
        ups = [g.to(dev) for g in grads]
        torch.autograd.backward(outs, ups)
        torch.autograd.backward(plain, ups)
        for k, x, y in zip(NAMES, a, b):
            assert torch.equal(_bits(x.grad), _bits(y.grad)), (k, "scene gradient")
        assert p.grad is not None and t.grad is not None and ls.grad is not None
        # the matrices are those of the float64 formula, to one rounding
        p64, t64, l64 = (v.detach().cpu().double() for v in (p, t, ls))
        for k in range(max(T, 1)):
            A = float(l64[k].exp()) * pref.rotation(p64[k])
            assert float((M[k, :3, :3].cpu().double() - A).abs().max()) <= pref.U * float(A.abs().max()) * 1.01
            assert torch.equal(M[k, :3, 3].cpu(), t[k].detach().cpu()) and M[k, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_more_transforms_than_the_tables_hold(hip_device):
    from latentsplat_amd.pose import pose_scene
    scene = tref.random_scene(10, 4, 0)
    p, t, ls = (v.to(hip_device) for v in pref.random_poses(MAXT + 1, 1))
    with pytest.raises(_lib.LsrError, match="LSR_POSE_MAX_TRANSFORMS"):
        pose_scene(*(scene[k].to(hip_device) for k in NAMES), p, t, ls)


def test_capture_in_a_graph(hip_device):
    """No host read anywhere: forward and backward of the op are captured and replayed."""
    from latentsplat_amd.pose import pose_scene
    dev = hip_device
    scene, poses, idx, grads = _case(1031, 16, 3, True, 12, dev)
    ins = [scene[k].to(dev) for k in NAMES]
    ups = [g.to(dev) for g in grads]
    leaves = [v.to(dev).requires_grad_(True) for v in poses]
    idx = idx.to(dev)
    eager = torch.autograd.grad(pose_scene(*ins, *leaves, idx), leaves, ups)
    side = torch.cuda.Stream(dev)                # warm-up on a side stream, as torch.cuda.graph asks for
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.autograd.grad(pose_scene(*ins, *leaves, idx), leaves, ups)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = torch.autograd.grad(pose_scene(*ins, *leaves, idx), leaves, ups)
    for c in captured:
        c.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    for a, b in zip(eager, captured):
        assert torch.equal(_bits(a), _bits(b))


# ---- inside a scene ----

def _angle(R: torch.Tensor) -> float:
    return float(torch.acos(((torch.trace(R) - 1) / 2).clamp(-1, 1)))


def _posed_child():
    """Body of the LSR_DETERMINISTIC=1 child process of test_posed_render_with_poses."""
    import tempfile
    from latentsplat_amd.pose import PartPoses, pose_scene
    from latentsplat_amd.rasterizer import rasterize_views
    from latentsplat_amd.scene_model import activate_scene
    from tests import test_scene_transform_gpu as tsg
    dev = torch.device("cuda:0")
    ok, failure = True, ""
    try:
        with tempfile.TemporaryDirectory() as tmp:
            sc, scene = tsg._degree3_scene(os.path.join(tmp, "scene.ply"), dev)
        rng = np.random.default_rng(8)
        idx = torch.from_numpy(rng.integers(-1, 4, size=tsg.G).astype(np.int32)).to(dev)
        views = tsg._views(sc.extrinsics, sc, sc.near, sc.far, dev)
        cot = torch.randn((tsg.VIEWS, 3, H, W), generator=torch.Generator().manual_seed(3)).to(dev)
        with torch.no_grad():
            unposed = scene.render(views, H, W)[0]
            identity = PartPoses(3, learn_scale=True).to(dev)
            assert torch.equal(scene.render(views, H, W, poses=identity, transform_idx=idx)[0], unposed), \
                "the render at identity poses differs from the unposed render"
        poses = PartPoses(3, learn_scale=True).to(dev)
        p, t, ls = pref.random_poses(3, 4, t_max=0.3)
        with torch.no_grad():
            poses.rotation.copy_(p + torch.tensor([2.0, 0, 0, 0]))             # a moderate rotation, not normalised
            poses.translation.copy_(t)
            poses.log_scale.copy_(0.4 * ls)
        posed = scene.render(views, H, W, poses=poses, transform_idx=idx)[0]
        (posed * cot).sum().backward()
        got = {k: v.grad.clone() for k, v in list(scene.named_parameters()) + list(poses.named_parameters())}
        act = scene.activated(poses=poses, transform_idx=idx)
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in list(scene.named_parameters()) + list(poses.named_parameters())}
        xyz, rest, scaling, rotation = pose_scene(leaf["_xyz"], leaf["_features_rest"], leaf["_scaling"], leaf["_rotation"],
                                                  leaf["rotation"], leaf["translation"], leaf["log_scale"], idx)
        assert torch.equal(act.means.detach(), xyz.detach()) and torch.equal(act.shs[:, 1:].detach(), rest.detach())
        shs, opac, cov = activate_scene(leaf["_features_dc"], rest, leaf["_opacity"], scaling, rotation)
        color = rasterize_views(views, H, W, scene.active_sh_degree, xyz, cov, opac, shs=shs)[0]
        assert torch.equal(color.detach(), posed.detach()), "the explicit chain renders other bits"
        assert float((color.detach() - unposed).abs().max()) > 1e-2, "the poses move nothing in the image"
        (color * cot).sum().backward()
        for k in got:
            assert got[k].abs().max() > 0, k
            assert torch.equal(got[k].view(torch.int32), leaf[k].grad.view(torch.int32)), f"gradient of {k} differs from the explicit chain's"
    except AssertionError as e:
        ok, failure = False, (str(e).splitlines() or ["assert"])[0]
    print("EQUAL", ok, failure)


def test_posed_render_with_poses(hip_device):
    """LSR_DETERMINISTIC=1 (read once per process: a child): pose and scene gradients of scene.render(poses=) equal those
    of the explicit chain pose_scene -> activate_scene -> rasterize_views bit for bit; identity poses render the unposed
    scene's bits."""
    code = "import sys; sys.path.insert(0, %r)\nfrom tests import test_pose_grad_gpu as m\nm._posed_child()\n" % util.ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LSR_DETERMINISTIC="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("EQUAL True"), line


# ---- recovery of a known similarity ----

# 100 steps of Adam with the step size decaying to 1/20: the stock loop has then cut the rotation error ~1200-fold, the
# translation error ~140-fold and the scale error, the slowest, 5.5-fold, and every error is still on its way down: the
# two loops' errors agree to 2 %.  From ~120 steps on both sit at the float32 floor (3e-5 .. 1e-4, where the rasterizer's
# atomic sums differ run to run) and their ratio scatters between 0.4 and 6: a comparison there measures that noise.
STEPS, LR = 100, 4e-3
KNOWN = dict(axis=(0.3, 1.0, -0.2), degrees=3.0, shift=(0.03, -0.02, 0.025), scale=1.05)      # shift in scene extents


def _moved_pair(path, dev):
    """(cameras' scene description, the unmoved scene, a copy moved by the known similarity, the similarity, the extent)"""
    from latentsplat_amd.transform import similarity_matrix
    from tests import test_scene_transform_gpu as tsg
    sc, scene = tsg._degree3_scene(path, dev)
    extent = float((scene._xyz.detach() - scene._xyz.detach().median(dim=0).values).abs().quantile(0.95, dim=0).max())
    axis = np.array(KNOWN["axis"]) / np.linalg.norm(KNOWN["axis"])
    half = np.radians(KNOWN["degrees"]) / 2
    M = similarity_matrix(np.concatenate([[np.cos(half)], np.sin(half) * axis]), np.array(KNOWN["shift"]) * extent, KNOWN["scale"])
    moved = tsg._scene_from([getattr(scene, "_" + k).detach() for k in NAMES], scene, dev).transform_(M)
    return sc, scene, moved, M, extent


def _errors(poses, M, extent):
    """(rotation angle, translation / extent, |log scale|) of  fitted o known  against the identity."""
    E = poses.as_matrices()[0] @ M
    s = float(torch.linalg.det(E[:3, :3]).pow(1 / 3))
    return _angle(E[:3, :3] / s), float(E[:3, 3].norm()) / extent, abs(float(np.log(s)))


def _fit(moved, views, target, extent, dev, stock=None):
    from latentsplat_amd.losses import photometric_loss
    from latentsplat_amd.pose import PartPoses
    from latentsplat_amd.rasterizer import rasterize_views
    from latentsplat_amd.scene_model import activate_scene
    poses = PartPoses(1, learn_scale=True).to(dev)
    opt = torch.optim.Adam([dict(params=[poses.rotation, poses.log_scale], lr=LR), dict(params=[poses.translation], lr=LR * extent)])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 0.05 ** (i / STEPS))
    params = [getattr(moved, "_" + k).detach() for k in NAMES]
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        if stock is None:
            color = moved.render(views, H, W, poses=poses)[0]
        else:
            xyz, rest, scaling, rotation = stock(*params, poses.rotation, poses.translation, poses.log_scale)
            shs, opac, cov = activate_scene(moved._features_dc.detach(), rest, moved._opacity.detach(), scaling, rotation)
            color = rasterize_views(views, H, W, moved.active_sh_degree, xyz, cov, opac, shs=shs)[0]
        photometric_loss(color, target).backward()
        opt.step()
        sched.step()
    return poses


def test_recovery_of_a_known_similarity(hip_device, tmp_path):
    """The scene moved by a known similarity (3 degrees, 3 % of the extent, scale 1.05) is fitted back to renders of the
    unmoved scene with Adam on the photometric loss, once with the library's pose gradient and once with the stock float32
    torch composition's (the same loop, the same start).  Condition on the inputs: the stock loop cuts each of the three
    errors at least fivefold.  The library's final errors are no worse than 1.5 x the stock loop's (both follow the same
    trajectory up to float32 gradient noise)."""
    from tests import test_scene_transform_gpu as tsg
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        from bench_pose_grad import StockPose
    finally:
        sys.path.pop(0)
    dev = hip_device
    sc, scene, moved, M, extent = _moved_pair(tmp_path / "scene.ply", dev)
    for v in moved.parameters():
        v.requires_grad_(False)
    views = tsg._views(sc.extrinsics, sc, sc.near, sc.far, dev)
    with torch.no_grad():
        target = scene.render(views, H, W)[0]
    from latentsplat_amd.pose import PartPoses
    start = _errors(PartPoses(1, learn_scale=True), M, extent)
    ours = _errors(_fit(moved, views, target, extent, dev), M, extent)
    stock = _errors(_fit(moved, views, target, extent, dev, StockPose(3, dev)), M, extent)
    names = ("rotation [rad]", "translation [extents]", "log scale")
    print("[pose] recovery: " + "; ".join(f"{k}: start {a:.3e}, ours {b:.3e}, stock {c:.3e}" for k, a, b, c in zip(names, start, ours, stock)))
    for k, a, b, c in zip(names, start, ours, stock):
        assert c <= a / 5, f"{k}: the stock loop does not converge on these inputs ({a:.3e} -> {c:.3e}): the test tests nothing"
        assert b <= 1.5 * c, f"{k}: ours {b:.3e} against stock {c:.3e}"


def test_align_tool(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    sc, scene, moved, M, extent = _moved_pair(tmp_path / "scene.ply", hip_device)
    scene.save_ply(tmp_path / "fixed.ply")
    moved.save_ply(tmp_path / "moving.ply")
    tool = os.path.join(util.ROOT, "tools", "align_ply.py")
    steps = 40
    r = subprocess.run([sys.executable, tool, str(tmp_path / "moving.ply"), "--to", str(tmp_path / "fixed.ply"), "--out",
                        str(tmp_path / "out"), "--views", "4", "--size", "64", "--steps", str(steps), "--learn-scale"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(line) == {"matrix", "first_loss", "last_loss"}
    result = json.load(open(tmp_path / "out" / "align.json"))
    assert len(result["matrix"]) == 16 and len(result["loss"]) == steps and result["gaussians"] == scene.num_gaussians
    assert result["learn_scale"] is True and result["views"] == 4 and result["size"] == 64
    assert result["loss"][-1] < result["loss"][0], "the fit did not lower the loss"
    fitted = torch.tensor(result["matrix"], dtype=torch.float64).reshape(4, 4)
    assert fitted[3].tolist() == [0.0, 0.0, 0.0, 1.0] and float(torch.linalg.det(fitted[:3, :3])) > 0
    # the written scene is the moving one moved by the recovered matrix
    aligned = GaussianScene.from_ply(tmp_path / "out" / "aligned.ply", hip_device)
    again = GaussianScene.from_ply(tmp_path / "moving.ply", hip_device).transform_(fitted)
    assert aligned.num_gaussians == scene.num_gaussians
    assert torch.allclose(aligned._xyz.detach(), again._xyz.detach(), rtol=1e-6, atol=1e-6)
