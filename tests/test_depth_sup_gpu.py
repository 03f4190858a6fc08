"""Depth supervision on the GPU (latentsplat_amd/depth_sup.py, csrc/depth_loss.hip): the inverse-depth loss against the
float64 statement of tests/depth_sup_ref.py under the project's rule (kernel error at most 4 x the stock float32
composition's own error, floor 2^-20 x scale), the properties include/lsr_depth_loss.h promises (planted pixels, written
outputs, the same bits every call, views that do not depend on their neighbours, graph capture, refusals), the units through
the render, the priors through prepare_images, and Capture / tools/train_colmap.py with both kinds of supervision."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import colmap_ref as cr
from tests import depth_sup_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = _lib.DEPTH_LOSS_CHUNK
# (5, h, w) with h w = 2 C + 7 for the C pixels one workgroup owns: 4103 = 11 x 373
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 7, 9), (3, 8, 8), (2, 5, 13), (2, 32, 32), (3, 37, 29), (5, 11, 373), (300, 4, 4)]
CONFIGS = [("given", "pixels", False), ("given", "weights", True), ("given", "weights", False), ("given", "pixels", True),
           ("fit", "pixels", True), ("fit", "weights", False), ("fit", "pixels", False), ("fit", "weights", True)]
QUANTITIES = ("loss", "per_view", "inverse_depth", "affine", "grad_depth", "grad_alpha")
GRAD_LOSS = 1.75


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def _case(V, H, W, align, normalize, weighted):
    """The case, its upstream per-view gradient, the float64 reference and the stock float32 composition: computed once."""
    assert 2 * CHUNK + 7 == 11 * 373
    case = ref.loss_case(V, H, W, seed=1000 * V + 10 * H + W, align=align, normalize=normalize, weighted=weighted,
                         zero_row=1 if align == "given" and V >= 2 else None, flat_row=1 if align == "fit" and V >= 2 else None)
    ref.check_loss_case(case)
    gpv = np.random.default_rng(V + H).uniform(-1.0, 1.0, V).astype(np.float32)
    want = ref.loss_and_grads(case, torch.float64, GRAD_LOSS, gpv)
    stock = ref.loss_and_grads(case, torch.float32, GRAD_LOSS, gpv)
    for a in list(want.values()) + list(stock.values()) + [v for v in case.values() if isinstance(v, np.ndarray)] + [gpv]:
        a.setflags(write=False)
    return case, gpv, want, stock


def _dev(case, dev):
    f = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    return [f(case[k]) for k in ("depth", "alpha", "views", "target", "weight", "affine")]


def _run(case, dev, gpv=None, grad_loss=GRAD_LOSS, tensors=None):
    """Forward with every output, backward into NaN-filled buffers; a dict of device tensors."""
    from latentsplat_amd.depth_sup import inverse_depth_backward, inverse_depth_forward
    depth, alpha, views, target, weight, affine = tensors if tensors is not None else _dev(case, dev)
    modes = dict(align=case["align"], normalize=case["normalize"], alpha_min=case["alpha_min"])
    out = inverse_depth_forward(depth, alpha, views, target, weight, affine, want=("loss", "per_view", "inverse_depth", "affine"), **modes)
    filled = dict(depth=torch.full_like(depth, float("nan")), alpha=torch.full_like(alpha, float("nan")))
    g = inverse_depth_backward(depth, alpha, views, target, weight, out["workspace"],
                               None if grad_loss is None else torch.tensor([grad_loss], dtype=torch.float32, device=dev),
                               None if gpv is None else torch.from_numpy(np.array(gpv)).to(dev), out=filled, **modes)
    assert g["depth"] is filled["depth"] and g["alpha"] is filled["alpha"]
    out.update(grad_depth=g["depth"], grad_alpha=g["alpha"])
    return out


@pytest.mark.parametrize("align,normalize,weighted", CONFIGS)
@pytest.mark.parametrize("V,H,W", SHAPES)
def test_loss_against_float64(hip_device, V, H, W, align, normalize, weighted):
    case, gpv, want, stock = _case(V, H, W, align, normalize, weighted)
    got = _run(case, hip_device, gpv)
    show = f"({V},{H},{W}) {align} {normalize} {'weight' if weighted else 'mask'}"
    for k in QUANTITIES:
        assert bool(torch.isfinite(got[k]).all()), (show, k, "not finite: a gradient buffer was not written in full, or a planted pixel leaked")
        ref.held(k, got[k].double().cpu().numpy(), want[k], stock[k], show)
    # planted pixels: I = 0 and no gradient, exactly
    p = torch.from_numpy(np.array(case["planted"])).to(hip_device)
    if bool(p.any()):
        for k in ("inverse_depth", "grad_depth", "grad_alpha"):
            assert bool((got[k][p] == 0).all()), (show, k)
    # refused rows: per_view 0, gradient rows 0, affine (0, 0)
    for v in case["refusals"]:
        assert float(got["per_view"][v]) == 0.0 and float(got["affine"][v].abs().max()) == 0.0, (show, v)
        assert float(got["grad_depth"][v].abs().max()) == 0.0 and float(got["grad_alpha"][v].abs().max()) == 0.0, (show, v)
    if V >= 2 and H * W >= 12:
        assert len(case["refusals"]) == 1 and float(got["per_view"].abs().sum()) > 0 and float(got["grad_depth"].abs().max()) > 0
    # the same bits every call
    again = _run(case, hip_device, gpv)
    for k in QUANTITIES:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (show, k)


def test_slot_40_scales_are_honoured(hip_device):
    case, _, want, _ = _case(3, 37, 29, "given", "pixels", False)
    assert sorted(set(case["views"][:, 40].tolist())) == [0.5, 1.0, 2.5]
    got = _run(case, hip_device)
    live = ~torch.from_numpy(np.array(case["planted"])).to(hip_device)
    # depth = s z alpha was rendered: the map is 1 / z whatever s is (z in 2 .. 4)
    inv = got["inverse_depth"][live]
    assert 0.2 < float(inv.min()) and float(inv.max()) < 0.6


@pytest.mark.parametrize("align,normalize,weighted", [("given", "weights", False), ("fit", "pixels", True)])
@pytest.mark.parametrize("V,H,W", [(2, 7, 9), (3, 37, 29), (5, 11, 373)])
def test_a_view_alone_equals_its_rows_of_the_batch(hip_device, V, H, W, align, normalize, weighted):
    """Upstream through grad_per_view, which does not carry the 1 / V of the mean.  The slices are contiguous, and with
    H W % 4 != 0 their planes are aligned otherwise than in the batch."""
    case, gpv, _, _ = _case(V, H, W, align, normalize, weighted)
    dev = hip_device
    tensors = _dev(case, dev)
    batch = _run(case, dev, gpv, grad_loss=None, tensors=tensors)
    for v in range(V):
        alone = _run(case, dev, gpv[v:v + 1], grad_loss=None, tensors=[None if t is None else t[v:v + 1] for t in tensors])
        for k in QUANTITIES[1:]:
            assert np.array_equal(_bits(alone[k][0]), _bits(batch[k][v])), (v, k)
        assert np.array_equal(_bits(alone["loss"]), _bits(alone["per_view"]))                 # one view: the mean is the view
    assert float(batch["grad_depth"].abs().max()) > 0


def test_planes_that_are_aligned_differently_give_the_same_bits(hip_device):
    """Each input moved, in turn, to an address that is 4, 8, 12 bytes off a 16-byte boundary: every array decides its own
    access width, and no number changes."""
    case, gpv, _, _ = _case(2, 32, 32, "fit", "weights", True)
    dev = hip_device
    base = _run(case, dev, gpv)
    names = ("depth", "alpha", "views", "target", "weight")
    for which in (0, 1, 3, 4):
        for shift in (1, 2, 3):
            tensors = _dev(case, dev)
            t = tensors[which]
            room = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev)
            moved = room[shift:shift + t.numel()].view(t.shape)
            moved.copy_(t)
            assert moved.data_ptr() % 16 == 4 * shift and moved.is_contiguous()
            tensors[which] = moved
            got = _run(case, dev, gpv, tensors=tensors)
            for k in QUANTITIES:
                assert np.array_equal(_bits(got[k]), _bits(base[k])), (names[which], shift, k)
            assert float(room[:shift].abs().sum()) == 0 and float(room[shift + t.numel():].abs().sum()) == 0


def test_every_optional_output_in_turn_and_the_loss_function(hip_device):
    from latentsplat_amd import inverse_depth_loss
    from latentsplat_amd.depth_sup import inverse_depth_backward, inverse_depth_forward
    case, _, want, stock = _case(3, 37, 29, "fit", "pixels", True)
    dev = hip_device
    depth, alpha, views, target, weight, affine = _dev(case, dev)
    modes = dict(align="fit", normalize="pixels", alpha_min=case["alpha_min"])
    full = _run(case, dev, None, grad_loss=1.0)
    for only in ("loss", "per_view", "inverse_depth", "affine"):
        got = inverse_depth_forward(depth, alpha, views, target, weight, None, want=(only,), **modes)
        assert set(got) == {only, "workspace"} and np.array_equal(_bits(got[only]), _bits(full[only]))
    one = torch.ones(1, device=dev)
    for only in ("depth", "alpha"):
        got = inverse_depth_backward(depth, alpha, views, target, weight, full["workspace"], one, want=(only,), **modes)
        assert set(got) == {only} and np.array_equal(_bits(got[only]), _bits(full["grad_" + only]))
    # the autograd function: the same bits, extras on request, no gradient for the target or the weight
    d, a, t, w = (x.clone().requires_grad_(True) for x in (depth, alpha, target, weight))
    extras = {}
    loss = inverse_depth_loss(d, a, views, t, w, outputs=extras, **modes)
    assert loss.shape == () and np.array_equal(_bits(loss.reshape(1)), _bits(full["loss"]))
    for k in ("per_view", "inverse_depth", "affine"):
        assert np.array_equal(_bits(extras[k]), _bits(full[k])) and not extras[k].requires_grad
    (loss * 1.0).backward()
    assert np.array_equal(_bits(d.grad), _bits(full["grad_depth"])) and np.array_equal(_bits(a.grad), _bits(full["grad_alpha"]))
    assert t.grad is None and w.grad is None
    # defaults: (1, 0) under "given", the mask from target > 0, alpha_min 0.01
    plain = ref.loss_case(2, 9, 7, 3, plant=False)
    pd, pa, pv, pt, _, _ = _dev(plain, dev)
    got = float(inverse_depth_loss(pd, pa, pv, pt))
    ones = dict(plain, affine=None, alpha_min=0.01)
    assert got == pytest.approx(float(ref.loss_and_grads(ones, torch.float64)["loss"][0]), rel=1e-6)


def test_graph_capture_replays_the_eager_bits(hip_device):
    """Forward and backward of both align modes captured in one torch.cuda.graph and replayed on new inputs."""
    from latentsplat_amd.depth_sup import inverse_depth_backward, inverse_depth_forward
    dev = hip_device
    ca, _, _, _ = _case(3, 37, 29, "fit", "pixels", True)
    cb = ref.loss_case(3, 37, 29, seed=77, align="fit", normalize="pixels", weighted=True)
    depth, alpha, views, target, weight, _ = _dev(ca, dev)
    affine = torch.from_numpy(np.random.default_rng(1).uniform(0.5, 2.0, (3, 2)).astype(np.float32)).to(dev)
    up = torch.tensor([0.5], device=dev)
    names = ("loss", "per_view", "inverse_depth", "affine")
    bufs = {}
    for align in ("fit", "given"):
        bufs[align] = dict(fwd={k: torch.empty(s, device=dev) for k, s in zip(names, ((1,), (3,), (3, 37, 29), (3, 2)))},
                           bwd=dict(depth=torch.empty_like(depth), alpha=torch.empty_like(alpha)))
        from latentsplat_amd.depth_sup import workspace_bytes
        bufs[align]["fwd"]["workspace"] = torch.empty(workspace_bytes(3, 37, 29, align), dtype=torch.uint8, device=dev)

    def step():
        res = []
        for align in ("fit", "given"):
            modes = dict(align=align, normalize="pixels", alpha_min=ca["alpha_min"])
            out = inverse_depth_forward(depth, alpha, views, target, weight, affine if align == "given" else None, want=names,
                                        out=bufs[align]["fwd"], **modes)
            g = inverse_depth_backward(depth, alpha, views, target, weight, out["workspace"], up, out=bufs[align]["bwd"], **modes)
            res += [out[k] for k in names] + [g["depth"], g["alpha"]]
        return res

    side = torch.cuda.Stream(dev)                # warm-up on a side stream, as torch.cuda.graph asks for
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for dst, key in ((depth, "depth"), (alpha, "alpha"), (views, "views"), (target, "target"), (weight, "weight")):
        dst.copy_(torch.from_numpy(np.array(cb[key])).to(dev))
    graph.replay()
    torch.cuda.synchronize(dev)
    replayed = [t.clone() for t in captured]
    for t in captured:
        t.fill_(float("nan"))
    eager = step()
    for a, b in zip(replayed, eager):
        assert bool(torch.isfinite(a).all()) and np.array_equal(_bits(a), _bits(b))
    assert float(replayed[0]) > 0 and float(replayed[6]) > 0


def test_refusals_come_before_any_gpu_work(hip_device):
    from latentsplat_amd.depth_sup import inverse_depth_backward, inverse_depth_forward, inverse_depth_loss
    dev = hip_device
    case = ref.loss_case(2, 8, 8, 2)
    depth, alpha, views, target, _, affine = _dev(case, dev)
    sentinel = {k: torch.full(s, 7.0, device=dev) for k, s in (("loss", (1,)), ("per_view", (2,)), ("inverse_depth", (2, 8, 8)), ("affine", (2, 2)))}
    for bad in (dict(alpha_min=-0.5), dict(alpha_min=float("nan")), dict(alpha_min=float("inf"))):
        with pytest.raises(_lib.LsrError, match="invalid"):
            inverse_depth_forward(depth, alpha, views, target, None, affine, want=tuple(sentinel), out=sentinel, **bad)
        with pytest.raises(_lib.LsrError, match="invalid"):
            inverse_depth_backward(depth, alpha, views, target, None, torch.zeros(4096, dtype=torch.uint8, device=dev),
                                   torch.ones(1, device=dev), out=dict(depth=sentinel["inverse_depth"]), want=("depth",), **bad)
    torch.cuda.synchronize(dev)
    assert all(bool((t == 7.0).all()) for t in sentinel.values())
    for kw in (dict(align="median"), dict(normalize="points")):
        with pytest.raises(_lib.LsrError, match="align is one of"):
            inverse_depth_loss(depth, alpha, views, target, **kw)
    for args in ((depth, alpha[:1], views, target), (depth, alpha, views[:, :40], target), (depth, alpha, views, target[:, :4]),
                 (depth[0], alpha[0], views, target[0]), (depth.double(), alpha, views, target), (depth, alpha, views, target, target[:1])):
        with pytest.raises(_lib.LsrError):
            inverse_depth_loss(*args)
    with pytest.raises(_lib.LsrError, match="affine"):
        inverse_depth_loss(depth, alpha, views, target, None, affine[:1])
    with pytest.raises(_lib.LsrError, match="grad_loss or grad_per_view"):
        inverse_depth_backward(depth, alpha, views, target, None, torch.zeros(4096, dtype=torch.uint8, device=dev))


# ---- units through the render ----

@pytest.mark.parametrize("scale_invariant", [True, False])
def test_units_through_the_render(hip_device, scale_invariant):
    """One opaque fronto-parallel Gaussian on the optical axis at depth z0: a single splat's depth / alpha is its tz = s z0, so
    the map at the centre pixel is 1 / z0 in the capture's units with or without the scene scale, and the loss against that
    target there is 0, both within 2^-20 relative."""
    from latentsplat_amd import GaussianScene, inverse_depth_loss
    from latentsplat_amd.rasterizer import build_view_table
    dev = hip_device
    z0, H, W = 3.0, 17, 17
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    scene = GaussianScene.from_tensors(xyz=f([[0.0, 0.0, z0]]), features_dc=f([[[0.5, 0.2, -0.3]]]), features_rest=torch.zeros((1, 0, 3)),
                                       opacity=f([[8.0]]), scaling=f([[math.log(0.3), math.log(0.3), math.log(0.05)]]),
                                       rotation=f([[1.0, 0.0, 0.0, 0.0]])).to(dev)
    ext = torch.eye(4, device=dev)[None]
    intr = torch.tensor([[[0.8, 0.0, 0.5], [0.0, 0.8, 0.5], [0.0, 0.0, 1.0]]], device=dev)
    views = build_view_table(ext, intr, torch.tensor([0.4], device=dev), torch.tensor([40.0], device=dev), torch.zeros(3, device=dev),
                             scale_invariant=scale_invariant)
    s = float(views[0, 40])
    assert (s != 1.0) == scale_invariant
    with torch.no_grad():
        _, _, mask, depth, _ = scene.render(views, H, W)
    assert float(mask[0, 8, 8]) > 0.9
    target = torch.zeros((1, H, W), device=dev)
    target[0, 8, 8] = 1.0 / z0
    extras = {}
    loss = inverse_depth_loss(depth, mask, views, target, normalize="weights", outputs=extras)
    centre = float(extras["inverse_depth"][0, 8, 8])
    print(f"scale_invariant={scale_invariant}: s = {s:.6g}, I(centre) z0 - 1 = {centre * z0 - 1:.3e}, loss z0 = {float(loss) * z0:.3e}")
    assert abs(centre * z0 - 1.0) <= 2.0 ** -20
    assert float(loss) * z0 <= 2.0 ** -20
    assert float(extras["inverse_depth"][0, 0, 0]) == 0.0            # nothing was rendered in the corner


# ---- priors through prepare_images ----

def test_prepare_depth_priors_is_the_block_mean_for_a_power_of_two_reduction(hip_device):
    from latentsplat_amd.depth_sup import prepare_depth_priors
    from latentsplat_amd.images import SourceCamera
    rng = np.random.default_rng(12)
    prior = rng.integers(0, 65536, (3, 32, 48)).astype(np.uint16)
    prior[0, :4, :4] = 65535
    prior[1, :4, :4] = 0
    for r in (2, 4):
        H, W = 32 // r, 48 // r
        got = prepare_depth_priors(prior, SourceCamera(1, 40.0, 40.0, 24.0, 16.0), H, W, 40.0 / r, 40.0 / r, hip_device)
        want = prior.astype(np.float64).reshape(3, H, r, W, r).mean(axis=(2, 4)) / 65536.0
        err = float(np.abs(got.double().cpu().numpy() - want).max())
        print(f"reduction {r}: largest error {err:.3e} (2^-22 = {2.0 ** -22:.3e}, the 16-bit quantum 2^-16 = {2.0 ** -16:.3e})")
        assert got.shape == (3, H, W) and got.dtype == torch.float32 and err <= 2.0 ** -22


def test_prepare_depth_priors_of_an_opencv_source(hip_device):
    from latentsplat_amd.depth_sup import prepare_depth_priors
    from latentsplat_amd.images import SourceCamera
    dev = hip_device
    rng = np.random.default_rng(13)
    Hs, Ws, H, W, r = 40, 56, 20, 28, 2.0
    ys, xs = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    prior = np.clip(20000 + 15000 * np.sin(0.2 * xs) * np.cos(0.15 * ys) + rng.integers(-300, 300, (2, Hs, Ws)), 0, 65535).astype(np.uint16)
    params = [45.0, 44.0, 27.3, 20.6, 0.05, -0.01, 0.002, -0.003]
    cam = cr.camera_numbers(4, params)
    fxo, fyo = cam["fx"] / r, cam["fy"] / r
    planes = np.stack([(prior >> 8).astype(np.uint8), (prior & 255).astype(np.uint8), np.zeros(prior.shape, np.uint8)], axis=-1)
    image, _, fragile = cr.prepare_ref(planes, cam, H, W, fxo, fyo)
    want = (65280.0 * image[:, 0] + 255.0 * image[:, 1]) / 65536.0
    stock_image, _ = cr.stock_prepare(torch.from_numpy(planes).to(dev), cam, H, W, fxo, fyo)
    stock = (65280.0 * stock_image[:, 0] + 255.0 * stock_image[:, 1]) / 65536.0
    got = prepare_depth_priors(prior, SourceCamera.from_colmap(4, params), H, W, fxo, fyo, dev)
    assert fragile.mean() <= 0.01
    keep = ~fragile
    err = lambda t: float(np.abs(t.double().cpu().numpy() - want)[..., keep].max())
    mine, theirs = err(got), err(stock)
    print(f"OPENCV prior: error {mine:.3e}, stock {theirs:.3e}, ratio {mine / theirs if theirs else float('nan'):.3f}")
    assert theirs < 1e-4 and mine <= 1.1 * theirs
    assert float(got.max()) > 0.3


# ---- Capture and the trainer ----

VIEWS, W0, H0, LEFT = 4, 24, 16, 8


@pytest.fixture(scope="module")
def world(hip_device, tmp_path_factory):
    """4 images of 24 x 16 around 90 points; the principal point 8 pixels left of the centre, so that the target camera has 8
    columns the photograph does not cover, some of them under sparse points; every image observes every point (some project
    outside, some lie behind)."""
    from latentsplat_amd.depth_sup import encode_pgm16
    rng = np.random.default_rng(21)
    c2w = np.zeros((VIEWS, 4, 4))
    for k in range(VIEWS):
        ang = 2 * math.pi * k / VIEWS + 0.3
        offset = np.array([math.cos(ang), 0.2 * math.sin(2 * ang), math.sin(ang)])
        forward = -offset / np.linalg.norm(offset)
        right = np.cross([0.0, 1.0, 0.0], forward)
        right /= np.linalg.norm(right)
        c2w[k, :3, 0], c2w[k, :3, 1], c2w[k, :3, 2], c2w[k, :3, 3] = right, np.cross(forward, right), forward, 4.0 * offset
        c2w[k, 3, 3] = 1.0
    xyz = np.concatenate([rng.uniform(-1.2, 1.2, (80, 3)), rng.uniform(-6.0, 6.0, (10, 3))])
    rgb = rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    ys, xs = np.meshgrid(np.arange(H0), np.arange(W0), indexing="ij")
    photos = [np.stack([127 + 100 * np.sin(0.3 * xs + k), 127 + 100 * np.cos(0.4 * ys - k), 40 * k + 0 * xs], -1).astype(np.uint8) for k in range(VIEWS)]
    camera = dict(id=2, model=1, width=W0, height=H0, params=[20.0, 19.0, W0 / 2.0 - LEFT, H0 / 2.0])
    names = [f"img_{(3 * k) % VIEWS}.npy" for k in range(VIEWS)]                       # file order is not name order
    root = tmp_path_factory.mktemp("depth_capture")
    observed = [rng.permutation(len(xyz)) for _ in range(VIEWS)]
    model = ref.write_capture_with_observations(root, c2w, [camera], [2] * VIEWS, photos, names, xyz, rgb, observed)
    # priors for three of the four images, as .pgm, .npy and .pgm at half the photograph's size
    priors = root / "priors"
    os.makedirs(priors)
    for k, name in enumerate(sorted(names)[:3]):
        h, w = (H0 // 2, W0 // 2) if k == 2 else (H0, W0)
        py, px = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        a = (65536 * (0.15 + 0.1 * px / w + 0.05 * py / h + 0.01 * k)).astype(np.uint16)
        if k == 1:
            np.save(priors / (os.path.splitext(name)[0] + ".npy"), a)
        else:
            with open(priors / (os.path.splitext(name)[0] + ".pgm"), "wb") as f:
                f.write(encode_pgm16(a))
    return dict(root=root, model=model, names=names, xyz=xyz, priors=priors)


def test_capture_sparse_depth_and_priors(hip_device, world):
    from latentsplat_amd.capture import Capture
    from latentsplat_amd.depth_sup import sparse_inverse_depth
    dev = hip_device
    cap = Capture.load(world["root"], device=dev, observations=True)
    idx = list(range(VIEWS))
    assert cap.sizes == [(H0, W0)] * VIEWS and cap.model.obs_offsets is not None
    assert int(cap.model.obs_offsets[-1]) == VIEWS * len(world["xyz"])                 # the observation without a point is left out
    coverage = cap.coverage(idx)
    assert bool((coverage[:, :, :LEFT] == 0).all()) and bool((coverage[:, :, LEFT:] == 1).all())
    got = cap.sparse_depth(idx)
    near = 0.01 * cap.cameras_extent
    filled_uncovered = 0
    for k in idx:
        row = cap.model.names.index(cap.names[k])
        host = sparse_inverse_depth(cap.model, row, H0, W0, 20.0, 19.0, near)
        filled_uncovered += int((host[:, :LEFT] > 0).sum())
        host[:, :LEFT] = 0                                                              # coverage 0: cleared
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), host.view(np.uint32)), k
        assert 15 <= int((host > 0).sum()) <= 80
    assert filled_uncovered > 0                                                         # the clearing had something to clear
    assert torch.equal(cap.sparse_depth([2, 0]), got[[2, 0]])
    # the priors: three found, aligned to the sparse points; the fourth image has none
    assert cap.load_depth_priors(world["priors"]) == 3
    prior, affine = cap.depth_priors(idx)
    assert prior.shape == (VIEWS, H0, W0) and affine.shape == (VIEWS, 2)
    assert float(prior[3].abs().max()) == 0 and affine[3].tolist() == [0.0, 0.0]
    assert bool((prior[:3, :, LEFT:] > 0.1).all()) and bool((prior[:3, :, :LEFT] == 0).all()) and bool((affine[:3, 0] > 0).all())
    print("prior alignments:", affine.tolist())
    plain = Capture.load(world["root"], device=dev)
    with pytest.raises(_lib.LsrError, match="loaded without"):
        plain.sparse_depth([0])
    with pytest.raises(_lib.LsrError, match="loaded without"):
        plain.load_depth_priors(world["priors"])
    with pytest.raises(_lib.LsrError, match="no depth priors"):
        Capture.load(world["root"], device=dev, observations=True).depth_priors([0])


def test_train_colmap_with_depth_supervision(hip_device, world, tmp_path):
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_colmap
    common = [str(world["root"]), "--steps", "12", "--hold", "0", "--batch", "2", "--seed", "3", "--densify-interval", "0"]
    runs = {"sparse": ["--depth-sparse", "0.01"], "priors": ["--depth-priors", str(world["priors"])],
            "fit": ["--depth-priors", str(world["priors"]), "--depth-align", "fit", "--depth-sparse", "0.01"], "plain": []}
    res = {}
    for label, flags in runs.items():
        res[label] = train_colmap.main(common + ["--out", str(tmp_path / label)] + flags)
        with open(tmp_path / label / "metrics.json") as f:
            stored = json.load(f)
        assert stored["loss_first"] == res[label]["loss_first"]
        if label == "plain":
            assert "depth_loss_first" not in stored and "depth_loss_last" not in stored
        else:
            first, last = stored["depth_loss_first"], stored["depth_loss_last"]
            print(f"train_colmap {label}: depth loss {first:.5f} -> {last:.5f}, loss {stored['loss_first']:.5f} -> {stored['loss_last']:.5f}")
            assert math.isfinite(first) and math.isfinite(last) and first > 0 and math.isfinite(stored["loss_last"])
    assert res["priors"]["depth_priors"] == 3
    # without either flag: the first step is the step the trainer took before it knew of depth, bit for bit
    import random
    from latentsplat_amd.capture import Capture
    from latentsplat_amd.losses import photometric_loss
    dev = hip_device
    cap = Capture.load(world["root"], "sparse/0", "images", 1.0, dev)
    train, _ = cap.split(0)
    scene = cap.initial_scene(3)
    (H, W), idx = train_colmap.batches(cap.size_groups(train), 2, random.Random(3)).pop()
    cover = cap.coverage(idx)[:, None]
    with torch.no_grad():
        render = scene.render(cap.views(idx, torch.zeros(3, device=dev)), H, W)[0]
    first = float(photometric_loss(render * cover, cap.targets(idx) * cover, 0.2))
    assert first == res["plain"]["loss_first"]
    assert res["sparse"]["loss_first"] > first and res["priors"]["loss_first"] > first
