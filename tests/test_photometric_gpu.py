"""The photometric loss on the MI355X: lsr_photometric_forward / _backward against the float64 restatement
(tests/photometric_ref.py), held to the stock float32 composition's own error on the same inputs; determinism, the autograd
surface, graph capture, the metric mode and the fitting tool with the D-SSIM term.

The bars: per quantity, the kernel's largest error against float64 must be within 4 x the largest error of the stock
composition (torch CPU conv2d in float32, autograd for the gradient) on the same inputs, with a floor of 2^-20 of the
quantity's scale (1 for S, |loss| for the scalars, max |gradient| for gradients).  Every element is on the bar."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import photometric_ref as ref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu

T = ref.TILE
SHAPES = [(1, 1, 1, 1), (1, 3, 7, 5), (2, 3, 11, 11), (1, 3, 10, 12), (2, 3, 37, 53), (3, 1, 64, 64), (1, 4, 33, 17),
          # one below, at and one above the kernel's tile edge, in each dimension
          (1, 2, T - 1, T), (1, 2, T, T + 1), (1, 2, T + 1, T - 1),
          # the trip counts of a full-size fit (tests/test_photometric_cpu.py pins what each one reaches): the shift 0.5 of
          # every image from 145 px a side, interior tiles whose halo lies inside the image, more than 64 and more than
          # 128 slots per image (k_photo_finish's lanes take a second and a third slot), more than 16 and more than 32
          # images (its waves take a second and a third image)
          (1, 3, 160, 160), (2, 3, 96, 352), (1, 1, 33, 2081), (17, 1, 7, 5), (33, 2, 11, 11)]
FULL_SIZE = (1, 3, 160, 160)
LAMBDAS = (0.0, 0.2, 1.0)
FLOOR = 2.0 ** -20
MARGIN = 4.0
WORST = {}          # quantity -> worst kernel error / composition error seen (printed per test)
WORST_AT_HALF = {}  # the same over the shapes whose shift is 0.5 alone: every image of a real fit


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Inputs and, per lambda, the float64 results and the float32 composition's: computed once, shared, never modified."""
    x, y = ref.make_pair(shape, kind, seed=100 + sum(shape))
    per_lambda = {}
    for lam in LAMBDAS:
        want = ref.results(x, y, lam)
        want["grad"] = ref.gradient(x, y, lam)
        per_lambda[lam] = (want, ref.stock_results(torch.from_numpy(x), torch.from_numpy(y), lam))
    return x, y, per_lambda


def _held(name, got, want, stock, scale, show, worst=WORST):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    err_stock = float(np.abs(stock - want).max())
    bar = max(MARGIN * err_stock, FLOOR * scale)
    ratio = err / err_stock if err_stock > 0 else (0.0 if err == 0 else float("inf"))
    if np.isfinite(ratio):
        worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"{show} {name:9s} kernel {err:.3e}  composition {err_stock:.3e}  ratio {ratio:.3f}  bar {bar:.3e}")
    assert err <= bar, (show, name, err, err_stock, bar)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_the_restatement_within_the_compositions_error(hip_device, shape, kind):
    from latentsplat_amd.losses import photometric_backward, photometric_forward, photometric_loss
    x, y, per_lambda = _case(shape, kind)
    xd, yd = torch.from_numpy(x).to(hip_device), torch.from_numpy(y).to(hip_device)
    one = torch.ones(1, device=hip_device)
    worst = WORST_AT_HALF if ref.photo_shift(*shape[2:]) == 0.5 else WORST
    for lam in LAMBDAS:
        want, stock = per_lambda[lam]
        show = f"{shape} {kind} lambda={lam}:"
        out = photometric_forward(xd, yd, lam, want=("loss", "l1", "ssim", "ssim_map", "saved"))
        grad = photometric_backward(xd, yd, out["saved"], one, lam).cpu().numpy()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        scale = abs(want["loss"])
        _held("loss", got["loss"][0], want["loss"], stock["loss"], scale, show, worst)
        _held("l1", got["l1"], want["l1"], stock["l1"], scale, show, worst)
        _held("ssim", got["ssim"], want["ssim"], stock["ssim"], scale, show, worst)
        _held("map", got["ssim_map"], want["map"], stock["map"], 1.0, show, worst)
        _held("grad", grad, want["grad"], stock["grad"], float(np.abs(want["grad"]).max()), show, worst)
        # through autograd: the same launches, the same bits
        leaf = xd.clone().requires_grad_(True)
        loss = photometric_loss(leaf, yd, lam)
        loss.backward()
        assert loss.shape == () and np.array_equal(loss.detach().cpu().numpy(), got["loss"][0])
        assert np.array_equal(leaf.grad.cpu().numpy(), grad)
    print("worst kernel error / composition error so far:", {k: round(v, 3) for k, v in WORST.items()},
          "at shift 0.5:", {k: round(v, 3) for k, v in WORST_AT_HALF.items()})


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def test_two_calls_give_the_same_bits(hip_device):
    from latentsplat_amd.losses import photometric_backward, photometric_forward
    for shape in ((2, 3, 37, 53), FULL_SIZE):
        x, y, _ = _case(shape, "noise")
        xd, yd = torch.from_numpy(x).to(hip_device), torch.from_numpy(y).to(hip_device)
        up = torch.full((1,), 0.7, device=hip_device)
        runs = []
        for _ in range(2):
            out = photometric_forward(xd, yd, 0.2, want=("loss", "l1", "ssim", "ssim_map", "saved"))
            out["grad"] = photometric_backward(xd, yd, out["saved"], up, 0.2)
            runs.append({k: _bits(v) for k, v in out.items()})
        for k in runs[0]:
            assert np.array_equal(runs[0][k], runs[1][k]), (shape, k)


def test_autograd_surface(hip_device):
    from latentsplat_amd import l1, photometric_loss, ssim
    x, y, per_lambda = _case((2, 3, 37, 53), "noise")
    xd, yd = torch.from_numpy(x).to(hip_device), torch.from_numpy(y).to(hip_device)

    def grad_of(fn, image):
        leaf = image.clone().requires_grad_(True)
        fn(leaf).backward()
        return leaf.grad

    g1 = grad_of(lambda t: photometric_loss(t, yd), xd)
    g3 = grad_of(lambda t: 3 * photometric_loss(t, yd), xd)
    three = (3 * g1).cpu().numpy()
    assert (np.abs(g3.cpu().numpy() - three) <= np.spacing(np.abs(three))).all()          # 1 ulp
    # a permuted (non-contiguous) image gives the contiguous bits, and its gradient comes back in its own layout
    hwc = xd.permute(0, 2, 3, 1).contiguous()
    leaf = hwc.clone().requires_grad_(True)
    view = leaf.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    loss = photometric_loss(view, yd)
    loss.backward()
    assert np.array_equal(_bits(loss), _bits(photometric_loss(xd, yd)))
    assert np.array_equal(_bits(leaf.grad.permute(0, 3, 1, 2).contiguous()), _bits(g1))
    # differentiable in the image only
    with pytest.raises(_lib.LsrError, match="image only"):
        photometric_loss(xd, yd.clone().requires_grad_(True))
    with pytest.raises(_lib.LsrError, match="one shape"):
        photometric_loss(xd, yd[:, :, :-1])
    # (C, H, W) is V = 1
    g_chw = grad_of(lambda t: photometric_loss(t, yd[0]), xd[0])
    g_one = grad_of(lambda t: photometric_loss(t, yd[:1]), xd[:1])
    assert g_chw.shape == xd[0].shape and np.array_equal(_bits(g_chw), _bits(g_one[0]))
    assert np.array_equal(_bits(photometric_loss(xd[0], yd[0])), _bits(photometric_loss(xd[:1], yd[:1])))
    # lambda 1 is 1 - SSIM, lambda 0 the L1 mean; the value-only entry points agree with the loss's parts
    want = per_lambda[0.2][0]
    s, m = ssim(xd, yd, return_map=True)
    assert m.shape == xd.shape and s.shape == () and ssim(xd, yd, per_image=True).shape == (2,)
    assert abs(float(photometric_loss(xd, yd, 1.0)) - (1 - float(s))) <= 2e-7
    assert abs(float(photometric_loss(xd, yd, 0.0)) - float(l1(xd, yd))) <= 1e-8
    assert np.abs(ssim(xd, yd, per_image=True).cpu().numpy() - want["ssim"]).max() <= 1e-5
    assert np.abs(l1(xd, yd, per_image=True).cpu().numpy() - want["l1"]).max() <= 1e-7


def test_graph_capture_replays_on_new_inputs(hip_device):
    from latentsplat_amd import photometric_loss
    dev = hip_device
    xa, y, _ = _case((2, 3, 37, 53), "noise")
    xb, _, _ = _case((2, 3, 37, 53), "smooth")
    yd = torch.from_numpy(y).to(dev)
    static = torch.from_numpy(xa).to(dev).requires_grad_(True)

    def step():
        loss = photometric_loss(static, yd)
        grad, = torch.autograd.grad(loss, static)
        return loss, grad

    side = torch.cuda.Stream(dev)                # warm-up on a side stream, as torch.cuda.graph asks for
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step()
    with torch.no_grad():
        static.copy_(torch.from_numpy(xb).to(dev))
    graph.replay()
    torch.cuda.synchronize(dev)
    leaf = torch.from_numpy(xb).to(dev).requires_grad_(True)
    eager = photometric_loss(leaf, yd)
    eager.backward()
    assert np.array_equal(_bits(loss), _bits(eager))
    assert np.array_equal(_bits(grad), _bits(leaf.grad))


@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 3, 11, 11), FULL_SIZE])
def test_metric_mode(hip_device, shape):
    """compute_ssim: sample covariance, the mean over the interior pixels ((1, 3, 11, 11) has one per plane; at
    (1, 3, 160, 160) the crop cuts through the sixteen outer tiles and leaves the nine inner ones whole)."""
    from latentsplat_amd import compute_ssim
    for kind in ("noise", "smooth"):
        x, y, _ = _case(shape, kind)
        want = ref.results(x, y, 1.0, 121 / 120, 5)
        stock = ref.stock_results(torch.from_numpy(x), torch.from_numpy(y), 1.0, 121 / 120, 5, grad=False)
        got = compute_ssim(torch.from_numpy(y).to(hip_device), torch.from_numpy(x).to(hip_device))
        assert got.shape == (shape[0],)
        _held("metric", got.cpu().numpy(), want["ssim"], stock["ssim"], abs(want["loss"]), f"{shape} {kind} compute_ssim:")


def test_metric_mode_needs_a_window(hip_device):
    from latentsplat_amd import compute_ssim
    x, y, _ = _case((1, 3, 10, 12), "noise")
    with pytest.raises(_lib.LsrError, match="invalid"):
        compute_ssim(torch.from_numpy(y).to(hip_device), torch.from_numpy(x).to(hip_device))


def test_fit_tool_with_the_dssim_term(hip_device, tmp_path):
    from latentsplat_amd.ply_import import load_ply
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    G = 2000
    path = tmp_path / "point_cloud.ply"
    sref.write_scene_file(path, G, 64, 2)            # the scene file of tests/test_scene_params_gpu.py
    out = tmp_path / "fit"
    res = fit_ply.main([str(path), "--out", str(out), "--views", "3", "--size", "48", "--steps", "20", "--lambda-dssim", "0.2"])
    print("fit:", res)
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
    assert res["lambda_dssim"] == 0.2 and res["steps"] == 20 and res["gaussians"] == G
    assert json.load(open(out / "fit.json")) == res
    fitted = load_ply(out / "point_cloud.ply", hip_device)
    assert fitted.means.shape == (G, 3)
    for t in (fitted.means, fitted.covariances, fitted.opacities, fitted.shs, fitted.scales, fitted.rotations):
        assert torch.isfinite(t).all()
