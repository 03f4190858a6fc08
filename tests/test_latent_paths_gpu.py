"""The latent epilogue on the MI355X at fractional and per-axis scales and on every path of its kernels, against the
float64 restatement (tests/latent_ref.py), held to the stock float32 composition's own error on the same inputs.

Each case of ref.CASES is run as (a) the resize alone, (b) mask mode with noise and colour; cases 1, 2, 5 and 8 also as
(c) variational with noise (planted clamp values; the default interval and, once, (-10, 2)) and (d) variational without
noise, each with (e) the gradient of z alone, of skip alone and of both.  Isotropic cases go through the public
rescale / sample_rescale_skip with a Fraction, the others through _LatentEpilogue.apply; the ABI modes the wrappers never
select (outputs.z == NULL, d_features pre-filled with NaN) through ctypes.  The bars are in tests/latent_ref.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import latent_ref as ref

pytestmark = pytest.mark.gpu

CASE_IDS = sorted(ref.CASES)
VARIATIONAL_RUNS = [(c, ref.DEFAULT_INTERVAL) for c in ref.VARIATIONAL_CASES] + [(2, ref.NARROW_INTERVAL)]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


def _run(case, inp, dev, noise=True, color=True):
    """One forward on the device -> (features leaf, dict(sample, skip, z, logvar)), all (V, ., ., .)."""
    from latentsplat_amd.decoder import latent_epilogue as le
    V, Cc, H, W, oh, ow = ref.CASES[case]
    feats = inp["features"].to(dev).requires_grad_(True)
    nz = inp["noise"].to(dev) if noise else None
    col = inp["color"].to(dev) if color else None
    variational = inp["variational"]
    if ref.is_isotropic(case):
        ep = le.sample_rescale_skip(feats[None], inp["mask"].to(dev)[None], None if col is None else col[None],
                                    Fraction(H, oh), variational, noise=None if nz is None else nz[None],
                                    deterministic=nz is None, logvar_interval=inp["interval"])
        skip = ep.skip_z if color else ep.latent_sample
        return feats, dict(sample=ep.latent_sample[0], skip=skip[0], z=ep.z[0], logvar=ep.logvar[0])
    mode = le.LOGVAR_FROM_FEATURES if variational else le.LOGVAR_FROM_MASK
    skip, z, logvar = le._LatentEpilogue.apply(feats, None if variational else inp["mask"].to(dev), nz, col, (oh, ow), mode,
                                               True, True, inp["interval"])
    return feats, dict(sample=skip[:, 3 if color else 0:], skip=skip, z=z, logvar=logvar)


def _grads(feats, out, inp, dev, color=True):
    g_z, g_skip = inp["g_z"].to(dev), (inp["g_skip"] if color else inp["g_skip"][:, 3:]).to(dev)
    grads = {}
    grads["z"], = torch.autograd.grad([out["z"]], feats, [g_z], retain_graph=True)
    grads["skip"], = torch.autograd.grad([out["skip"]], feats, [g_skip], retain_graph=True)
    grads["both"], = torch.autograd.grad([out["z"], out["skip"]], feats, [g_z, g_skip], retain_graph=True)
    return {m: _np(g) for m, g in grads.items()}


def _hold_epilogue(case, inp, out, grads, want, stock, tag, variational):
    Cc = ref.CASES[case][1]
    for k in ("sample", "skip", "z", "logvar"):
        ref.held(k, _np(out[k]), want[k], stock[k], "value", tag)
    for m in ref.GRAD_MODES:
        g, w, s = grads[m], want["grad_" + m], stock["grad_" + m]
        # the mean half and the logvar half each at their own scale
        ref.held(f"d_mean ({m})", g[:, :Cc], w[:, :Cc], s[:, :Cc], "grad", tag)
        if variational:
            ref.held(f"d_logvar ({m})", g[:, Cc:], w[:, Cc:], s[:, Cc:], "grad", tag)


def _print_worst():
    print("worst kernel error / stock error so far:", {k: round(v, 3) for k, v in ref.WORST.items()})


@pytest.mark.parametrize("case", CASE_IDS)
def test_resize_only(hip_device, case):
    """(a): z and its gradient, no posterior, no skip.

    Case 7 (1024 x 4 -> 1 x 1, one output that nearly cancels: 4.8e-3) is the tightest: the bar there is the floor, 4.6e-9.
    With the forward's 256 row lanes added one after another the kernel was 5.5e-9 from float64 (stock: 1.0e-9); added
    pairwise it is 2.9e-9."""
    from latentsplat_amd.decoder import latent_epilogue as le
    V, Cc, H, W, oh, ow = ref.CASES[case]
    inp = ref.make_inputs(case)
    want, stock = ref.resize_pair(case)
    x = inp["features"].to(hip_device).requires_grad_(True)
    if ref.is_isotropic(case):
        z = le.rescale(x, Fraction(oh, H))
    else:
        z = le._LatentEpilogue.apply(x, None, None, None, (oh, ow), le.LOGVAR_FROM_MASK, False, False, ref.DEFAULT_INTERVAL)[1]
    assert z.shape == (V, Cc, oh, ow)
    grad, = torch.autograd.grad([z], x, [inp["g_z"].to(hip_device)])
    tag = f"case {case} (a):"
    ref.held("resize z", _np(z), want["z"], stock["z"], "resize", tag)
    ref.held("resize grad", _np(grad), want["grad"], stock["grad"], "resize", tag)
    _print_worst()


@pytest.mark.parametrize("case", CASE_IDS)
def test_mask_mode_with_noise_and_colour(hip_device, case):
    """(b) with (e): logvar = log(1 - mask) with exact 0 and 1 in the mask."""
    inp = ref.make_inputs(case)
    want, stock = ref.epilogue_pair(case)
    feats, out = _run(case, inp, hip_device)
    grads = _grads(feats, out, inp, hip_device)
    assert np.array_equal(_bits(out["skip"][:, :3]), inp["color"].numpy().view(np.uint32))     # colour: a copy
    assert np.array_equal(_bits(out["skip"][:, 3:]), _bits(out["sample"]))
    _hold_epilogue(case, inp, out, grads, want, stock, f"case {case} (b):", False)
    _print_worst()


@pytest.mark.parametrize("case,interval", VARIATIONAL_RUNS)
def test_variational_with_noise(hip_device, case, interval):
    """(c) with (e): the logvar half holds both ends of the interval, their float32 neighbours and > 10 % outside on
    each side; the gradient passes at both ends, inclusive, and nowhere outside."""
    Cc = ref.CASES[case][1]
    inp = ref.make_inputs(case, True, interval)
    want, stock = ref.epilogue_pair(case, True, interval)
    feats, out = _run(case, inp, hip_device)
    grads = _grads(feats, out, inp, hip_device)
    assert np.array_equal(_bits(out["skip"][:, :3]), inp["color"].numpy().view(np.uint32))
    _hold_epilogue(case, inp, out, grads, want, stock, f"case {case} (c) {interval}:", True)
    lv = inp["features"][:, Cc:].numpy()
    lo, hi = np.float32(interval[0]), np.float32(interval[1])
    outside = (lv < lo) | (lv > hi)
    assert outside.mean() >= 0.2 and (lv == lo).sum() >= 8 and (lv == hi).sum() >= 8
    for m in ref.GRAD_MODES:
        d_lv = grads[m][:, Cc:]
        assert (d_lv[outside] == 0).all(), (m, "gradient outside the clamp interval")
        assert (d_lv[lv == lo] != 0).all() and (d_lv[lv == hi] != 0).all(), (m, "no gradient at an end of the interval")
    _print_worst()


@pytest.mark.parametrize("case", ref.VARIATIONAL_CASES)
def test_variational_without_noise(hip_device, case):
    """(d) with (e): the sample is the mean, bit for bit, and the logvar half gets an exact zero gradient."""
    Cc = ref.CASES[case][1]
    inp = ref.make_inputs(case, True)
    want, stock = ref.epilogue_pair(case, True, ref.DEFAULT_INTERVAL, False)
    feats, out = _run(case, inp, hip_device, noise=False)
    grads = _grads(feats, out, inp, hip_device)
    assert np.array_equal(_bits(out["sample"]), inp["features"][:, :Cc].numpy().view(np.uint32))
    assert np.array_equal(_bits(out["skip"][:, :3]), inp["color"].numpy().view(np.uint32))
    for m in ref.GRAD_MODES:
        assert (grads[m][:, Cc:] == 0).all(), m
    _hold_epilogue(case, inp, out, grads, want, stock, f"case {case} (d):", True)
    _print_worst()


def test_colourless_skip_at_a_fractional_scale(hip_device):
    """color_channels == 0: `skip` is the sample alone (case 2, scalar path)."""
    inp = ref.make_inputs(2)
    want, stock = ref.epilogue_pair(2, False, ref.DEFAULT_INTERVAL, True, False)
    feats, out = _run(2, inp, hip_device, color=False)
    grads = _grads(feats, out, inp, hip_device, color=False)
    _hold_epilogue(2, inp, out, grads, want, stock, "case 2 (b) no colour:", False)
    _print_worst()


# ---- the C ABI directly -------------------------------------------------------------------------------------------

def _abi(case, inp, dev, noise=True):
    V, Cc, H, W, oh, ow = ref.CASES[case]
    variational = inp["variational"]
    t = {k: inp[k].to(dev).contiguous() for k in ("features", "mask", "noise", "color", "g_z", "g_skip")}
    dims = _lib.LatentDims(V, Cc, H, W, oh, ow, 1 if variational else 0, 3, inp["interval"][0], inp["interval"][1], 0, 0)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    ins = _lib.LatentInputs(p(t["features"]), None if variational else p(t["mask"]), p(t["noise"]) if noise else None, p(t["color"]))
    return _lib.load(), dims, ins, t, p


def _abi_forward(case, inp, dev, want_z, noise=True):
    lib, dims, ins, t, p = _abi(case, inp, dev, noise)
    V, Cc, H, W, oh, ow = ref.CASES[case]
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    skip, z, logvar = nan(V, 3 + Cc, H, W), nan(V, Cc, oh, ow) if want_z else None, nan(V, Cc if inp["variational"] else 1, H, W)
    outs = _lib.LatentOutputs(p(skip), p(z), p(logvar))
    torch.cuda.synchronize(dev)
    assert lib.lsr_latent_forward(C.byref(dims), C.byref(ins), C.byref(outs), None) == 0
    torch.cuda.synchronize(dev)
    return skip, z, logvar


@pytest.mark.parametrize("variational", [False, True], ids=["mask", "variational"])
@pytest.mark.parametrize("case", ref.ABI_CASES)
def test_abi_without_z_gives_the_same_skip_and_logvar(hip_device, case, variational):
    """outputs.z == NULL splits the rows into ceil(H / 8) bands instead of out_height: every element of skip and logvar
    is still written (the buffers start as NaN), with the bits of the call that also wants z."""
    inp = ref.make_inputs(case, variational)
    skip, z, logvar = _abi_forward(case, inp, hip_device, True)
    skip_noz, _, logvar_noz = _abi_forward(case, inp, hip_device, False)
    for t in (skip, z, logvar, skip_noz, logvar_noz):
        assert not torch.isnan(t).any()
    assert np.array_equal(_bits(skip), _bits(skip_noz)) and np.array_equal(_bits(logvar), _bits(logvar_noz))
    want, stock = ref.epilogue_pair(case, variational)
    tag = f"case {case} abi {'variational' if variational else 'mask'}:"
    for k, got in (("skip", skip_noz), ("logvar", logvar_noz), ("z", z)):
        ref.held(k, _np(got), want[k], stock[k], "value", tag)
    _print_worst()


@pytest.mark.parametrize("run", ["mask", "variational", "deterministic"])
@pytest.mark.parametrize("case", ref.ABI_CASES)
def test_abi_backward_writes_every_element(hip_device, case, run):
    """d_features is written, not accumulated: pre-filled with NaN it holds the gradient afterwards, for g_z alone, g_skip
    alone and both; in mask mode, variational with noise and variational without (the logvar half is then zeros)."""
    variational, noise = run != "mask", run != "deterministic"
    Cc = ref.CASES[case][1]
    inp = ref.make_inputs(case, variational)
    want, stock = ref.epilogue_pair(case, variational, ref.DEFAULT_INTERVAL, noise)
    lib, dims, ins, t, p = _abi(case, inp, hip_device, noise)
    for m in ref.GRAD_MODES:
        d = torch.full_like(t["features"], float("nan"))
        gr = _lib.LatentOutGrads(p(t["g_skip"]) if m != "z" else None, p(t["g_z"]) if m != "skip" else None)
        torch.cuda.synchronize(hip_device)
        assert lib.lsr_latent_backward(C.byref(dims), C.byref(ins), C.byref(gr), p(d), None) == 0
        torch.cuda.synchronize(hip_device)
        got = _np(d)
        assert not np.isnan(got).any(), (m, int(np.isnan(got).sum()))
        tag = f"case {case} abi backward {run} ({m}):"
        ref.held(f"d_mean ({m})", got[:, :Cc], want["grad_" + m][:, :Cc], stock["grad_" + m][:, :Cc], "grad", tag)
        if variational:
            ref.held(f"d_logvar ({m})", got[:, Cc:], want["grad_" + m][:, Cc:], stock["grad_" + m][:, Cc:], "grad", tag)
            if not noise:
                assert (got[:, Cc:] == 0).all()
    _print_worst()


def test_abi_rejects_an_upscale(hip_device):
    """out_height > height (or width) is LSR_EINVAL, forward and backward; nothing is launched."""
    case = 2
    V, Cc, H, W, oh, ow = ref.CASES[case]
    lib, dims, ins, t, p = _abi(case, ref.make_inputs(case), hip_device)
    z = torch.zeros(V, Cc, H + 1, W + 1, device=hip_device)             # room for whatever size is asked for
    d = torch.zeros_like(t["features"])
    for bad_h, bad_w in ((H + 1, ow), (oh, W + 1), (0, ow)):
        dims.out_height, dims.out_width = bad_h, bad_w
        outs = _lib.LatentOutputs(None, p(z), None)
        assert lib.lsr_latent_forward(C.byref(dims), C.byref(ins), C.byref(outs), None) == -1       # LSR_EINVAL
        gr = _lib.LatentOutGrads(None, p(z))
        assert lib.lsr_latent_backward(C.byref(dims), C.byref(ins), C.byref(gr), p(d), None) == -1
    dims.out_height, dims.out_width = H, W                               # the identity resize is the limit: accepted
    assert lib.lsr_latent_forward(C.byref(dims), C.byref(ins), C.byref(_lib.LatentOutputs(None, p(z), None)), None) == 0
    torch.cuda.synchronize(hip_device)
    want = (t["features"] + torch.sqrt(torch.clamp(1 - t["mask"], min=float(np.exp(-30.0))))[:, None] * t["noise"]).cpu()
    assert torch.allclose(z.flatten()[:V * Cc * H * W].reshape(V, Cc, H, W).cpu(), want, rtol=2e-5, atol=2e-5)


# ---- repeatability ------------------------------------------------------------------------------------------------

def _all_bits(case, inp, dev):
    feats, out = _run(case, inp, dev)
    grads = _grads(feats, out, inp, dev)
    res = {k: _bits(v) for k, v in out.items()}
    res.update({"grad_" + m: g.view(np.uint32) for m, g in grads.items()})
    return res


@pytest.mark.parametrize("variational", [False, True], ids=["mask", "variational"])
def test_two_calls_and_a_side_stream_give_the_same_bits(hip_device, variational):
    inp = ref.make_inputs(1, variational)
    first, second = _all_bits(1, inp, hip_device), _all_bits(1, inp, hip_device)
    side = torch.cuda.Stream(hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        third = _all_bits(1, inp, hip_device)
    torch.cuda.current_stream(hip_device).wait_stream(side)
    for k in first:
        assert np.array_equal(first[k], second[k]), k
        assert np.array_equal(first[k], third[k]), (k, "side stream")
