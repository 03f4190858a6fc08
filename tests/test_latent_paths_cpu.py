"""The latent epilogue's float64 restatement and case table (tests/latent_ref.py), before any GPU is involved: the
restatement is the oracle's composition and reproduces the reference-generated fixtures; every case selects the kernel path
its comment names; the stock float32 composition alone is within the bars of tests/test_latent_paths_gpu.py on every
case's inputs (the inputs are fair); the clamp values planted into the variational cases are where they should be."""
import os

import numpy as np
import pytest
import torch

from oracle import latent_oracle as lo
from tests import latent_ref as ref
from tests.test_latent_cpu import GOLDEN, load_case

CASE_IDS = sorted(ref.CASES)
# (case, interval) of the variational runs: the default interval everywhere and, once, a narrow one
VARIATIONAL_RUNS = [(c, ref.DEFAULT_INTERVAL) for c in ref.VARIATIONAL_CASES] + [(2, ref.NARROW_INTERVAL)]


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[7:-4])
def test_restatement_matches_fixtures_and_oracle(path):
    z, b, v, inp = load_case(path)
    flat = lambda t: t.reshape(b * v, *t.shape[-3:])
    H, W = inp["features"].shape[-2:]
    f = inp["factor"]
    case = dict(features=flat(inp["features"]), mask=inp["mask"].reshape(b * v, H, W), noise=flat(inp["noise"]),
                color=flat(inp["color"]), g_z=flat(torch.tensor(z["g_z"])), g_skip=flat(torch.tensor(z["g_skip"])),
                size=(H // f, W // f), variational=inp["variational"], interval=ref.DEFAULT_INTERVAL)
    got = ref.compose(case, torch.float64)
    shaped = lambda k: z[k].reshape(-1, *z[k].shape[-3:])
    # the fixtures, at the tolerances tests/test_latent_cpu.py holds the oracle to
    np.testing.assert_allclose(np.broadcast_to(got["logvar"], shaped("logvar").shape), shaped("logvar"), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["sample"], shaped("sample"), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["skip"], shaped("skip"), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["z"], shaped("z"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["grad_both"], z["d_feature_all"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["grad_z"], z["d_feature_z"], rtol=1e-5, atol=1e-6)
    # the oracle on the same inputs, at the same tolerances
    inp["features"].requires_grad_()
    out = lo.latent_epilogue(**inp)
    ((out["z"] * torch.tensor(z["g_z"])).sum() + (out["skip"] * torch.tensor(z["g_skip"])).sum()).backward()
    o = lambda t: flat(t.detach()).numpy()
    np.testing.assert_allclose(np.broadcast_to(got["logvar"], o(out["logvar"]).shape), o(out["logvar"]), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["sample"], o(out["sample"]), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["skip"], o(out["skip"]), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["z"], o(out["z"]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["grad_both"], o(inp["features"].grad), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", CASE_IDS)
def test_stock_composition_is_the_oracle_with_an_explicit_size(case):
    """oracle.latent_epilogue(size=) and the stock float32 composition are the same operators: the same bits."""
    for variational in (False, True) if case in ref.VARIATIONAL_CASES else (False,):
        inp = ref.make_inputs(case, variational)
        stock = ref.compose(inp, torch.float32, modes=())
        out = lo.latent_epilogue(inp["features"], inp["mask"], inp["noise"], inp["color"], None, variational, size=inp["size"])
        for k in ("sample", "z", "skip"):
            assert np.array_equal(stock[k], out[k].to(torch.float64).numpy()), (case, variational, k)
        assert np.array_equal(np.broadcast_to(stock["logvar"], out["logvar"].shape), out["logvar"].to(torch.float64).numpy())
    x = ref.make_inputs(case)["features"]
    assert np.array_equal(lo.rescale(x, None, ref.CASES[case][4:]).to(torch.float64).numpy(), ref.resize_pair(case)[1]["z"])


def test_oracle_rescale_keeps_its_integer_factor():
    x = torch.randn(2, 3, 24, 40, generator=torch.Generator().manual_seed(3))
    assert lo.rescale(x, 4).shape == (2, 3, 6, 10)
    assert torch.equal(lo.rescale(x, 4), lo.rescale(x, None, (6, 10)))
    assert torch.equal(lo.rescale(x, 4), lo.rescale(x, 4, (6, 10)))


# case -> what it must select: float4 path, its row lanes, columns per thread on the scalar path, W % 4 == 0 (the colour
# copy's float4 branch), forward bands with and without z, backward bands, rows of the last backward band
SELECTS = {
    1: dict(float4=True, lanes=16, w4=True, fwd=36, fwd_noz=6, bwd=3, last=16),
    2: dict(float4=False, cols=1, w4=False, fwd=30, fwd_noz=6, bwd=3, last=13),
    3: dict(float4=True, lanes=1, w4=True, fwd=15, fwd_noz=5, bwd=3, last=8),
    4: dict(float4=True, lanes=256, w4=True, fwd=17, fwd_noz=3, bwd=2, last=1),
    5: dict(float4=False, cols=4, w4=False, fwd=11, fwd_noz=5, bwd=3, last=1),
    6: dict(float4=False, cols=4, w4=False, fwd=1, fwd_noz=2, bwd=1, last=16),
    7: dict(float4=True, lanes=256, w4=True, fwd=1, fwd_noz=128, bwd=64, last=16),
    8: dict(float4=False, cols=2, w4=True, fwd=10, fwd_noz=4, bwd=2, last=14),
    9: dict(float4=False, cols=1, w4=True, fwd=7, fwd_noz=1, bwd=1, last=7),
    10: dict(float4=False, cols=1, w4=True, fwd=33, fwd_noz=13, bwd=7, last=4),
    11: dict(float4=False, cols=2, w4=False, fwd=3, fwd_noz=2, bwd=1, last=9),
    12: dict(float4=False, cols=3, w4=True, fwd=3, fwd_noz=2, bwd=1, last=9),
}


@pytest.mark.parametrize("case", CASE_IDS)
def test_case_selects_the_path_it_names(case):
    V, C, H, W, oh, ow = ref.CASES[case]
    want = SELECTS[case]
    assert 1 <= oh <= H and 1 <= ow <= W <= ref.THREADS * ref.MAX_COLS
    assert ref.uses_float4_path(W) == want["float4"]
    if want["float4"]:
        assert ref.row_lanes(W) == want["lanes"]
    else:
        assert ref.columns_per_thread(W) == want["cols"]
    assert (W % 4 == 0) == want["w4"]
    assert ref.forward_bands(H, oh) == want["fwd"] and ref.forward_bands(H, oh, want_z=False) == want["fwd_noz"]
    assert ref.backward_bands(H) == want["bwd"] and H - (want["bwd"] - 1) * ref.BWD_ROWS == want["last"]


def test_the_table_covers_what_it_claims():
    C = ref.CASES
    assert set(C) == set(range(1, 13)) and set(ref.VARIATIONAL_CASES) == {1, 2, 5, 8} and set(ref.ABI_CASES) == {2, 4}
    # the float4 path's widths are exactly 4, 8, ..., 1024; its two ends are in the table
    assert [w for w in range(1, 1025) if ref.uses_float4_path(w)] == [4 << k for k in range(9)]
    assert {C[3][3], C[4][3]} == {1024, 4}
    # W % 4 == 0 off the float4 path: 12, 260, 768
    assert all(w % 4 == 0 and not ref.uses_float4_path(w) for w in (C[9][3], C[8][3], C[12][3]))
    # 2, 3 and 4 columns per thread, odd widths among them, up to the limit
    assert {ref.columns_per_thread(C[c][3]) for c in (11, 12, 5)} == {2, 3, 4} and C[5][3] % 2 == 1 and C[11][3] == ref.THREADS + 1
    # non-integer scales, per-axis scales, whole-image windows wider than a wave
    assert all(C[c][2] % C[c][4] and C[c][3] % C[c][5] for c in (1, 2, 3, 10))
    assert [ref.is_isotropic(c) for c in sorted(C)] == [True, True, True, False, True, False, False, False, False, True, False, True]
    assert C[6][4:] == (1, 1) and C[6][3] > 64 and C[7][4:] == (1, 1) and C[7][2] > 64
    # H not a multiple of the backward's band
    assert sum(C[c][2] % ref.BWD_ROWS != 0 for c in C) >= 8


def _stock_held(case, variational, interval, noise, tag):
    want, stock = ref.epilogue_pair(case, variational, interval, noise, True)
    for k in ("sample", "skip", "z", "logvar"):
        ref.held(k, stock[k], want[k], stock[k], "value", tag)
    for m in ref.GRAD_MODES:
        ref.held("grad_" + m, stock["grad_" + m], want["grad_" + m], stock["grad_" + m], "grad", tag)
    inp = ref.make_inputs(case, variational, interval)
    cc = 3
    assert np.array_equal(stock["skip"][:, :cc], inp["color"].numpy()) and np.array_equal(want["skip"][:, :cc], inp["color"].numpy())
    return want, stock


@pytest.mark.parametrize("case", CASE_IDS)
def test_stock_float32_is_within_the_bars(case):
    want, stock = ref.resize_pair(case)
    ref.held("resize z", stock["z"], want["z"], stock["z"], "resize", f"case {case} (a):")
    ref.held("resize grad", stock["grad"], want["grad"], stock["grad"], "resize", f"case {case} (a):")
    _stock_held(case, False, ref.DEFAULT_INTERVAL, True, f"case {case} (b):")
    # the resize of float32 ATen is within 1e-4 of its scale of float64 ATen: the yardstick is not degenerate
    assert np.abs(stock["z"] - want["z"]).max() <= 1e-4 * np.abs(want["z"]).max()


@pytest.mark.parametrize("case,interval", VARIATIONAL_RUNS)
def test_stock_float32_is_within_the_bars_variational(case, interval):
    _stock_held(case, True, interval, True, f"case {case} (c) {interval}:")
    want, stock = _stock_held(case, True, interval, False, f"case {case} (d) {interval}:")
    C = ref.CASES[case][1]
    inp = ref.make_inputs(case, True, interval)
    for r in (want, stock):
        assert np.array_equal(r["sample"], inp["features"][:, :C].numpy())
        assert all((r["grad_" + m][:, C:] == 0).all() for m in ref.GRAD_MODES)


@pytest.mark.parametrize("case,interval", VARIATIONAL_RUNS)
def test_planted_clamp_values(case, interval):
    C = ref.CASES[case][1]
    inp = ref.make_inputs(case, True, interval)
    lv = inp["features"][:, C:].numpy()
    assert lv.dtype == np.float32 and np.isfinite(lv).all()
    lo_, hi_ = np.float32(interval[0]), np.float32(interval[1])
    inf = np.float32(np.inf)
    for value in (lo_, hi_, np.nextafter(lo_, -inf), np.nextafter(lo_, inf), np.nextafter(hi_, -inf), np.nextafter(hi_, inf)):
        assert (lv == value).sum() >= 8, value
    assert float(lo_) == interval[0] and float(hi_) == interval[1]          # exactly -30.0 and 20.0 (-10.0 and 2.0)
    assert (lv < lo_).mean() >= 0.10 and (lv > hi_).mean() >= 0.10
    assert ((lv > lo_) & (lv < hi_)).mean() >= 0.20         # and a fair share strictly inside
    # the rule the kernel is held to: torch passes the gradient at both ends, inclusive, and nowhere outside
    want, _ = ref.epilogue_pair(case, True, interval, True, True)
    d_lv = want["grad_both"][:, C:]
    assert (d_lv[(lv < lo_) | (lv > hi_)] == 0).all()
    assert (d_lv[lv == lo_] != 0).all() and (d_lv[lv == hi_] != 0).all()
    # and no gradient vanishes in float32 at the lower end, where std = exp(lo / 2) is smallest
    assert (np.abs(d_lv[lv == lo_]) > 1e-30).all()
