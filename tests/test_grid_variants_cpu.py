"""The grid-size / work-queue cases of tests/grid_variants.py without a GPU: which variant each case reaches (the restated
launch predicates against the hand-written table), and the conditions under which the GPU test's bars mean something,
checked on the oracle alone."""
import numpy as np
import pytest
import torch

from tests import grid_variants as gv
from tests import util

ALL = list(gv.CASES) + list(gv.SHARED_CASES)


@pytest.mark.parametrize("name", list(gv.CASES))
def test_per_view_cases_reach_what_the_table_says(name):
    for record in (False, True):
        for depth_grad in (False, True):
            got = gv.variants_of(name, 256, depth_grad=depth_grad, record=record)
            assert got == gv.expected(name, record=record), (name, record, depth_grad)


@pytest.mark.parametrize("name,fuse", list(gv.EXPECT_SHARED))
def test_shared_cases_reach_what_the_table_says(name, fuse):
    assert gv.variants_of(name, 256, fuse=fuse) == gv.expected(name, fuse=fuse)


def test_the_table_covers_every_switch_both_ways():
    """Every column of the table takes each of its values in some case: dropping a case shows here what is lost."""
    rows = [gv.expected(k) for k in gv.CASES] + [gv.expected(k, fuse=f) for k, f in gv.EXPECT_SHARED]
    seen = {col: {r[col] for r in rows} for col in rows[0]}
    for col in ("narrow", "segments", "pre_lds", "fold", "scatter_lds", "fwd_queue", "bin_queue", "reorder", "bwd_queue"):
        assert seen[col] == {True, False}, col
    assert seen["scan_in_regs"] == {None, True, False}
    assert seen["vb"] == {None, 1, 2, 4}
    assert {"rows", "half"} <= seen["fwd_kernel"]
    # the unsplit static branch and the queue branch of k_render_bwd for the payload widths no other test compares
    assert gv.expected("static36")["bwd_parts_log2"] == 0 and not gv.expected("static36")["bwd_queue"]
    assert {gv.padded_channels(gv.CASES[k]["nch"]) for k in gv.CASES if gv.expected(k)["bwd_queue"]} == {4, 8, 12, 36}
    # wide records with no LDS histogram / no LDS reservation, and with both
    assert any(not r["narrow"] and not r["scatter_lds"] and not r["pre_lds"] for r in rows)
    assert any(not r["narrow"] and r["scatter_lds"] and r["pre_lds"] for r in rows)
    # the work queue of the <8, depth gradient> instance between its 3072 slots and the 4096 of the plain one
    assert 3072 < 2 * gv.CASES["queue8"]["V"] * 33 * 33 and gv.variants_of("queue8", 256, depth_grad=True)["bwd_queue"]


def test_switches_flip_where_the_sources_say():
    """The restated predicates on both sides of each threshold (256 compute units)."""
    v = lambda H, W, V, nch, **kw: gv.variants(H, W, V, nch, kw.pop("dg", False), kw.pop("record", True), kw.pop("shared", False),
                                               kw.pop("fused", False), 256, **kw)
    assert v(16, 4080, 1, 4)["narrow"] and not v(16, 4081, 1, 4)["narrow"]
    assert v(512, 512, 1, 4)["segments"] and not v(512, 528, 1, 4)["segments"]            # T 1024 / 1056
    assert v(1024, 1024, 1, 4)["pre_lds"] and not v(1024, 1040, 1, 4)["pre_lds"]          # T 4096 / 4160
    assert v(512, 512, 4, 4)["fold"] and not v(512, 528, 4, 4)["fold"]                    # N 4096 / 4224
    assert v(512, 512, 8, 4)["scan_in_regs"] and not v(512, 528, 8, 4)["scan_in_regs"]    # N 8192 / 8448
    assert v(1024, 2048, 1, 4)["scatter_lds"] and not v(1024, 2064, 1, 4)["scatter_lds"]  # T 8192 / 8256
    assert v(256, 384, 1, 4)["fwd_kernel"] == "quad" and v(256, 400, 1, 4)["fwd_kernel"] == "rows"   # items 768 / 800
    assert v(512, 768, 1, 8)["fwd_kernel"] == "rows" and v(512, 784, 1, 8)["fwd_kernel"] == "half"   # items 3072 / 3136
    for nch, at in ((4, 6144), (8, 4096), (12, 3072), (36, 2048)):       # 2 x 16 x 16 tiles per view = 512 items
        assert not v(256, 256, at // 512, nch)["fwd_queue"] and v(256, 272, at // 512, nch)["fwd_queue"], nch
    assert v(256, 272, 12, 4)["bin_queue"] and not v(256, 272, 12, 4, pairs=3000 * 12 * 272 + 1)["bin_queue"]
    assert not v(256, 256, 8, 4)["reorder"] and v(256, 272, 8, 4)["reorder"]              # items 4096 / 4352
    assert v(256, 256, 32, 4)["reorder"] and not v(256, 272, 32, 4)["reorder"]            # items 16384 / 17408
    assert not v(256, 272, 8, 4, record=False)["reorder"] and not v(256, 272, 8, 12)["reorder"]
    for nch, dg, slots in ((4, False, 4096), (8, False, 4096), (8, True, 3072), (12, False, 2048), (36, True, 1024)):
        a, b = v(256, 256, slots // 512, nch, dg=dg), v(256, 272, slots // 512, nch, dg=dg)
        assert (a["bwd_parts_log2"], a["bwd_queue"]) == (0, False) and b["bwd_queue"], (nch, dg)
        assert v(256, 256, 1, nch, dg=dg)["bwd_parts_log2"] == {4096: 3, 3072: 2, 2048: 2, 1024: 1}[slots]
    assert v(64, 64, 3, 7, shared=True)["vb"] == 2 and v(64, 64, 5, 7, shared=True)["vb"] == 4 and v(64, 64, 4, 7)["vb"] == 1
    f = lambda V, **kw: gv.variants(528, 528, V, 7, False, True, True, True, 256, **kw)
    assert f(7)["pre_lds"] and not f(8)["pre_lds"]                                        # Vg T 7623 / 8712
    assert not f(7, coef_words=12288)["pre_lds"]                                          # (12288 + 7623) x 4 > 64 KB


def _oracle_views(name):
    """The oracle's forward of every view of a case, as the GPU test compares it."""
    sc, H, W = gv.make_case_scene(name)
    if name in gv.CASES:
        bi = util.boundary_inputs(sc, H, W, bg=(0.3, 0.1, 0.5))
        return [util.oracle_forward(bi, v) for v in range(bi["V"])], H, W, sc.means.shape[0]
    # the shared scenes go through the scene-level inputs (test_parity_gpu._fused_scene_check: per-view scene scales)
    from latentsplat_amd.decoder import cuda_splatting as cs
    from latentsplat_amd.rasterizer import make_view_table
    V = sc.extrinsics.shape[0]
    cams, scale = cs._scaled_cameras(sc.extrinsics, sc.intrinsics, sc.near * torch.linspace(1.0, 1.3, V), sc.far, True)
    views = make_view_table(cams.view_matrix, cams.full_projection, cams.campos, cams.tan_fov_x, cams.tan_fov_y,
                            torch.tensor([[0.2, 0.1, 0.4]]).expand(V, 3), scale)
    n = lambda t: None if t is None else t.detach().contiguous().numpy()
    outs = []
    for v in range(V):
        m, c6, op, sh, cp, ft = util.to_boundary(views, v, sc.means, sc.covariances, sc.opacities[:, None], sc.color_sh, None, None,
                                                 sc.feature_sh, True)
        vw = views[v]
        view = util.orc.View(H, W, float(vw[35]), float(vw[36]), vw[37:40].numpy(), vw[0:16].numpy().reshape(4, 4),
                             vw[16:32].numpy().reshape(4, 4), vw[32:35].numpy(), 3)
        outs.append(util.orc.forward(view, n(m), n(c6), n(op), n(sh), None, n(ft)))
    return outs, H, W, sc.means.shape[0]


@pytest.mark.parametrize("name", ALL)
def test_case_guards_hold_on_the_oracle(name):
    """What the GPU test's assertions presuppose (util.assert_close_except_fragile / assert_grad_close_except_fragile
    budgets: max_fragile_frac 0.02, max_direct_frac 0.01), on the oracle alone, and that the strips really hold tile
    coordinates a byte cannot."""
    outs, H, W, G = _oracle_views(name)
    direct = []
    for v, o in enumerate(outs):
        assert o["P"] > 0, f"{name}: view {v} has no pairs"
        fragile_px = len(np.unique(o["fragile"][:, 0])) if len(o["fragile"]) else 0
        assert fragile_px <= 0.02 * H * W, f"{name}: view {v}: {fragile_px} fragile pixels of {H * W}"
        direct.append(util.fragile_gaussians(o, W)[0])
    union = np.unique(np.concatenate(direct))
    assert len(union) <= 0.01 * G, f"{name}: {len(union)} of {G} Gaussians are fragile in some view"
    for v, o in enumerate(outs):
        assert not o["fragile_overflow"], f"{name}: view {v}: fragile list overflow"
    if name in ("wide_x", "tall_y"):
        axis = 0 if name == "wide_x" else 1
        for v, o in enumerate(outs):
            rect = o["rect"][o["radii"] > 0]
            assert rect[:, 2 + axis].max() >= 256, f"{name}: view {v}: no rectangle coordinate beyond a byte on the long axis"
            assert rect[:, 3 - axis].max() <= 3
