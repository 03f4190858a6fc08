"""Scene export on the MI355X: lsr_ply_pack_scene against the float64 restatement (tests/scene_export_ref.py), degenerate
covariances, the file round trip through load_ply, a saved "reference"-convention scene through the rasterizer, the
export at size, and tools/convert_ply.py.

Worst reconstruction error | R S^2 R^T - Sigma | / max |Sigma| measured on one MI355X (the bar is 1e-5): see DESIGN.md
section 2.9."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import ply_import_ref as iref
from tests import scene_export_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

FLOOR = np.float32(0.5) * np.log(np.float32(1e-37))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pack(inp, dev, *, cov_elems=9, channel_major=False, **kw):
    from latentsplat_amd.ply_export import pack_scene
    shs = inp["shs"].transpose(0, 2, 1) if channel_major else inp["shs"]
    cov = inp["cov"] if cov_elems == 9 else ref.pack6(inp["cov"])
    return pack_scene(_t(inp["means"], dev), _t(inp["opacities"], dev), _t(shs, dev), covariances=_t(cov, dev),
                      channel_major=channel_major, **kw).cpu().numpy()


@pytest.mark.parametrize("K", [1, 4, 9, 16, 25])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
def test_pack_matches_the_restatement(hip_device, n, K):
    inp = ref.make_inputs(n, K, seed=100 * K + n)
    worst, first = 0.0, None
    for convention in ("3dgs", "reference"):
        for channel_major in (False, True):
            for cov_elems in (6, 9):
                rows = _pack(inp, hip_device, cov_elems=cov_elems, channel_major=channel_major, convention=convention)
                what = f"n={n} K={K} {convention} channel_major={channel_major} cov{cov_elems}"
                worst = max(worst, ref.assert_rows(rows, inp, K, convention, what))
                if convention == "3dgs":                    # neither layout nor the covariance's packing changes a bit
                    first = rows if first is None else first
                    assert np.array_equal(rows.view(np.uint32), first.view(np.uint32)), what
    print(f"n={n} K={K}: worst reconstruction error {worst:.3e} of the largest covariance entry")
    if K > 1:                                               # K_out < K_in: the lower bands, unchanged
        K_out = {4: 1, 9: 4, 16: 4, 25: 16}[K]
        deg = {1: 0, 4: 1, 16: 3}[K_out]
        for convention in ("3dgs", "reference"):
            rows = _pack(inp, hip_device, channel_major=True, convention=convention, max_sh_degree=deg)
            ref.assert_rows(rows, inp, K_out, convention, f"n={n} K={K}->{K_out} {convention}")


def _degenerate_batch():
    rng = np.random.default_rng(21)
    m = 64
    q = rng.standard_normal((m, 4))
    a, b = rng.uniform(0.01, 1.0, (m, 1)), rng.uniform(0.01, 1.0, (m, 1))
    zero = np.zeros((m, 1))
    build = lambda s, qq=q: ref.covariances_from(qq, np.concatenate(s, 1))
    ident = np.tile([1.0, 0, 0, 0], (m, 1))
    parts = dict(isotropic=build([a, a, a]), two_equal_large=build([a, a, b]), two_equal_small=build([a, b, b]),
                 diagonal=build([a, b, 0.5 * (a + b)], ident), rank_1=build([a, zero, zero]), rank_2=build([a, b, zero]),
                 zero=np.zeros((m, 3, 3)), ratio_1e4=build([a, 1e-4 * a, 1e-4 * a]), ratio_1e4_one=build([a, b, 1e-4 * a]))
    scene = ref.make_inputs(200, 1, seed=22)["cov"].astype(np.float64)
    parts["scene_1e-6"] = scene * 1e-12
    parts["scene_1e3"] = scene * 1e6
    assert not np.abs(parts["diagonal"][:, [0, 0, 1], [1, 2, 2]]).any()          # exactly diagonal
    names = [k for k, v in parts.items() for _ in range(len(v))]
    return names, np.concatenate(list(parts.values())).astype(np.float32)


def test_degenerate_and_extreme_covariances(hip_device):
    names, cov = _degenerate_batch()
    n = len(names)
    inp = ref.make_inputs(n, 1, seed=23)
    inp["cov"] = cov
    for cov_elems in (6, 9):
        rows = _pack(inp, hip_device, cov_elems=cov_elems, convention="3dgs")
        assert np.isfinite(rows).all()
        worst = ref.assert_rows(rows, inp, 1, "3dgs", f"degenerate batch cov{cov_elems}")
        rel = ref.reconstruction_error(rows, 1, cov)
        for kind in dict.fromkeys(names):
            sel = np.array([k == kind for k in names])
            print(f"{kind}: worst reconstruction error {rel[sel].max():.3e}")
        col = ref.columns(1)
        zero = np.array([k == "zero" for k in names])
        assert np.allclose(rows[zero][:, col["scale"]], FLOOR, rtol=1e-6)            # scales = the floor
        flat = np.array([k in ("rank_1", "rank_2") for k in names])
        lam = np.exp(2.0 * rows[flat][:, col["scale"]].astype(np.float64))
        big = np.abs(cov[flat].astype(np.float64)).reshape(-1, 9).max(1)
        assert (lam[:, 2] < 1e-5 * big).all()                                        # the clamped eigenvalue is below the bar
        assert worst <= 1e-5


def _f(t):
    return t.cpu().numpy()


def test_file_round_trip(hip_device, tmp_path):
    from latentsplat_amd.decoder.types import Gaussians
    from latentsplat_amd.ply_export import pack_scene, save_gaussians, save_ply
    from latentsplat_amd.ply_import import load_ply, read_header
    dev = hip_device
    n, K = 1000, 16
    inp = ref.make_inputs(n, K, seed=31)
    means, opac, shs, cov = (_t(inp[k], dev) for k in ("means", "opacities", "shs", "cov"))
    save_ply(tmp_path / "sub" / "a.ply", means, opac, shs, covariances=cov, convention="3dgs")
    s = load_ply(tmp_path / "sub" / "a.ply", dev)
    assert s.sh_degree == 3
    assert np.array_equal(_f(s.means), inp["means"]) and np.array_equal(_f(s.shs), inp["shs"])
    assert np.abs(_f(s.opacities)[:, 0].astype(np.float64) - inp["opacities"]).max() <= 1e-6
    big = np.abs(inp["cov"].astype(np.float64)).reshape(n, 9).max(1, keepdims=True)
    err = np.abs(_f(s.covariances).astype(np.float64) - ref.pack6(inp["cov"].astype(np.float64))) / big
    print(f"round trip: covariances off by {err.max():.3e} of the largest entry")
    assert err.max() <= 1e-5
    # two calls, the same bits
    a = pack_scene(means, opac, shs, covariances=cov, convention="reference")
    b = pack_scene(means, opac, shs, covariances=cov, convention="reference")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # convention=None: the one the process renders with (the default, "3dgs": a pure re-layout)
    d = pack_scene(means, opac, shs, covariances=cov)
    assert np.array_equal(ref.stored_shs(_f(d), K), inp["shs"]) and not torch.equal(d, a)
    # truncation keeps the originals
    save_ply(tmp_path / "deg1.ply", means, opac, shs, covariances=cov, convention="3dgs", max_sh_degree=1)
    s1 = load_ply(tmp_path / "deg1.ply", dev)
    assert s1.sh_degree == 1 and np.array_equal(_f(s1.shs), inp["shs"][:, :4, :])
    assert os.path.getsize(tmp_path / "deg1.ply") == read_header(tmp_path / "deg1.ply").data_offset + n * 26 * 4
    # the decoder's container: scene 1 of a batch of two
    other = ref.make_inputs(n, K, seed=32)
    g = Gaussians(means=torch.stack([_t(other["means"], dev), means]), covariances=torch.stack([_t(other["cov"], dev), cov]),
                  opacities=torch.stack([_t(other["opacities"], dev), opac]),
                  color_harmonics=torch.stack([_t(other["shs"], dev), shs]).transpose(2, 3).contiguous())
    save_gaussians(tmp_path / "g.ply", g, scene=1, convention="3dgs")
    assert (tmp_path / "g.ply").read_bytes() == (tmp_path / "sub" / "a.ply").read_bytes()
    # an empty scene: a header-only file
    e = torch.empty
    save_ply(tmp_path / "empty.ply", e((0, 3), device=dev), e((0,), device=dev), e((0, 4, 3), device=dev),
             covariances=e((0, 3, 3), device=dev), convention="3dgs")
    layout = read_header(tmp_path / "empty.ply")
    assert (layout.n, layout.sh_coeffs, layout.stride) == (0, 4, 26)
    assert os.path.getsize(tmp_path / "empty.ply") == layout.data_offset
    assert load_ply(tmp_path / "empty.ply", dev).means.shape == (0, 3)


def test_scales_rotations_round_trip(hip_device, tmp_path):
    from latentsplat_amd.ply_export import save_ply
    from latentsplat_amd.ply_import import load_ply
    names = iref.standard_names(4)
    table = iref.make_table(777, names, seed=41)
    iref.write_ply(tmp_path / "in.ply", names, table)
    s1 = load_ply(tmp_path / "in.ply", hip_device)
    save_ply(tmp_path / "out.ply", s1.means, s1.opacities, s1.shs, scales=s1.scales, rotations=s1.rotations, convention="3dgs")
    s2 = load_ply(tmp_path / "out.ply", hip_device)
    assert np.array_equal(_f(s2.means), _f(s1.means)) and np.array_equal(_f(s2.shs), _f(s1.shs)) and s2.sh_degree == 1
    np.testing.assert_allclose(_f(s2.scales), _f(s1.scales), rtol=2e-5, atol=0)
    q1 = _f(s1.rotations)
    q1 = q1 * np.where(q1[:, :1] < 0, -1.0, 1.0).astype(np.float32)                   # saved with w >= 0
    assert (_f(s1.rotations)[:, 0] < 0).any()
    np.testing.assert_allclose(_f(s2.rotations), q1, rtol=0, atol=2e-5)
    p = _f(s1.opacities).astype(np.float64)
    inside = (p >= 1e-4) & (p <= 1 - 1e-4)
    assert np.abs(_f(s2.opacities).astype(np.float64) - p)[inside].max() <= 1e-6


# ---- a saved scene through the rasterizer ----

H = W = 64
G, VIEWS = 2000, 2


@pytest.mark.parametrize("degree", [2, 4])
def test_reference_convention_scene_renders_the_same_after_saving(hip_device, tmp_path, degree):
    """The point of the feature: coefficients meant under "reference", saved, render the same under "3dgs"."""
    from latentsplat_amd.ply_export import save_ply
    from latentsplat_amd.ply_import import load_ply
    from latentsplat_amd.rasterizer import build_view_table, get_color_sh_convention, rasterize_views, set_color_sh_convention
    dev = hip_device
    sc = util.make_scene(G, image_size=W, views=VIEWS, color_sh_degree=degree, feature_channels=None)
    K = (degree + 1) ** 2
    shs = sc.color_sh.transpose(1, 2).contiguous().to(dev)                       # (G, K, 3)
    save_ply(tmp_path / "ref.ply", sc.means.to(dev), sc.opacities.to(dev), sc.color_sh.to(dev), covariances=sc.covariances.to(dev),
             convention="reference", channel_major=True)
    s = load_ply(tmp_path / "ref.ply", dev)
    assert s.sh_degree == degree and s.shs.shape == (G, K, 3)
    views = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                             torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False)
    before = get_color_sh_convention()
    try:
        with torch.no_grad():
            set_color_sh_convention("3dgs")
            a = rasterize_views(views, H, W, degree, s.means, s.covariances, s.opacities, shs=s.shs)
            set_color_sh_convention("reference")
            b = rasterize_views(views, H, W, degree, s.means, s.covariances, s.opacities, shs=shs)
    finally:
        set_color_sh_convention(before)
    assert (_f(a[4]) > 0).sum() > G // 2 and _f(a[2]).max() > 0.5                # a non-trivial render
    assert np.array_equal(_f(a[4]), _f(b[4]))
    diff = np.abs(_f(a[0]).astype(np.float64) - _f(b[0]))
    print(f"degree {degree}: colour differs by at most {diff.max():.3e}")
    assert diff.max() <= 1e-4
    assert np.array_equal(_f(a[2]).view(np.uint32), _f(b[2]).view(np.uint32))        # mask
    assert np.array_equal(_f(a[3]).view(np.uint32), _f(b[3]).view(np.uint32))        # depth
    # ... and it is the basis change that does it: the untouched coefficients under "3dgs" are another picture
    with torch.no_grad():
        c = rasterize_views(views, H, W, degree, s.means, s.covariances, s.opacities, shs=shs)
    print(f"degree {degree}: without the basis change the colour is off by {np.abs(_f(c[0]) - _f(b[0])).max():.3e}")
    assert np.abs(_f(c[0]) - _f(b[0])).max() > 1e-3          # ten times the bar above


def test_pack_at_size(hip_device, tmp_path):
    from latentsplat_amd.ply_export import save_ply
    from latentsplat_amd.ply_import import read_header
    n, K = 393_216, 25
    inp = ref.make_inputs(n, K, seed=51)
    rows = _pack(inp, hip_device, cov_elems=9, channel_major=True, convention="reference")
    worst = ref.assert_rows(rows, inp, K, "reference", "at size")
    print(f"n={n}: worst reconstruction error {worst:.3e} of the largest covariance entry")
    dev = hip_device
    save_ply(tmp_path / "big.ply", _t(inp["means"], dev), _t(inp["opacities"], dev), _t(inp["shs"], dev),
             covariances=_t(inp["cov"], dev), convention="reference")
    layout = read_header(tmp_path / "big.ply")
    assert (layout.n, layout.stride) == (n, 89)
    assert os.path.getsize(tmp_path / "big.ply") == layout.data_offset + n * 89 * 4
    with open(tmp_path / "big.ply", "rb") as f:
        f.seek(layout.data_offset)
        assert f.read() == rows.tobytes()


def test_convert_tool(hip_device, tmp_path):
    from latentsplat_amd.ply_export import save_ply
    from latentsplat_amd.ply_import import load_ply
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import convert_ply
    finally:
        sys.path.pop(0)
    names = iref.standard_names(25)
    table = iref.make_table(500, names, seed=61)
    iref.write_ply(tmp_path / "deg4.ply", names, table)
    status = convert_ply.main([str(tmp_path / "deg4.ply"), str(tmp_path / "deg3.ply"), "--max-degree", "3"])
    assert status["sh_degree_in"] == 4 and status["sh_degree_out"] == 3 and status["gaussians"] == 500
    s = load_ply(tmp_path / "deg4.ply", hip_device)
    out = load_ply(tmp_path / "deg3.ply", hip_device)
    assert out.sh_degree == 3 and np.array_equal(_f(out.shs), _f(s.shs)[:, :16, :]) and np.array_equal(_f(out.means), _f(s.means))
    save_ply(tmp_path / "same.ply", s.means, s.opacities, s.shs, scales=s.scales, rotations=s.rotations, convention="3dgs",
             max_sh_degree=3)
    assert (tmp_path / "deg3.ply").read_bytes() == (tmp_path / "same.ply").read_bytes()
    # re-basing: the same as save_ply with convention="reference"
    convert_ply.main([str(tmp_path / "deg4.ply"), str(tmp_path / "rebased.ply"), "--from-convention", "reference"])
    save_ply(tmp_path / "same2.ply", s.means, s.opacities, s.shs, scales=s.scales, rotations=s.rotations, convention="reference")
    assert (tmp_path / "rebased.ply").read_bytes() == (tmp_path / "same2.ply").read_bytes()
    assert load_ply(tmp_path / "rebased.ply", hip_device).sh_degree == 4
