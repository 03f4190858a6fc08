"""The 3DGS activation map on the MI355X: lsr_scene_activate_forward / _backward against the float64 restatement
(tests/scene_params_ref.py) and against the import's unpack kernel, the optional pieces, determinism, the gradients a
render sends down, the GaussianScene module and the fitting tool."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import ply_import_ref as ref
from tests import scene_params_ref as sref
from tests import util

pytestmark = pytest.mark.gpu

# the launch caps its grid at 2048 workgroups of 256 Gaussians: one n just past that, where workgroups take a second chunk
PAST_THE_GRID = 2048 * 256 + 3
SHAPES = [(1, 1), (63, 4), (64, 9), (65, 25), (255, 1), (256, 16), (257, 16), (1031, 4), (1031, 25)]
CASES = [(n, K, m) for n, K in SHAPES for m in (1.0, 0.5)] + [(PAST_THE_GRID, 1, 0.5)]
H = W = 64
G, VIEWS = 2000, 2


def _dev(p: dict, dev, keys=sref.PARAMS):
    return [torch.from_numpy(p[k]).to(dev) for k in keys]


def _np(d: dict) -> dict:
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("n,K,m", CASES)
def test_forward_and_backward_match_the_restatement(hip_device, n, K, m):
    from latentsplat_amd.ply_import import layout_from_names, unpack_table
    from latentsplat_amd.scene_model import activate_backward, activate_forward, activate_scene
    p = sref.make_params(n, K, seed=1000 * K + n)
    up = sref.make_upstream(n, K, seed=n + K)
    t = _dev(p, hip_device)
    got = _np(activate_forward(*t, scale_modifier=m))
    assert set(got) == {"shs", "opacities", "cov3D", "scales", "rotations"}
    ref.assert_matches(got, sref.expected(p, m))
    assert np.array_equal(got["shs"], np.concatenate([p["features_dc"], p["features_rest"]], 1))
    # the import's kernel, fed the same raw values as a row table: the same bar, scaled by m and m^2
    names = ref.standard_names(K)
    rows = torch.from_numpy(sref.expected_rows(p)).to(hip_device)
    unpacked = _np(unpack_table(rows, layout_from_names(names, n), want=("shs", "opacities", "scales", "rotations", "cov3D")))
    unpacked["scales"], unpacked["cov3D"] = unpacked["scales"] * np.float32(m), unpacked["cov3D"] * np.float32(m * m)
    ref.assert_matches(got, unpacked)
    # backward, as the kernel and through autograd
    g = [torch.from_numpy(up[k]).to(hip_device) for k in ("shs", "opacities", "cov3D")]
    back = _np(activate_backward(*t, *g, scale_modifier=m))
    sref.assert_backward_matches(back, p, up, m, show=f"n={n} K={K} m={m}")
    leaves = [x.clone().requires_grad_(True) for x in t]
    outs = activate_scene(*leaves, scale_modifier=m)
    torch.autograd.backward(outs, g)
    for k, leaf in zip(sref.PARAMS, leaves):
        assert np.array_equal(leaf.grad.cpu().numpy(), back[k]), k
    for k, o in zip(("shs", "opacities", "cov3D"), outs):
        assert np.array_equal(o.detach().cpu().numpy(), got[k]), k


def test_optional_pieces(hip_device):
    from latentsplat_amd.scene_model import activate_backward, activate_forward, activate_scene
    n, K, m = 300, 9, 0.5
    p = sref.make_params(n, K, seed=21)
    up = sref.make_upstream(n, K, seed=22)
    t = _dev(p, hip_device)
    g = {k: torch.from_numpy(v).to(hip_device) for k, v in up.items()}
    full = _np(activate_forward(*t, scale_modifier=m))
    for only in ("shs", "opacities", "cov3D", "scales", "rotations"):             # each output alone
        got = activate_forward(*t, scale_modifier=m, want=(only,))
        assert list(got) == [only] and np.array_equal(got[only].cpu().numpy(), full[only])
    with pytest.raises(_lib.LsrError, match="unknown outputs"):
        activate_forward(*t, want=("cov3d",))
    all_back = _np(activate_backward(*t, g["shs"], g["opacities"], g["cov3D"], scale_modifier=m))
    for only in sref.PARAMS:                                                     # each gradient alone, in the kernel
        got = activate_backward(*t, g["shs"], g["opacities"], g["cov3D"], scale_modifier=m, want=(only,))
        assert list(got) == [only] and np.array_equal(got[only].cpu().numpy(), all_back[only])
    # each upstream gradient alone: the parameters it does not reach get None
    reached = dict(shs=("features_dc", "features_rest"), opacities=("opacity",), cov3D=("scaling", "rotation"))
    for i, name in enumerate(("shs", "opacities", "cov3D")):
        leaves = [x.clone().requires_grad_(True) for x in t]
        outs = activate_scene(*leaves, scale_modifier=m)
        outs[i].backward(g[name])
        grads = {k: leaf.grad for k, leaf in zip(sref.PARAMS, leaves)}
        assert sorted(k for k, v in grads.items() if v is not None) == sorted(reached[name])
        sref.assert_backward_matches(_np({k: v for k, v in grads.items() if v is not None}), p, {name: up[name]}, m)
        for k in reached[name]:
            assert np.array_equal(grads[k].cpu().numpy(), all_back[k]), k
        # ... and in the kernel, a NULL upstream gradient is zero
        direct = _np(activate_backward(*t, *[g[k] if k == name else None for k in ("shs", "opacities", "cov3D")], scale_modifier=m))
        sref.assert_backward_matches(direct, p, {name: up[name]}, m)
        for k in sref.PARAMS:
            if k not in reached[name]:
                assert not direct[k].any(), k
    # a parameter that does not require grad gets none; the others are unchanged bit for bit
    for frozen in sref.PARAMS:
        leaves = [x.clone().requires_grad_(k != frozen) for k, x in zip(sref.PARAMS, t)]
        torch.autograd.backward(activate_scene(*leaves, scale_modifier=m), [g[k] for k in ("shs", "opacities", "cov3D")])
        for k, leaf in zip(sref.PARAMS, leaves):
            assert (leaf.grad is None) if k == frozen else np.array_equal(leaf.grad.cpu().numpy(), all_back[k]), (frozen, k)
    # an empty scene
    empty = [x[:0] for x in t]
    assert activate_forward(*empty)["shs"].shape == (0, K, 3)
    assert activate_backward(*empty, None, None, None)["rotation"].shape == (0, 4)
    # a quaternion of norm 0 is NaN for that Gaussian and for no other
    bad = [x.clone() for x in t]
    bad[4][7] = 0.0
    out = _np(activate_forward(*bad, scale_modifier=m))
    assert np.isnan(out["cov3D"][7]).all() and np.isnan(out["rotations"][7]).all()
    keep = np.arange(n) != 7
    assert np.array_equal(out["cov3D"][keep], full["cov3D"][keep]) and np.array_equal(out["shs"], full["shs"])


def test_two_calls_give_identical_bits(hip_device):
    from latentsplat_amd.scene_model import activate_backward, activate_forward
    n, K = 5000, 16
    p = sref.make_params(n, K, seed=31)
    up = sref.make_upstream(n, K, seed=32)
    t = _dev(p, hip_device)
    g = [torch.from_numpy(up[k]).to(hip_device) for k in ("shs", "opacities", "cov3D")]
    a, b = (_np(activate_forward(*t)) for _ in range(2))
    c, d = (_np(activate_backward(*t, *g)) for _ in range(2))
    for x, y in ((a, b), (c, d)):
        for k in x:
            assert np.array_equal(x[k], y[k]), k


# ---- the module, a render's gradients, the tool ----

@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("scene_model") / "point_cloud.ply"
    sc, table, names = sref.write_scene_file(path, G, W, VIEWS)
    return path, sc, table, names


def _views(sc, dev, requires_grad=False):
    from latentsplat_amd.rasterizer import build_view_table
    views = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                             torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False)
    return views.detach().requires_grad_(requires_grad)


def test_module_load_activate_save(hip_device, scene_file, tmp_path):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.ply_import import load_ply, read_header
    path, sc, table, names = scene_file
    scene = GaussianScene.from_ply(path, hip_device)
    p = sref.split_table(table, names)
    for k, v in p.items():                                   # the parameters are the file's columns, bit for bit
        assert np.array_equal(getattr(scene, "_" + k).detach().cpu().numpy(), v), k
    assert scene.max_sh_degree == 1 and scene.active_sh_degree == 1 and scene._xyz.device == hip_device
    act, loaded = scene.activated(), load_ply(path, hip_device)
    assert act.means is scene._xyz and act.sh_degree == 1
    f = lambda s: dict(means=s.means, shs=s.shs, opacities=s.opacities, scales=s.scales, rotations=s.rotations, cov3D=s.covariances)
    ref.assert_matches(_np({k: v.detach() for k, v in f(act).items()}), _np(f(loaded)))
    assert act.covariances.requires_grad and not act.scales.requires_grad and not act.rotations.requires_grad
    scene.save_ply(tmp_path / "saved.ply")
    layout = read_header(tmp_path / "saved.ply")
    saved = np.fromfile(tmp_path / "saved.ply", "<f4", offset=layout.data_offset).reshape(G, -1)
    assert np.array_equal(saved, table)
    # state dicts carry over under the published names
    other = GaussianScene.from_tensors(**{k: torch.zeros_like(torch.from_numpy(v)) for k, v in p.items()}).to(hip_device)
    other.load_state_dict(scene.state_dict())
    assert np.array_equal(other.rows().cpu().numpy(), table)


def test_render_gradients_are_the_kernels_backward_of_what_the_rasterizer_sends_down(hip_device, scene_file, monkeypatch):
    """One GaussianScene.render and one backward.  The three activated tensors that render feeds to rasterize_views are
    kept (retain_grad), so the gradients the rasterizer sends down in THIS pass are known; the module's parameter
    gradients must be the restatement's backward of exactly those, at the bars of the backward, and the kernel's own
    backward of them bit for bit.  This isolates the new kernel from the rasterizer's atomic sums."""
    import latentsplat_amd.rasterizer as rasterizer
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.scene_model import activate_backward
    path, sc, table, names = scene_file
    dev = hip_device
    scene = GaussianScene.from_ply(path, dev)
    views = _views(sc, dev)
    cot = torch.randn((VIEWS, 3, H, W), generator=torch.Generator().manual_seed(9)).to(dev)
    fed = {}
    real = rasterizer.rasterize_views

    def recording(views_, h, w, degree, means3D, cov3D, opacities, shs=None, **kw):
        for t in (cov3D, opacities, shs):
            t.retain_grad()
        fed.update(degree=degree, means=means3D, cov3D=cov3D, opacities=opacities, shs=shs)
        return real(views_, h, w, degree, means3D, cov3D, opacities, shs=shs, **kw)

    monkeypatch.setattr(rasterizer, "rasterize_views", recording)
    color = scene.render(views, H, W)[0]
    (color * cot).sum().backward()
    assert fed["degree"] == 1 and fed["shs"].shape == (G, 4, 3)
    assert fed["means"] is scene._xyz                           # the means gradient is the rasterizer's own, bit for bit
    assert torch.isfinite(scene._xyz.grad).all() and scene._xyz.grad.abs().max() > 0
    up = {k: fed[k].grad for k in ("shs", "opacities", "cov3D")}
    assert all(v is not None and v.abs().max() > 0 for v in up.values())
    got = {k: getattr(scene, "_" + k).grad.cpu().numpy() for k in sref.PARAMS}
    sref.assert_backward_matches(got, sref.split_table(table, names), _np(up), 1.0, show="render gradients")
    params = [scene._features_dc, scene._features_rest, scene._opacity, scene._scaling, scene._rotation]
    kernel = _np(activate_backward(*params, up["shs"], up["opacities"], up["cov3D"]))
    for k in sref.PARAMS:
        assert np.array_equal(got[k], kernel[k]), k


def test_active_sh_degree(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    renders = {}
    for name, rest_scale in (("with_bands", 1.0), ("dc_only", 0.0)):
        sc, _, _ = sref.write_scene_file(tmp_path / f"{name}.ply", G, W, VIEWS, rest_scale=rest_scale)
        scene = GaussianScene.from_ply(tmp_path / f"{name}.ply", hip_device)
        scene.active_sh_degree = 0
        views = _views(sc, hip_device)
        with torch.no_grad():
            low = scene.render(views, H, W)[0].cpu().numpy()
            scene.oneup_sh_degree()
            assert scene.active_sh_degree == 1
            high = scene.render(views, H, W)[0].cpu().numpy()
            scene.oneup_sh_degree()
            assert scene.active_sh_degree == 1                   # no further than the stored bands
        renders[name] = (low, high)
    assert np.abs(renders["with_bands"][0] - renders["with_bands"][1]).max() > 1e-3     # one more band is rendered
    assert np.array_equal(renders["dc_only"][0], renders["dc_only"][1])                 # zero bands add nothing
    assert np.array_equal(renders["dc_only"][0], renders["with_bands"][0])              # degree 0 never reads them


def test_pose_refinement_composes(hip_device, scene_file):
    from latentsplat_amd import GaussianScene
    path, sc, _, _ = scene_file
    scene = GaussianScene.from_ply(path, hip_device)
    views = _views(sc, hip_device, requires_grad=True)
    scene.render(views, H, W, scale_modifier=0.5)[0].square().sum().backward()
    assert views.grad is not None and torch.isfinite(views.grad).all() and views.grad.abs().max() > 0
    assert all(torch.isfinite(q.grad).all() and q.grad.abs().max() > 0 for q in scene.parameters())


def test_fit_tool(hip_device, scene_file, tmp_path):
    from latentsplat_amd.ply_import import load_ply
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import fit_ply
    finally:
        sys.path.pop(0)
    path = scene_file[0]
    out = tmp_path / "fit"
    res = fit_ply.main([str(path), "--out", str(out), "--views", "3", "--size", "48", "--steps", "20"])
    print("fit:", res)
    assert np.isfinite(res["loss_first"]) and np.isfinite(res["loss_last"]) and res["loss_last"] < res["loss_first"]
    assert res["steps"] == 20 and res["gaussians"] == G and res["sh_degree"] == 1
    assert json.load(open(out / "fit.json")) == res
    fitted = load_ply(out / "point_cloud.ply", hip_device)
    assert fitted.means.shape == (G, 3) and fitted.sh_degree == 1
    for t in (fitted.means, fitted.covariances, fitted.opacities, fitted.shs, fitted.scales, fitted.rotations):
        assert torch.isfinite(t).all()
