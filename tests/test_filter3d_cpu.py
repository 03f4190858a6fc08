"""The 3D smoothing filter without a GPU: the exports, the argument checks of the C ABI (returned before any GPU work, with
NULL device pointers), the refusals of the Python layer, and the float64 restatement (tests/filter3d_ref.py) against a
hand-computed case, finite differences and its own fused parameters."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import SceneDims, SceneInGrads, SceneOutGrads, SceneOutputs, SceneParams
from tests import filter3d_ref as fref
from tests import scene_params_ref as sref

NEW = ("lsr_filter3d_workspace_bytes", "lsr_filter3d_compute", "lsr_scene_activate_filtered_forward",
       "lsr_scene_activate_filtered_backward")
EINVAL, ENULL = -1, -2


def test_exports():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    import latentsplat_amd
    for name in ("compute_filter_3d", "activate_scene_filtered", "fused_parameters"):
        assert latentsplat_amd._LAZY[name] == "filter3d" and callable(getattr(latentsplat_amd, name))
    assert lib.lsr_abi_version() == 10


def _compute(n=5, V=2, width=64, margin=0.15, variance=0.2, mode=0, xyz=None, views=None, filt=None, ws=None):
    return _lib.load().lsr_filter3d_compute(n, xyz, V, views, width, margin, variance, mode, filt, None, ws, None)


@pytest.mark.parametrize("bad", [
    dict(n=-1), dict(n=1 << 28), dict(V=0), dict(V=-3), dict(V=_lib.FILTER3D_MAX_VIEWS + 1), dict(width=0), dict(width=-64),
    dict(margin=-0.01), dict(margin=float("nan")), dict(margin=float("inf")), dict(variance=0.0), dict(variance=-0.2),
    dict(variance=float("nan")), dict(variance=float("inf")), dict(mode=2), dict(mode=-1),
])
def test_invalid_arguments_are_refused_before_any_gpu_work(bad):
    one = C.c_void_p(256)                     # never dereferenced: the checks come first
    assert _compute(**bad, xyz=one, views=one, filt=one, ws=one) == EINVAL
    if "n" not in bad:
        assert _compute(n=0, **bad) == EINVAL                                    # ... also with nothing to do


def test_null_pointers_and_the_empty_call():
    one = C.c_void_p(256)
    full = dict(xyz=one, views=one, filt=one, ws=one)
    for missing in full:
        assert _compute(**dict(full, **{missing: None})) == ENULL, missing
    assert _compute(n=0) == 0                 # n == 0 launches nothing and needs nothing
    assert _compute(n=0, mode=1, V=_lib.FILTER3D_MAX_VIEWS) == 0
    lib = _lib.load()
    assert lib.lsr_filter3d_workspace_bytes(0, 4) == 0 and lib.lsr_filter3d_workspace_bytes(10, 0) == 0
    assert lib.lsr_filter3d_workspace_bytes(10, _lib.FILTER3D_MAX_VIEWS + 1) == 0
    a, b = lib.lsr_filter3d_workspace_bytes(10, 4), lib.lsr_filter3d_workspace_bytes(10, 200)
    assert 0 < a < b <= 64 + 64 * 200 and lib.lsr_filter3d_workspace_bytes(1 << 20, 4) == a      # per camera, not per Gaussian


def _dims(n=100, K=4, m=1.0, r0=0, r1=0):
    return SceneDims(n=n, sh_coeffs=K, scale_modifier=m, reserved0=r0, reserved1=r1)


def _filtered(fn, dims, params, filt, a, b=None):
    lib = _lib.load()
    r = lambda s: None if s is None else C.byref(s)
    if fn == "forward":
        return lib.lsr_scene_activate_filtered_forward(r(dims), r(params), filt, r(a), None)
    return lib.lsr_scene_activate_filtered_backward(r(dims), r(params), filt, r(a), r(b), None)


def test_the_filtered_activation_checks_what_the_unfiltered_one_checks():
    one = C.c_void_p(256)                     # 16-byte aligned, never dereferenced
    params = SceneParams(one, one, one, one, one)
    for fn, a, b in (("forward", SceneOutputs(), None), ("backward", SceneOutGrads(), SceneInGrads())):
        call = lambda dims, p=params, f=one: _filtered(fn, dims, p, f, a, b)
        assert call(_dims(), f=None) == ENULL                                     # the one new code: no filter
        assert call(_dims(n=0), f=None) == 0 and call(_dims(n=0)) == 0
        assert call(_dims(n=-1)) == EINVAL and call(_dims(K=5)) == EINVAL
        assert call(_dims(m=0.0)) == EINVAL and call(_dims(m=float("nan"))) == EINVAL
        assert call(_dims(r0=1)) == EINVAL and call(_dims(r1=1)) == EINVAL       # the reserved fields stay refused
        assert call(_dims(K=1)) == EINVAL                                          # features_rest given with K == 1
        assert call(_dims(), p=SceneParams(one, one, None, one, one)) == ENULL
        assert call(_dims(), p=SceneParams(one, one, one, one, C.c_void_p(260))) == EINVAL      # the quad's alignment
        assert call(None) == ENULL and _filtered(fn, _dims(), None, one, a, b) == ENULL
    assert _filtered("forward", _dims(), params, one, None) == ENULL
    assert _filtered("backward", _dims(), params, one, SceneOutGrads(), None) == ENULL


def _cpu_scene(n=5, K=4):
    from latentsplat_amd import GaussianScene
    p = sref.make_params(n, K, seed=3)
    return GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in p.items()}), p


def test_cpu_tensors_are_refused():
    from latentsplat_amd import activate_scene_filtered, compute_filter_3d, fused_parameters
    scene, p = _cpu_scene()
    t = [torch.from_numpy(p[k]) for k in sref.PARAMS]
    views = torch.from_numpy(fref.circle_views(2))
    filt = torch.full((5, 1), 0.01)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        compute_filter_3d(torch.from_numpy(p["xyz"]), views, 64)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        activate_scene_filtered(*t, filt)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        fused_parameters(t[2], t[3], filt)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.render(views, 16, 16, filter_3d=filt)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.activated(filter_3d=filt)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.compute_filter_3d(views, 64)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.save_ply("/nonexistent/never_written.ply", filter_3d=filt)


def test_a_stale_filter_is_refused():
    """A filter computed for another number of Gaussians (before a densification, a growth or a pruning) is refused by
    its length alone, before anything else is looked at."""
    scene, _ = _cpu_scene(n=5)
    views = torch.from_numpy(fref.circle_views(2))
    for stale in (torch.zeros(4, 1), torch.zeros(6), torch.zeros(5, 2), torch.zeros(0, 1)):
        with pytest.raises(_lib.LsrError, match="stale"):
            scene.render(views, 16, 16, filter_3d=stale)
        with pytest.raises(_lib.LsrError, match="stale"):
            scene.activated(filter_3d=stale)
        with pytest.raises(_lib.LsrError, match="stale"):
            scene.save_ply("/nonexistent/never_written.ply", filter_3d=stale)
    # the module holds no filter: its parameters and state are what they were
    assert [k for k, _ in scene.named_parameters()] == ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    assert not list(scene.buffers())


def _three_cameras(scale=1.0):
    """Three cameras looking along +z from z = 0, -1 and -3 with tanfov 0.5, 0.25, 0.5: at width 100 their focal
    lengths are 100, 200 and 100."""
    ext = np.tile(np.eye(4), (3, 1, 1))
    ext[:, 2, 3] = (0.0, -1.0, -3.0)
    return fref.view_records(ext, (0.5, 0.25, 0.5), (0.5, 0.25, 0.5), scale)


def test_the_restatement_against_a_hand_computed_case():
    """G0 = (0, 0, 2) lies inside all three cameras at depths 2, 3, 5.  G1 = (1.2, 0, 2): for the first camera the image
    edge is at |x| = 0.5 * 2 = 1 and the widened frustum at 1.3, so it is seen only inside the 15 % margin; the second
    (limit 1.3 * 0.25 * 3 = 0.975) does not see it; the third (image edge 2.5) does.  G2 = (0, 0, -4) is behind all three.
    Published: smallest depth over the largest focal length (200).  Per view: the largest focal / depth.  The mixed focal
    lengths make the modes differ: G0 is bound by the second camera's 200 / 3, not by 200 / 2."""
    xyz = np.array([[0, 0, 2], [1.2, 0, 2], [0, 0, -4]], np.float32)
    sd = np.sqrt(float(np.float32(0.2)))
    for scale in (1.0, 0.5):
        views = _three_cameras(scale)
        pub = fref.filter_ref(xyz, views, 100)
        assert pub["seen"].tolist() == [True, True, False] and pub["F"] == 200.0 and pub["near"] == 0
        np.testing.assert_allclose(pub["filter"], np.array([2 / 200, 2 / 200, 2 / 200]) * sd, rtol=1e-6)
        per = fref.filter_ref(xyz, views, 100, per_view=True)
        np.testing.assert_allclose(per["filter"], np.array([3 / 200, 2 / 100, 2 / 100]) * sd, rtol=1e-6)
        # without the margin the first camera no longer sees G1: its depth is the third camera's 5, and G2 inherits it
        tight = fref.filter_ref(xyz, views, 100, margin=0.0)
        assert tight["seen"].tolist() == [True, True, False]
        np.testing.assert_allclose(tight["filter"], np.array([2 / 200, 5 / 200, 5 / 200]) * sd, rtol=1e-6)
        np.testing.assert_allclose(fref.filter_ref(xyz, views, 100, margin=0.0, per_view=True)["filter"],
                                   np.array([3 / 200, 5 / 100, 5 / 100]) * sd, rtol=1e-6)
    # equal focal lengths: the two modes agree
    same = fref.view_records(np.tile(np.eye(4), (2, 1, 1)), 0.5, 0.5)
    same[1, 14] = 1.0
    a, b = fref.filter_ref(xyz, same, 100), fref.filter_ref(xyz, same, 100, per_view=True)
    np.testing.assert_allclose(a["filter"], b["filter"], rtol=1e-12)
    # nothing seen: zeros; a NaN position is unseen and takes the fallback
    assert not fref.filter_ref(xyz[2:], _three_cameras(), 100)["filter"].any()
    bad = xyz.copy()
    bad[0, 1] = np.nan
    got = fref.filter_ref(bad, _three_cameras(), 100)
    assert got["seen"].tolist() == [False, True, False] and np.allclose(got["filter"], 2 / 200 * sd)
    # at a scene scale of 0.5 the near plane 0.2 of the scaled space lies at depth 0.4: a point at depth 0.3 is culled
    close = np.array([[0, 0, 0.3]], np.float32)
    assert fref.filter_ref(close, _three_cameras(1.0)[:1], 100)["seen"][0] and not fref.filter_ref(close, _three_cameras(0.5)[:1], 100)["seen"][0]


def test_the_builders_leave_no_pair_at_a_threshold():
    views = fref.circle_views(5, seed=2)
    pts = fref.draw_points(500, views, seed=4)
    ref = fref.filter_ref(pts, views, 64)
    assert ref["near"] == 0 and 0 < ref["seen"].sum() < 500
    pz = np.stack([fref.project(pts.astype(np.float64), r.astype(np.float64))[2] for r in views])
    assert (pz < fref.NEAR).any() and (pz > fref.NEAR).any()
    pts_t, valid = fref.threshold_points(views[0])
    one = fref.filter_ref(pts_t, views[:1], 64)
    assert one["near"] == 0 and np.array_equal(one["seen"], valid) and valid.any() and not valid.all()
    # a pair ON a threshold is counted
    assert fref.filter_ref(fref.world_point(views[0], (0, 0, fref.NEAR * (1 + 5e-5)))[None], views[:1], 64)["near"] == 1


def test_restatement_gradients_against_finite_differences():
    p = sref.make_params(6, 4, seed=2)
    up = sref.make_upstream(6, 4, seed=3)
    filt = fref.make_filter(6, seed=4)
    filt[:3, 0] = np.exp(p["scaling"][:3].mean(1))           # filters of the size of the scales: both terms matter
    g = fref.gradients(p, filt, up, 0.5)
    up64 = {k: torch.from_numpy(v.astype(np.float64)) for k, v in up.items()}
    f64 = torch.from_numpy(filt.astype(np.float64))

    def loss(q):
        out = fref.forward64({k: torch.from_numpy(q[k]) for k in sref.PARAMS}, f64, 0.5)
        return float(sum((out[k] * up64[k]).sum() for k in up64))

    base = {k: p[k].astype(np.float64) for k in sref.PARAMS}
    rng = np.random.default_rng(0)
    for k in sref.PARAMS:
        d = rng.standard_normal(base[k].shape)
        h = 1e-6
        plus, minus = dict(base), dict(base)
        plus[k], minus[k] = base[k] + h * d, base[k] - h * d
        fd = (loss(plus) - loss(minus)) / (2 * h)
        assert abs(fd - float((g[k] * d).sum())) <= 1e-6 * max(1.0, abs(fd)), k
    # the closed form of include/lsr_scene.h for the opacity coefficient's share of d scaling
    only_o = fref.gradients(p, filt, dict(opacities=up["opacities"]), 0.5)
    s, f = np.exp(p["scaling"].astype(np.float64)), filt.astype(np.float64)
    v = s * s + f * f
    o = 1.0 / (1.0 + np.exp(-p["opacity"].astype(np.float64)))
    c = (s / np.sqrt(v)).prod(1, keepdims=True)
    np.testing.assert_allclose(only_o["scaling"], up["opacities"] * o * c * f * f / v, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(only_o["opacity"], up["opacities"] * c * o * (1 - o), rtol=1e-10, atol=1e-300)
    # a zero filter is the unfiltered map
    zero = fref.gradients(p, np.zeros((6, 1), np.float32), up, 0.5)
    plain = sref.gradients(p, up, 0.5)
    for k in sref.PARAMS:
        # (entries that are differences of larger terms carry those terms' float64 rounding)
        np.testing.assert_allclose(zero[k], plain[k], rtol=1e-12, atol=1e-12 * np.abs(plain[k]).max())


def test_fused_parameters_reproduce_the_filtered_activation():
    """logit(o c) and log(sqrt(v_k)), activated WITHOUT a filter, are the filtered activation: to 1e-12 in float64."""
    n, K = 200, 4
    p = sref.make_params(n, K, seed=11)
    filt = fref.make_filter(n, seed=12)
    for m in (1.0, 0.5):
        want = fref.expected(p, filt, m)
        opacity, scaling = fref.fused64(p["opacity"], p["scaling"], filt)
        fused = {k: torch.from_numpy(np.asarray(p[k], np.float64)) for k in sref.PARAMS}
        fused["opacity"], fused["scaling"] = torch.from_numpy(opacity), torch.from_numpy(scaling)
        got = {k: v.numpy() for k, v in sref.forward64(fused, m).items()}
        for k in ("shs", "opacities", "scales", "rotations"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0.0, err_msg=k)
        bound = 1e-12 * np.abs(want["cov3D"]).max(1, keepdims=True)
        assert (np.abs(got["cov3D"] - want["cov3D"]) <= bound).all()
    # a zero filter fuses to the parameters themselves
    opacity, scaling = fref.fused64(p["opacity"], p["scaling"], np.zeros((n, 1)))
    np.testing.assert_allclose(scaling, p["scaling"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(opacity, p["opacity"], rtol=1e-12, atol=1e-14)
