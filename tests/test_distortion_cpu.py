"""The depth distortion regulariser without a GPU: the identity D = A M2 - M1^2 against the brute-force pair sum and the 2DGS
recurrence, the exports, the argument checks of the C ABI (returned before any GPU work, with device pointers that are never
dereferenced), the refusals of the Python layer, depth_pivot against a hand computation, and the restatement
(tests/distortion_ref.py) under torch.autograd.gradcheck."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import DistortionDims
from tests import distortion_ref as dref
from tests import normals_ref as nref

NEW = ("lsr_scene_depth_moments_workspace_bytes", "lsr_scene_depth_moments_forward", "lsr_scene_depth_moments_backward",
       "lsr_distortion_loss_workspace_bytes", "lsr_distortion_loss_forward", "lsr_distortion_loss_backward")
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5
ONE = C.c_void_p(256)                         # 16-byte aligned, never dereferenced: the checks come first


@pytest.mark.parametrize("count", [1, 2, 3, 50])
def test_the_identity(count):
    """sum_{j<i} w_i w_j (m_i - m_j)^2 = A M2 - M1^2 = the running recurrence of 2DGS, in float64 to 1e-12 relative."""
    for seed in range(5):
        rng = np.random.default_rng(100 * count + seed)
        w = dref.blend_weights(rng.uniform(0.01, 0.9, count))
        m = rng.uniform(0.5, 6.0, count)
        brute = dref.pair_sum(w, m)
        scale = max(brute, 1e-300)
        assert abs(dref.moment_form(w, m) - brute) <= 1e-12 * max(scale, w.sum() * (w * m * m).sum())
        assert abs(dref.recurrence_2dgs(w, m) - brute) <= 1e-12 * max(scale, w.sum() * (w * m * m).sum())
        if count == 1:
            assert brute == 0.0
        else:
            assert brute > 0
        # ... and D does not move with a constant subtracted from every m: the pivot
        assert abs(dref.pair_sum(w, m - 3.0) - brute) <= 1e-12 * max(scale, 1.0)


def test_exports():
    lib = _lib.load()
    header = open(__file__.rsplit("tests", 1)[0] + "include/lsr_distortion.h").read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name in header, name
    import latentsplat_amd
    for name in ("gaussian_depth_moments", "distortion_loss", "distortion_map", "depth_pivot"):
        assert latentsplat_amd._LAZY[name] == "distortion" and callable(getattr(latentsplat_amd, name))
    assert hasattr(latentsplat_amd.GaussianScene, "render_with_distortion") and hasattr(latentsplat_amd.GaussianScene, "render_surface")
    assert lib.lsr_abi_version() == 10        # new symbols, the same ABI
    assert (_lib.DIST_LINEAR, _lib.DIST_NDC, _lib.DIST_DISPARITY) == (0, 1, 2) and C.sizeof(DistortionDims) == 24


def _moments(fn, n=5, V=2, space=1, **p):
    lib = _lib.load()
    a = dict(xyz=ONE, views=ONE, pivot=ONE, out=ONE, grad=ONE, ws=ONE)
    a.update(p)
    if fn == "forward":
        return lib.lsr_scene_depth_moments_forward(n, a["xyz"], V, a["views"], a["pivot"], space, a["out"], a["ws"], None)
    return lib.lsr_scene_depth_moments_backward(n, a["xyz"], V, a["views"], a["pivot"], space, a["grad"], a["out"], a["ws"], None)


@pytest.mark.parametrize("fn", ["forward", "backward"])
def test_depth_moments_arguments(fn):
    for bad in (dict(n=-1), dict(n=1 << 28), dict(V=0), dict(V=-2), dict(V=_lib.DIST_MAX_VIEWS + 1), dict(space=3), dict(space=-1)):
        assert _moments(fn, **bad) == EINVAL, bad
        if "n" not in bad:
            assert _moments(fn, n=0, **bad) == EINVAL                      # ... also with nothing to do
    assert _moments(fn, ws=C.c_void_p(264)) == EINVAL                        # a camera record moves as one aligned load
    assert _moments(fn, **{"out" if fn == "forward" else "grad": C.c_void_p(260)}) == EINVAL      # a pair moves as 8 bytes
    names = ("xyz", "views", "out", "ws") + (("grad",) if fn == "backward" else ())
    for missing in names:
        assert _moments(fn, **{missing: None}) == ENULL, missing
    # (a NULL pivot is pivot 0: the launch would follow, so it is not called here; the GPU tests do)
    none = {k: None for k in names + ("pivot",)}
    for space in (0, 1, 2):
        assert _moments(fn, n=0, space=space, **none) == 0                   # n == 0 launches nothing and needs nothing
    assert _moments(fn, n=0, V=_lib.DIST_MAX_VIEWS, **none) == 0
    lib = _lib.load()
    size = lib.lsr_scene_depth_moments_workspace_bytes
    assert size(0, 4) == 0 and size(-1, 4) == 0 and size(10, 0) == 0 and size(10, _lib.DIST_MAX_VIEWS + 1) == 0 and size(1 << 28, 4) == 0
    assert size(10, 4) == 4 * 48 == size(1 << 20, 4) == size(10, 4)


def _dims(V=2, H=8, W=9, r0=0, r1=0, r2=0):
    return DistortionDims(num_images=V, height=H, width=W, reserved0=r0, reserved1=r1, reserved2=r2)


def _loss(fn, dims, **p):
    lib = _lib.load()
    a = dict(moment_map=ONE, alpha=ONE, weight=ONE, ws=ONE, grad_loss=ONE)
    a.update(p)
    d = None if dims is None else C.byref(dims)
    if fn == "forward":
        return lib.lsr_distortion_loss_forward(d, a["moment_map"], a["alpha"], a["weight"], a["ws"], ONE, None, None, None)
    return lib.lsr_distortion_loss_backward(d, a["moment_map"], a["alpha"], a["weight"], a["grad_loss"], ONE, ONE, None)


@pytest.mark.parametrize("fn", ["forward", "backward"])
def test_distortion_loss_arguments(fn):
    for bad in (dict(V=0), dict(H=0), dict(W=-1), dict(r0=1), dict(r1=1), dict(r2=-1)):
        assert _loss(fn, _dims(**bad)) == EINVAL, bad
    assert _loss(fn, _dims(V=1, H=1 << 15, W=1 << 15)) == EUNSUPPORTED        # 2 V H W = 2^31
    assert _loss(fn, _dims(V=4, H=1 << 14, W=1 << 14)) == EUNSUPPORTED
    assert _loss(fn, None) == ENULL
    names = ("moment_map", "alpha") + (("ws",) if fn == "forward" else ("grad_loss",))
    for missing in names:
        assert _loss(fn, _dims(), **{missing: None}) == ENULL, missing
    if fn == "forward":
        assert _loss(fn, _dims(), ws=C.c_void_p(264)) == EINVAL
    else:                                                                     # nothing wanted: nothing launched
        assert _lib.load().lsr_distortion_loss_backward(C.byref(_dims()), ONE, ONE, None, ONE, None, None, None) == 0
    size = _lib.load().lsr_distortion_loss_workspace_bytes
    assert size(None) == 0 and size(C.byref(_dims(V=0))) == 0 and size(C.byref(_dims(r1=1))) == 0
    assert size(C.byref(_dims(V=1, H=1 << 15, W=1 << 15))) == 0
    small, large = (size(C.byref(_dims(V=v, H=70, W=97))) for v in (1, 40))
    assert 0 < small <= large and large >= 40 * 4 * 8                         # one double per 2048 pixels: 4 per image
    assert small == size(C.byref(_dims(V=1, H=70, W=97)))                     # pure


def test_cpu_tensors_and_other_refusals():
    from latentsplat_amd import GaussianScene, distortion_loss, distortion_map, gaussian_depth_moments
    from tests import scene_params_ref as sref
    case = dref.scene_case(5, 2, seed=1)
    views, xyz = nref.to(torch.float32, case["views"], case["xyz"])
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        gaussian_depth_moments(views, xyz)
    with pytest.raises(_lib.LsrError, match="space"):
        gaussian_depth_moments(views, xyz, space="log")
    with pytest.raises(_lib.LsrError, match="requires grad"):
        gaussian_depth_moments(views.clone().requires_grad_(True), xyz)
    with pytest.raises(_lib.LsrError, match="requires grad"):
        gaussian_depth_moments(views, xyz, pivot=torch.zeros(2, requires_grad=True))
    img = dref.image_case(2, 5, 4, seed=1, weighted=True)
    mm, alpha, weight = nref.to(torch.float32, img["moment_map"], img["alpha"], img["weight"])
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        distortion_loss(mm, alpha, weight)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        distortion_map(mm, alpha)
    p = sref.make_params(5, 4, seed=3)
    scene = GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in p.items()})
    for render in (scene.render_with_distortion, scene.render_surface):
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            render(views, 16, 16)
        with pytest.raises(_lib.LsrError, match="features"):
            render(views, 16, 16, features=torch.zeros(5, 3))
        with pytest.raises(_lib.LsrError, match="features"):
            render(views, 16, 16, feature_sh=torch.zeros(5, 3, 4))


def test_depth_pivot_against_a_hand_computation():
    """One camera at (1, 2, -3) looking down +z with a scene scale of 2 in slot 40: the point (1.5, 2.5, 1) is 4 in front."""
    from latentsplat_amd.distortion import depth_pivot, with_near_far
    ext = np.eye(4)[None].copy()
    ext[0, :3, 3] = (1.0, 2.0, -3.0)
    views = torch.from_numpy(nref.view_records(ext, 0.5, 0.5, scale=2.0))
    assert float(views[0, 40]) == 2.0 and float(views[0, 14]) == 6.0          # the translation is stored scaled
    point = (1.5, 2.5, 1.0)
    assert depth_pivot(views, point, "linear").dtype == torch.float32
    assert abs(float(depth_pivot(views, point, "linear")[0]) - 4.0) < 1e-6
    assert abs(float(depth_pivot(views, point, "disparity")[0]) - 0.25) < 1e-7
    with pytest.raises(_lib.LsrError, match="near < far"):                    # a NATIVE table carries 0 / 0
        depth_pivot(views, point, "ndc")
    for near, far in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.1, float("inf"))):
        with pytest.raises(_lib.LsrError, match="near < far"):
            depth_pivot(with_near_far(views, near, far), point, "ndc")
    nf = with_near_far(views, 0.5, 50.0)
    assert torch.equal(nf[:, :42], views[:, :42]) and float(views[0, 42]) == 0.0
    want = 50.0 / 49.5 * (1.0 - 0.5 / 4.0)
    assert abs(float(depth_pivot(nf, point, "ndc")[0]) - want) < 1e-6
    # the restatement's own pivot and depths agree
    assert abs(float(dref.pivot_of(nf.numpy(), point, "ndc")[0]) - want) < 1e-6
    z = dref.depths(nf.double(), torch.tensor([point], dtype=torch.float64))
    assert abs(float(z[0, 0]) - 4.0) < 1e-12


def test_gradcheck_of_both_restatements():
    for space in dref.SPACES:
        case = dref.scene_case(4, 2, seed=2, scale40=(0.5, 2.0), space=space)
        views, xyz, pivot = nref.to(torch.float64, case["views"], case["xyz"], case["pivot"])
        xyz.requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: dref.depth_moments(views, x, space, pivot), (xyz,), eps=1e-6, atol=1e-7)
    img = dref.image_case(2, 6, 5, seed=4, weighted=True)
    mm, alpha, weight = nref.to(torch.float64, img["moment_map"], img["alpha"], img["weight"])
    mm.requires_grad_(True)
    alpha.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: dref.distortion(a, b, weight)["loss"], (mm, alpha), eps=1e-6, atol=1e-9)
    # a row behind the camera or not finite gives (0, 0) and no gradient
    case = dref.scene_case(6, 2, seed=3, space="linear")
    case["xyz"][1] = (0.0, 0.0, 1e4)
    case["xyz"][2, 0] = np.nan
    views, xyz = nref.to(torch.float64, case["views"], case["xyz"])
    xyz.requires_grad_(True)
    out = dref.depth_moments(views, xyz, "linear")
    out.sum().backward()
    assert not out[:, 2].any() and not xyz.grad[2].any() and bool(torch.isfinite(xyz.grad).all())
    assert not out[:, 1].all()                 # 10^4 along z is behind one of two cameras on a circle


def test_the_gpu_cases_reach_the_second_trips():
    """What the GPU test's cases reach in csrc/distortion.hip, so that nobody trims them without seeing what goes: a lane's
    second Gaussian (grid-stride beyond LSR_DIST_MAX_BLOCKS workgroups), a compaction lane's second camera, a view's second
    chunk and its unaligned planes."""
    from tests.test_distortion_gpu import B_SHAPES, MANY_VIEWS, PAST_ONE_TRIP
    assert PAST_ONE_TRIP > _lib.DIST_THREADS * _lib.DIST_MAX_BLOCKS and MANY_VIEWS > _lib.DIST_THREADS
    assert any(H * W > _lib.DIST_CHUNK for _, H, W in B_SHAPES) and any(H * W % 4 for _, H, W in B_SHAPES)
    assert any(H * W % 4 == 0 and V > 1 for V, H, W in B_SHAPES)
