"""The depth-normal consistency regulariser without a GPU: the exports, the argument checks of the C ABI (returned before
any GPU work, with device pointers that are never dereferenced), the refusals of the Python layer, and the restatement
(tests/normals_ref.py) against an analytic plane, its own invariants, torch.autograd.gradcheck and the conditions its case
builders promise."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import NormalDims
from tests import normals_ref as nref
from tests import scene_params_ref as sref

NEW = ("lsr_scene_normals_workspace_bytes", "lsr_scene_normals_forward", "lsr_scene_normals_backward",
       "lsr_normal_consistency_workspace_bytes", "lsr_normal_consistency_forward", "lsr_normal_consistency_backward")
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5
ONE = C.c_void_p(256)                         # 16-byte aligned, never dereferenced: the checks come first


def test_exports():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    import latentsplat_amd
    for name in ("gaussian_normals", "normal_consistency_loss", "depth_to_normals", "flatten_loss"):
        assert latentsplat_amd._LAZY[name] == "normals" and callable(getattr(latentsplat_amd, name))
    assert hasattr(latentsplat_amd.GaussianScene, "render_with_normals")
    assert lib.lsr_abi_version() == 10        # new symbols, the same ABI


def _normals(fn, n=5, V=2, **p):
    lib = _lib.load()
    a = dict(xyz=ONE, scaling=ONE, rotation=ONE, views=ONE, out=ONE, grad=ONE, ws=ONE)
    a.update(p)
    if fn == "forward":
        return lib.lsr_scene_normals_forward(n, a["xyz"], a["scaling"], a["rotation"], V, a["views"], a["out"], a["ws"], None)
    return lib.lsr_scene_normals_backward(n, a["xyz"], a["scaling"], a["rotation"], V, a["views"], a["grad"], a["out"], a["ws"], None)


@pytest.mark.parametrize("fn", ["forward", "backward"])
def test_scene_normals_arguments(fn):
    for bad in (dict(n=-1), dict(n=1 << 28), dict(V=0), dict(V=-2), dict(V=_lib.NORMALS_MAX_VIEWS + 1)):
        assert _normals(fn, **bad) == EINVAL, bad
        if "n" not in bad:
            assert _normals(fn, n=0, **bad) == EINVAL                      # ... also with nothing to do
    assert _normals(fn, rotation=C.c_void_p(260)) == EINVAL                  # the quaternion moves as one 16-byte quad
    names = ("xyz", "scaling", "rotation", "views", "out", "ws") + (("grad",) if fn == "backward" else ())
    for missing in names:
        assert _normals(fn, **{missing: None}) == ENULL, missing
    none = {k: None for k in names}
    assert _normals(fn, n=0, **none) == 0                                    # n == 0 launches nothing and needs nothing
    assert _normals(fn, n=0, V=_lib.NORMALS_MAX_VIEWS, **none) == 0
    lib = _lib.load()
    assert lib.lsr_scene_normals_workspace_bytes(0, 4) == 0 and lib.lsr_scene_normals_workspace_bytes(10, 0) == 0
    assert lib.lsr_scene_normals_workspace_bytes(10, _lib.NORMALS_MAX_VIEWS + 1) == 0
    assert lib.lsr_scene_normals_workspace_bytes(10, 4) == 4 * 64 == lib.lsr_scene_normals_workspace_bytes(1 << 20, 4)


def _dims(V=2, H=8, W=9, alpha_min=0.5, r0=0, r1=0):
    return NormalDims(num_images=V, height=H, width=W, alpha_min=alpha_min, reserved0=r0, reserved1=r1)


def _nc(fn, dims, **p):
    lib = _lib.load()
    a = dict(normal_map=ONE, depth=ONE, alpha=ONE, views=ONE, ws=ONE, grad_loss=ONE, loss=ONE)
    a.update(p)
    d = None if dims is None else C.byref(dims)
    if fn == "forward":
        return lib.lsr_normal_consistency_forward(d, a["normal_map"], a["depth"], a["alpha"], a["views"], a["ws"], a["loss"],
                                                  None, None, None, None)
    return lib.lsr_normal_consistency_backward(d, a["normal_map"], a["depth"], a["alpha"], a["views"], a["grad_loss"],
                                               ONE, ONE, ONE, None)


@pytest.mark.parametrize("fn", ["forward", "backward"])
def test_normal_consistency_arguments(fn):
    for bad in (dict(V=0), dict(H=0), dict(W=-1), dict(alpha_min=0.0), dict(alpha_min=-0.5), dict(alpha_min=float("nan")),
                dict(alpha_min=float("inf")), dict(r0=1), dict(r1=1)):
        assert _nc(fn, _dims(**bad)) == EINVAL, bad
    assert _nc(fn, _dims(V=4, H=1 << 14, W=1 << 14)) == EUNSUPPORTED       # 3 V H W >= 2^31
    assert _nc(fn, None) == ENULL
    names = ("normal_map", "depth", "alpha", "views") + (("ws",) if fn == "forward" else ("grad_loss",))
    for missing in names:
        assert _nc(fn, _dims(), **{missing: None}) == ENULL, missing
    if fn == "forward":
        assert _nc(fn, _dims(), ws=C.c_void_p(264)) == EINVAL
    lib = _lib.load()
    assert lib.lsr_normal_consistency_workspace_bytes(None) == 0
    assert lib.lsr_normal_consistency_workspace_bytes(C.byref(_dims(V=0))) == 0
    small, large = (lib.lsr_normal_consistency_workspace_bytes(C.byref(_dims(V=v, H=70, W=97))) for v in (1, 40))
    assert 0 < small <= large and large >= 40 * 3 * 4 * 8                    # one double per 32 x 32 tile


def test_cpu_tensors_are_refused():
    from latentsplat_amd import GaussianScene, depth_to_normals, gaussian_normals, normal_consistency_loss
    case = nref.scene_case(5, 2, seed=1)
    views, xyz, scaling, rotation = nref.to(torch.float32, case["views"], case["xyz"], case["scaling"], case["rotation"])
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        gaussian_normals(views, xyz, scaling, rotation)
    img = nref.image_case(2, 5, 4, seed=1)
    N, depth, alpha, v2 = nref.to(torch.float32, img["normal_map"], img["depth"], img["alpha"], img["views"])
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        normal_consistency_loss(N, depth, alpha, v2)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        depth_to_normals(depth, alpha, v2)
    p = sref.make_params(5, 4, seed=3)
    scene = GaussianScene.from_tensors(**{k: torch.from_numpy(v) for k, v in p.items()})
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.render_with_normals(views, 16, 16)
    # the payload carries the normals: a caller's own is refused, before anything else is looked at
    with pytest.raises(_lib.LsrError, match="features"):
        scene.render_with_normals(views, 16, 16, features=torch.zeros(5, 3))
    with pytest.raises(_lib.LsrError, match="features"):
        scene.render_with_normals(views, 16, 16, feature_sh=torch.zeros(5, 3, 4))


def test_flatten_loss():
    from latentsplat_amd.normals import flatten_loss
    s = torch.tensor([[0.0, -1.0, 2.0], [-3.0, -2.0, -2.5]], dtype=torch.float64, requires_grad=True)
    want = (np.exp(-1.0) + np.exp(-3.0)) / 2
    assert abs(float(flatten_loss(s).detach()) - want) < 1e-15
    flatten_loss(s).backward()
    np.testing.assert_allclose(s.grad.numpy(), [[0, np.exp(-1.0) / 2, 0], [np.exp(-3.0) / 2, 0, 0]], rtol=1e-15)


def test_an_analytic_plane_under_an_offcentre_principal_point():
    """Depth rendered from the plane <n, X> = d in camera space, D(p) = d / <n, r(p)>, under a camera with an off-centre
    principal point and unequal fovs: every valid pixel's n~ is the plane's unit normal, turned toward the camera, and every
    interior pixel is valid."""
    H, W = 9, 11
    views = nref.view_records(nref.circle_extrinsics(2, seed=3), (0.5, 0.4), (0.3, 0.45), cx=(0.2, -0.15), cy=(-0.1, 0.25),
                              scale=(1.0, 0.5))
    tv = torch.from_numpy(views.astype(np.float64))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    n = torch.tensor([0.3, -0.2, -1.0], dtype=torch.float64)
    n = n / n.norm()                                   # faces the camera: z < 0
    depth = []
    for v in range(2):
        rx, ry = nref.pixel_rays(tv[v], H, W, xs, ys)
        # ndc = 0 at the centre pixel of an odd-sized image: its ray is -c tan(fov), not the optical axis
        assert abs(float(rx[H // 2, W // 2]) + (0.2, -0.15)[v] * float(views[v, 35])) < 1e-6
        assert abs(float(ry[H // 2, W // 2]) + (-0.1, 0.25)[v] * float(views[v, 36])) < 1e-6
        depth.append(-3.0 / (n[0] * rx + n[1] * ry + n[2]))
    depth = torch.stack(depth)
    alpha = torch.full_like(depth, 0.8)
    out = nref.consistency(torch.zeros(2, 3, H, W, dtype=torch.float64), depth * alpha, alpha, tv)
    assert bool(out["valid"][:, 1:-1, 1:-1].all()) and int(out["valid"].sum()) == 2 * (H - 2) * (W - 2)
    got = out["depth_normals"].permute(0, 2, 3, 1)[out["valid"]]
    assert float((got - n).abs().max()) < 1e-12
    # N = alpha n at every pixel: e = 0, so the loss is 0; N = 0: e = alpha at the valid pixels
    N = (alpha[..., None] * n).permute(0, 3, 1, 2)
    assert abs(float(nref.consistency(N, depth * alpha, alpha, tv)["loss"])) < 1e-13
    assert abs(float(out["loss"]) - 0.8 * (H - 2) * (W - 2) / (H * W)) < 1e-13


def test_gaussian_normals_are_unit_and_face_the_camera():
    case = nref.scene_case(200, 3, seed=5, scale40=(1.0, 0.5, 2.0), ties="two")
    views, xyz, scaling, rotation = nref.to(torch.float64, case["views"], case["xyz"], case["scaling"], case["rotation"])
    out = nref.gaussian_normals(views, xyz, scaling, rotation)
    assert float((out.norm(dim=-1) - 1).abs().max()) < 1e-6          # (the float32 view matrix is a rotation to 1e-7)
    for v in range(3):
        Wm = views[v, :16].reshape(4, 4).T
        p = (views[v, 40] * xyz) @ Wm[:3, :3].T + Wm[:3, 3]             # camera-space position: the camera sits at 0
        assert bool(((out[v] * -p).sum(-1) > 0).all())
    # activated scales pick the same axis as log-scales; a NaN row gives 0
    assert torch.equal(out, nref.gaussian_normals(views, xyz, torch.exp(scaling), rotation))
    rotation[7] = 0.0
    xyz[9, 1] = float("nan")
    bad = nref.gaussian_normals(views, xyz, scaling, rotation)
    assert not bad[:, 7].any() and not bad[:, 9].any() and torch.equal(bad[:, 10:], out[:, 10:])


def test_gradcheck_of_both_restatements():
    case = nref.scene_case(4, 2, seed=2)
    views, xyz, scaling, rotation = nref.to(torch.float64, case["views"], case["xyz"], case["scaling"], case["rotation"])
    rotation.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q: nref.gaussian_normals(views, xyz, scaling, q), (rotation,), eps=1e-6, atol=1e-7)
    img = nref.image_case(2, 6, 5, seed=4, offcentre=True, holes=False)
    N, depth, alpha, v2 = nref.to(torch.float64, img["normal_map"], img["depth"], img["alpha"], img["views"])
    N.requires_grad_(True)
    depth.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: nref.consistency(a, b, alpha, v2)["loss"], (N, depth), eps=1e-6, atol=1e-8)
    # alpha: only through D (the leading alpha is detached), so the finite difference is of the loss minus its leading term
    alpha.requires_grad_(True)
    g, =torch.autograd.grad(nref.consistency(N.detach(), depth.detach(), alpha, v2)["loss"], alpha)
    h = 1e-6
    d = torch.from_numpy(np.random.default_rng(0).standard_normal(tuple(alpha.shape)))
    with torch.no_grad():
        f = lambda al: float(nref.consistency(N, depth, al, v2)["loss"]) - float((al * nref.consistency(N, depth, al, v2)["valid"]).sum()) / al.numel()
        fd = (f(alpha + h * d) - f(alpha - h * d)) / (2 * h)
    assert abs(fd - float((g * d).sum())) <= 1e-7 * max(1.0, abs(fd))


def test_the_gpu_cases_reach_both_loops_of_the_finish_kernel():
    """k_image_mean_finish (csrc/lsr_image_sum.h): wave w of 16 adds the images w, w + 16, ..., lane l of 64 the tiles l, l + 64, ... of
    an image.  What the GPU test's cases reach, so that nobody trims them without seeing what goes."""
    from tests.test_normals_gpu import FINISH_WAVES, PAST_THE_FINISH, SIZES, TILE, WAVE
    assert (FINISH_WAVES, WAVE, TILE) == (16, 64, 32)
    tiles = lambda H, W: ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    assert max(tiles(H, W) for H, W in SIZES) == 12                       # the sizes of the cross-product stop short of both
    reached = {(V, H, W): (V, tiles(H, W)) for V, H, W, _ in PAST_THE_FINISH}
    assert reached == {(17, 3, 3): (17, 1), (33, 5, 4): (33, 1), (1, 3, 2049): (1, 65), (1, 3, 2081): (1, 66), (2, 257, 225): (2, 72),
                       (2, 258, 225): (2, 72)}
    views, slots = [r[0] for r in reached.values()], [r[1] for r in reached.values()]
    assert any(FINISH_WAVES < v <= 2 * FINISH_WAVES for v in views) and any(v > 2 * FINISH_WAVES for v in views)
    assert sum(s > WAVE for s in slots) >= 3 and WAVE + 1 in slots        # one lane alone takes a second tile; more do
    assert any(H > 2 * TILE + 1 and W > 2 * TILE + 1 and V > 1 for V, H, W, _ in PAST_THE_FINISH)   # interior tiles, two images
    second_trip = 0                                                       # cases whose tiles from the 65th on hold valid pixels
    for V, H, W, offcentre in PAST_THE_FINISH:
        kw = dict(offcentre=True, scale40=tuple(np.linspace(0.5, 2.0, V)), zero_block=True) if offcentre else {}
        case = nref.image_case(V, H, W, seed=H + W + V, **kw)             # as the GPU test's _image_refs forms it
        nref.check_image_case(case)
        out = nref.consistency(*nref.to(torch.float64, case["normal_map"], case["depth"], case["alpha"], case["views"]))
        ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
        padded = torch.nn.functional.pad(out["valid"], (0, tx * TILE - W, 0, ty * TILE - H))
        per_tile = padded.reshape(V, ty, TILE, tx, TILE).any(4).any(2).reshape(V, ty * tx)     # in the order of the slots
        second_trip += bool(per_tile[:, WAVE:].any(1).all())
        assert len(np.unique(out["per_view"].numpy())) == V               # no two images share a mean: a swap shows
    assert second_trip >= 2


def test_the_builders_keep_every_case_off_its_thresholds():
    for n, V, kw in ((1, 1, {}), (65, 3, dict(quat_scale=1e-3)), (257, 5, dict(quat_scale=1e3, ties="two")),
                     (100, 3, dict(ties="three", scale40=(0.5, 1.0, 2.0)))):
        nref.check_scene_case(nref.scene_case(n, V, seed=n + V, **kw))
    for (H, W) in ((3, 3), (1, 5), (2, 7), (5, 4), (33, 31), (65, 34), (70, 97)):
        for V, kw in ((1, dict(offcentre=False)), (3, dict(offcentre=True, scale40=(0.5, 1.0, 2.0), zero_block=True))):
            case = nref.image_case(V, H, W, seed=H + W + V, **kw)
            nref.check_image_case(case)
            out = nref.consistency(*nref.to(torch.float64, case["normal_map"], case["depth"], case["alpha"], case["views"]))
            assert (int(out["valid"].sum()) > 0) == (H >= 3 and W >= 3), (H, W)
            if H >= 33:      # invalid pixels inside, at the seams and next to the borders; valid ones on both sides of a seam
                v = out["valid"][0]
                assert not v[H // 2, W // 2] and not v[1, 2] and v[5, 31 if W > 33 else 20] and v[min(32, H - 2), 5]
