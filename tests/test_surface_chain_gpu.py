"""The regularised renders end to end on the MI355X: GaussianScene.render_with_normals, render_with_distortion and
render_surface under ``poses=``, ``transforms=``, ``filter_3d`` and ``antialiasing``, followed by the losses, against ONE
float64 chain of the same composition (tests/surface_chain_ref.py).  One backward over the weighted sum of the terms, so the
gradients of several operators accumulate into the same leaves: ``_xyz`` collects from the rasterizer and the moments,
``_rotation`` from the activation and the normals, the pose tensors from every posed tensor.

The bars: every gradient tensor within ``GRAD_TOL = 1e-3`` of the 2-norm of the float64 tensor (the bar of
tests/test_camera_grads_gpu.py::_kernel_vs_oracle and of the two chain tests this one extends); the consistency term within
``1e-5 max(|want|, 1e-3)`` and the distortion term within ``1e-4 |want|`` (the bars of those two tests); the L1 colour term and
the inverse-depth term, means over the pixels of float32 images like the consistency term, under the bar of that term.
tests/test_surface_chain_cpu.py holds every case used here to the conditions under which a pass means something."""
import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import distortion_ref as dref
from tests import surface_chain_ref as sc

pytestmark = pytest.mark.gpu

GRAD_TOL = sc.GRAD_TOL
RENDERS = ("normals", "distortion", "surface")
IMAGES = {"normals": ("color", "normal_map", "mask", "depth"), "distortion": ("color", "moment_map", "mask", "depth"),
          "surface": ("color", "normal_map", "moment_map", "mask", "depth")}
GEOMETRY = ("xyz", "scaling", "rotation", "opacity")


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int32)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poses(values, dev):
    from latentsplat_amd.pose import PartPoses
    poses = PartPoses(sc.PARTS, learn_scale=True).to(dev)
    with torch.no_grad():
        for p, v in zip((poses.rotation, poses.translation, poses.log_scale), values):
            p.copy_(_t(v, dev))
    return poses


def _setup(name, dev) -> dict:
    """The device side of a case: the scene, the table and every tensor the render and the losses take."""
    case = sc.inputs(name)
    d = dict(case=case, scene=dref.scene_of(case["params"], dev), views=_t(case["views"], dev), kw={})
    for k in ("pivot", "dist_weight", "target", "depth_target", "idx"):
        d[k] = _t(case.get(k), dev)
    if "poses" in case:
        d["poses"] = _poses(case["poses"], dev)
        d["kw"].update(poses=d["poses"], transform_idx=d["idx"])
    if "matrices" in case:
        d["kw"].update(transforms=_t(case["matrices"], dev), transform_idx=d["idx"])
    if "filt" in case:
        d["kw"]["filter_3d"] = _t(case["filt"], dev)
    if case["antialiasing"]:
        d["kw"]["antialiasing"] = True
    return d


def _render(d: dict, kw=None) -> dict:
    """The render of a case, with the case's keywords unless ``kw`` replaces them: name -> image, and ``radii``."""
    case, scene = d["case"], d["scene"]
    render, kw = case["render"], (d["kw"] if kw is None else kw)
    H, W = case["H"], case["W"]
    if render == "normals":
        out = scene.render_with_normals(d["views"], H, W, **kw)
    elif render == "distortion":
        out = scene.render_with_distortion(d["views"], H, W, space=case["space"], pivot=d["pivot"], **kw)
    else:
        out = scene.render_surface(d["views"], H, W, space=case["space"], pivot=d["pivot"], **kw)
    return dict(zip(IMAGES[render] + ("radii",), out))


def _terms(d: dict, img: dict, views=None) -> dict:
    """The terms the case weighs, from the images of one render: name -> scalar tensor."""
    from latentsplat_amd import distortion_loss, normal_consistency_loss
    from latentsplat_amd.depth_sup import inverse_depth_loss
    case, views = d["case"], (d["views"] if views is None else views)
    terms = {}
    if "photo" in case["weights"]:
        terms["photo"] = (img["color"] - d["target"]).abs().mean()
    if "normal" in case["weights"]:
        terms["normal"] = normal_consistency_loss(img["normal_map"], img["depth"], img["mask"], views, case["alpha_min"])
    if "dist" in case["weights"]:
        terms["dist"] = distortion_loss(img["moment_map"], img["mask"], d["dist_weight"])
    if "depth" in case["weights"]:
        terms["depth"] = inverse_depth_loss(img["depth"], img["mask"], views, d["depth_target"])
    return terms


def _total(d: dict, terms: dict) -> torch.Tensor:
    return sum(float(d["case"]["weights"][k]) * terms[k] for k in sc.TERMS if k in terms)


def _check_terms(name, terms, want):
    for k, v in terms.items():
        got, ref = float(v.detach()), want["terms"][k]
        bar = 1e-4 * abs(ref) if k == "dist" else 1e-5 * max(abs(ref), 1e-3)
        print(f"{name} term {k:6s} {got:.7e} against {ref:.7e}  error {abs(got - ref):.2e}  bar {bar:.2e}")
        assert ref > 0 and abs(got - ref) <= bar, (name, k)


def _check_grads(name, got: dict, want: dict):
    """``max |got - want| <= GRAD_TOL ||want||_2`` per tensor; prints the ratio of every tensor first."""
    missed = []
    for k, g in got.items():
        err, norm = float(np.abs(g.detach().cpu().numpy().astype(np.float64) - want[k]).max()), float(np.linalg.norm(want[k]))
        print(f"{name} grad {k:14s} max error {err:.3e}  norm {norm:.3e}  ratio {err / norm:.2e}")
        if not (norm > 0 and err <= GRAD_TOL * norm):
            missed.append(k)
    assert not missed, (name, missed)


def _scene_leaves(d: dict) -> dict:
    names = sc.SCENE if "photo" in d["case"]["weights"] else GEOMETRY
    return {k: getattr(d["scene"], "_" + k) for k in names}


@pytest.mark.parametrize("name", sc.POSED)
def test_pose_and_scene_gradients_against_the_float64_chain(hip_device, name):
    """poses= (3 parts, raw quaternions, learnable scale, an index with rows out of range) through each render and its
    losses: the terms, the gradients of the three pose tensors and those that reach the canonical parameters."""
    d, want = _setup(name, hip_device), sc.reference(name)
    terms = _terms(d, _render(d))
    _check_terms(name, terms, want)
    pose = dict(zip(sc.POSE, (d["poses"].rotation, d["poses"].translation, d["poses"].log_scale)))
    leaves = {**{"pose." + k: v for k, v in pose.items()}, **_scene_leaves(d)}
    got = dict(zip(leaves, torch.autograd.grad(_total(d, terms), list(leaves.values()))))
    _check_grads(name, got, {**{"pose." + k: v for k, v in want["pose_grad"].items()}, **want["grad"]})


@pytest.mark.parametrize("name", sc.TRANSFORMED)
def test_transforms_gradients_against_the_float64_chain(hip_device, name):
    """transforms= (3 similarities with the same index) through each render and its losses: the gradients arrive at the
    canonical parameters through the adjoint of the transform."""
    d, want = _setup(name, hip_device), sc.reference(name)
    terms = _terms(d, _render(d))
    _check_terms(name, terms, want)
    leaves = _scene_leaves(d)
    _check_grads(name, dict(zip(leaves, torch.autograd.grad(_total(d, terms), list(leaves.values())))), want["grad"])


@pytest.mark.parametrize("name", sc.GRID + ("combined",))
def test_unposed_gradients_against_the_float64_chain(hip_device, name):
    """The (filter_3d, antialiasing) grid of the unposed renders, one case per render with slot 40 != 1, and ``combined``: one
    backward over photometric + 0.05 consistency + 100 distortion + depth, where an operator whose gradient failed to
    accumulate into ``_xyz`` or ``_rotation`` next to the others' misses by far more than the bar (the CPU test measures each
    term's part)."""
    d, want = _setup(name, hip_device), sc.reference(name)
    terms = _terms(d, _render(d))
    _check_terms(name, terms, want)
    leaves = _scene_leaves(d)
    _check_grads(name, dict(zip(leaves, torch.autograd.grad(_total(d, terms), list(leaves.values())))), want["grad"])


@pytest.mark.parametrize("render", RENDERS)
def test_identity_poses_render_the_bits_of_the_unposed_call(hip_device, render):
    d = _setup(f"poses-{render}-layered", hip_device)
    identity = _poses(([[1.0, 0, 0, 0]] * sc.PARTS, np.zeros((sc.PARTS, 3)), np.zeros(sc.PARTS)), hip_device)
    with torch.no_grad():
        posed = _render(d, dict(poses=identity, transform_idx=d["idx"]))
        plain = _render(d, {})
        moved = _render(d)
    for k in IMAGES[render] + ("radii",):
        assert np.array_equal(_bits(posed[k]), _bits(plain[k])), k
    assert float(plain["mask"].max()) > 0.5
    assert not np.array_equal(_bits(moved[IMAGES[render][1]]), _bits(plain[IMAGES[render][1]]))     # the case's own poses move it


def test_render_surface_with_poses_is_the_explicit_composition(hip_device):
    """pose_scene -> activate_scene -> gaussian_normals / gaussian_depth_moments -> cat -> rasterize_views: the same bits."""
    from latentsplat_amd import gaussian_depth_moments, gaussian_normals
    from latentsplat_amd.pose import pose_scene
    from latentsplat_amd.rasterizer import rasterize_views
    from latentsplat_amd.scene_model import activate_scene
    for name in ("poses-surface-layered", "poses-surface-scene500"):
        d = _setup(name, hip_device)
        case, scene, P = d["case"], d["scene"], d["poses"]
        with torch.no_grad():
            got = _render(d)
            xyz, rest, scaling, rotation = pose_scene(scene._xyz, scene._features_rest, scene._scaling, scene._rotation,
                                                      P.rotation, P.translation, P.log_scale, d["idx"])
            shs, opacities, cov = activate_scene(scene._features_dc, rest, scene._opacity, scaling, rotation)
            normals = gaussian_normals(d["views"], xyz, scaling, rotation)
            moments = gaussian_depth_moments(d["views"], xyz, case["space"], d["pivot"])
            color, feature, mask, depth, radii = rasterize_views(d["views"], case["H"], case["W"], scene.active_sh_degree, xyz, cov,
                                                                 opacities, shs=shs, features=torch.cat((normals, moments), -1))
        want = dict(color=color, normal_map=feature[:, :3], moment_map=feature[:, 3:], mask=mask, depth=depth, radii=radii)
        for k, v in want.items():
            assert np.array_equal(_bits(got[k]), _bits(v)), (name, k)
        assert float(got["normal_map"].abs().max()) > 0.1 and float(got["moment_map"].abs().max()) > 0


@pytest.mark.parametrize("name", sc.TABLE)
def test_a_table_that_requires_grad_is_refused_and_detached_gives_the_rasterizers_gradient(hip_device, name):
    """render_with_normals / render_surface refuse a table that requires grad.  With ``views.detach()`` for the operators and
    the leaf for the render, the table receives the rasterizer's gradient alone: the float64 chain with every operator's own
    reading of the table cut.  The tensor the bar is taken over is a view's record: a single block of it can be zero by
    symmetry (the first camera of ``forward_views`` stands at the origin, where the scene scale in slot 40 is a homothety about
    the camera and moves no pixel: 3e-9 in float64 against blocks of 5e-2), and no float32 result is within 1e-3 of that."""
    from latentsplat_amd import gaussian_depth_moments, gaussian_normals
    from tests.test_camera_grads_gpu import BLOCKS
    d = _setup(name, hip_device)
    case, scene = d["case"], d["scene"]
    leaf = d["views"].clone().requires_grad_(True)
    with pytest.raises(_lib.LsrError, match="views requires grad"):
        _render(dict(d, views=leaf))
    payload = [gaussian_normals(leaf.detach(), scene._xyz, scene._scaling, scene._rotation)]
    if case["render"] == "surface":
        payload.append(gaussian_depth_moments(leaf.detach(), scene._xyz, case["space"], d["pivot"]))
    color, feature, mask, depth, _ = scene.render(leaf, case["H"], case["W"], features=torch.cat(payload, -1))
    img = dict(color=color, normal_map=feature[:, :3], moment_map=feature[:, 3:], mask=mask, depth=depth)
    with pytest.raises(_lib.LsrError, match="views requires grad"):
        _terms(d, img, leaf)
    terms = _terms(d, img, leaf.detach())
    want = sc.reference(name, sc.TABLE_EDGES, True)
    _check_terms(name, terms, want)
    got, = torch.autograd.grad(_total(d, terms), leaf)
    got, ref = got.cpu().numpy().astype(np.float64), want["views_grad"]
    assert not got[:, 41:].any() and not ref[:, 41:].any()
    for v in range(got.shape[0]):
        for block, sl in BLOCKS.items():
            err, norm = float(np.abs(got[v, sl] - ref[v, sl]).max()), float(np.linalg.norm(ref[v, sl]))
            print(f"{name} view {v} {block:7s} max error {err:.3e}  norm {norm:.3e}")
        err, norm = float(np.abs(got[v] - ref[v]).max()), float(np.linalg.norm(ref[v]))
        print(f"{name} grad views[{v}]      max error {err:.3e}  norm {norm:.3e}  ratio {err / norm:.2e}")
        assert norm > 0 and err <= GRAD_TOL * norm, (name, v)
