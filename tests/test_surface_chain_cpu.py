"""The float64 chain of the composed objective (tests/surface_chain_ref.py) held to itself, and the conditions under which
tests/test_surface_chain_gpu.py means anything, without a GPU: the chain gives the numbers of the two chains it replaces;
its pose gradients are the central differences of the objective; in every GPU case every term is alive and every edge the
case exists for carries at least 10 x GRAD_TOL of the gradient it feeds (so that a kernel that dropped the edge could not
pass); the share of the view table's gradient that the normal regulariser's operators used to leave out, measured; and the
refusals that replace that silent omission."""
import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import distortion_ref as dref
from tests import filter3d_ref as fref
from tests import normals_ref as nref
from tests import scene_params_ref as sref
from tests import surface_chain_ref as sc

BAR = sc.SENSITIVITY * sc.GRAD_TOL


# ---- the two chains this one replaces, as they stood ----

def _old_normals_chain(params, filt, views, H, W, antialiasing, alpha_min):
    from oracle import torch_oracle as TO
    t = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in params.items()}
    rec = torch.from_numpy(views.astype(np.float64))
    act = fref.forward64(t, torch.from_numpy(filt.astype(np.float64)).reshape(-1, 1))
    normals = nref.gaussian_normals(rec, t["xyz"], t["scaling"], t["rotation"])
    maps = []
    for v in range(rec.shape[0]):
        r, s = rec[v], rec[v, 40]
        _, feat, mask, depth, _ = TO.rasterize(H, W, r[35], r[36], r[37:40], r[0:16], r[16:32], r[32:35], 0, t["xyz"] * s,
                                               act["cov3D"] * s * s, act["opacities"], features=normals[v], antialiasing=antialiasing)
        maps.append((feat, mask[0], depth[0]))
    N, alpha, depth = (torch.stack([m[i] for m in maps]) for i in range(3))
    loss = nref.consistency(N, depth, alpha, rec, alpha_min)["loss"]
    loss.backward()
    return float(loss.detach()), {k: t[k].grad.numpy() for k in ("xyz", "scaling", "rotation", "opacity")}


def _old_distortion_chain(params, views, H, W, space, pivot, weight):
    from oracle import torch_oracle as TO
    t = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in params.items()}
    rec = torch.from_numpy(views.astype(np.float64))
    act = sref.forward64(t)
    moments = dref.depth_moments(rec, t["xyz"], space, torch.from_numpy(np.asarray(pivot, np.float64)))
    maps = []
    for v in range(rec.shape[0]):
        r, s = rec[v], rec[v, 40]
        _, feat, mask, _, _ = TO.rasterize(H, W, r[35], r[36], r[37:40], r[0:16], r[16:32], r[32:35], 0, t["xyz"] * s,
                                           act["cov3D"] * s * s, act["opacities"], features=moments[v])
        maps.append((feat, mask[0]))
    mm, alpha = torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps])
    out = dref.distortion(mm, alpha, torch.from_numpy(np.asarray(weight, np.float64)))
    out["loss"].backward()
    return (float(out["loss"].detach()), out["distortion"].detach().numpy(), mm.detach().numpy(),
            {k: t[k].grad.numpy() for k in ("xyz", "scaling", "rotation", "opacity")})


def _same(got, want, show):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max()), show


def _identity(n, seed):
    p = np.zeros((sc.PARTS, 4), np.float32)
    p[:, 0] = 1.0
    return (p, np.zeros((sc.PARTS, 3), np.float32), np.zeros(sc.PARTS, np.float32)), sc.part_index(n, seed)


@pytest.mark.parametrize("filtered,antialiasing", [(False, False), (True, True)])
def test_the_chain_gives_the_old_normals_chain(filtered, antialiasing):
    """The scene, views and size of test_normals_gpu.py::test_scene_gradients_against_the_float64_chain; also under identity
    poses, which move nothing."""
    params, views, H, W = sc.cube_scene(2000, 4), nref.make_views(2, seed=8), 48, 40
    filt = sc.filter_of(params, views, W) if filtered else np.zeros((2000, 1), np.float32)
    want_loss, want = _old_normals_chain(params, filt, views, H, W, antialiasing, 0.3)
    poses, idx = _identity(2000, 1)
    for kw in (dict(), dict(poses=poses, idx=idx)):
        if kw and filtered:
            continue                      # (a posed scene takes no filter_3d)
        got = sc.chain(params, views, H, W, dict(normal=1.0), filt=filt, antialiasing=antialiasing, alpha_min=0.3, **kw)
        _same(got["terms"]["normal"], want_loss, "loss")
        for k in want:
            _same(got["grad"][k], want[k], k)
        assert want_loss > 1e-3 and not got["grad"]["features_rest"].any()


def test_the_chain_gives_the_old_distortion_chain():
    """The scene, views and size of test_distortion_gpu.py::test_scene_gradients_against_the_float64_chain."""
    params, views, H, W = dref.layered_params(200, 7, 2.0, 6.0), dref.forward_views(2), 48, 40
    weight = np.random.default_rng(1).uniform(0.0, 1.0, (2, H, W)).astype(np.float32)
    poses, idx = _identity(200, 2)
    for space in dref.SPACES:
        pivot = dref.pivot_of(views, (0.0, 0.0, 4.0), space)
        want = _old_distortion_chain(params, views, H, W, space, pivot, weight)
        _same(dref.float64_chain(params, views, H, W, space, pivot, weight)[0], want[0], space)
        for kw in (dict(), dict(poses=poses, idx=idx)):
            got = sc.chain(params, views, H, W, dict(dist=1.0), space=space, pivot=pivot, dist_weight=weight, **kw)
            _same(got["terms"]["dist"], want[0], space)
            _same(got["maps"]["distortion"], want[1], space)
            _same(got["maps"]["moment_map"], want[2], space)
            for k in want[3]:
                _same(got["grad"][k], want[3][k], (space, k))
            if kw:                        # the identity is a pose like any other: it has a gradient
                assert all(np.abs(got["pose_grad"][k]).max() > 0 for k in sc.POSE)


# ---- the pose gradients are those of the objective ----

FD_STEP = 1e-6
FD_TOL = 1e-6     # relative.  The sweep on this case (all four terms, each alone, the three coordinates): at h = 1e-6 and 1e-7
                  # the central difference is within 1.8e-7 of autograd at worst (2.9e-9, 1.1e-8, 1.9e-11, 8.2e-10 for the
                  # quaternion under photo / normal / dist / depth at 1e-6); at 1e-5 and above a quaternion step crosses a
                  # discontinuity of the render (a 1 / 255 gate, a rectangle) and the difference is off by O(1); at 1e-8 the
                  # cancellation in the difference reaches 1e-6.  1e-6 at h = 1e-6 is 5 x the worst agreement seen.


def _leading_alpha(case, res) -> float:
    """``mean over views of sum_valid alpha / (H W)``: the part of the consistency loss whose gradient the regulariser leaves
    out by definition (the leading alpha of e is a constant weight).  A finite difference sees it; autograd does not."""
    m = res["maps"]
    t = torch.from_numpy
    valid = nref.consistency(t(m["normal_map"]), t(m["depth"]), t(m["alpha"]), t(case["views"].astype(np.float64)),
                             case["alpha_min"])["valid"].numpy()
    return float((valid * m["alpha"]).sum((1, 2)).mean() / (case["H"] * case["W"]))


@pytest.mark.parametrize("tensor,at", [("rotation", (1, 2)), ("translation", (0, 1)), ("log_scale", (2,))])
def test_pose_gradients_are_central_differences_of_the_objective(tensor, at):
    name = "poses-surface-layered"
    case, want = sc.inputs(name), sc.reference(name)["pose_grad"][tensor][at]
    which = sc.POSE.index(tensor)

    def objective(step):
        poses = [a.astype(np.float64) for a in case["poses"]]
        poses[which][at] += step
        res = sc.chain(case["params"], case["views"], case["H"], case["W"], case["weights"], grads=False,
                       **dict(sc.chain_kwargs(case), poses=poses))
        return res["total"] - case["weights"]["normal"] * _leading_alpha(case, res)

    fd = (objective(FD_STEP) - objective(-FD_STEP)) / (2 * FD_STEP)
    print(f"{tensor}{at}: central difference {fd:.9e}  autograd {want:.9e}  relative {abs(fd - want) / abs(want):.2e}")
    assert abs(want) > 1e-4 and abs(fd - want) <= FD_TOL * abs(want)


# ---- the conditions of the GPU cases ----

@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_every_term_of_every_case_is_alive(name):
    res = sc.reference(name, (), sc.CASES[name]["mode"] == "table")
    print(name, res["terms"])
    assert set(res["terms"]) == set(sc.CASES[name]["weights"]) and all(v > 0 for v in res["terms"].values())
    if "normal" in res["terms"]:
        assert res["terms"]["normal"] > 1e-3
    reached = [k for k in sc.SCENE if "photo" in res["terms"] or not k.startswith("features")]
    assert all(np.linalg.norm(res["grad"][k]) > 0 for k in reached)
    if sc.CASES[name]["mode"] in ("poses", "transforms"):
        idx = sc.inputs(name)["idx"]
        assert ((idx < 0) | (idx >= sc.PARTS)).sum() > 10 and all((idx == k).sum() > 10 for k in range(sc.PARTS))
    if sc.CASES[name]["mode"] == "poses":
        p = sc.inputs(name)["poses"][0]
        assert np.abs(np.linalg.norm(p, axis=1) - 1).min() > 0.05          # quaternions that are not normalised


def test_the_cases_cover_what_the_issue_lists():
    c = sc.CASES
    for render in ("normals", "distortion", "surface"):
        assert any(v["render"] == render and v["mode"] == "poses" and v["scale40"] != 1.0 for v in c.values())
        assert any(v["render"] == render and v["mode"] == "transforms" for v in c.values())
        assert any(v["render"] == render and v["mode"] is None and v["scale40"] != 1.0 for v in c.values())
        for scene in sc.SCENES:
            assert any(v["render"] == render and v["mode"] == "poses" and v["scene"] == scene for v in c.values())
    grid = lambda render: {(v["filtered"], v["antialiasing"]) for k, v in c.items() if k in sc.GRID and v["render"] == render}
    assert grid("normals") == {(False, False), (False, True), (True, False), (True, True)}
    assert grid("distortion") >= {(False, True), (True, False)} and grid("surface") >= {(False, True), (True, False)}
    assert c["combined"]["weights"] == dict(photo=1.0, normal=0.05, dist=100.0, depth=1.0)
    for v in c.values():
        s = np.broadcast_to(np.asarray(v["scale40"], np.float64), (2,))
        assert set(s.tolist()) <= {0.5, 1.0, 2.5}


@pytest.mark.parametrize("name", sc.POSED)
def test_the_operators_own_paths_carry_the_pose_gradients(name):
    """normals -> posed rotation -> pose quaternion, and moments -> posed xyz -> every pose tensor: cutting either in the chain
    moves the pose gradients it feeds by at least 10 x GRAD_TOL of their norm.  A device path that lost one cannot pass."""
    full, w = sc.reference(name)["pose_grad"], sc.CASES[name]["weights"]
    assert all(np.linalg.norm(full[k]) > 0 for k in sc.POSE)
    if "normal" in w:
        cut = sc.reference(name, ("normals->rotation",))["pose_grad"]
        moved = {k: sc.moved(full[k], cut[k]) for k in sc.POSE}
        print(name, "normals -> rotation:", {k: f"{v:.4f}" for k, v in moved.items()})
        assert moved["rotation"] >= BAR
        assert moved["translation"] == 0 and moved["log_scale"] == 0       # the path ends in the quaternion alone
    if "dist" in w:
        cut = sc.reference(name, ("moments->xyz",))["pose_grad"]
        moved = {k: sc.moved(full[k], cut[k]) for k in sc.POSE}
        print(name, "moments -> xyz:", {k: f"{v:.4f}" for k, v in moved.items()})
        assert all(v >= BAR for v in moved.values())


@pytest.mark.parametrize("name", sc.TRANSFORMED)
def test_the_operators_own_paths_carry_the_canonical_gradients(name):
    """Under ``transforms=`` the same two paths end in the canonical ``_rotation`` and ``_xyz``."""
    full, w = sc.reference(name)["grad"], sc.CASES[name]["weights"]
    if "normal" in w:
        assert sc.moved(full["rotation"], sc.reference(name, ("normals->rotation",))["grad"]["rotation"]) >= BAR
    if "dist" in w:
        assert sc.moved(full["xyz"], sc.reference(name, ("moments->xyz",))["grad"]["xyz"]) >= BAR


def test_every_term_of_the_combined_objective_weighs_in():
    """photometric + 0.05 consistency + 100 distortion + depth: each term alone holds at least 10 x GRAD_TOL of every
    geometric gradient of the sum, so an operator whose gradient failed to accumulate into a shared leaf shows."""
    case, full = sc.inputs("combined"), sc.reference("combined")["grad"]
    for term in sc.TERMS:
        alone = sc.chain(case["params"], case["views"], case["H"], case["W"], {term: case["weights"][term]},
                         **sc.chain_kwargs(case))["grad"]
        part = {k: float(np.abs(alone[k]).max() / np.linalg.norm(full[k])) for k in ("xyz", "scaling", "rotation", "opacity")}
        print(term, {k: f"{v:.3f}" for k, v in part.items()})
        assert all(v >= BAR for v in part.values()), term
    assert np.linalg.norm(full["features_rest"]) > 0 and np.linalg.norm(full["features_dc"]) > 0


# ---- the view table ----

def test_the_share_of_the_table_gradient_the_normal_regulariser_left_out():
    """render_with_normals -> normal_consistency_loss on ``layered_params(200, 7, 2.0, 6.0)`` under ``forward_views(2)`` at
    32 x 32, alpha_min 0.3, the table a leaf.  The full gradient has norm 0.1898; without the two operators' own dependence
    on the table 0.1893; the two differ by 26.9 % of the full norm (12 % over the view matrices, 35 % over the projections).
    Per operator: gaussian_normals alone 30.2 %, normal_consistency_loss alone 41.2 % (the two partly cancel).  Each is far
    above 10 x GRAD_TOL = 1 %: camera gradients through these operators were wrong, not merely inexact."""
    full = sc.reference("table-normals", (), True)["views_grad"]
    cut = {e: sc.reference("table-normals", e, True)["views_grad"]
           for e in (("normals.views",), ("consistency.views",), ("normals.views", "consistency.views"))}
    both = cut[("normals.views", "consistency.views")]
    shares = {" + ".join(e): sc.share(full, g) for e, g in cut.items()}
    print(f"norm {np.linalg.norm(full):.4f} partial {np.linalg.norm(both):.4f}", {k: f"{v:.4f}" for k, v in shares.items()},
          f"view matrices {sc.share(full[:, :16], both[:, :16]):.3f} projections {sc.share(full[:, 16:32], both[:, 16:32]):.3f}")
    assert abs(np.linalg.norm(full) - 0.1898) < 1e-4 and abs(np.linalg.norm(both) - 0.1893) < 1e-4
    assert abs(shares["normals.views + consistency.views"] - 0.269) < 1e-3
    assert abs(sc.share(full[:, :16], both[:, :16]) - 0.12) < 5e-3 and abs(sc.share(full[:, 16:32], both[:, 16:32]) - 0.35) < 5e-3
    assert all(sc.moved(full, g) >= BAR for g in cut.values())


def test_every_operator_leaves_out_more_of_the_table_gradient_than_the_bar():
    """render_surface with the four terms: what each of gaussian_normals, normal_consistency_loss, gaussian_depth_moments
    (which always refused) and inverse_depth_loss contributes to the table gradient through its own reading of the table."""
    full = sc.reference("table-surface", (), True)["views_grad"]
    for edge in sc.TABLE_EDGES:
        cut = sc.reference("table-surface", (edge,), True)["views_grad"]
        print(f"{edge:18s} share {sc.share(full, cut):.4f}  largest entry / norm {sc.moved(full, cut):.4f}")
        assert sc.moved(full, cut) >= BAR, edge
    # the scale in slot 40 is the only slot inverse_depth_loss reads
    cut = sc.reference("table-surface", ("depth.views",), True)["views_grad"]
    assert np.array_equal(np.delete(full, 40, axis=1), np.delete(cut, 40, axis=1)) and (full[:, 40] != cut[:, 40]).all()


def test_a_table_that_requires_grad_is_refused_before_any_device_check():
    """CPU tensors: without the flag the operators refuse the device; with it they refuse the table first."""
    from latentsplat_amd import gaussian_normals, normal_consistency_loss
    from latentsplat_amd.depth_sup import inverse_depth_loss
    case = nref.scene_case(5, 2, seed=1)
    views, xyz, scaling, rotation = nref.to(torch.float32, *(case[k] for k in ("views", "xyz", "scaling", "rotation")))
    img = nref.image_case(2, 5, 4, seed=1)
    N, depth, alpha, iviews = nref.to(torch.float32, *(img[k] for k in ("normal_map", "depth", "alpha", "views")))
    leaf = lambda t: t.clone().requires_grad_(True)
    calls = {"gaussian_normals": lambda v: gaussian_normals(v, xyz, scaling, rotation),
             "normal_consistency_loss": lambda v: normal_consistency_loss(N, depth, alpha, v, 0.5),
             "inverse_depth_loss": lambda v: inverse_depth_loss(depth, alpha, v, torch.ones_like(depth))}
    for who, call in calls.items():
        table = views if who == "gaussian_normals" else iviews
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            call(table)
        with pytest.raises(_lib.LsrError, match=who + ": views requires grad.*pass views.detach\\(\\); the rasterizer hands"):
            call(leaf(table))
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            call(leaf(table).detach())
