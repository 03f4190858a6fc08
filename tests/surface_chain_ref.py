"""The composed objective of the geometric regularisers in float64 on the host: what ``GaussianScene.render_with_normals``,
``render_with_distortion`` and ``render_surface`` compute, followed by the losses, as ONE torch autograd chain that is
assembled only from restatements the suite already has:

  * the posed parameters: ``pose_grad_ref.forward`` (differentiable in the poses); matrices go through ``transform_ref.split``
    / ``transform_ref.quaternion`` first and are constants;
  * the activation: ``scene_params_ref.forward64``, or ``filter3d_ref.forward64`` under a 3D filter;
  * the payloads: ``normals_ref.gaussian_normals`` and ``distortion_ref.depth_moments``;
  * the render: ``oracle.torch_oracle.rasterize`` per view, with its ``antialiasing`` flag;
  * the terms: ``normals_ref.consistency``, ``distortion_ref.distortion``, ``depth_sup_ref.loss_statement`` and, for the
    colour, the plain L1 ``mean |colour - target|``.

:func:`chain` returns every term, the weighted sum and its gradients with respect to the scene parameters, the three pose
tensors and, when asked, the view table.  ``detach`` cuts single edges of the graph: what a test uses to show that an edge
matters (the sensitivity conditions of tests/test_surface_chain_cpu.py) and to state the partial table gradient a caller
asks for with ``views.detach()``.

The module also holds the cases tests/test_surface_chain_gpu.py runs (:data:`CASES`), so that the CPU test can hold every
one of them to its conditions without a GPU, and :func:`reference`, the cached float64 result of a case."""
from __future__ import annotations

import functools
from math import isqrt

import numpy as np
import torch

from tests import depth_sup_ref as sup
from tests import distortion_ref as dref
from tests import filter3d_ref as fref
from tests import normals_ref as nref
from tests import pose_grad_ref as pref
from tests import scene_params_ref as sref
from tests import transform_ref as tref

GRAD_TOL = 1e-3      # max |got - want| <= GRAD_TOL ||want||_2 per tensor (tests/test_camera_grads_gpu.py::_kernel_vs_oracle)
SENSITIVITY = 10.0   # an edge matters when cutting it moves a gradient tensor by at least SENSITIVITY x GRAD_TOL of its norm
SCENE = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
POSE = ("rotation", "translation", "log_scale")
TERMS = ("photo", "normal", "dist", "depth")
# the edges `detach` can cut
EDGES = ("normals->rotation", "moments->xyz", "normals.views", "consistency.views", "moments.views", "depth.views")


def _t64(a, grad: bool = False) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, np.float64).copy()).requires_grad_(grad)


def poses_of_matrices(matrices: np.ndarray):
    """``(p (T, 4), t (T, 3), ls (T,))`` float64 of similarities ``(T, 4, 4)``: ``transform_ref``'s reading of a matrix."""
    p, t, ls = [], [], []
    for M in np.asarray(matrices, np.float64).reshape(-1, 4, 4):
        s, R, tr = tref.split(M)
        p.append(tref.quaternion(R))
        t.append(tr)
        ls.append(np.log(s))
    return np.stack(p), np.stack(t), np.asarray(ls)


def chain(params: dict, views: np.ndarray, H: int, W: int, weights: dict, *, poses=None, matrices=None, idx=None, filt=None,
          antialiasing: bool = False, space: str = "ndc", pivot=None, alpha_min: float = 0.3, dist_weight=None, target=None,
          depth_target=None, depth_weight=None, depth_alpha_min: float = 0.01, views_leaf: bool = False, detach=(),
          grads: bool = True) -> dict:
    """The objective ``sum_k weights[k] * term_k`` over the terms named in ``weights`` (:data:`TERMS`) in float64.

    ``params``: the six canonical raw tensors (numpy).  ``poses = (p, t, ls)`` (``ls`` may be ``None``) or ``matrices (T, 4,
    4)``, with ``idx`` (out of range: not moved), pose the scene first.  ``filt (n, 1)``: the 3D filter inside the activation.
    ``views (V, 44)``: the table; ``views_leaf`` makes it a leaf whose every slot is an independent variable.  ``space`` /
    ``pivot``: the moments'.  ``alpha_min``: the consistency loss's.  ``dist_weight (V, H, W)``: the distortion loss's pixel
    weights.  ``target (V, 3, H, W)``: the colour target.  ``depth_target`` / ``depth_weight`` / ``depth_alpha_min``: the
    inverse-depth loss's (``align="given"`` with no affine, ``normalize="pixels"``: the defaults of ``inverse_depth_loss``).
    ``detach``: edges of :data:`EDGES` to cut.

    Returns ``terms`` (name -> float), ``total``, ``maps`` (the rendered images and the distortion map, numpy) and, with
    ``grads``, ``grad`` (name of :data:`SCENE` -> numpy), ``pose_grad`` (name of :data:`POSE` -> numpy; only with ``poses``)
    and ``views_grad`` (only with ``views_leaf``)."""
    from oracle import torch_oracle as TO
    assert set(weights) <= set(TERMS) and set(detach) <= set(EDGES) and not (poses is not None and matrices is not None)
    t = {k: _t64(params[k], grads) for k in SCENE}
    rec = _t64(views, grads and views_leaf)
    cut = lambda x, edge: x.detach() if edge in detach else x
    pose = None
    xyz, rest, scaling, rotation = t["xyz"], t["features_rest"], t["scaling"], t["rotation"]
    if poses is not None or matrices is not None:
        if poses is not None:
            pose = [_t64(poses[0], grads), _t64(poses[1], grads), None if poses[2] is None else _t64(poses[2], grads)]
        else:
            pose = [_t64(a) for a in poses_of_matrices(matrices)]
        xyz, rest, scaling, rotation = pref.forward(xyz, rest, scaling, rotation, *pose, idx)
    posed = dict(t, xyz=xyz, features_rest=rest, scaling=scaling, rotation=rotation)
    act = sref.forward64(posed) if filt is None else fref.forward64(posed, _t64(filt).reshape(-1, 1))
    payload, at = [], {}
    if "normal" in weights:
        at["normal"] = (0, 3)
        payload.append(nref.gaussian_normals(cut(rec, "normals.views"), xyz, scaling, cut(rotation, "normals->rotation")))
    if "dist" in weights:
        at["dist"] = (3 * len(payload), 3 * len(payload) + 2)
        payload.append(dref.depth_moments(cut(rec, "moments.views"), cut(xyz, "moments->xyz"), space,
                                          None if pivot is None else _t64(pivot)))
    features = torch.cat(payload, -1) if payload else None
    degree = isqrt(1 + t["features_rest"].shape[1]) - 1
    images = []
    for v in range(rec.shape[0]):
        r, s = rec[v], rec[v, 40]
        color, feat, mask, depth, _ = TO.rasterize(H, W, r[35], r[36], r[37:40], r[0:16], r[16:32], r[32:35], degree, xyz * s,
                                                   act["cov3D"] * s * s, act["opacities"], shs=act["shs"],
                                                   features=None if features is None else features[v], antialiasing=antialiasing)
        images.append((color, feat, mask[0], depth[0]))
    color, alpha, depth = (torch.stack([m[i] for m in images]) for i in (0, 2, 3))
    feat = None if features is None else torch.stack([m[1] for m in images])
    terms, maps = {}, dict(color=color, alpha=alpha, depth=depth)
    if "photo" in weights:
        terms["photo"] = (color - _t64(target)).abs().mean()
    if "normal" in weights:
        maps["normal_map"] = feat[:, at["normal"][0]:at["normal"][1]]
        terms["normal"] = nref.consistency(maps["normal_map"], depth, alpha, cut(rec, "consistency.views"), alpha_min)["loss"]
    if "dist" in weights:
        maps["moment_map"] = feat[:, at["dist"][0]:at["dist"][1]]
        out = dref.distortion(maps["moment_map"], alpha, None if dist_weight is None else _t64(dist_weight))
        terms["dist"], maps["distortion"] = out["loss"], out["distortion"]
    if "depth" in weights:
        terms["depth"] = sup.loss_statement(depth, alpha, cut(rec, "depth.views"), _t64(depth_target),
                                            None if depth_weight is None else _t64(depth_weight), alpha_min=depth_alpha_min)["loss"]
    total = sum(float(weights[k]) * terms[k] for k in TERMS if k in weights)
    res = dict(terms={k: float(v.detach()) for k, v in terms.items()}, total=float(total.detach()),
               maps={k: v.detach().numpy() for k, v in maps.items()})
    if grads:
        leaves = dict(t)
        if poses is not None:
            leaves.update({"pose." + k: p for k, p in zip(POSE, pose) if p is not None})
        if views_leaf:
            leaves["views"] = rec
        got = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
        g = {k: (np.zeros(tuple(leaf.shape)) if v is None else v.numpy()) for (k, leaf), v in zip(leaves.items(), got)}
        res["grad"] = {k: g[k] for k in SCENE}
        if poses is not None:
            res["pose_grad"] = {k: g["pose." + k] for k in POSE if "pose." + k in g}
        if views_leaf:
            res["views_grad"] = g["views"]
    return res


# ---- the scenes and the cases ----

PARTS = 3
ALPHA_MIN = 0.3
NEAR, FAR = dref.NEAR, dref.FAR


def cube_scene(n: int, seed: int) -> dict:
    """The scene of tests/test_normals_gpu.py (``_scene``) as raw parameters: n Gaussians in a cube around the origin."""
    p = sref.make_params(n, 4, seed=seed)
    rng = np.random.default_rng(seed)
    p["xyz"] = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    p["scaling"] = np.log(rng.uniform(0.03, 0.12, (n, 3))).astype(np.float32)
    p["opacity"] = rng.uniform(0.0, 3.0, (n, 1)).astype(np.float32)
    return p


def circle_views(seed: int, scale40=1.0) -> np.ndarray:
    """2 cameras of ``normals_ref.make_views`` with near / far in slots 42 / 43 (NATIVE: the rasterizer does not read them)."""
    views = nref.make_views(2, seed=seed, scale=scale40)
    views[:, 42], views[:, 43] = NEAR, FAR
    return views


def part_poses(seed: int):
    """float32 poses of :data:`PARTS` parts near the identity: quaternions NOT normalised (norms 0.5 .. 2), learnable scale."""
    rng = np.random.default_rng(seed)
    p = np.array([1.0, 0.0, 0.0, 0.0]) + 0.08 * rng.standard_normal((PARTS, 4))
    p *= rng.uniform(0.5, 2.0, (PARTS, 1)) / np.linalg.norm(p, axis=1, keepdims=True)
    t = 0.08 * rng.standard_normal((PARTS, 3))
    ls = 0.06 * rng.standard_normal(PARTS)
    return p.astype(np.float32), t.astype(np.float32), ls.astype(np.float32)


def part_index(n: int, seed: int) -> np.ndarray:
    """int32 ``(n,)`` drawn from -1 .. PARTS: both ends are out of range, and those rows are not moved."""
    idx = np.random.default_rng(seed).integers(-1, PARTS + 1, n).astype(np.int32)
    assert set(idx.tolist()) == set(range(-1, PARTS + 1))
    return idx


def part_matrices(seed: int) -> np.ndarray:
    """The float32 similarities of :func:`part_poses`, as a caller of ``transforms=`` builds them."""
    p, t, ls = part_poses(seed)
    out = []
    for k in range(PARTS):
        R = pref.rotation(torch.from_numpy(p[k].astype(np.float64))).numpy()
        out.append(tref.matrix(R, t[k].astype(np.float64), float(np.exp(np.float64(ls[k])))))
    return np.stack(out)


# What every case fixes.  The weights of the terms are part of the case: the CPU test holds every term and every edge to
# its sensitivity condition under them.
# The 0.05 of the training tools would leave the normals' own path (normals -> rotation -> pose quaternion) at 0.4 % of the
# quaternion gradient under the other three terms, below the condition; the posed and table cases of render_surface weigh
# the consistency term 0.5, where it is 4 %.
COMBINED = dict(photo=1.0, normal=0.05, dist=100.0, depth=1.0)
WEIGHTS = {"normals": dict(normal=1.0), "distortion": dict(dist=1.0), "surface": dict(COMBINED, normal=0.5)}
SCENES = {"scene500": dict(H=48, W=40), "layered": dict(H=32, W=32)}


def _case(render, scene, mode, scale40=1.0, space="ndc", filtered=False, antialiasing=False, seed=0, weights=None):
    return dict(render=render, scene=scene, mode=mode, scale40=scale40, space=space, filtered=filtered,
                antialiasing=antialiasing, seed=seed, weights=dict(WEIGHTS[render] if weights is None else weights))


CASES = {
    # poses= through the three renders (tests 'pose and scene gradients', 'identity poses', 'explicit composition')
    "poses-normals-scene500": _case("normals", "scene500", "poses", scale40=(0.5, 2.5)),
    "poses-normals-layered": _case("normals", "layered", "poses"),
    "poses-distortion-scene500": _case("distortion", "scene500", "poses", space="linear"),
    "poses-distortion-layered": _case("distortion", "layered", "poses", scale40=(2.5, 0.5)),
    "poses-surface-scene500": _case("surface", "scene500", "poses", space="disparity"),
    "poses-surface-layered": _case("surface", "layered", "poses", scale40=(0.5, 2.5)),
    # transforms= through the three renders
    "transforms-normals-layered": _case("normals", "layered", "transforms", scale40=(2.5, 0.5)),
    "transforms-distortion-scene500": _case("distortion", "scene500", "transforms"),
    "transforms-surface-layered": _case("surface", "layered", "transforms"),
    # the option grid of the unposed chains: (filter_3d, antialiasing), one case per render with slot 40 != 1
    "plain-normals-FF": _case("normals", "layered", None, scale40=(0.5, 2.5)),
    "plain-normals-FT": _case("normals", "layered", None, antialiasing=True),
    "plain-normals-TF": _case("normals", "layered", None, filtered=True),
    "plain-normals-TT": _case("normals", "scene500", None, filtered=True, antialiasing=True),
    "plain-distortion-FT": _case("distortion", "layered", None, antialiasing=True, scale40=(2.5, 0.5)),
    "plain-distortion-TF": _case("distortion", "scene500", None, filtered=True, space="linear"),
    "plain-surface-FT": _case("surface", "scene500", None, antialiasing=True, scale40=(0.5, 2.5)),
    "plain-surface-TF": _case("surface", "layered", None, filtered=True),
    # one backward over photometric + 0.05 consistency + 100 distortion + depth
    "combined": _case("surface", "layered", None, weights=COMBINED),
    # the table as a leaf: the partial gradient a caller asks for with views.detach()
    "table-normals": _case("normals", "layered", "table"),
    "table-surface": _case("surface", "layered", "table"),
}
POSED = tuple(k for k, c in CASES.items() if c["mode"] == "poses")
TRANSFORMED = tuple(k for k, c in CASES.items() if c["mode"] == "transforms")
GRID = tuple(k for k in CASES if k.startswith("plain-"))
TABLE = tuple(k for k, c in CASES.items() if c["mode"] == "table")
TABLE_EDGES = ("normals.views", "consistency.views", "moments.views", "depth.views")


def filter_of(params: dict, views: np.ndarray, W: int) -> np.ndarray:
    """``(n, 1)`` float32: the 3D filter of the positions for ``views`` (``filter3d_ref.filter_ref``), which the GPU test
    passes as ``filter_3d`` and the chain takes as ``filt``: both sides use the same numbers."""
    return fref.filter_ref(params["xyz"], views, W)["filter"].astype(np.float32).reshape(-1, 1)


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """Everything a case consists of, as float32 / int32 numpy arrays: what the device call and the chain both start from."""
    c = CASES[name]
    H, W = SCENES[c["scene"]]["H"], SCENES[c["scene"]]["W"]
    if c["scene"] == "scene500":
        params, views = cube_scene(500, 2 + c["seed"]), circle_views(6 + c["seed"], c["scale40"])
        point = (0.0, 0.0, 0.0)
    else:
        params, views = dref.layered_params(200, 7 + c["seed"], 2.0, 6.0), dref.forward_views(2, c["scale40"])
        point = (0.0, 0.0, 4.0)
    n = params["xyz"].shape[0]
    rng = np.random.default_rng(100 + c["seed"])
    out = dict(c, H=H, W=W, params=params, views=views, alpha_min=ALPHA_MIN)
    if c["mode"] in ("poses", "transforms"):
        out["idx"] = part_index(n, 5 + c["seed"])
        out["poses" if c["mode"] == "poses" else "matrices"] = part_poses(9 + c["seed"]) if c["mode"] == "poses" else \
            part_matrices(9 + c["seed"])
    if c["filtered"]:
        out["filt"] = filter_of(params, views, W)
    w = c["weights"]
    if "dist" in w:
        out["pivot"] = dref.pivot_of(views, point, c["space"])
        out["dist_weight"] = rng.uniform(0.0, 1.0, (2, H, W)).astype(np.float32)
    if "photo" in w:
        out["target"] = rng.uniform(0.0, 1.0, (2, 3, H, W)).astype(np.float32)
    if "depth" in w:
        # an inverse depth of the scenes' range (both stand about 4 from their cameras) where a target exists; 0 (no target) at three pixels in ten
        tgt = rng.uniform(0.15, 0.4, (2, H, W))
        tgt[rng.random((2, H, W)) < 0.3] = 0.0
        out["depth_target"] = tgt.astype(np.float32)
    return out


def chain_kwargs(case: dict) -> dict:
    keys = ("poses", "matrices", "idx", "filt", "antialiasing", "space", "pivot", "alpha_min", "dist_weight", "target",
            "depth_target")
    return {k: case[k] for k in keys if k in case}


@functools.lru_cache(maxsize=None)
def reference(name: str, detach: tuple = (), views_leaf: bool = False) -> dict:
    """The float64 result of a case, computed once per process and left unchanged by its readers."""
    case = inputs(name)
    return chain(case["params"], case["views"], case["H"], case["W"], case["weights"], detach=detach, views_leaf=views_leaf,
                 **chain_kwargs(case))


def moved(full: np.ndarray, partial: np.ndarray) -> float:
    """How far cutting an edge moves a gradient tensor: the largest difference over the tensor's 2-norm (the measure of
    :data:`GRAD_TOL`)."""
    return float(np.abs(full - partial).max() / np.linalg.norm(full))


def share(full: np.ndarray, partial: np.ndarray) -> float:
    """``||full - partial||_2 / ||full||_2``: the share of a gradient that an omitted dependence carries."""
    return float(np.linalg.norm(full - partial) / np.linalg.norm(full))
