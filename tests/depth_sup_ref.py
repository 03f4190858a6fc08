"""Depth supervision (latentsplat_amd/depth_sup.py, include/lsr_depth_loss.h) restated for the tests: the targets as plain
Python loops in float64, the loss as one torch statement evaluated in float64 (the reference) and in float32 (the "stock"
composition a user would write with PyTorch: the error yardstick), the case builder, and a capture writer with 2D
observations.

The error rule is that of tests/normals_ref.py (:func:`held`, imported from there): per quantity, the kernel's largest error
against float64 is at most ``max(MARGIN = 4 x the stock composition's own largest error, 2^-20 x max |want|)``.

The case builder guarantees that a float32 kernel and the float64 reference take the same branch everywhere, so no pixel is
excluded from a comparison (:func:`check_loss_case` asserts it):
  * every alpha is at least 1e-2 away from ``alpha_min``;
  * every unplanted residual has ``|r| >= 1e-3 max |I|`` under the float64 ``(a, b)``: no sign hangs on a rounding;
  * a fit is at least 100 x clear of its refusal threshold, unless the case plants a refusal."""
import math
import os

import numpy as np
import torch

from tests import colmap_ref as cr
from tests.normals_ref import FLOOR, MARGIN, VIEW_FLOATS, WORST, held       # noqa: F401  (the project's rule, re-exported)

ALPHA_MIN = 0.05
FIT_THRESHOLD = 2.0 ** -24
SCALES = (0.5, 1.0, 2.5)


# ---- section 2: the targets ----

def rotation_of(qvec) -> np.ndarray:
    return cr.qvec_to_rotmat(np.asarray(qvec, np.float64))


def sparse_inverse_depth_loop(xyz_of_id: dict, observed_ids, qvec, tvec, H: int, W: int, fx: float, fy: float, near: float) -> np.ndarray:
    """One observation at a time, in Python floats (float64)."""
    R, t = rotation_of(qvec), np.asarray(tvec, np.float64)
    out = [[0.0] * W for _ in range(H)]
    for pid in observed_ids:
        x, y, z = (float(c) for c in xyz_of_id[int(pid)])
        px, py, pz = (float(R[k, 0]) * x + float(R[k, 1]) * y + float(R[k, 2]) * z + float(t[k]) for k in range(3))
        if pz <= near:
            continue
        j, i = math.floor(fx * px / pz + W / 2), math.floor(fy * py / pz + H / 2)
        if not (0 <= j < W and 0 <= i < H):
            continue
        out[i][j] = max(out[i][j], 1.0 / pz)
    return np.array(out, np.float64).astype(np.float32)


def align_ref(sparse: np.ndarray, prior: np.ndarray):
    a, b = np.asarray(sparse, np.float64), np.asarray(prior, np.float64)
    both = (a > 0) & (b > 0)
    a, b = a[both], b[both]
    if a.size <= 10 or not a.max() - a.min() > 1e-3:
        return 0.0, 0.0
    ta, tb = np.median(a), np.median(b)
    scale = np.mean(np.abs(a - ta)) / np.mean(np.abs(b - tb))
    return float(scale), float(ta - tb * scale)


# ---- section 3: the loss ----

def inverse_depth_map(depth: torch.Tensor, alpha: torch.Tensor, views: torch.Tensor, alpha_min: float):
    """``(I, ok)`` in the dtype of the inputs; differentiable in depth and alpha where ``ok``."""
    s = views[:, 40].reshape(-1, 1, 1)
    ok = (alpha > alpha_min) & (depth > 0) & torch.isfinite(alpha) & torch.isfinite(depth)
    d, a = torch.where(ok, depth, torch.ones_like(depth)), torch.where(ok, alpha, torch.zeros_like(alpha))
    return torch.where(ok, s * a / d, torch.zeros_like(depth)), ok


def weights_of(target: torch.Tensor, weight) -> torch.Tensor:
    return weight if weight is not None else (target > 0).to(target.dtype)


def fit_sums(I: torch.Tensor, target: torch.Tensor, w: torch.Tensor) -> dict:
    sm = lambda x: x.sum((1, 2))
    return dict(count=sm((w > 0).to(I.dtype)), Sw=sm(w), St=sm(w * target), SI=sm(w * I), Stt=sm(w * target * target), StI=sm(w * target * I))


def fit_affine(I: torch.Tensor, target: torch.Tensor, w: torch.Tensor):
    """``(affine (V, 2), clearance (V,))``: the weighted least squares of the header from its five sums, in the dtype of the
    inputs, and det / (Sw Stt) over the refusal threshold (inf-safe: 0 where nothing weighs in)."""
    m = fit_sums(I.detach(), target, w)
    det = m["Sw"] * m["Stt"] - m["St"] * m["St"]
    ok = (m["count"] >= 2) & (m["Sw"] > 0) & (det > FIT_THRESHOLD * (m["Sw"] * m["Stt"]))
    safe = torch.where(ok, det, torch.ones_like(det))
    a = torch.where(ok, (m["Sw"] * m["StI"] - m["St"] * m["SI"]) / safe, torch.zeros_like(det))
    b = torch.where(ok, (m["SI"] - a * m["St"]) / torch.where(ok, m["Sw"], torch.ones_like(det)), torch.zeros_like(det))
    good = ok & torch.isfinite(a) & torch.isfinite(b) & (a != 0)
    a, b = torch.where(good, a, torch.zeros_like(a)), torch.where(good, b, torch.zeros_like(b))
    denom = m["Sw"] * m["Stt"]
    clearance = torch.where(denom > 0, det / torch.where(denom > 0, denom, torch.ones_like(denom)), torch.zeros_like(det)) / FIT_THRESHOLD
    return torch.stack([a, b], -1), clearance


def loss_statement(depth, alpha, views, target, weight=None, affine=None, align="given", normalize="pixels", alpha_min=ALPHA_MIN) -> dict:
    """Section 3 in the dtype of the inputs: ``loss``, ``per_view``, ``inverse_depth``, ``affine``."""
    V, H, W = depth.shape
    I, _ = inverse_depth_map(depth, alpha, views, alpha_min)
    w = weights_of(target, weight)
    if align == "fit":
        ab = fit_affine(I, target, w)[0]
    elif affine is None:
        ab = torch.tensor([1.0, 0.0], dtype=depth.dtype).repeat(V, 1)
    else:
        ab = affine
    ab = ab.detach()
    a, b = ab[:, 0].reshape(-1, 1, 1), ab[:, 1].reshape(-1, 1, 1)
    r = w * (I - (a * target + b))
    N = torch.full((V,), float(H * W), dtype=depth.dtype) if normalize == "pixels" else w.sum((1, 2))
    usable = (ab[:, 0] != 0) & (N > 0)
    per_view = torch.where(usable, r.abs().sum((1, 2)) / torch.where(usable, N, torch.ones_like(N)), torch.zeros_like(N))
    return dict(loss=per_view.mean(), per_view=per_view, inverse_depth=I, affine=ab)


def to(dt, *arrays):
    return [None if a is None else torch.from_numpy(np.asarray(a)).to(dt) for a in arrays]


def loss_and_grads(case: dict, dt, grad_loss: float = 1.0, grad_per_view=None) -> dict:
    """The statement and its gradients under ``grad_loss * loss + <grad_per_view, per_view>``, in ``dt``, as float64 numpy."""
    depth, alpha, views, target, weight, affine = to(dt, case["depth"], case["alpha"], case["views"], case["target"], case["weight"],
                                                     case["affine"])
    depth.requires_grad_(True)
    alpha.requires_grad_(True)
    out = loss_statement(depth, alpha, views, target, weight, affine, case["align"], case["normalize"], case["alpha_min"])
    total = out["loss"] * grad_loss
    if grad_per_view is not None:
        total = total + (out["per_view"] * torch.from_numpy(np.asarray(grad_per_view)).to(dt)).sum()
    if total.requires_grad:
        total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = {k: v.detach().double().numpy() for k, v in out.items()}
    res["loss"] = res["loss"].reshape(1)
    res.update(grad_depth=zero(depth).double().numpy(), grad_alpha=zero(alpha).double().numpy())
    return res


# ---- the case builder ----

def loss_case(V: int, H: int, W: int, seed: int, align: str = "given", normalize: str = "pixels", weighted: bool = False,
              plant: bool = True, zero_row=None, flat_row=None, alpha_min: float = ALPHA_MIN) -> dict:
    """float32 arrays ``depth, alpha, target (V, H, W)``, ``views (V, 44)``, ``weight`` or None, ``affine (V, 2)`` or None that
    meet the conditions of the module docstring (asserted before returning).  The surface is z = 2 .. 4 under alpha in
    [0.3, 0.99], rendered as ``depth = s z alpha`` with the slot-40 scales 0.5, 1, 2.5 in turn; the target is the affine
    preimage of ``1 / z`` plus an error of either sign and of 0.005 to 0.008.  ``plant``: pixels with depth 0,
    negative, NaN, +inf, and alpha 0, below the gate, NaN, +inf (``planted`` marks them).  ``zero_row``: a view whose given
    row is (0, 0); ``flat_row``: a view whose target is constant (a fit must refuse it)."""
    refusals = set(v for v in (flat_row,) if v is not None)
    for attempt in range(200):
        rng = np.random.default_rng(seed + 7919 * attempt)
        views = rng.standard_normal((V, VIEW_FLOATS)).astype(np.float32)
        scale = np.array([SCALES[v % 3] for v in range(V)], np.float64)
        views[:, 40] = scale
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        depth, alpha, target = (np.empty((V, H, W), np.float32) for _ in range(3))
        weight = np.empty((V, H, W), np.float32) if weighted else None
        affine = np.empty((V, 2), np.float32)
        planted = np.zeros((V, H, W), bool)
        for v in range(V):
            ph = rng.uniform(0, 6.28, 3)
            z = 3.0 + 0.6 * np.sin(0.31 * xs + ph[0]) * np.cos(0.23 * ys + ph[1]) + 0.3 * rng.uniform(-1, 1, (H, W))
            al = 0.645 + 0.3 * np.sin(0.17 * xs + 0.11 * ys + ph[2]) + 0.04 * rng.uniform(-1, 1, (H, W))
            alpha[v] = al
            depth[v] = scale[v] * z * alpha[v].astype(np.float64)
            a0, b0 = rng.uniform(0.5, 2.0), rng.uniform(-0.05, 0.1)
            affine[v] = (a0, b0)
            # (small against the spread of 1 / z, 0.26 .. 0.48: a least-squares fit then moves the residuals by less than they are)
            err = rng.uniform(0.005, 0.008, (H, W)) * rng.choice([-1.0, 1.0], (H, W))
            t = (1.0 / z + err - float(affine[v, 1])) / float(affine[v, 0])
            if weighted:
                wv = rng.uniform(0.2, 1.0, (H, W))
                wv[rng.random((H, W)) < 0.25] = 0.0
                weight[v] = wv
            else:
                t[rng.random((H, W)) < 0.3] = 0.0                   # a sparse target: > 0 is the mask
            target[v] = t
        if flat_row is not None:
            target[flat_row] = 0.75
        if zero_row is not None:
            affine[zero_row] = 0.0
        if plant and H * W >= 12:
            flat = rng.permutation(H * W)[:8]
            for k, at in enumerate(flat):
                for v in range(V):
                    i, j = divmod(int(at + v) % (H * W), W)
                    planted[v, i, j] = True
                    if k < 4:
                        depth[v, i, j] = (0.0, -1.5, np.nan, np.inf)[k]
                    else:
                        alpha[v, i, j] = (0.0, alpha_min - 0.02, np.nan, np.inf)[k - 4]
        case = dict(depth=depth, alpha=alpha, views=views, target=target, weight=weight, affine=None if align == "fit" else affine,
                    align=align, normalize=normalize, alpha_min=alpha_min, planted=planted, refusals=refusals | ({zero_row} - {None}))
        if H * W < 2 and align == "fit":
            case["refusals"] = set(range(V))                       # one pixel: nothing to fit
        if _conditions(case) is None:
            return case
    raise AssertionError(("no case meets the conditions", V, H, W, seed, _conditions(case)))


def _conditions(case: dict):
    """None, or the first condition of the module docstring the case misses."""
    al = case["alpha"].astype(np.float64)
    finite = np.isfinite(al)
    if not (np.abs(al[finite] - case["alpha_min"]) >= 1e-2).all():
        return "alpha"
    depth, alpha, views, target, weight, affine = to(torch.float64, case["depth"], case["alpha"], case["views"], case["target"],
                                                     case["weight"], case["affine"])
    I, ok = inverse_depth_map(depth, alpha, views, case["alpha_min"])
    w = weights_of(target, weight)
    if case["align"] == "fit":
        ab, clearance = fit_affine(I, target, w)
        for v in range(depth.shape[0]):
            if v in case["refusals"]:
                if float(ab[v, 0]) != 0.0 or not float(clearance[v]) <= 1e-2:
                    return "a planted refusal that is not clear"
            elif not float(clearance[v]) >= 100.0:
                return "fit"
    else:
        ab = affine if affine is not None else torch.tensor([1.0, 0.0], dtype=torch.float64).repeat(depth.shape[0], 1)
    r = I - (ab[:, :1, None] * target + ab[:, 1:, None])
    live = (w > 0) & ok & ~torch.from_numpy(case["planted"]) & (ab[:, 0] != 0).reshape(-1, 1, 1)
    if bool(live.any()) and not float(r.abs()[live].min()) >= 1e-3 * float(I.abs().max()):
        return "residual"
    return None


def check_loss_case(case: dict) -> None:
    assert _conditions(case) is None, _conditions(case)


# ---- a capture with observations ----

def sample_model_with_points(seed: int = 0) -> dict:
    """``colmap_ref.sample_model`` with every observation's point id mapped onto an id the model has (the sample draws
    0 .. 6, the points are numbered otherwise)."""
    model = cr.sample_model(seed)
    ids = [p["id"] for p in model["points"]]
    for im in model["images"]:
        im["points2D"] = [(x, y, pid if pid == 2 ** 64 - 1 else ids[pid]) for x, y, pid in im["points2D"]]
    return model


def expected_observations(model: dict):
    """``(offsets, xy, ids)`` of the observations with a point, in file order."""
    offsets, xy, ids = [0], [], []
    for im in model["images"]:
        for x, y, pid in im["points2D"]:
            if pid != 2 ** 64 - 1:
                xy.append((x, y))
                ids.append(pid)
        offsets.append(len(ids))
    return np.array(offsets, np.int64), np.array(xy, np.float64).reshape(-1, 2), np.array(ids, np.uint64)


def write_capture_with_observations(root, c2w, cameras, camera_of, photographs, names, points_xyz, points_rgb, observed, fmt="bin",
                                    sparse="sparse/0") -> dict:
    """``colmap_ref.write_capture``, then the model files again with image ``k`` observing the points ``observed[k]`` (rows
    of ``points_xyz``; the measured position is the row number, twice: the readers keep it, the targets do not use it) and
    one observation without a point in front."""
    model = cr.write_capture(root, c2w, cameras, camera_of, photographs, names, points_xyz, points_rgb, fmt=fmt, sparse=sparse)
    for k, im in enumerate(model["images"]):
        im["points2D"] = [(0.5, 0.25, 2 ** 64 - 1)] + [(float(r), float(r) + 0.5, model["points"][int(r)]["id"]) for r in observed[k]]
    cr.write_files(os.path.join(str(root), sparse), cr.binary_files(model) if fmt == "bin" else cr.text_files(model))
    return model


def with_observation(model: dict, k: int, obs) -> dict:
    """``model`` with the observation ``obs = (x, y, point id)`` appended to image ``k``."""
    images = [dict(im) for im in model["images"]]
    images[k] = dict(images[k], points2D=list(images[k]["points2D"]) + [obs])
    return {**model, "images": images}


def write_check_set(directory) -> int:
    """The set of ``colmap_ref.write_check_set`` plus models whose observations the new walk must read or refuse: what
    ``make -C latentsplat_amd/csrc colmap-check MODELS=DIR`` runs over."""
    n = cr.write_check_set(directory)
    good = sample_model_with_points()
    text = cr.text_files(good)
    extra = {"obs_bin": cr.binary_files(good), "obs_txt": text,
             "obs_nan_bin": cr.binary_files(with_observation(good, 0, (float("nan"), 0.0, 3))),
             "obs_inf_txt": cr.text_files(with_observation(good, 2, (0.0, float("-inf"), 2 ** 64 - 1))),
             "obs_incomplete_txt": {**text, "images.txt": _append_to_observations(text["images.txt"], b" 1.5")},
             "obs_long_token_txt": {**text, "images.txt": _append_to_observations(text["images.txt"], b" " + b"9" * 2000)},
             "obs_count_2_61_bin": {**cr.binary_files(good), "images.bin": _huge_observation_count(good)}}
    for label, files in extra.items():
        cr.write_files(os.path.join(str(directory), label), files)
    return n + len(extra)


def _append_to_observations(images_txt: bytes, tail: bytes) -> bytes:
    """images.txt with ``tail`` appended to the observation line of the first image that has observations."""
    lines = images_txt.split(b"\n")
    records = [k for k, line in enumerate(lines) if line and not line.startswith(b"#")]
    at = next(k for k in records if len(lines[k].split()) % 3 == 0 and len(lines[k].split()) != 10)
    return b"\n".join(lines[:at] + [lines[at] + tail] + lines[at + 1:])


def _huge_observation_count(model: dict) -> bytes:
    """images.bin with the LAST image's observation count replaced by 2^61 (its own observations still follow)."""
    import struct
    last = dict(model["images"][-1], points2D=[(1.0, 2.0, model["points"][0]["id"])])
    body = cr.binary_files({**model, "images": model["images"][:-1] + [last]})["images.bin"]
    return body[:-32] + struct.pack("<Q", 2 ** 61) + body[-24:]


if __name__ == "__main__":
    import sys
    print(f"{write_check_set(sys.argv[1])} model directories written to {sys.argv[1]}")
