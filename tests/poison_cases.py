"""Scenes with non-finite and degenerate Gaussians for tests/test_poison_{cpu,gpu}.py.

One seeded make_scene cloud (G = 707 = 11 * 64 + 3 rows, 3 views: 2121 (view, Gaussian) items, more than the 2048 one
k_preprocess workgroup owns; 48 x 48 = 3 x 3 tiles; colour SH degree 2, 4 latent channels of SH degree 1), turned into
rasterizer-boundary inputs (util.boundary_inputs) and EDITED THERE, so that every path (per-view, shared, fused, oracle)
sees the same bits.  The edited rows sit at 0, 63, 64, 65, G - 1 (first / last lane of a wave, first lane of the next, the
tail) and a seeded handful in between, never more than 10 % of the rows.

Classes (``make(cls)``):
  A  non-finite geometry the oracle culls in every view — means: NaN everywhere / NaN in one component / +Inf z / -Inf y;
     covariances: all NaN / one NaN entry / all Inf / 1e30 I / -I / indefinite diag(-1, -1, 0.01) — every such row also
     carries NaN opacity, NaN colour SH and NaN latent SH;
  B  finite but degenerate geometry, the oracle defines the result — covariances: zero / rank 1 / rank 2 / 1e-30 I /
     1e12 I (covers every tile) / 1e18 I; means: the camera centre of view 1, the near-cull plane of view 0 and one ulp
     either side of it;
  C  finite out-of-range opacity on visible rows: 0, -0.5, 1, 2, 1/255 -+ one ulp;
  D  non-finite payload on visible rows (NaN / Inf opacity, NaN in one colour SH coefficient, NaN in one latent channel),
     all of them around pixel (13, 13) so that their rectangles touch at most 4 of the 9 tiles in every view.
  AB the rows of A followed by the rows of B in one scene (the sanitizer run of the oracle).
Every class comes with its CONTROL: the same arrays whose edited rows hold finite values and a mean behind every camera
(benign culling); G, the indices and the workgroup layout are identical.

The dict of a case is util.boundary_inputs' plus ``feature_sh`` (G, C, Kf): the latent harmonics ``features`` was
evaluated from (the fused paths take them instead).  ``features`` is re-evaluated from the edited means / harmonics, by
the same per-Gaussian expression, so the rows that were not edited keep their bits."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from latentsplat_amd.decoder import cuda_splatting as cs
from tests import util

G, VIEWS, SIZE = 707, 3, 48
G_CHUNKS = 64 * 65 + 1          # more than 64 chunks of 64 Gaussians (the camera-gradient reduction)
SEED = 4243                     # the first seed from 4242 whose view-1 camera centre lies in front of views 0 and 2 (z > 0.2 there)
BG = (0.3, 0.1, 0.5)
FX = 0.8                        # make_scene's normalised focal length
NAN, INF = float("nan"), float("inf")
F32 = np.float32
ALPHA_MIN = F32(1.0) / F32(255.0)
NEAR_CULL = F32(0.2)


@dataclass
class Case:
    cls: str
    bi: dict            # the edited boundary inputs
    ctrl: dict          # the control
    rows: np.ndarray    # (n,) edited rows, ascending
    kinds: list         # what each edited row holds
    G: int


def edited_rows(G: int, n: int, seed: int = SEED) -> np.ndarray:
    fixed = [0, 63, 64, 65, G - 1]
    assert len(fixed) <= n <= G // 10
    pool = np.setdiff1d(np.arange(G), fixed)
    extra = np.random.default_rng(seed).choice(pool, n - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, extra])).astype(np.int64)


def _clone(bi: dict) -> dict:
    out = dict(bi)
    for k, t in bi.items():
        if torch.is_tensor(t):
            out[k] = t.clone()
    return out


def base(G: int = G, seed: int = SEED) -> dict:
    sc = util.make_scene(G, image_size=SIZE, views=VIEWS, color_sh_degree=2, feature_channels=4, feature_sh_degree=1, seed=seed)
    bi = util.boundary_inputs(sc, SIZE, SIZE, bg=BG)
    bi["feature_sh"] = sc.feature_sh
    return _clone(bi)


def refresh_features(bi: dict) -> None:
    """``features`` (V, G, C) from the (edited) means and latent harmonics, as boundary_inputs evaluates them."""
    with np.errstate(all="ignore"):
        bi["features"] = cs._payload(bi["means"], bi["cams"].campos, None, bi["feature_sh"][None], True)[3].contiguous()


# ---- geometry in boundary space (view 0 is the identity camera with tan(fov / 2) = 0.5 / FX) ----
def place(u, v, z):
    """mean whose view-0 pixel is (u, v) * SIZE at view-space depth z"""
    return [(u - 0.5) / FX * z, (v - 0.5) / FX * z, z]


def iso(s_px, z):
    """packed isotropic covariance of s_px pixels standard deviation at depth z"""
    s = s_px * z / (FX * SIZE)
    return [s * s, 0.0, 0.0, s * s, 0.0, s * s]


def _eye(x):
    return [x, 0.0, 0.0, x, 0.0, x]


def _variants(cls: str, bi: dict):
    """[(kind, edit)]: ``edit(set_mean, set_cov, row, rng)`` — geometry only; the payload edits follow in make()."""
    S2 = iso(2.0, 6.0)[0]
    vis_mean = lambda rng: place(rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(4.0, 9.0))
    if cls == "A":
        means = [("mean NaN", [NAN, NAN, NAN]), ("mean NaN in y", None), ("mean +Inf z", None), ("mean -Inf y", None)]
        covs = [("cov NaN", [NAN] * 6), ("cov one NaN entry", None), ("cov Inf", [INF] * 6), ("cov 1e30 I", _eye(1e30)),
                ("cov -I", _eye(-1.0)), ("cov indefinite", [-1.0, 0.0, 0.0, -1.0, 0.0, 0.01])]
        out = []
        for kind, m in means:
            def edit(sm, scv, r, rng, kind=kind, m=m):
                mm = vis_mean(rng) if m is None else list(m)
                if kind == "mean NaN in y": mm[1] = NAN
                if kind == "mean +Inf z": mm[2] = INF
                if kind == "mean -Inf y": mm[1] = -INF
                sm(r, mm); scv(r, iso(2.0, 6.0))
            out.append((kind, edit))
        for kind, c in covs:
            def edit(sm, scv, r, rng, kind=kind, c=c):
                cc = iso(2.0, 6.0) if c is None else list(c)
                if kind == "cov one NaN entry": cc[1] = NAN
                sm(r, vis_mean(rng)); scv(r, cc)
            out.append((kind, edit))
        return out
    if cls == "B":
        s = S2 ** 0.5
        v = [s, 0.5 * s, 0.2 * s]
        rank1 = [v[0] * v[0], v[0] * v[1], v[0] * v[2], v[1] * v[1], v[1] * v[2], v[2] * v[2]]
        covs = [("cov zero", [0.0] * 6), ("cov rank 1", rank1), ("cov rank 2", [S2, 0.0, 0.0, S2, 0.0, 0.0]),
                ("cov 1e-30 I", _eye(1e-30)), ("cov 1e12 I", _eye(1e12)), ("cov 1e18 I", _eye(1e18))]
        out = []
        for kind, c in covs:
            out.append((kind, lambda sm, scv, r, rng, c=c: (sm(r, vis_mean(rng)), scv(r, c))))
        centre = [float(x) for x in bi["cams"].campos[1]]
        out.append(("mean at the camera centre of view 1", lambda sm, scv, r, rng: (sm(r, centre), scv(r, iso(2.0, 4.0)))))
        for kind, z in (("mean on the near-cull plane of view 0", NEAR_CULL), ("mean one ulp behind the near-cull plane", np.nextafter(NEAR_CULL, F32(0))),
                        ("mean one ulp in front of the near-cull plane", np.nextafter(NEAR_CULL, F32(1)))):
            out.append((kind, lambda sm, scv, r, rng, z=z: (sm(r, [0.0, 0.0, z]), scv(r, iso(2.0, float(z))))))
        return out
    if cls == "C":
        ops = [("opacity 0", 0.0), ("opacity -0.5", -0.5), ("opacity 1", 1.0), ("opacity 2", 2.0),
               ("opacity 1/255 - ulp", np.nextafter(ALPHA_MIN, F32(0))), ("opacity 1/255 + ulp", np.nextafter(ALPHA_MIN, F32(1)))]
        return [(k, lambda sm, scv, r, rng: (sm(r, vis_mean(rng)), scv(r, iso(2.5, 6.0)))) for k, _ in ops]
    if cls == "D":
        kinds = ["opacity NaN", "opacity Inf", "colour SH one NaN coefficient", "latent SH one NaN channel"]
        near13 = lambda rng: place(rng.uniform(12.5, 14.5) / SIZE, rng.uniform(12.5, 14.5) / SIZE, rng.uniform(5.0, 6.0))
        return [(k, lambda sm, scv, r, rng: (sm(r, near13(rng)), scv(r, iso(1.0, 5.5)))) for k in kinds]
    raise KeyError(cls)


C_OPACITIES = {"opacity 0": 0.0, "opacity -0.5": -0.5, "opacity 1": 1.0, "opacity 2": 2.0,
               "opacity 1/255 - ulp": float(np.nextafter(ALPHA_MIN, F32(0))), "opacity 1/255 + ulp": float(np.nextafter(ALPHA_MIN, F32(1)))}


def make(cls: str, G: int = G, seed: int = SEED) -> Case:
    b = base(G, seed)
    classes = ["A", "B"] if cls == "AB" else [cls]
    variants = [(c, k, e) for c in classes for k, e in _variants(c, b)]
    n = max(len(variants), 5)
    rows = edited_rows(G, n, seed)
    bi, ctrl = _clone(b), _clone(b)
    rng = np.random.default_rng(seed + 1)
    kinds = []

    def set_mean(r, m):
        bi["means"][:, r] = torch.tensor(m, dtype=torch.float32)

    def set_cov(r, c):
        bi["cov6"][:, r] = torch.tensor(c, dtype=torch.float32)

    for k, r in enumerate(rows):
        c, kind, edit = variants[k % len(variants)]
        r = int(r)
        edit(set_mean, set_cov, r, rng)
        if c == "A":
            bi["opac"][r] = NAN
            bi["shs"][r] = NAN
            bi["feature_sh"][r] = NAN
        elif c == "C":
            bi["opac"][r] = C_OPACITIES[kind]
        elif c == "D":
            if kind == "opacity NaN": bi["opac"][r] = NAN
            if kind == "opacity Inf": bi["opac"][r] = INF
            if kind == "colour SH one NaN coefficient": bi["shs"][r, 3, 1] = NAN
            if kind == "latent SH one NaN channel": bi["feature_sh"][r, 2] = NAN
        kinds.append(kind)
        # control: behind every camera, everything else the base scene's finite values
        ctrl["means"][:, r] = torch.tensor([0.05 * k, -0.05 * k, -4.0 - 0.1 * k], dtype=torch.float32)
    refresh_features(bi)
    refresh_features(ctrl)
    return Case(cls, bi, ctrl, rows, kinds, G)


def rows_of(case: Case, prefix: str) -> np.ndarray:
    return np.array([r for r, k in zip(case.rows, case.kinds) if k.startswith(prefix)], np.int64)


def rect_tiles(o: dict, rows, gx: int) -> set:
    """tiles (y * gx + x) inside the oracle's rectangles of ``rows``"""
    out = set()
    for r in rows:
        x0, y0, x1, y1 = (int(t) for t in o["rect"][r])
        out |= {y * gx + x for y in range(y0, y1) for x in range(x0, x1)}
    return out


def write_flat_scene(path, bi: dict) -> None:
    """The flat binary oracle/poison_driver.c reads: int32 header (V, G, H, W, sh_degree, K, C), then per view
    tanfovx tanfovy bg[3] viewmatrix[16] projmatrix[16] campos[3], then means (V,G,3), cov6 (V,G,6), opacities (G),
    shs (G,K,3), features (V,G,C), all float32."""
    c = bi["cams"]
    V, Gn, K, C = bi["V"], bi["means"].shape[1], bi["shs"].shape[1], bi["features"].shape[-1]
    f = lambda t: np.ascontiguousarray(t.detach().numpy(), np.float32).tobytes()
    with open(path, "wb") as fh:
        fh.write(np.array([V, Gn, bi["H"], bi["W"], bi["sh_degree"], K, C], np.int32).tobytes())
        for v in range(V):
            fh.write(np.array([float(c.tan_fov_x[v]), float(c.tan_fov_y[v])], np.float32).tobytes())
            fh.write(f(bi["bg"][v])); fh.write(f(c.view_matrix[v])); fh.write(f(c.full_projection[v])); fh.write(f(c.campos[v]))
        for k in ("means", "cov6", "opac", "shs", "features"):
            fh.write(f(bi[k]))
