"""Cases, seeds and bars of the antialiased gradients against the float64 oracle (tests/test_antialias_grads_{cpu,gpu}.py;
DESIGN.md §2.21): every ``k_preprocess_bwd<PARTS, FMA, CAM, AA = true>`` instance and every input layout of the projection
backward, 32 x 32 with 150-200 Gaussians.

Bars (``hold``).  The reference is autograd through ``oracle.torch_oracle.rasterize(antialiasing=True)`` in float64; "stock" is
the same with ``rho_dtype=torch.float32`` (only the factor from float32 casts: the error a float32 statement of rho makes by
itself, the project's 4 x rule, tests/antialias_ref.py ``MARGIN``); "constant" detaches the factor (a backward WITHOUT rho's
term).
  * view record, per view and per block as ``_kernel_vs_oracle`` has it: err <= max(TOL x block norm, 4 x stock error);
  * inputs, per tensor: err <= max(CLEAN_TOL x max |want|, 4 x stock error).
Every case must be able to tell (``preconditions``, CPU only): the C oracle's forward under the mode has no fragile
evaluation, and the "constant" oracle lies at least 10 bars from the oracle proper for means, cov and the vm and tanfov
blocks of every view (and the scale block where the case is about it).

Measured on the MI355X (all 16 cases pass; worst over the cases).  Kernel error / bar: near 0.29, means 0.19, features 0.14,
cov 0.13, opac 0.13, colours 0.09, shs / feature_sh 0.04, scale 0.035, every other block of the record <= 0.006.  Kernel error
/ stock error: means 32, cov 28, opac 19, features 28, colours 16, shs 14, feature_sh 18; vm 36, tanfov 36, pm 123, campos 85,
bg 179, near 378, far 1104, scale 1929 — far above 4 everywhere, and that is what this stock statement must give: it rounds
ONE quantity to float32, the factor (2^-24 relative per (view, Gaussian); pm, campos, bg, near, far do not depend on rho at
all, and the scale block of a camera near the origin hardly), while the kernels run the whole chain in float32 — projection,
conic, exponent, blend, the atomic moment sums.  Their error against the float64 oracle is the classic mode's against the
same oracle (1e-6 ... 4e-6 of a tensor's largest entry, 1e-6 ... 3e-4 of a block's norm), which is what TOL and CLEAN_TOL are
for; the 4 x stock term never binds here, so the first term of each bar is the check.  It is tight enough: a backward
without rho's term sits 25 ... 580 bars away, and the three mutants of DESIGN.md §2.21 fail 3, 16 and 16 of the 16 cases."""
from __future__ import annotations

import functools

import numpy as np
import torch

from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.synthetic import make_scene
from oracle import torch_oracle as TO
from tests import antialias_ref as ref
from tests import camera_grad_cases as cases
from tests.test_parity_gpu import CLEAN_TOL

TOL = 1e-3                 # tests/test_camera_grads_gpu.py _kernel_vs_oracle
SEPARATION = 10.0
SUB_PIXEL = dict(sigma_px=(0.05, 0.6), opacity_scale=0.9)     # rho far from 1: its term dominates
BLOCKS = dict(vm=slice(0, 16), pm=slice(16, 32), campos=slice(32, 35), tanfov=slice(35, 37), bg=slice(37, 40), scale=slice(40, 41))
DEPTH_BLOCKS = dict(near=slice(42, 43), far=slice(43, 44))

# Scene seeds, searched on the CPU: the first for which ``preconditions`` holds (no fragile evaluation of the C oracle's
# forward fed o rho; 10-bar separation).  The classic table (camera_grad_cases.SEEDS) is not used under the mode.
# (Searched from 300 upwards, the A4 pair from (300, 340); only the clamped case needed a second try: seed 300 is free of
# fragile evaluations but separates the vm block of view 0 by 6 bars only.)
SEEDS = {"V1": 300, "V3": 300, "V5": 300, "A1": 300, "A2": 300, "A2-depth": 300, "A4": (300, 340), "A4-depth": (300, 340),
         "A5": 300, "scale": 300, "floor": 300, "clamped": 301}
INSTANCES = ("V1", "V1-contraction", "V3", "V3-contraction", "V5", "V5-contraction")
LAYOUTS = ("A1", "A2", "A2-contraction", "A2-depth", "A4", "A4-depth", "A5")
NAMES = INSTANCES + LAYOUTS + ("scale", "floor", "clamped")
PARTS = {"V1": 1, "V3": 2, "V5": 4, "A1": 4, "A2": 4, "A4": 4, "A5": 4, "scale": 4, "floor": 1, "clamped": 2}
NEEDLES = 12               # per population of the floor case


def _seed(name):
    return SEEDS[name] if name in SEEDS else SEEDS[name.replace("-contraction", "")]


def _direct_case(sc, contraction=False):
    """precomputed colour + 4 direct features, packed covariances, shared by the views"""
    G = sc.means.shape[0]
    cp = torch.rand(G, 3, generator=torch.Generator().manual_seed(G))
    feats = sc.feature_sh[..., 0].contiguous()
    return cases.Case(cases.cams32(sc), 32, 32, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                      dict(colors_precomp=cp, features=feats), None, 4, contraction=contraction)


def _instances(V, contraction, seed):
    """V = 1 / 3 / 5 shared views of sub-pixel splats: parts = 1 / 2 / 4; with the contraction the FMA instances"""
    return _direct_case(make_scene(160, image_size=32, views=V, seed=seed, color_sh_degree=None, feature_channels=4, **SUB_PIXEL),
                        contraction)


def _scale(seed):
    """near = 0.5 ... 0.8 per view, as the "scaled" case of tests/test_antialias_gpu.py: scale slots 2, 1.67, 1.43, 1.25 over
    the unscaled means.  The cameras are moved off the origin: the projected covariance seen from a camera AT the origin is
    invariant under the scene scale (means s x, covariances s^2 Sigma: the same picture), so rho would have no scale term there
    — view 0 of make_scene sits exactly at the origin."""
    sc = make_scene(160, image_size=32, views=4, seed=seed, color_sh_degree=None, feature_channels=4, **SUB_PIXEL)
    sc.near = torch.tensor([0.5, 0.6, 0.7, 0.8])
    sc.extrinsics = sc.extrinsics.clone()
    sc.extrinsics[:, :3, 3] += torch.tensor([0.2, -0.15, 0.25])
    c = _direct_case(sc)
    assert float((c.views[:, 40] - 1.0).abs().min()) > 0.2 and float(c.views[:, 40].max() - c.views[:, 40].min()) > 0.5
    return c


def needle_ratio(below: bool) -> float:
    """det0 / det of the two needle populations: a factor 2.5 below / above the floor"""
    return ref.FLOOR / 2.5 if below else ref.FLOOR * 2.5


def _floor(seed):
    """One view at the identity (scale slot 1): 160 ordinary Gaussians, then NEEDLES axis-aligned needles below the floor and
    NEEDLES above it (rows 160 .., 160 + NEEDLES ..): 3 px long, the thin axis chosen so that det0 / det is needle_ratio(),
    alternately along x and y, world covariance diag(.., .., 0) (b = 0 exactly at the identity, off the axis too), centred within
    0.2 px of a pixel row / column so that o' G passes 1/255 somewhere, opacity 0.95."""
    H = W = 32
    sc = make_scene(160, image_size=32, views=1, seed=seed, color_sh_degree=None, feature_channels=4)
    sc.near = torch.ones(1)
    gen = torch.Generator().manual_seed(seed)
    n = 2 * NEEDLES
    tan = 0.5 / float(sc.intrinsics[0, 0, 0])
    f = W / (2.0 * tan)
    z = 2.0 + 2.0 * torch.rand(n, generator=gen, dtype=torch.float64)
    cell = torch.randint(4, 28, (n, 2), generator=gen).double()
    along_x = torch.arange(n) % 2 == 0
    long_off, thin_off = torch.rand(n, generator=gen, dtype=torch.float64) - 0.5, 0.4 * torch.rand(n, generator=gen, dtype=torch.float64) - 0.2
    px = cell[:, 0] + torch.where(along_x, long_off, thin_off)
    py = cell[:, 1] + torch.where(along_x, thin_off, long_off)
    mean = torch.stack([((2 * px + 1) / W - 1) * tan * z, ((2 * py + 1) / H - 1) * tan * z, z], -1)
    long2 = 9.0
    k = (long2 + ref.LOWPASS) / long2
    r = torch.tensor([needle_ratio(True)] * NEEDLES + [needle_ratio(False)] * NEEDLES, dtype=torch.float64)
    thin2 = ref.LOWPASS * r * k / (1.0 - r * k)
    world = (z / f) ** 2
    cov = torch.zeros(n, 3, 3, dtype=torch.float64)
    cov[:, 0, 0] = torch.where(along_x, torch.full_like(z, long2), thin2) * world
    cov[:, 1, 1] = torch.where(along_x, thin2, torch.full_like(z, long2)) * world
    sc.means = torch.cat([sc.means, mean.float()])
    sc.covariances = torch.cat([sc.covariances, cov.float()])
    sc.opacities = torch.cat([sc.opacities, torch.full((n,), 0.95)])
    sc.feature_sh = torch.cat([sc.feature_sh, 0.3 * torch.randn(n, 4, 1, generator=gen)])
    return _direct_case(sc)


def _clamped(seed):
    """util.make_edge_scene("outside"), V = 2, colour SH degree 2: visible Gaussians whose EWA Jacobian is clamped (120 filler
    Gaussians instead of the classic case's 200: 160 in all)"""
    from tests import util
    sc, _ = util.make_edge_scene("outside", H=32, W=32, views=2, seed=seed, color_sh_degree=2, feature_channels=None, filler=120)
    return cases._colour_case(sc, 2, 32, 32)


def build(name, seed=None):
    seed = _seed(name) if seed is None else seed
    base = name.replace("-contraction", "")
    con = name.endswith("-contraction")
    if base in ("V1", "V3", "V5"):
        c = _instances(int(base[1]), con, seed)
    elif base == "A1":
        c = cases._a1(seed=seed)
    elif base in ("A2", "A2-depth"):
        c = cases._a2(contraction=con, mode=cases.MODE if base == "A2-depth" else None, seed=seed)
    elif base in ("A4", "A4-depth"):
        c = cases._a4(mode=cases.MODE if base == "A4-depth" else None, seed=seed)
    elif base == "A5":
        c = cases._a5(seed=seed)
    elif base == "scale":
        c = _scale(seed)
    elif base == "floor":
        c = _floor(seed)
    elif base == "clamped":
        c = _clamped(seed)
    else:
        raise KeyError(name)
    c.name = name
    c.parts = PARTS[base.replace("-depth", "")]
    c.sub_pixel = base in ("V1", "V3", "V5", "scale")
    c.rho_blocks = ("vm", "tanfov") + (("scale",) if base == "scale" else ())
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name)


def blocks_of(c):
    return dict(BLOCKS, **DEPTH_BLOCKS) if c.mode is not None else BLOCKS


def factors(c, dtype=None):
    """(V, G) rho of the case through the oracle's own statement, no grad"""
    out = []
    with torch.no_grad():
        for v in range(c.V):
            _, m, c6, _ = cases.view_inputs(c.views, v, c.means, c.cov, c.opac, c.scenes)
            rec = c.views[v].double()
            out.append(TO.opacity_factor(c.H, c.W, rec[35], rec[36], rec[0:16], m * rec[40], c6 * rec[40] ** 2, dtype=dtype))
    return torch.stack(out)


def payload_of(c):
    from tests.test_camera_grads_gpu import _payload_of
    return _payload_of({k: (v.double() if torch.is_tensor(v) else v) for k, v in c.kw.items()})


def forwards(c):
    return cases.oracle_forwards(c.views, c.H, c.W, c.means, c.cov, c.opac, payload_of(c), c.scenes, antialiasing=True)


def oracle_grads(c, rho_dtype):
    from tests.test_camera_grads_gpu import _oracle_grads
    return _oracle_grads(c.views, c.H, c.W, c.means, c.cov, c.opac, c.kw, c.C, c.scenes, antialiasing=True, rho_dtype=rho_dtype)


@functools.lru_cache(maxsize=None)
def references(name):
    """(want, stock, constant) gradient dicts of the case: computed once, shared, never modified"""
    c = case(name)
    return tuple(oracle_grads(c, rd) for rd in (None, torch.float32, "constant"))


def bars(c, want, stock):
    """{("views", v, block) | (tensor,): (bar, stock error)}"""
    out = {}
    for v in range(c.V):
        for name, sl in blocks_of(c).items():
            es = float((stock["views"][v, sl] - want["views"][v, sl]).abs().max())
            out[("views", v, name)] = (max(TOL * max(float(want["views"][v, sl].norm()), 1e-6), ref.MARGIN * es), es)
    for k in want:
        if k != "views":
            es = float((stock[k] - want[k]).abs().max())
            out[(k,)] = (max(CLEAN_TOL * float(want[k].abs().max()), ref.MARGIN * es), es)
    return out


def _err(key, got, want):
    if key[0] == "views":
        sl = dict(BLOCKS, **DEPTH_BLOCKS)[key[2]]
        return float((got["views"][key[1], sl] - want["views"][key[1], sl]).abs().max())
    return float((got[key[0]] - want[key[0]]).abs().max())


def separation_keys(c):
    return [("means",), ("cov",)] + [("views", v, b) for v in range(c.V) for b in c.rho_blocks]


def preconditions(c, refs=None, show=True):
    """What holds on the CPU alone, before any GPU run.  Returns the smallest separation in bars."""
    fw = forwards(c)
    fragile = cases.fragile_counts(None, c.H, c.W, None, None, None, None, forwards=fw)
    assert fragile == [0] * c.V, (c.name, fragile)
    assert cases.view_parallel_shape(c)[0] == c.parts, (c.name, cases.view_parallel_shape(c))
    assert 150 <= c.G <= 200 and (c.H, c.W) == (32, 32)
    vis = torch.from_numpy(np.stack([f["radii"] for f in fw]) > 0)
    rho = factors(c)
    median = float(rho[vis].median())
    if c.sub_pixel:
        assert median < 0.5, (c.name, median)
    want, stock, const = refs if refs is not None else references(c.name)
    b = bars(c, want, stock)
    away = {k: _err(k, const, want) / b[k][0] for k in separation_keys(c)}
    worst = min(away, key=away.get)
    if show:
        print(f"{c.name:16s} visible {int(vis.sum())}, median rho {median:.3f}; without rho's term: at least {away[worst]:.0f} bars away ({worst})")
    assert away[worst] >= SEPARATION, (c.name, worst, away[worst])
    if c.name == "floor":
        floor_preconditions(c, fw, want, const, b)
    if c.name == "clamped":   # visible Gaussians beyond 1.3 tan(fov), by the forward's own float32 decision
        n = 0
        for v in range(c.V):
            rec = c.views[v]
            inx, iny = TO._clamp_mask(rec[:16].reshape(4, 4), c.means * rec[40], float(rec[35]), float(rec[36]))
            n += int((~(inx & iny) & vis[v]).sum())
        assert n >= 8, n
    return away[worst]


def floor_rows():
    return torch.arange(160, 160 + NEEDLES), torch.arange(160 + NEEDLES, 160 + 2 * NEEDLES)


def floor_preconditions(c, fw, want, const, b):
    """det0 / det of the needles lies a factor >= 2 below / above the floor in the float64 and the float32 statement; both
    populations reach pixels; below the floor the rows of dL/dcov carry no rho term, above it they do."""
    below, above = floor_rows()
    rec = c.views[0].double()
    assert float(rec[40]) == 1.0 and torch.equal(rec[:16].reshape(4, 4), torch.eye(4, dtype=torch.float64))
    for dt in (torch.float64, torch.float32):
        k = lambda x: x.to(dt)
        inx, iny = TO._clamp_mask(rec[:16].reshape(4, 4), c.means.double(), float(rec[35]), float(rec[36]))
        c2 = TO._project(dt, c.H, c.W, k(rec[35]), k(rec[36]), k(rec[:16].reshape(4, 4)), k(c.means), k(c.cov), inx, iny)[1]
        a0, bb, c0 = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
        ratio = ((a0 * c0 - bb * bb) / ((a0 + ref.LOWPASS) * (c0 + ref.LOWPASS) - bb * bb)).double()
        assert float(ratio[below].max()) <= ref.FLOOR / 2 and float(ratio[below].min()) > 0, (dt, ratio[below])
        assert float(ratio[above].min()) >= ref.FLOOR * 2 and float(ratio[above].max()) <= ref.FLOOR * 4, (dt, ratio[above])
    reach = want["opac"][:, 0] != 0
    assert int(reach[below].sum()) >= NEEDLES // 2 and int(reach[above].sum()) >= NEEDLES // 2, (reach[below], reach[above])
    bar = b[("cov",)][0]
    d = (const["cov"] - want["cov"]).abs().amax(-1)
    assert float(d[below].max()) == 0.0, d[below]
    assert bool((d[above][reach[above]] > SEPARATION * bar).all()), (d[above], bar)


WORST: dict = {}


def hold(c, got, refs=None):
    """Every block of every view and every input tensor of the kernel's gradients ``got`` at its bar; prints kernel error, stock
    error and their ratio (as antialias_ref.held does) and records the worst ratio per kind in WORST."""
    want, stock, _ = refs if refs is not None else references(c.name)
    assert set(got) == set(want), (sorted(got), sorted(want))
    failed = []
    for key, (bar, es) in bars(c, want, stock).items():
        assert bool(torch.isfinite(got[key[0]]).all()), (c.name, key)
        err = _err(key, got, want)
        ratio = err / es if es > 0 else (0.0 if err == 0 else float("inf"))
        kind = key[2] if key[0] == "views" else key[0]
        if np.isfinite(ratio):
            WORST[kind] = max(WORST.get(kind, 0.0), ratio)
        WORST["bar:" + kind] = max(WORST.get("bar:" + kind, 0.0), err / bar)
        where = f"view {key[1]} {key[2]}" if key[0] == "views" else f"dL/d{key[0]}"
        print(f"{c.name:16s} {where:16s} kernel {err:.3e}  stock {es:.3e}  ratio {ratio:9.3f}  bar {bar:.3e}  kernel / bar {err / bar:.3f}")
        if not err <= bar:
            failed.append((key, err, bar))
    print("worst so far, kernel / stock:", ", ".join(f"{k} {v:.2f}" for k, v in sorted(WORST.items()) if not k.startswith("bar:")))
    print("worst so far, kernel / bar:  ", ", ".join(f"{k[4:]} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith("bar:")))
    assert not failed, (c.name, failed)
