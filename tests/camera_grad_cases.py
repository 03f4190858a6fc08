"""Helpers shared by tests/test_camera_grads_{cpu,gpu}.py: the float64 camera chain, the view table of a synthetic scene, the
C oracle's forward per view (fragile evaluations, radii), scenes padded with Gaussians that every view culls, and the cases
that reach the view-parallel kernel instances (A*) and the non-degenerate forms of the camera-gradient reduction (B*).

Why padding is free: a Gaussian culled in every view contributes exactly zero to dL/d(view record) — in the kernels
(``cv = live && vis``) and in the oracle — and oracle/torch_oracle.py compacts to the visible Gaussians before anything dense
happens.  A scene may therefore carry any number of 64-Gaussian chunks while the oracle pays for ~200 Gaussians."""
from __future__ import annotations

import functools
import os
import re

import torch

from latentsplat_amd import rasterizer as R
from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.decoder.geometry import eval_sh, get_fov
from latentsplat_amd.synthetic import make_scene
from oracle import oracle as orc
from oracle import torch_oracle as TO
from tests import depth_modes_util as du

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain64(ext, intr, near, far, scale_invariant=True):
    """Reference-style camera math in float64 PyTorch: 1/near scaling, fov, projection, inverse (cuda_splatting.py)."""
    scale = 1 / near if scale_invariant else torch.ones_like(near)
    e = torch.cat([torch.cat([ext[:, :3, :3], ext[:, :3, 3:] * scale[:, None, None]], -1), ext[:, 3:, :]], -2)
    nr, fr = near * scale, far * scale
    fov = get_fov(intr)
    tx, ty = (0.5 * fov[:, 0]).tan(), (0.5 * fov[:, 1]).tan()
    P = torch.zeros((ext.shape[0], 4, 4), dtype=ext.dtype)
    P[:, 0, 0] = 1 / tx
    P[:, 1, 1] = 1 / ty
    P[:, 2, 2] = fr / (fr - nr)
    P[:, 2, 3] = -(fr * nr) / (fr - nr)
    P[:, 3, 2] = 1
    vt = torch.linalg.inv(e).transpose(1, 2)
    return vt, vt @ P.transpose(1, 2), e[:, :3, 3], tx, ty, scale


def cams32(sc, bg=(0.2, 0.5, 0.7), mode=None):
    """float32 (V, 44) view table of the scene's cameras; ``mode``: a depth mode (slots 41-43 then carry it and near / far)"""
    near, far, ext = sc.near.to(F64), sc.far.to(F64), sc.extrinsics.to(F64)
    if mode is not None:
        # Off the origin, as tests/test_depth_modes_gpu.py::test_camera_gradients has it: with a mode every image of a camera
        # AT the origin is invariant under the scene scale (d reads z / near), so dL/dscale there is the float residue of
        # terms that cancel — not a quantity with a relative bar.
        ext = ext.clone()
        ext[:, :3, 3] += torch.tensor([0.03, -0.02, 0.05], dtype=F64)
        near = near * 1.2
    vt, full, cp, tx, ty, s = chain64(ext, sc.intrinsics.to(F64), near, far)
    bgt = torch.tensor(bg, dtype=F64)
    if mode is None:
        return R.make_view_table(vt, full, cp, tx, ty, bgt, s)
    return R.make_view_table(vt, full, cp, tx, ty, bgt, s, depth_mode=mode, near=near, far=far)


def view_inputs(views32, v, means, cov, opac, scenes):
    V = views32.shape[0]
    sidx = v if scenes is None else v // (V // scenes)
    m, c, o = (means, cov, opac) if scenes is None else (means[sidx], cov[sidx], opac[sidx])
    c6 = c if c.shape[-1] == 6 else torch.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], -1)
    return sidx, m.double(), c6.double(), o.double()


def with_depth_channel(pl, rec, m):
    """A table with a depth mode: the payload d of the mode (the public helper, from the record and the UNSCALED means) as one
    more feature channel — same weights, no background: exactly the depth image's blend."""
    if int(rec[41]) != 0:
        d = du.payload(rec[None], 0, m)[:, None]
        pl["features"] = d if pl.get("features") is None else torch.cat([pl["features"], d], 1)
    return pl


def oracle_forwards(views32, H, W, means, cov, opac, payload, scenes=None, antialiasing=False):
    """Per view: the C oracle's forward (float32, the kernels' decisions bit for bit): ``radii``, ``fragile`` ...
    ``antialiasing``: the C oracle has no such mode and needs none: it is fed the per-view opacities o rho, rho from the
    float32 statement of the factor (oracle.torch_oracle.opacity_factor), which is what the mode composites."""
    out = []
    for v in range(views32.shape[0]):
        sidx, m, c6, o = view_inputs(views32, v, means, cov, opac, scenes)
        rec = views32[v].double()
        s = rec[40]
        with torch.no_grad():
            pl = with_depth_channel(payload(m * s, rec[32:35], sidx), rec, m)
        deg = pl.pop("sh_degree", 0)
        n = lambda k: None if pl.get(k) is None else pl[k].float().contiguous().numpy()
        if antialiasing:
            with torch.no_grad():
                o = o.float() * TO.opacity_factor(H, W, rec[35], rec[36], rec[0:16], m * s, c6 * s * s, dtype=torch.float32)[:, None]
        view = orc.View(H, W, float(views32[v, 35]), float(views32[v, 36]), views32[v, 37:40].numpy(),
                        views32[v, 0:16].reshape(4, 4).numpy(), views32[v, 16:32].reshape(4, 4).numpy(),
                        views32[v, 32:35].numpy(), deg)
        out.append(orc.forward(view, (m * s).float().numpy(), (c6 * s * s).float().numpy(), o.float().numpy(),
                               n("shs"), n("colors_precomp"), n("features")))
    return out


def fragile_counts(views32, H, W, means, cov, opac, payload, scenes=None, forwards=None, antialiasing=False):
    """Per view: evaluations the C oracle's forward flags as fragile (a decision within rounding of a threshold)."""
    fw = forwards if forwards is not None else oracle_forwards(views32, H, W, means, cov, opac, payload, scenes, antialiasing)
    return [len(f["fragile"]) + (1 << 20 if f["fragile_overflow"] else 0) for f in fw]


def sh_payload(deg, shs_g, axes="3dgs"):
    """colour SH in float64: the oracle's own basis (3DGS axes) or the reference axes B(z, x, y) as colours_precomp"""
    def f(ms, cp, sidx):
        sh = shs_g if shs_g.dim() == 3 else shs_g[sidx]
        sh = sh.double()
        if axes == "3dgs":
            return dict(shs=sh, sh_degree=deg)
        d = ms - cp[None]
        d = d / d.norm(dim=-1, keepdim=True)
        b = TO.sh_basis(deg, d[:, [2, 0, 1]])
        return dict(colors_precomp=torch.clamp_min(torch.einsum("gk,gkc->gc", b, sh[:, : b.shape[1]]) + 0.5, 0.0))
    return f


def latent_sh_payload(cdeg, shs, fdeg, fsh):
    """colour SH (3DGS axes) + latent features 0.5 + eval_sh(direction) as the fused kernels evaluate them"""
    def f(ms, cp, sidx):
        d = ms - cp[None]
        d = d / d.norm(dim=-1, keepdim=True)
        out = sh_payload(cdeg, shs)(ms, cp, sidx)
        out["features"] = 0.5 + eval_sh(fdeg, (fsh if fsh.dim() == 3 else fsh[sidx]).double(), d)
        return out
    return f


# ---------------------------------------------------------------------------------------------------------------------
# padded scenes
# ---------------------------------------------------------------------------------------------------------------------
def pad_scene(sc, total, forced=(), seed=0):
    """The scene's Gaussians scattered over ``total`` index positions; every other position holds a Gaussian BEHIND every
    synthetic camera (z in [-21, -1], |x|, |y| <= 1; the cameras sit within 0.3 of the origin, turned by at most 0.15 rad),
    with random covariance / opacity / harmonics: culled in every view (radii == 0).  ``forced`` positions are occupied, by
    the scene's Gaussians closest to the optical axis of view 0 (on screen in every view).  Returns the padded scene and
    the sorted positions of the scene's Gaussians (``placed``)."""
    gen = torch.Generator().manual_seed(seed)
    n = sc.means.shape[0]
    forced = torch.tensor(sorted(forced), dtype=torch.int64)
    free = torch.ones(total, dtype=torch.bool)
    free[forced] = False
    rest = free.nonzero()[:, 0]
    rest = rest[torch.randperm(rest.numel(), generator=gen)[: n - forced.numel()]]
    central = torch.argsort((sc.means[:, :2] / sc.means[:, 2:]).abs().amax(1))
    pos = torch.empty(n, dtype=torch.int64)
    pos[central[: forced.numel()]] = forced
    pos[central[forced.numel():]] = rest

    def fill(t, pad):
        if t is None:
            return None
        out = pad((total,) + tuple(t.shape[1:]))
        out[pos] = t
        return out

    rnd = lambda shape: torch.randn(shape, generator=gen)
    u = lambda shape: torch.rand(shape, generator=gen)
    means = fill(sc.means, lambda sh: torch.cat([u((total, 2)) * 2 - 1, -1 - 20 * u((total, 1))], 1))
    a = 0.05 * rnd((total, 3, 3))
    cov = fill(sc.covariances, lambda sh: a @ a.transpose(1, 2) + 1e-4 * torch.eye(3))
    opac = fill(sc.opacities, lambda sh: u(sh))
    csh = fill(sc.color_sh, lambda sh: 0.3 * rnd(sh))
    fsh = fill(sc.feature_sh, lambda sh: 0.3 * rnd(sh))
    return type(sc)(means, cov, opac, csh, fsh, sc.extrinsics, sc.intrinsics, sc.near, sc.far), torch.sort(pos)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the reduction's arithmetic, from the constants in the sources (views.hip k_view_grad_partial)
# ---------------------------------------------------------------------------------------------------------------------
def kernel_constant(name, path):
    src = open(os.path.join(ROOT, "latentsplat_amd", "csrc", path)).read()
    return int(re.search(r"constexpr int " + name + r"\s*=\s*(\d+)\s*;", src).group(1))


def reduction_shape(G, H, W):
    """How k_view_grad_partial cuts G Gaussians and H x W pixels: chunks of 64, ``per`` chunks and ``pper`` pixels per slice,
    ``rows`` thread rows (a row adds every rows-th chunk of its slice), the number of threads, the slices"""
    split, threads = kernel_constant("kCamSplit", "lsr_internal.h"), kernel_constant("kCamThreads", "views.hip")
    slots = kernel_constant("kCamSlots", "lsr_internal.h")
    chunks = (G + 63) // 64
    return dict(chunks=chunks, split=split, threads=threads, rows=threads // slots, per=-(-chunks // split),
                pper=-(-(H * W) // split))


def sh_backward_lds_bytes(cdeg, C, fdeg, coff=3):
    """sh.hip sh_backward's ``shm``: coefficient rows (or the colour basis array, if larger) + the channel gradients"""
    waves = kernel_constant("kShThreads", "sh.hip") // 64
    ks0, ks1 = 3 * (cdeg + 1) ** 2, C * (fdeg + 1) ** 2
    offF = (64 * ks0 + 3) & ~3
    area = max(offF + 64 * ks1, waves * 64 * kernel_constant("kShBasisC", "sh.hip"))
    return (area + waves * 64 * ((coff + C) | 1)) * 4


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """What ``_kernel_vs_oracle`` takes: table, image size, Gaussians, the op's keywords, the oracle's payload function.
    ``placed``: positions of the scene's Gaussians in a B case's (padded) scene, else None."""
    def __init__(self, views, H, W, means, cov, opac, kw, payload, C, scenes=None, contraction=False, mode=None, placed=None):
        self.views, self.H, self.W, self.means, self.cov, self.opac = views, H, W, means, cov, opac
        self.kw, self.payload, self.C, self.scenes, self.contraction, self.mode, self.placed = kw, payload, C, scenes, contraction, mode, placed
        self.V, self.G = views.shape[0], means.shape[-2]

    def forwards(self):
        return oracle_forwards(self.views, self.H, self.W, self.means, self.cov, self.opac, self.payload, self.scenes)


# scene seeds per case, chosen so that the C oracle's forward of every view reports no fragile evaluation
SEEDS = dict(A1=100, A2=101, A3=100, A4=(100, 140), A5=100, A6=102, B1=100, B2=100, B3=100, B4=100)
MODE = "relative_disparity"


def _colour_case(sc, deg, H, W, mode=None, placed=None):
    shs = sc.color_sh.transpose(1, 2).contiguous()          # (G, K, 3)
    return Case(cams32(sc, mode=mode), H, W, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                dict(shs=shs, sh_degree=deg), sh_payload(deg, shs), 0, mode=mode, placed=placed)


def _a1(seed=None, **scene):
    """V = 4, shared scene, colour SH degree 2: parts == 4 exactly, one full SH view chunk (nv = 4).  (``seed`` / ``scene``,
    here and below: another seed than SEEDS' and further make_scene keywords, for the callers that keep a seed table of
    their own — tests/antialias_grad_cases.py.)"""
    return _colour_case(make_scene(160, image_size=32, views=4, seed=SEEDS["A1"] if seed is None else seed, color_sh_degree=2,
                                   feature_channels=None, **scene), 2, 32, 32)


def _a2(contraction=False, mode=None, seed=None, **scene):
    """V = 5, shared scene, colour degree 1 + 4 latent channels of degree 2, 3 x 3 covariances: parts == 4 with views split
    2 / 1 / 1 / 1 over the parts, SH view chunks nv = 4, 1"""
    sc = make_scene(160, image_size=32, views=5, seed=SEEDS["A2"] if seed is None else seed, color_sh_degree=1, feature_channels=4,
                    feature_sh_degree=2, **scene)
    shs, fsh = sc.color_sh.transpose(1, 2).contiguous(), sc.feature_sh.contiguous()
    return Case(cams32(sc, mode=mode), 32, 32, sc.means, sc.covariances.contiguous(), sc.opacities[:, None],
                dict(shs=shs, sh_degree=1, feature_sh=fsh), latent_sh_payload(1, shs, 2, fsh), 4, contraction=contraction, mode=mode)


def _a3():
    """V = 7, colors_precomp + 13 direct features: no SH backward, the reduction is told sh = 0; dL/dcampos is exactly zero"""
    sc = make_scene(160, image_size=32, views=7, seed=SEEDS["A3"], color_sh_degree=None, feature_channels=13)
    cp = torch.rand(160, 3, generator=torch.Generator().manual_seed(13))
    feats = sc.feature_sh[..., 0].contiguous()
    return Case(cams32(sc), 32, 32, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                dict(colors_precomp=cp, features=feats), lambda ms, cpos, s: dict(colors_precomp=cp.double(), features=feats.double()), 13)


def _a4(mode=None, seed=None, **scene):
    """b = 2 scenes x v = 5 views, colour SH degree 2: blockIdx.y = 1 with parts == 4, the vg offset in both kernels"""
    scs = [make_scene(160, image_size=32, views=5, seed=s, color_sh_degree=2, feature_channels=None, **scene)
           for s in (SEEDS["A4"] if seed is None else seed)]
    st = lambda f: torch.stack([f(s) for s in scs]).contiguous()
    shs = st(lambda s: s.color_sh.transpose(1, 2))
    return Case(torch.cat([cams32(s, mode=mode) for s in scs]), 32, 32, st(lambda s: s.means), st(lambda s: cs._pack_covariances(s.covariances)),
                st(lambda s: s.opacities[:, None]), dict(shs=shs, sh_degree=2), sh_payload(2, shs), 0, scenes=2, mode=mode)


def _a5(seed=None, **scene):
    """V = 5 with per-view (V, G, ...) means / covariances / opacities / harmonics (a different scene per view): the
    chunk = 1 path of k_sh_bwd, non-zero view strides in the camera instances"""
    seed = SEEDS["A5"] if seed is None else seed
    cam = make_scene(1, image_size=32, views=5, seed=seed)
    scs = [make_scene(160, image_size=32, views=1, seed=seed + 1000 * (k + 1), color_sh_degree=2, feature_channels=None, **scene)
           for k in range(5)]
    st = lambda f: torch.stack([f(s) for s in scs]).contiguous()
    shs = st(lambda s: s.color_sh.transpose(1, 2))
    return Case(cams32(cam), 32, 32, st(lambda s: s.means), st(lambda s: cs._pack_covariances(s.covariances)),
                st(lambda s: s.opacities[:, None]), dict(shs=shs, sh_degree=2), sh_payload(2, shs), 0, scenes=5)


A6_CHANNELS = 13


def _a6():
    """V = 16, colour SH degree 4 + 13 latent channels of degree 2: sh_backward asks for
    (64 * 75 + 64 * 117 + 4 * 64 * 17) * 4 = 66 560 bytes of dynamic LDS (> 65 536: allow_big_lds<4, 3, true>; 12 channels
    would take 62 208); SH view chunks nv = 4, 4, 4, 4"""
    sc = make_scene(160, image_size=32, views=16, seed=SEEDS["A6"], color_sh_degree=4, feature_channels=A6_CHANNELS, feature_sh_degree=2)
    shs, fsh = sc.color_sh.transpose(1, 2).contiguous(), sc.feature_sh.contiguous()
    return Case(cams32(sc), 32, 32, sc.means, cs._pack_covariances(sc.covariances), sc.opacities[:, None],
                dict(shs=shs, sh_degree=4, feature_sh=fsh), latent_sh_payload(4, shs, 2, fsh), A6_CHANNELS)


# B1-B3: total Gaussians, views, positions that must hold an on-screen Gaussian
B_SHAPES = dict(
    # 66 chunks, per = 2: chunk 0; chunk 63 = the last chunk of the full slice 31; chunk 64 (slice 32); the partial chunk 65
    B1=(4197, 2, (0, 63 * 64 + 5, 64 * 64 + 1, 4196)),
    # 516 chunks, per = 9: chunk 0; chunk 8 = in-slice offset 8 (thread row 0, second trip); chunk 512 = offset 8 of slice 56,
    # the last chunk of the last full slice; chunk 513 (ragged slice 57); the partial chunk 515
    B2=(33000, 2, (0, 8 * 64 + 3, 512 * 64 + 7, 513 * 64 + 9, 32999)),
    # 16 386 chunks, per = 257: chunk 256 = in-slice offset 256 (the dpart loop's second trip); the partial chunk 16 385
    B3=(1048700, 1, (0, 64 * 256, 64 * 256 + 1, 64 * 256 + 2, 1048699)),
)


def _b(name):
    total, V, forced = B_SHAPES[name]
    deg = 1 if name == "B3" else 2
    sc = make_scene(200, image_size=32, views=V, seed=SEEDS[name], color_sh_degree=deg, feature_channels=None)
    padded, placed = pad_scene(sc, total, forced, seed=SEEDS[name])
    return _colour_case(padded, deg, 32, 32, mode=MODE if name == "B3" else None, placed=placed)


def _b4():
    """G = 600 unpadded, 128 x 160, V = 1, colour SH degree 2, large opaque Gaussians: pper = 320 pixels per slice (the
    background loop's second trip), final T from ~0 to 1 over the image"""
    sc = make_scene(600, image_size=128, views=1, seed=SEEDS["B4"], color_sh_degree=2, feature_channels=None, sigma_px=(2.0, 8.0),
                    opacity_scale=1.0)
    return _colour_case(sc, 2, 128, 160, placed=torch.arange(600))


CASES = {"A1": _a1, "A2": _a2, "A2-contraction": functools.partial(_a2, contraction=True), "A2-depth": functools.partial(_a2, mode=MODE),
         "A3": _a3, "A4": _a4, "A4-depth": functools.partial(_a4, mode=MODE), "A5": _a5, "A6": _a6,
         "B1": functools.partial(_b, "B1"), "B2": functools.partial(_b, "B2"), "B3": functools.partial(_b, "B3"), "B4": _b4}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def oracle64_forward(c):
    """(V, G) radii and the V (1, H, W) masks of the float64 oracle"""
    radii, masks = [], []
    with torch.no_grad():
        for v in range(c.V):
            sidx, m, c6, o = view_inputs(c.views, v, c.means, c.cov, c.opac, c.scenes)
            rec = c.views[v].double()
            s = rec[40]
            pl = c.payload(m * s, rec[32:35], sidx)
            deg = pl.pop("sh_degree", 0)
            out = TO.rasterize(c.H, c.W, rec[35], rec[36], rec[37:40], rec[0:16], rec[16:32], rec[32:35], deg, m * s, c6 * s * s, o, **pl)
            radii.append(out[4])
            masks.append(out[2])
    return torch.stack(radii), masks


def assert_background_mask(mask):
    """B4: final T = 1 - mask from ~0 to 1, strictly in between on a good share of the pixels"""
    assert bool((mask < 0.1).any()) and bool((mask > 0.9).any())
    assert float(((mask > 0.01) & (mask < 0.99)).float().mean()) > 0.25


def view_parallel_shape(c):
    """(parts of launch_preprocess_backward, the nv sequence of k_sh_bwd's view-chunk loop) for the case's views per group"""
    waves = kernel_constant("kShThreads", "sh.hip") // 64
    per_view = c.scenes == c.V
    vpg = c.V if (c.scenes is None or per_view) else c.V // c.scenes
    chunk = 1 if per_view else waves
    return (4 if vpg >= 4 else (2 if vpg >= 2 else 1)), [min(chunk, vpg - v0) for v0 in range(0, vpg, chunk)]


def assert_reduction_structure(name, c, radii):
    """A B case reaches the part of k_view_grad_partial it is about, given the (V, G) radii of a forward: the slicing
    restated from kCamSplit / kCamThreads / kCamSlots as the sources have them (retuned constants: the shapes need retuning)."""
    r = reduction_shape(c.G, c.H, c.W)
    per, rows, threads, split, chunks = r["per"], r["rows"], r["threads"], r["split"], r["chunks"]
    if name == "B4":
        assert r["pper"] == 320 and r["pper"] > threads, r      # thread 0 adds pixels p0 and p0 + 256 of its slice
        return
    visible = (radii > 0).any(0)
    pad = torch.ones(c.G, dtype=torch.bool)
    pad[c.placed] = False
    assert int(radii[:, pad].abs().max()) == 0
    vis_chunks = torch.unique(visible.nonzero()[:, 0] // 64)
    has = lambda ch: bool((vis_chunks == ch).any())
    used = -(-chunks // per)                                     # slices that hold a chunk
    assert c.G % 64 != 0 and bool(visible[0]) and bool(visible[c.G - 1])        # chunk 0; the last, partial chunk
    offsets = vis_chunks % per
    if name == "B1":
        assert (chunks, per, used) == (66, 2, 33) and 1 < per <= rows and used < split, r
        assert has(63) and has(64) and has(65)                   # last chunk of the full slice 31; both chunks of slice 32
    elif name == "B2":
        assert (chunks, per, used, chunks - (used - 1) * per, split - used) == (516, 9, 58, 3, 6) and per > rows, r
        assert has(512) and has(513) and has(515)                # offset 8 of the full slice 56; the ragged slice 57
        assert int((offsets >= rows).sum()) >= 2                 # thread row 0's second trip, in more than one slice
    elif name == "B3":
        assert (chunks, per) == (16386, 257) and per > threads and used == split, r
        assert has(threads) and int(offsets.max()) >= threads    # chunk 256 = in-slice offset 256: the dpart loop's second trip
    else:
        raise KeyError(name)
