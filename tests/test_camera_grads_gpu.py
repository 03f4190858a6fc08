"""Camera gradients on the MI355X: dL/d(view record) from lsr_backward_views against autograd through the float64
PyTorch oracle (oracle/torch_oracle.py), the chain into extrinsics / intrinsics / near / far / background through the
public surfaces, bitwise non-interference with the existing outputs and gradients, reproducibility, and pose recovery."""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd import rasterizer as R
from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.decoder.geometry import eval_sh
from latentsplat_amd.synthetic import make_scene
from oracle import oracle as orc
from oracle import torch_oracle as TO
from tests import camera_grad_cases as cases
from tests.camera_grad_cases import (cams32 as _cams32, chain64 as _chain64, fragile_counts, oracle_forwards,  # noqa: F401
                                     sh_payload as _sh_payload, view_inputs as _view_inputs, with_depth_channel)

pytestmark = pytest.mark.gpu
F64 = torch.float64
BLOCKS = dict(vm=slice(0, 16), pm=slice(16, 32), campos=slice(32, 35), tanfov=slice(35, 37), bg=slice(37, 40),
              scale=slice(40, 41))


# scene seeds, chosen so that the C oracle's forward of every view reports no fragile evaluation (fragile_counts)
SEEDS = dict(colour=11, precomp=6, latent=21, groups=40, edge=0, depth=3, ortho=7, decoder=50)


def _oracle_view(v, vm, pm, cp, tx, ty, bg, s, H, W, means, cov6, opac, payload, **mode):
    """One view through the float64 oracle; ``payload(ms, campos)`` -> dict(shs=.., colors_precomp=.., features=..,
    sh_degree=..) given the SCALED means.  ``mode``: the oracle's ``antialiasing`` / ``rho_dtype``."""
    ms, cv = means * s, cov6 * s * s
    pl = payload(ms, cp)
    deg = pl.pop("sh_degree", 0)
    col, feat, mask, depth, _ = TO.rasterize(H, W, tx, ty, bg, vm, pm, cp, deg, ms, cv, opac, **pl, **mode)
    return col, feat, mask, depth


def _loss(col, feat, mask, depth, w):
    out = 0.0
    if col is not None:
        out = out + (col * w["col"]).sum()
    if feat is not None:
        out = out + (feat * w["feat"][: feat.shape[0]]).sum()
    return out + (mask * w["mask"]).sum() + (depth * w["depth"]).sum()


def _weights(V, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [dict(col=torch.randn(3, H, W, generator=g, dtype=F64), feat=torch.randn(max(C, 1), H, W, generator=g, dtype=F64),
                 mask=torch.randn(1, H, W, generator=g, dtype=F64), depth=0.05 * torch.randn(1, H, W, generator=g, dtype=F64))
            for _ in range(V)]


def _scene(G, size, V, seed, **kw):
    sc = make_scene(G, image_size=size, views=V, seed=seed, **kw)
    return sc


def _poison_view_grad_workspace(V, G, dev):
    """Best effort against stale memory: the reduction workspace is torch.empty, so a partial record that no kernel wrote
    is noticed only if the block is not zero.  A block of that size filled with 0xFF (NaN as float) and freed again is what the
    caching allocator most likely hands to the op's backward."""
    d = _lib.Dims(num_views=V, num_gaussians=G, height=32, width=32, feat_channels=0, color_mode=1, sh_degree=0, sh_coeffs=1,
                  cov_elems=6)
    n = R._lib.load().lsr_view_grad_workspace_bytes(ctypes.byref(d))
    assert n > 0
    torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)


def _op_grad(views32, H, W, means, cov, opac, kw, C, contraction=False, poison=False, antialiasing=False, leaves=None):
    """(views.grad, radii) of the HIP op under the loss of ``_weights(V, H, W, C)``, on the host.  ``antialiasing``: the op's
    keyword (omitted when off).  ``leaves``: a dict — means, cov, opac and the payload tensors of ``kw`` require grad as well
    (the plain backward instances run next to the camera ones) and their gradients are left in it, on the host."""
    dev = torch.device("cuda:0")
    V = views32.shape[0]
    w = _weights(V, H, W, C)
    lib = R._lib.load()
    lib.lsr_set_projection_contraction(1 if contraction else 0)
    try:
        views = views32.to(dev).requires_grad_(True)
        leaf = (lambda t: t.to(dev).requires_grad_(True)) if leaves is not None else (lambda t: t.to(dev))
        dk = {k: (leaf(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        geo = dict(means=leaf(means), cov=leaf(cov), opac=leaf(opac))
        held = dict(geo, **{k: v for k, v in dk.items() if torch.is_tensor(v)})
        deg = dk.pop("sh_degree", 0)
        if antialiasing:
            dk["antialiasing"] = True
        col, feat, mask, depth, radii = R.rasterize_views(views, H, W, deg, geo["means"], geo["cov"], geo["opac"], **dk)
        loss = 0.0
        for v in range(V):
            loss = loss + _loss(None if col is None else col[v].double(), None if feat is None else feat[v].double(),
                                mask[v][None].double(), depth[v][None].double(), {k: t.to(dev) for k, t in w[v].items()})
        if poison:
            _poison_view_grad_workspace(V, means.shape[-2], dev)
        loss.backward()
        if leaves is not None:
            leaves.update({k: t.grad.cpu() for k, t in held.items()})
    finally:
        lib.lsr_set_projection_contraction(0)
    return views.grad.cpu(), radii.cpu()


def _kernel_vs_oracle(views32, H, W, means, cov, opac, kw, payload, C, scenes=None, contraction=False, tol=1e-3, placed=None,
                      info=None, antialiasing=False):
    """dL/dviews of the HIP op vs autograd through the float64 oracle, per view and per block, on a scene whose C-oracle
    forward has no fragile evaluations (a gradient there may flip between two equally right answers).  A table with a
    depth mode (slot 41): the oracle blends the mode's payload d as one more feature channel, and near / far (slots 42, 43)
    are two more blocks.  ``antialiasing``: the op's and the oracle's mode; the C oracle (the gate, the radii) is fed o rho per
    view.  ``placed`` (a B case of camera_grad_cases: positions of the scene's Gaussians among padding): also
    the radii — 0 on the padding in every view, the C oracle's everywhere — and the reduction workspace is poisoned before
    the backward.  ``info`` receives what the caller asserts on."""
    V = views32.shape[0]
    fwds = oracle_forwards(views32, H, W, means, cov, opac, payload, scenes, antialiasing=antialiasing)
    assert fragile_counts(None, H, W, None, None, None, None, forwards=fwds) == [0] * V
    moded = bool((views32[:, 41] != 0).all())
    w = _weights(V, H, W, C)
    got32, radii = _op_grad(views32, H, W, means, cov, opac, kw, C, contraction, poison=placed is not None,
                            antialiasing=antialiasing)
    if placed is not None:
        want_radii = torch.from_numpy(np.stack([f["radii"] for f in fwds])).to(radii.dtype)
        pad = torch.ones(means.shape[-2], dtype=torch.bool)
        pad[placed] = False
        assert not bool(pad.any()) or int(radii[:, pad].abs().max()) == 0
        assert torch.equal(radii, want_radii)
    got = got32.double()
    blocks = dict(BLOCKS, near=slice(42, 43), far=slice(43, 44)) if moded else BLOCKS
    worst, wants, masks = 0.0, [], []
    for v in range(V):
        rec = views32[v].double().clone().requires_grad_(True)
        vm, pm, cp = rec[0:16], rec[16:32], rec[32:35]
        tx, ty, bg, s = rec[35], rec[36], rec[37:40], rec[40]
        sidx, m, c6, o = _view_inputs(views32, v, means, cov, opac, scenes)
        col, feat, mask, depth = _oracle_view(v, vm, pm, cp, tx, ty, bg, s, H, W, m, c6, o,
                                              lambda ms, cpos: with_depth_channel(payload(ms, cpos, sidx), rec, m),
                                              **(dict(antialiasing=True) if antialiasing else {}))
        if moded:
            depth, feat = feat[-1:], (feat[:-1] if feat.shape[0] > 1 else None)
        _loss(col, feat, mask, depth, w[v]).backward()
        want = rec.grad
        wants.append(want)
        masks.append(mask.detach())
        assert float(want[41].abs()) == 0.0 and float(got[v, 41].abs()) == 0.0
        if not moded:
            assert float(want[42:].abs().max()) == 0.0 and float(got[v, 42:].abs().max()) == 0.0
        for name, sl in blocks.items():
            err = float((got[v, sl] - want[sl]).abs().max())
            norm = float(want[sl].norm())
            ratio = err / max(norm, 1e-12)
            if norm > 1e-9:
                worst = max(worst, ratio)
            assert err <= tol * max(norm, 1e-6), (v, name, got[v, sl], want[sl])
    print(f"worst per-block error / norm: {worst:.2e}")
    if info is not None:
        info.update(got=got, want=torch.stack(wants), radii=radii, masks=masks, forwards=fwds)
    return worst


def _payload_of(kw):
    """The oracle's payload function from the op's keywords (``shs`` + ``sh_degree`` in the 3DGS axes, ``colors_precomp``,
    ``features``, ``feature_sh``; shared, per scene or per view), differentiable in the tensors of ``kw``."""
    deg, shs, fsh = kw.get("sh_degree", 0), kw.get("shs"), kw.get("feature_sh")
    pick = lambda t, base, sidx: t if t.dim() == base else t[sidx]

    def f(ms, cp, sidx):
        if fsh is not None:
            return cases.latent_sh_payload(deg, shs, math.isqrt(fsh.shape[-1]) - 1, fsh)(ms, cp, sidx)
        out = _sh_payload(deg, shs)(ms, cp, sidx) if shs is not None else {}
        for k in ("colors_precomp", "features"):
            if kw.get(k) is not None:
                out[k] = pick(kw[k], 2, sidx).double()
        return out
    return f


def _oracle_grads(views32, H, W, means, cov, opac, kw, C, scenes=None, **mode):
    """Autograd through the float64 oracle under the loss of ``_weights(V, H, W, C)`` with the record, means, cov, opac and
    the payload tensors of ``kw`` as leaves in the shapes the op takes them: dict of gradients (``views`` (V, 44); an input
    shared by the views holds the sum over them, a per-scene one the sum over its group, a per-view one each view's — what
    one leaf of that shape collects).  ``mode``: the oracle's ``antialiasing`` / ``rho_dtype``."""
    V = views32.shape[0]
    w = _weights(V, H, W, C)
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    rec_all = leaf(views32)
    geo = dict(means=leaf(means), cov=leaf(cov), opac=leaf(opac))
    kw64 = {k: (leaf(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    payload = _payload_of(kw64)
    moded = bool((views32[:, 41] != 0).all())
    for v in range(V):
        rec = rec_all[v]
        sidx, m, c6, o = _view_inputs(views32, v, geo["means"], geo["cov"], geo["opac"], scenes)
        col, feat, mask, depth = _oracle_view(v, rec[0:16], rec[16:32], rec[32:35], rec[35], rec[36], rec[37:40], rec[40], H, W,
                                              m, c6, o, lambda ms, cpos: with_depth_channel(payload(ms, cpos, sidx), rec, m), **mode)
        if moded:
            depth, feat = feat[-1:], (feat[:-1] if feat.shape[0] > 1 else None)
        _loss(col, feat, mask, depth, w[v]).backward()
    out = dict(views=rec_all.grad, **{k: t.grad for k, t in geo.items()})
    out.update({k: t.grad for k, t in kw64.items() if torch.is_tensor(t)})
    return out


def _kernel_and_oracle_grads(views32, H, W, means, cov, opac, kw, C, scenes=None, contraction=False, antialiasing=False,
                             rho_dtypes=(None,)):
    """One forward and backward of the HIP op with EVERY input a leaf (the plain instances of the projection backward and,
    for the record, the camera instances) and the float64 oracle's gradients of the same leaves, once per entry of
    ``rho_dtypes``: (got, [want, ...], radii), dicts keyed views / means / cov / opac / the tensors of ``kw``.  Gated like
    ``_kernel_vs_oracle`` on a C-oracle forward without fragile evaluations."""
    V = views32.shape[0]
    payload = _payload_of({k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()})
    fwds = oracle_forwards(views32, H, W, means, cov, opac, payload, scenes, antialiasing=antialiasing)
    assert fragile_counts(None, H, W, None, None, None, None, forwards=fwds) == [0] * V
    got = {}
    got["views"], radii = _op_grad(views32, H, W, means, cov, opac, kw, C, contraction, antialiasing=antialiasing, leaves=got)
    mode = lambda rd: dict(antialiasing=True, rho_dtype=rd) if antialiasing else {}
    wants = [_oracle_grads(views32, H, W, means, cov, opac, kw, C, scenes, **mode(rd)) for rd in rho_dtypes]
    return {k: t.double() for k, t in got.items()}, wants, radii


@pytest.mark.parametrize("axes", ["3dgs", "reference"])
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_colour_sh_camera_grads_match_oracle(hip_device, deg, axes):
    H = W = 32
    sc = _scene(160, H, 2, seed=SEEDS["colour"] + deg, color_sh_degree=deg, feature_channels=None)
    views = _cams32(sc)
    shs = sc.color_sh.transpose(1, 2).contiguous()          # (G, K, 3)
    cov6 = cs._pack_covariances(sc.covariances)
    R.set_color_sh_convention(axes)
    try:
        _kernel_vs_oracle(views, H, W, sc.means, cov6, sc.opacities[:, None], dict(shs=shs, sh_degree=deg),
                          _sh_payload(deg, shs, axes), 0)
    finally:
        R.set_color_sh_convention("3dgs")


@pytest.mark.parametrize("C", [4, 8, 13])
def test_precomp_colour_and_direct_features(hip_device, C):
    H = W = 32
    sc = _scene(160, H, 3, seed=SEEDS["precomp"] + C, color_sh_degree=None, feature_channels=C)
    views = _cams32(sc)
    g = torch.Generator().manual_seed(C)
    cp = torch.rand(sc.means.shape[0], 3, generator=g)
    feats = sc.feature_sh[..., 0].contiguous()
    cov6 = cs._pack_covariances(sc.covariances)
    _kernel_vs_oracle(views, H, W, sc.means, cov6, sc.opacities[:, None], dict(colors_precomp=cp, features=feats),
                      lambda ms, cpos, s: dict(colors_precomp=cp.double(), features=feats.double()), C)


@pytest.mark.parametrize("fdeg", [1, 2])
def test_fused_latent_sh_cov9_contraction(hip_device, fdeg):
    H = W = 32
    sc = _scene(160, H, 2, seed=SEEDS["latent"] + fdeg, color_sh_degree=1, feature_channels=4, feature_sh_degree=fdeg)
    views = _cams32(sc)
    shs = sc.color_sh.transpose(1, 2).contiguous()
    fsh = sc.feature_sh.contiguous()

    def payload(ms, cp, sidx):
        d = ms - cp[None]
        d = d / d.norm(dim=-1, keepdim=True)
        out = _sh_payload(1, shs)(ms, cp, sidx)
        out["features"] = 0.5 + eval_sh(fdeg, fsh.double(), d)
        return out

    _kernel_vs_oracle(views, H, W, sc.means, sc.covariances.contiguous(), sc.opacities[:, None],
                      dict(shs=shs, sh_degree=1, feature_sh=fsh), payload, 4, contraction=(fdeg == 2))


def test_view_groups(hip_device):
    """b = 2 scenes x v = 3 views in one call (views_per_group): per-scene inputs, per-view camera gradients."""
    H = W = 32
    scenes = [_scene(150, H, 3, seed=SEEDS["groups"] + k, color_sh_degree=2, feature_channels=None) for k in range(2)]
    views = torch.cat([_cams32(s) for s in scenes])
    means = torch.stack([s.means for s in scenes])
    cov6 = torch.stack([cs._pack_covariances(s.covariances) for s in scenes])
    opac = torch.stack([s.opacities[:, None] for s in scenes])
    shs = torch.stack([s.color_sh.transpose(1, 2) for s in scenes]).contiguous()
    _kernel_vs_oracle(views, H, W, means, cov6, opac, dict(shs=shs, sh_degree=2), _sh_payload(2, shs), 0, scenes=2)


# ---------------------------------------------------------------------------------------------------------------------
# 4+ views per group and more than 64 chunks (tests/camera_grad_cases.py: what each case reaches and why)
# ---------------------------------------------------------------------------------------------------------------------
def _run_case(name):
    c, info = cases.case(name), {}
    _kernel_vs_oracle(c.views, c.H, c.W, c.means, c.cov, c.opac, c.kw, c.payload, c.C, scenes=c.scenes,
                      contraction=c.contraction, placed=c.placed, info=info)
    return c, info


@pytest.mark.parametrize("name", ["A1", "A2", "A2-contraction", "A2-depth", "A3", "A4", "A4-depth", "A5", "A6"])
def test_view_parallel_instances_match_oracle(hip_device, name):
    """k_preprocess_bwd<4, *, true> (V >= 4 views per group) and every view chunk of k_sh_bwd<..., true>"""
    c, info = _run_case(name)
    assert cases.view_parallel_shape(c)[0] == 4
    if name == "A3":     # nothing depends on the camera position: exactly zero in the oracle, the zero-norm floor on the device
        assert float(info["want"][:, 32:35].abs().max()) == 0.0
    if c.mode is not None:
        assert bool((info["want"][:, 42:44].abs() > 0).all())
    if name == "A6":
        assert cases.sh_backward_lds_bytes(4, cases.A6_CHANNELS, 2) > 65536


@pytest.mark.parametrize("name", ["B1", "B2", "B3"])
def test_reduction_with_several_chunks_per_slice(hip_device, name):
    """k_view_grad_partial with per > 1 chunks per slice (B1), per > 8: the row loop wraps (B2), per > 256: the near / far
    loop wraps (B3), on scenes padded with Gaussians that every view culls"""
    c, info = _run_case(name)
    cases.assert_reduction_structure(name, c, info["radii"])
    if name == "B3":
        assert float(info["want"][0, 42].abs()) > 0 and float(info["want"][0, 43].abs()) > 0


def test_background_sum_over_more_than_256_pixels_per_slice(hip_device):
    """128 x 160: 320 pixels per slice; the background block at the bar with final T from ~0 to 1 over the image"""
    c, info = _run_case("B4")
    cases.assert_reduction_structure("B4", c, info["radii"])
    cases.assert_background_mask(info["masks"][0])


def test_reduction_is_bitwise_reproducible(hip_device):
    """views.grad of two identical runs of every B case, bit for bit: the reduction adds its records in a fixed order (no
    atomics) — the first time with more than 4 chunks.  The partial records are sums of the compositing backward's
    per-Gaussian records, whose cross-tile float atomics are order independent only under LSR_DETERMINISTIC=1 (the
    condition include/lsr_rasterizer.h states for this promise); the knob is read once per process, hence the subprocess."""
    code = r'''
import sys, torch
sys.path.insert(0, %r)
from tests import camera_grad_cases as cases
from tests.test_camera_grads_gpu import _op_grad
flags = []
for name in ("B1", "B2", "B3", "B4"):
    c = cases.case(name)
    a, b = (_op_grad(c.views, c.H, c.W, c.means, c.cov, c.opac, c.kw, c.C, poison=True)[0] for _ in range(2))
    flags.append(bool(torch.equal(a, b)) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0)
print("RESULT", *flags)
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LSR_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "RESULT True True True True", r.stdout


def edge_case():
    """util.make_edge_scene's `outside` population: visible Gaussians whose EWA Jacobian is clamped (1.3 tan(fov))"""
    from tests import util
    H = W = 32
    sc, _ = util.make_edge_scene("outside", H=H, W=W, views=2, seed=SEEDS["edge"], color_sh_degree=2, feature_channels=None)
    views = _cams32(sc)
    shs = sc.color_sh.transpose(1, 2).contiguous()
    cov6 = cs._pack_covariances(sc.covariances)
    return H, W, views, sc.means, cov6, sc.opacities[:, None], shs


def test_edge_scene_clamped_jacobian(hip_device):
    H, W, views, means, cov6, opac, shs = edge_case()
    # the clamp decision as the kernels take it (float32 t, IEEE ratio against 1.3f tanfov), on the visible Gaussians
    clamped = 0
    for v in range(views.shape[0]):
        vm, s = views[v, :16], views[v, 40]
        p = means * s
        t = [((vm[k] * p[:, 0] + vm[4 + k] * p[:, 1]) + vm[8 + k] * p[:, 2]) + vm[12 + k] for k in range(3)]
        lim = torch.tensor(1.3, dtype=torch.float32) * views[v, 35:37]
        out = ((t[0] / t[2]).abs() > lim[0]) | ((t[1] / t[2]).abs() > lim[1])
        view = orc.View(H, W, float(views[v, 35]), float(views[v, 36]), views[v, 37:40].numpy(),
                        views[v, 0:16].reshape(4, 4).numpy(), views[v, 16:32].reshape(4, 4).numpy(), views[v, 32:35].numpy(), 2)
        radii = orc.forward(view, p.numpy(), (cov6 * s * s).numpy(), opac.numpy(), shs.numpy())["radii"]
        clamped += int((out & torch.from_numpy(radii > 0)).sum())
    assert clamped >= 8, clamped
    _kernel_vs_oracle(views, H, W, means, cov6, opac, dict(shs=shs, sh_degree=2), _sh_payload(2, shs), 0)


def _surface_inputs(dev, V=2, G=200, size=32, seed=3, dtype=torch.float32):
    sc = _scene(G, size, V, seed=seed, color_sh_degree=1, feature_channels=4, feature_sh_degree=0)
    ext = sc.extrinsics.clone()
    ext[:, :3, 3] += torch.tensor([0.03, -0.02, 0.05])
    cams = [ext, sc.intrinsics, sc.near * 1.2, sc.far, torch.tensor([[0.2, 0.4, 0.6]]).repeat(V, 1)]
    return sc, [c.to(dev, dtype) for c in cams]


def _surface_reference(sc, cams, H, W, w):
    """float64 chain: reference-style scaling, then the torch oracle; gradients w.r.t. the five camera inputs"""
    ext, intr, near, far, bg = (c.detach().cpu().double().requires_grad_(True) for c in cams)
    vt, full, cp, tx, ty, s = _chain64(ext, intr, near, far)
    shs = sc.color_sh.transpose(1, 2).double()
    feats = 0.5 + TO.SH_C0 * sc.feature_sh[..., 0].double()
    loss = 0.0
    for v in range(ext.shape[0]):
        ms, cv = sc.means.double() * s[v], cs._pack_covariances(sc.covariances).double() * s[v] ** 2
        out = TO.rasterize(H, W, tx[v], ty[v], bg[v], vt[v], full[v], cp[v], 1, ms, cv, sc.opacities[:, None].double(),
                           shs=shs, features=feats)
        loss = loss + _loss(*out[:4], w[v])
    loss.backward()
    return [t.grad for t in (ext, intr, near, far, bg)]


def _assert_grads_close(got, want, tol, names=("extrinsics", "intrinsics", "near", "far", "background")):
    """Per input: max abs error <= tol x that input's gradient norm.  An input whose float64 gradient is exactly zero (e.g.
    `near` of the orthographic camera: it only reaches the depth row of the projection, which nothing reads) is held to
    tol x 1e-4 of the largest gradient norm of the call instead: float32 autograd leaves rounding residue there."""
    norms = [float(b.norm()) for b in want]
    floor = 1e-4 * max(norms)
    for n, a, b, norm in zip(names, got, want, norms):
        assert a is not None, n
        a = a.detach().cpu().double()
        err = float((a - b).abs().max())
        print(f"{n}: max err {err:.3e}, norm {norm:.3e}")
        assert err <= tol * max(norm, floor), (n, a, b)


def test_render_cuda_camera_gradient(hip_device):
    """Fails without the feature: render_cuda's table was detached, extrinsics.grad came back None."""
    dev = torch.device("cuda:0")
    H = W = 32
    sc, cams = _surface_inputs(dev)
    for c in cams:
        c.requires_grad_(True)
    V = cams[0].shape[0]
    w = _weights(V, H, W, 4)
    out = cs.render_cuda(*cams[:4], (H, W), cams[4], sc.means[None].to(dev), sc.covariances[None].to(dev),
                         sc.opacities[None].to(dev), sc.color_sh[None].to(dev), sc.feature_sh[None].to(dev))
    loss = sum(_loss(out.color[v].double(), out.feature[v].double(), out.mask[v][None].double(), out.depth[v][None].double(),
                     {k: t.to(dev) for k, t in w[v].items()}) for v in range(V))
    loss.backward()
    assert cams[0].grad is not None
    _assert_grads_close([c.grad for c in cams], _surface_reference(sc, cams, H, W, w), 2e-3)


def test_render_scenes_matches_render_cuda(hip_device):
    """render_scenes (the scene-major entry point) reaches the same camera gradient as render_cuda."""
    dev = torch.device("cuda:0")
    H = W = 32
    sc, cams = _surface_inputs(dev, V=3, seed=9)
    w = _weights(3, H, W, 4, seed=1)
    g = lambda t: {k: x.to(dev) for k, x in t.items()}

    def run(fn):
        leaves = [c.clone().requires_grad_(True) for c in cams]
        out = fn(leaves)
        sum(_loss(out.color[v].double(), out.feature[v].double(), out.mask[v][None].double(), out.depth[v][None].double(),
                  g(w[v])) for v in range(3)).backward()
        return [x.grad for x in leaves]

    gm = lambda t: t[None].to(dev)
    a = run(lambda c: cs.render_cuda(*c[:4], (H, W), c[4], gm(sc.means), gm(sc.covariances), gm(sc.opacities),
                                     gm(sc.color_sh), gm(sc.feature_sh)))
    b = run(lambda c: cs.render_scenes(*(x[None] for x in c[:4]), (H, W), c[4][0], gm(sc.means), gm(sc.covariances),
                                       gm(sc.opacities), gm(sc.color_sh), gm(sc.feature_sh)))
    for x, y in zip(a[:4], b[:4]):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-5 * float(x.abs().max()))


def test_render_depth_cuda_camera_gradient(hip_device):
    """A non-`depth` mode: the per-Gaussian value (1 / camera z) depends on the extrinsics as well as the table does."""
    dev = torch.device("cuda:0")
    H = W = 32
    sc, cams = _surface_inputs(dev, seed=SEEDS["depth"])
    V, G = 2, sc.means.shape[0]
    leaves = [c.clone().requires_grad_(True) for c in cams[:4]]
    gm = lambda t: t[None].expand(V, *t.shape).contiguous().to(dev)
    d = cs.render_depth_cuda(*leaves, (H, W), gm(sc.means), gm(sc.covariances), gm(sc.opacities), mode="disparity")
    w = [x["col"][0] for x in _weights(V, H, W, 0, seed=4)]
    sum((d[v].double() * w[v].to(dev)).sum() for v in range(V)).backward()
    # float64: the reference's _depth_as_color, its degree-0 SH colour, the scaled cameras and the oracle
    ext, intr, near, far = (c.detach().cpu().double().requires_grad_(True) for c in cams[:4])
    cam_z = torch.einsum("bij,gj->bgi", torch.linalg.inv(ext), torch.nn.functional.pad(sc.means.double(), (0, 1), value=1.0))[..., 2]
    vt, full, cp, tx, ty, s = _chain64(ext, intr, near, far)
    loss = 0.0
    for v in range(V):
        rgb = torch.clamp_min(0.5 + TO.SH_C0 * (1 / cam_z[v]), 0.0)[:, None].expand(G, 3)
        col = TO.rasterize(H, W, tx[v], ty[v], torch.zeros(3, dtype=F64), vt[v], full[v], cp[v], 0, sc.means.double() * s[v],
                           cs._pack_covariances(sc.covariances).double() * s[v] ** 2, sc.opacities[:, None].double(),
                           colors_precomp=rgb)[0]
        loss = loss + (col.mean(0) * w[v]).sum()
    loss.backward()
    _assert_grads_close([x.grad for x in leaves], [ext.grad, intr.grad, near.grad, far.grad], 2e-3,
                        names=("extrinsics", "intrinsics", "near", "far"))


def test_render_cuda_orthographic_camera_gradient(hip_device):
    """The fake orthographic camera (0.1 degree field of view, moved back ~1000 widths): the table was always PyTorch, the op
    now returns its gradient; colour SH through the moved camera, latent SH through the original one."""
    dev = torch.device("cuda:0")
    H = W = 32
    sc = _scene(200, H, 2, seed=SEEDS["ortho"], color_sh_degree=1, feature_channels=4, feature_sh_degree=1)
    V = 2
    ext0 = sc.extrinsics.clone()
    ext0[:, :3, 3] += torch.tensor([0.05, -0.03, -1.0])
    wd = torch.tensor([3.0, 2.5])
    cams = [ext0, wd, wd, sc.near, sc.far, torch.tensor([[0.2, 0.4, 0.6], [0.1, 0.1, 0.3]])]
    leaves = [c.to(dev).clone().requires_grad_(True) for c in cams]
    gm = lambda t: t[None].expand(V, *t.shape).contiguous().to(dev)
    out = cs.render_cuda_orthographic(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], (H, W), leaves[5], gm(sc.means),
                                      gm(sc.covariances), gm(sc.opacities), gm(sc.color_sh), gm(sc.feature_sh))
    w = _weights(V, H, W, 4, seed=6)
    sum(_loss(out.color[v].double(), out.feature[v].double(), out.mask[v][None].double(), out.depth[v][None].double(),
              {k: t.to(dev) for k, t in w[v].items()}) for v in range(V)).backward()
    # float64 restatement of render_cuda_orthographic
    ext, width, height, near, far, bg = (c.double().clone().requires_grad_(True) for c in cams)
    tan_x = torch.tan(0.5 * torch.deg2rad(torch.tensor(0.1, dtype=F64)))
    dist = 0.5 * width / tan_x
    tan_y = 0.5 * height / dist
    nr, fr = near + dist, far + dist
    e2 = torch.cat([ext[:, :, :2], ext[:, :, 2:3], (ext[:, :, 3] - dist[:, None] * ext[:, :, 2])[..., None]], -1)
    P = torch.zeros((V, 4, 4), dtype=F64)
    P[:, 0, 0], P[:, 1, 1] = 1 / tan_x, 1 / tan_y
    P[:, 2, 2], P[:, 2, 3], P[:, 3, 2] = fr / (fr - nr), -(fr * nr) / (fr - nr), 1
    vt = torch.linalg.inv(e2).transpose(1, 2)
    full = vt @ P.transpose(1, 2)
    shs = sc.color_sh.transpose(1, 2).double()
    loss = 0.0
    for v in range(V):
        d = sc.means.double() - ext[v, :3, 3][None]
        feats = 0.5 + eval_sh(1, sc.feature_sh.double(), d / d.norm(dim=-1, keepdim=True))
        o = TO.rasterize(H, W, tan_x, tan_y[v], bg[v], vt[v], full[v], e2[v, :3, 3], 1, sc.means.double(),
                         cs._pack_covariances(sc.covariances).double(), sc.opacities[:, None].double(), shs=shs, features=feats)
        loss = loss + _loss(*o[:4], w[v])
    loss.backward()
    _assert_grads_close([x.grad for x in leaves], [ext.grad, width.grad, height.grad, near.grad, far.grad, bg.grad], 2e-3,
                        names=("extrinsics", "width", "height", "near", "far", "background"))


def test_decoder_splatting_cuda_camera_gradient(hip_device):
    """DecoderSplattingCUDA.forward (scene-major: b = 2 scenes x v = 2 views, colour SH 1 + latent SH 1)."""
    from latentsplat_amd import decoder as dec
    dev = torch.device("cuda:0")
    H = W = 32
    b, v = 2, 2
    scs = [_scene(150, H, v, seed=SEEDS["decoder"] + k, color_sh_degree=1, feature_channels=4, feature_sh_degree=1) for k in range(b)]
    st = lambda name: torch.stack([getattr(x, name) for x in scs])
    ext0 = st("extrinsics").clone()
    ext0[..., :3, 3] += torch.tensor([0.03, -0.02, 0.05])
    cams = [ext0, st("intrinsics"), st("near") * 1.2, st("far")]
    leaves = [c.to(dev).clone().requires_grad_(True) for c in cams]
    gauss = dec.Gaussians(*(st(n).to(dev) for n in ("means", "covariances", "opacities", "color_sh", "feature_sh")))
    bgc = [0.2, 0.4, 0.6]
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), bgc).to(dev)
    out = d.forward(gauss, *leaves, (H, W))
    w = _weights(b * v, H, W, 4, seed=8)
    g = lambda k: {n: t.to(dev) for n, t in w[k].items()}
    sum(_loss(out.color[i, j].double(), out.feature_posterior.mean[i, j].double(), out.mask[i, j][None].double(),
              out.depth[i, j][None].double(), g(i * v + j)) for i in range(b) for j in range(v)).backward()
    ext, intr, near, far = (c.double().clone().requires_grad_(True) for c in cams)
    loss = 0.0
    for i in range(b):
        vt, full, cp, tx, ty, s = _chain64(ext[i], intr[i], near[i], far[i])
        shs = scs[i].color_sh.transpose(1, 2).double()
        for j in range(v):
            ms = scs[i].means.double() * s[j]
            dd = ms - cp[j][None]
            feats = 0.5 + eval_sh(1, scs[i].feature_sh.double(), dd / dd.norm(dim=-1, keepdim=True))
            o = TO.rasterize(H, W, tx[j], ty[j], torch.tensor(bgc, dtype=F64), vt[j], full[j], cp[j], 1, ms,
                             cs._pack_covariances(scs[i].covariances).double() * s[j] ** 2, scs[i].opacities[:, None].double(),
                             shs=shs, features=feats)
            loss = loss + _loss(*o[:4], w[i * v + j])
    loss.backward()
    _assert_grads_close([x.grad for x in leaves], [ext.grad, intr.grad, near.grad, far.grad], 2e-3,
                        names=("extrinsics", "intrinsics", "near", "far"))


def test_drop_in_rasterizer_camera_grads(hip_device):
    dev = torch.device("cuda:0")
    H = W = 32
    sc = _scene(200, H, 1, seed=17, color_sh_degree=2, feature_channels=None)
    views = _cams32(sc)[0]
    vm, pm, cp = (views[a:b].reshape(-1).to(dev).clone().requires_grad_(True) for a, b in ((0, 16), (16, 32), (32, 35)))
    s = float(views[40])
    settings = R.GaussianRasterizationSettings(H, W, float(views[35]), float(views[36]), views[37:40].to(dev), 1.0,
                                               vm.reshape(4, 4), pm.reshape(4, 4), 2, cp, False, False)
    means, cov6 = sc.means * s, cs._pack_covariances(sc.covariances) * s * s
    shs = sc.color_sh.transpose(1, 2).contiguous()
    col, _, mask, depth, _ = R.GaussianRasterizer(settings)(means3D=means.to(dev), means2D=None,
                                                             opacities=sc.opacities[:, None].to(dev), shs=shs.to(dev),
                                                             cov3D_precomp=cov6.to(dev))
    w = _weights(1, H, W, 0)[0]
    _loss(col.double(), None, mask.double(), depth.double(), {k: t.to(dev) for k, t in w.items()}).backward()
    ref = [views[a:b].double().clone().requires_grad_(True) for a, b in ((0, 16), (16, 32), (32, 35))]
    out = TO.rasterize(H, W, float(views[35]), float(views[36]), views[37:40].double(), ref[0], ref[1], ref[2], 2,
                       means.double(), cov6.double(), sc.opacities[:, None].double(), shs=shs.double())
    _loss(out[0], None, out[2], out[3], w).backward()
    _assert_grads_close([vm.grad, pm.grad, cp.grad], [r.grad for r in ref], 1e-3, names=("viewmatrix", "projmatrix", "campos"))


def test_camera_grads_change_nothing_else(hip_device):
    """Images and every other input gradient are bitwise those of the call without camera gradients."""
    dev = torch.device("cuda:0")
    H = W = 64
    sc, cams = _surface_inputs(dev, V=4, G=3000, size=64, seed=31)
    gt = torch.Generator().manual_seed(5)
    gc, gf = torch.randn(4, 3, H, W, generator=gt).to(dev), torch.randn(4, 4, H, W, generator=gt).to(dev)

    def run(cam_grad):
        cm = [c.clone().requires_grad_(cam_grad) for c in cams]
        leaves = [t[None].to(dev).clone().requires_grad_(True) for t in (sc.means, sc.covariances, sc.opacities,
                                                                          sc.color_sh, sc.feature_sh)]
        out = cs.render_cuda(*cm[:4], (H, W), cm[4], *leaves)
        ((out.color * gc).sum() + (out.feature * gf).sum() + out.depth.sum() + out.mask.sum()).backward()
        return [out.color, out.feature, out.mask, out.depth] + [x.grad for x in leaves], cm[0].grad

    a, ga = run(False)
    b, gb = run(True)
    assert ga is None and gb is not None
    # images: the straight-through table holds the device-built values bit for bit
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    # Gaussian gradients: the compositing backward's float atomics make two runs differ in the last bits unless the
    # deterministic mode is on (bit for bit there: test_camera_grads_bitwise_in_deterministic_mode)
    for x, y in zip(a[4:], b[4:]):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-6 * float(x.abs().max()))


def test_camera_grads_bitwise_in_deterministic_mode(hip_device, tmp_path):
    code = r'''
import sys, torch
sys.path.insert(0, %r)
from tests.test_camera_grads_gpu import _surface_inputs
from latentsplat_amd.decoder import cuda_splatting as cs
dev = torch.device("cuda:0")
sc, cams = _surface_inputs(dev, V=4, G=3000, size=64, seed=31)
g = torch.randn((4, 3, 64, 64), generator=torch.Generator().manual_seed(2)).to(dev)
def run(cam):
    cm = [c.clone().requires_grad_(cam) for c in cams]
    leaves = [t[None].to(dev).clone().requires_grad_(True) for t in (sc.means, sc.covariances, sc.opacities, sc.color_sh, sc.feature_sh)]
    out = cs.render_cuda(*cm[:4], (64, 64), cm[4], *leaves)
    ((out.color * g).sum() + out.feature.square().sum() + out.depth.sum()).backward()
    return torch.cat([x.grad.reshape(-1) for x in leaves]), (torch.cat([c.grad.reshape(-1) for c in cm]) if cam else None)
a, ca = run(True)
b, cb = run(True)
c, _ = run(False)
print("RESULT", bool(torch.equal(ca, cb)), bool(torch.equal(a, b)), bool(torch.equal(a, c)))
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LSR_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "RESULT True True True", r.stdout


def _so3(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.linalg.matrix_exp(K)


def test_pose_recovery(hip_device):
    """Perturb the camera by ~2 degrees and 5 % of the scene depth; 100 Adam steps on a 6-DoF correction recover it."""
    dev = torch.device("cuda:0")
    H = W = 64
    sc = _scene(3000, H, 1, seed=77, color_sh_degree=0, feature_channels=None, sigma_px=(1.5, 5.0))
    true = sc.extrinsics.to(dev)
    gm = lambda t: t[None].to(dev)

    def render(ext):
        return cs.render_cuda(ext, sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev), (H, W),
                              torch.zeros(1, 3, device=dev), gm(sc.means), gm(sc.covariances), gm(sc.opacities),
                              gm(sc.color_sh)).color

    with torch.no_grad():
        target = render(true)
    depth = float(sc.means[:, 2].median())
    rot0 = torch.tensor([0.6, -0.8, 0.0]) * math.radians(2.0)
    tr0 = torch.tensor([0.6, 0.0, 0.8]) * 0.05 * depth
    start = true.clone()
    start[0, :3, :3] = _so3(rot0.to(dev)) @ true[0, :3, :3]
    start[0, :3, 3] += tr0.to(dev)

    def pose_error(ext):
        dr = ext[0, :3, :3] @ true[0, :3, :3].T
        ang = torch.arccos(((dr.trace() - 1) / 2).clamp(-1, 1))
        return float(ang) / math.radians(1.0) + float((ext[0, :3, 3] - true[0, :3, 3]).norm()) / (0.01 * depth)

    w = torch.zeros(3, device=dev, requires_grad=True)
    t = torch.zeros(3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([{"params": [w], "lr": 1e-2}, {"params": [t], "lr": 1e-2 * depth}])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.97)

    def current():
        ext = torch.cat([torch.cat([_so3(w) @ start[0, :3, :3], (start[0, :3, 3] + t)[:, None]], 1), start[0, 3:]], 0)[None]
        return ext

    e0 = pose_error(start)
    for _ in range(100):
        opt.zero_grad()
        loss = (render(current()) - target).square().mean()
        loss.backward()
        opt.step()
        sched.step()
    e1 = pose_error(current().detach())
    print(f"pose error {e0:.3f} -> {e1:.4f}")
    assert e1 * 10 <= e0
