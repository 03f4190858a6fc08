"""Shared helpers for the parity tests: synthetic scene -> rasterizer-boundary inputs, oracle
runs, and access to the HIP library's workspaces for bit-exact intermediate comparisons."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from latentsplat_amd.decoder import cuda_splatting as cs  # noqa: E402
from latentsplat_amd.decoder import geometry  # noqa: E402
from latentsplat_amd.decoder.geometry import get_fov  # noqa: E402
from latentsplat_amd.synthetic import Scene, make_scene  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def boundary_inputs(scene: Scene, H: int, W: int, use_sh: bool = True, bg=(0.0, 0.0, 0.0)):
    """Everything that crosses the rasterizer boundary for each view of ``scene`` (CPU tensors),
    computed by the package's own wrapper math (pinned against the reference in
    test_golden_boundary.py).  Returns dict with per-view stacked tensors."""
    V = scene.extrinsics.shape[0]
    means = scene.means[None].expand(V, -1, -1)
    covs = scene.covariances[None].expand(V, -1, -1, -1)
    ext, nr, fr, means, covs = cs._scale_scene(scene.extrinsics, scene.near, scene.far, means, covs)
    fov_x, fov_y = get_fov(scene.intrinsics).unbind(-1)
    cams = cs._cameras(ext, nr, fr, fov_x, fov_y)
    csh = None if scene.color_sh is None else scene.color_sh[None]
    fsh = None if scene.feature_sh is None else scene.feature_sh[None]
    degree, shs, colors_precomp, features = cs._payload(means, cams.campos, csh, fsh, use_sh)
    bgt = torch.tensor(bg, dtype=torch.float32)[None].expand(V, 3)
    return dict(V=V, H=H, W=W, sh_degree=degree, cams=cams, bg=bgt,
                means=means.contiguous(), cov6=cs._pack_covariances(covs).contiguous(),
                opac=scene.opacities[:, None].contiguous(),
                shs=None if shs is None else shs[0].contiguous(),
                colors_precomp=None if colors_precomp is None else colors_precomp[0].contiguous(),
                features=None if features is None else features.contiguous())


def oracle_view(bi: dict, v: int) -> orc.View:
    c = bi["cams"]
    return orc.View(bi["H"], bi["W"], float(c.tan_fov_x[v]), float(c.tan_fov_y[v]), bi["bg"][v].numpy(),
                    c.view_matrix[v].contiguous().numpy(), c.full_projection[v].contiguous().numpy(),
                    c.campos[v].contiguous().numpy(), bi["sh_degree"])


def oracle_forward(bi: dict, v: int):
    n = lambda t: None if t is None else t.detach().numpy()
    feats = None if bi["features"] is None else n(bi["features"][v])
    return orc.forward(oracle_view(bi, v), n(bi["means"][v]), n(bi["cov6"][v]), n(bi["opac"]),
                       n(bi["shs"]), n(bi["colors_precomp"]), feats)


def oracle_backward(bi: dict, v: int, fwd: dict, g_color=None, g_feat=None, g_mask=None, g_depth=None):
    n = lambda t: None if t is None else t.detach().numpy()
    feats = None if bi["features"] is None else n(bi["features"][v])
    return orc.backward(oracle_view(bi, v), n(bi["means"][v]), n(bi["cov6"][v]), n(bi["opac"]),
                        n(bi["shs"]), n(bi["colors_precomp"]), feats, fwd, g_color, g_feat, g_mask, g_depth)


def view_table(bi: dict, device) -> torch.Tensor:
    from latentsplat_amd.rasterizer import make_view_table
    c = bi["cams"]
    return make_view_table(c.view_matrix.to(device), c.full_projection.to(device), c.campos.to(device),
                           c.tan_fov_x.to(device), c.tan_fov_y.to(device), bi["bg"].to(device))


class HipRun:
    """Runs the HIP forward through the C ABI directly (no autograd) and keeps the workspaces so
    tests can read intermediates back."""

    def __init__(self, bi: dict, device="cuda", shared_means=False, forward_flags=0):
        from latentsplat_amd import _lib
        from latentsplat_amd._lib import Dims, Inputs, Layout, Outputs
        self.lib = lib = _lib.load()
        dev = torch.device(device)
        V, H, W = bi["V"], bi["H"], bi["W"]
        self.views = view_table(bi, dev)
        t = lambda x: None if x is None else x.to(dev).contiguous()
        self.means = t(bi["means"][0] if shared_means else bi["means"])
        self.cov6 = t(bi["cov6"][0] if shared_means else bi["cov6"])
        self.opac, self.features = t(bi["opac"]), t(bi["features"])
        self.color = t(bi["shs"]) if bi["shs"] is not None else t(bi["colors_precomp"])
        G = bi["means"].shape[1]
        Cf = 0 if self.features is None else self.features.shape[-1]
        mode = 1 if bi["shs"] is not None else (2 if bi["colors_precomp"] is not None else 0)
        K = bi["shs"].shape[1] if bi["shs"] is not None else 0
        # the feature stride declared below assumes a (V,G,C) tensor; a (1,G,C) one would be read out of bounds
        assert self.features is None or self.features.shape[0] == V, \
            f"HipRun: features have leading dim {self.features.shape[0]}, expected {V} views"
        self.d = d = Dims(V, G, H, W, Cf, mode, bi["sh_degree"], K, 0 if shared_means else 3 * G,
                          0 if shared_means else 6 * G, 0, 0, Cf * G if Cf else 0, 6, 0, 0, 0, 0, 0, 0, forward_flags)
        self._forward(d, dev)

    def _forward(self, d, dev):
        """lsr_forward_prepare + lsr_forward_render of dims ``d`` on the input tensors held by ``self``."""
        from latentsplat_amd import _lib
        from latentsplat_amd._lib import Inputs, Layout, Outputs
        self.lib = lib = _lib.load()
        self.d = d
        V, G, H, W, Cf, mode = d.num_views, d.num_gaussians, d.height, d.width, d.feat_channels, d.color_mode
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        self.inp = Inputs(p(self.views), p(self.means), p(self.cov6), p(self.opac), p(self.color), p(self.features))
        u8 = dict(dtype=torch.uint8, device=dev)
        self.geom = torch.zeros(lib.lsr_geom_workspace_bytes(C.byref(d)), **u8)
        self.img = torch.zeros(lib.lsr_image_workspace_bytes(C.byref(d)), **u8)
        self.radii = torch.zeros((V, G), dtype=torch.int32, device=dev)
        npairs, maxtile = C.c_int64(0), C.c_int32(0)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.lsr_forward_prepare(C.byref(d), C.byref(self.inp), p(self.geom), p(self.radii),
                                           C.byref(npairs), C.byref(maxtile), stream), "prepare")
        self.P, self.maxtile = npairs.value, maxtile.value
        self.bin = torch.zeros(max(1, lib.lsr_binning_workspace_bytes(C.byref(d), self.P, self.maxtile)), **u8)
        f32 = dict(dtype=torch.float32, device=dev)
        self.color_out = torch.zeros((V, 3, H, W), **f32) if mode else None
        self.feat_out = torch.zeros((V, Cf, H, W), **f32) if Cf else None
        self.mask_out = torch.zeros((V, H, W), **f32)
        self.depth_out = torch.zeros((V, H, W), **f32)
        outs = Outputs(p(self.color_out), p(self.feat_out), p(self.mask_out), p(self.depth_out), p(self.radii))
        _lib.check(lib.lsr_forward_render(C.byref(d), C.byref(self.inp), p(self.geom), p(self.bin), p(self.img),
                                          self.P, self.maxtile, C.byref(outs), stream), "render")
        torch.cuda.synchronize(dev)
        self.layout = Layout()
        _lib.check(lib.lsr_get_layout(C.byref(d), self.P, C.byref(self.layout)), "layout")
        self.T = ((W + 15) // 16) * ((H + 15) // 16)

    def _view(self, ws, off, nbytes, dtype):
        return ws[off:off + nbytes].view(dtype)

    def tile_start(self):
        n = self.d.num_views * self.T + 1
        return self._view(self.geom, self.layout.geom_tile_start, n * 4, torch.int32).cpu().numpy().astype(np.int64)

    def point_list(self):
        return self._view(self.bin, self.layout.bin_point_list, max(self.P, 0) * 4, torch.int32).cpu().numpy().astype(np.int64)

    def rect(self):
        n = self.d.num_views * self.d.num_gaussians
        if self.layout.geom_bin_stride == 12:   # narrow records: u8 tile coordinates, f32 depth, u8 span[4]
            b = self._view(self.geom, self.layout.geom_bin, n * 12, torch.uint8).cpu().numpy().astype(np.int32).reshape(
                self.d.num_views, self.d.num_gaussians, 12)
            return b[:, :, :4]
        b = self._view(self.geom, self.layout.geom_bin, n * 16, torch.int16).cpu().numpy().astype(np.int32).reshape(
            self.d.num_views, self.d.num_gaussians, 8)
        return b[:, :, :4] & 0xFFFF

    def q(self):
        """(x,y,A,B), (C,o,z,clampbits) of every (view, Gaussian) screen-space record."""
        n = self.d.num_views * self.d.num_gaussians
        rf = self.layout.geom_rec_floats
        r = self._view(self.geom, self.layout.geom_rec, n * rf * 4, torch.float32).cpu().numpy().reshape(
            self.d.num_views, -1, rf)
        return r[:, :, 0:4], r[:, :, 4:8]

    def half_count(self):
        """(V*T, 2) lengths of the half-tile render lists."""
        n = self.d.num_views * self.T * 2
        return self._view(self.geom, self.layout.geom_half_count, n * 4, torch.int32).cpu().numpy().astype(np.int64).reshape(-1, 2)

    def half_list(self):
        """Raw half-list area: [2P] words `index | sub-block bits << 24` (tile with canonical list [s, s+n)
        owns [2s, 2s+2n), half h at 2s + h*n)."""
        return self._view(self.bin, self.layout.bin_half_list, max(self.P, 0) * 8, torch.int32).cpu().numpy().view(np.uint32)

    def n_considered(self):
        """n_contrib translated from positions in the HALF-TILE render lists (what the kernels keep) to
        positions in the canonical tile lists (what the published algorithm / the oracle keeps): a pixel
        that considered all of its half's list considered the whole tile list; otherwise it stopped
        at a specific entry, whose canonical position is looked up."""
        nc = self.n_contrib()
        ts, pl, hc, hl = self.tile_start(), self.point_list(), self.half_count(), self.half_list()
        V, H, W, T = self.d.num_views, self.d.height, self.d.width, self.T
        gx = (W + 15) // 16
        out = np.zeros_like(nc)
        for v in range(V):
            for t in range(T):
                s0, s1 = ts[v * T + t], ts[v * T + t + 1]
                n = s1 - s0
                ty, tx = divmod(t, gx)
                canon = pl[s0:s1]
                pos = None
                for h in range(2):
                    y0, x0 = ty * 16 + 8 * h, tx * 16
                    if y0 >= H:
                        continue
                    blk = nc[v, y0:y0 + 8, x0:x0 + 16]
                    cnt = hc[v * T + t, h]
                    lst = hl[2 * s0 + h * n: 2 * s0 + h * n + cnt] & 0x00FFFFFF
                    res = np.full(blk.shape, n, np.int64)
                    stopped = blk < cnt
                    if stopped.any():
                        if pos is None:
                            pos = {int(g): i for i, g in enumerate(canon)}
                        res[stopped] = [pos[int(lst[k])] for k in blk[stopped]]
                    out[v, y0:y0 + 8, x0:x0 + 16] = res
        return out

    def item_flags(self):
        """((V*T, 2) flags of the half-tile items, kHdrFlagsValid) as the forward compositing kernel left them."""
        n = self.d.num_views * self.T * 2
        f = self._view(self.geom, self.layout.geom_item_flags, n * 4, torch.int32).cpu().numpy().astype(np.int64).reshape(-1, 2)
        hdr = self._view(self.geom, self.layout.geom_header, 32, torch.int32).cpu().numpy()
        return f, int(hdr[6])

    def header(self):
        """The 64 words of the geometry workspace's header (lsr_internal.h kHdr*)."""
        return self._view(self.geom, self.layout.geom_header, 256, torch.int32).cpu().numpy().view(np.uint32).copy()

    def _item_block(self, k):
        """Offset and bytes of the k-th of the four consecutive per-item blocks of lsr_internal.h::geom_layout (tile_order,
        item_cost, tile_order2, half_count); the public layout exports only the last one and tile_start in front of them."""
        up = lambda x: (x + 255) // 256 * 256
        n = 2 * self.d.num_views * self.T
        block = up(n * 4)
        first = int(self.layout.geom_half_count) - 3 * block
        assert first == up(int(self.layout.geom_tile_start) + (self.d.num_views * self.T + 1) * 4), \
            "the geometry workspace's layout changed: tile_order / item_cost / tile_order2 are not where tests/util.py looks"
        return first + k * block, n * 4

    def item_cost(self):
        """(V*T, 2) lock-step iterations the RECORD forward counted per half-tile item (defined when header word 9 is set)."""
        off, nbytes = self._item_block(1)
        return self._view(self.geom, off, nbytes, torch.int32).cpu().numpy().astype(np.int64).reshape(-1, 2)

    def tile_order2(self):
        """The 2 V T work items `view T + tile | half << 28` in the order k_order_items gave them (header word 9)."""
        off, nbytes = self._item_block(2)
        return self._view(self.geom, off, nbytes, torch.int32).cpu().numpy().view(np.uint32).astype(np.int64)

    def n_contrib(self):
        n = self.d.num_views * self.d.height * self.d.width
        return self._view(self.img, self.layout.img_n_contrib, n * 4, torch.int32).cpu().numpy().reshape(
            self.d.num_views, self.d.height, self.d.width)

    def final_T(self):
        n = self.d.num_views * self.d.height * self.d.width
        return self._view(self.img, self.layout.img_final_T, n * 4, torch.float32).cpu().numpy().reshape(
            self.d.num_views, self.d.height, self.d.width)


def psnr(ground_truth: np.ndarray, predicted: np.ndarray) -> float:
    """PSNR of one (C,H,W) image in dB, as the reference's evaluation computes it (src/evaluation/metrics.py:13-20: both
    images clipped to [0, 1], mean squared error over channels and pixels, -10 log10).  Used to report the HIP render
    against the oracle's render of the same scene (BASELINE configs[4] names "PSNR vs reference")."""
    gt = np.clip(np.asarray(ground_truth, dtype=np.float64), 0.0, 1.0)
    pr = np.clip(np.asarray(predicted, dtype=np.float64), 0.0, 1.0)
    mse = float(((gt - pr) ** 2).mean())
    return float("inf") if mse == 0.0 else -10.0 * float(np.log10(mse))


PSNR_LOG: list = []     # (what, dB) records; tests/conftest.py prints them and adds them to parity_accounting.json


# ---- accounting of what the parity assertions actually held to the bar -------------------------
# Every call appends one record; tests/conftest.py prints the table at the end of the session and
# writes it to tests/_parity_accounting.json (so a reader sees how many pixels / rows were exempt).
ACCOUNTING: list = []


def _account(kind, what, total, strict, bounded, exempt, tol, scale, worst):
    ACCOUNTING.append(dict(kind=kind, what=what, total=int(total), held_to_bar=int(strict), flip_bounded=int(bounded),
                           exempt=int(exempt), tol=float(tol), scale=float(scale), worst_strict_err=float(worst)))


def assert_close_except_fragile(got, want, oracle_fwd, atol, what="", max_fragile_frac=0.02, flip_bound=2e-2, scale=1.0):
    """|got - want| <= atol on every pixel except those where the oracle saw an evaluation within
    float rounding of one of the algorithm's discontinuities (alpha == 1/255 skip, T == 1e-4 stop):
    there two correct float implementations may legitimately take different branches, which moves
    the pixel by up to alpha*T*c ~ 4e-3 (bounded at `flip_bound` = 2e-2 for unit-range channels; depth passes the bound
    in scene units).  Only such pixels may miss `atol` (at most
    2 % of the image may even be candidates); fragile pixels that meet the bar anyway count as held to
    it.  The counts are recorded in ACCOUNTING."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).reshape(-1, got.shape[-2], got.shape[-1]).max(0)
    frag = np.unique(oracle_fwd["fragile"][:, 0]) if len(oracle_fwd["fragile"]) else np.zeros(0, np.int64)
    assert not oracle_fwd["fragile_overflow"], f"{what}: fragile list overflow"
    assert len(frag) <= max(8, int(err.size * max_fragile_frac)), f"{what}: {len(frag)} of {err.size} pixels fragile (> {max_fragile_frac:.0%})"
    flat = err.reshape(-1)
    miss = flat > atol
    allowed = np.zeros(flat.size, bool)
    allowed[frag] = True
    stray = miss & ~allowed
    assert not stray.any(), f"{what}: {int(stray.sum())} non-fragile pixels off by more than {atol:.1e} (max abs err {flat[stray].max():.3e})"
    assert flat[miss].max(initial=0) <= flip_bound, f"{what}: fragile pixel moved more than one alpha step"
    # (`scale`: what `atol` was multiplied with — depth images are held to 1e-4 of the largest rendered depth, float32 sums
    # of values of 20-80; north_star's absolute 1e-4 is for latent / RGB — so that the accounting prints err / scale)
    _account("image", what, flat.size, flat.size - int(miss.sum()), int(miss.sum()), 0, atol / scale, scale, flat[~miss].max(initial=0))


def fragile_gaussians(oracle_fwd, W):
    """(direct, behind) for the gradient assertions.
    direct: Gaussians of the near-discontinuity evaluations themselves (either decision is correct;
            their own gradient moves by a flip-sized amount).
    behind: every OTHER Gaussian that contributes (alpha >= 1/255, power <= 0) to a pixel holding such
            an evaluation — its transmittance / accumulated-behind term changes if the decision flips.
            Gaussians of the pixel's tile list that do not reach the pixel are NOT affected and stay on
            the strict bar (round 1 exempted the whole tile list)."""
    fr = oracle_fwd["fragile"]
    if len(fr) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    gx = (W + 15) // 16
    xy, co = oracle_fwd["xy"].astype(np.float64), oracle_fwd["conic_opacity"].astype(np.float64)
    behind = []
    for pix in np.unique(fr[:, 0]):
        px, py = float(pix % W), float(pix // W)
        tile = (pix // W // 16) * gx + (pix % W) // 16
        s0, s1 = oracle_fwd["ranges"][tile]
        lst = oracle_fwd["point_list"][s0:s1].astype(np.int64)
        dx, dy = xy[lst, 0] - px, xy[lst, 1] - py
        power = -0.5 * (co[lst, 0] * dx * dx + co[lst, 2] * dy * dy) - co[lst, 1] * dx * dy
        alpha = np.minimum(0.99, co[lst, 3] * np.exp(np.minimum(power, 0.0)))
        behind.append(lst[(power <= 1e-6) & (alpha >= 1.0 / 255.0 - 1e-5)])
    direct = np.unique(fr[:, 1]).astype(np.int64)
    behind = np.setdiff1d(np.unique(np.concatenate(behind)), direct)
    return direct, behind


def assert_grad_close_except_fragile(got, want, direct, behind, tol, what="", min_strict=0.95, clean_tol=None, row_tol=None,
                                     max_direct_frac=0.01):
    """Per-Gaussian gradient rows against the oracle.  scale = max(1, max |want|) over the tensor.

    * Rows with no fragile evaluation nearby ("clean" rows — all but a fraction of a percent) are held to
      ``clean_tol * scale`` (default: ``tol``) and, when ``row_tol`` is given, ALSO to the per-row mixed bar
      ``row_tol * max(1, |want_row|_inf)`` — a small-magnitude row is then not hidden by the tensor's largest entry.
    * A row may miss the ``tol * scale`` bar ONLY if it belongs to a fragile evaluation (`direct`: either
      decision is correct, exempt) or shares a pixel with one (`behind`: flip-sized bound of 5e-3 * scale).
    * At least `min_strict` of all rows must be within ``tol * scale``.
    ACCOUNTING records the worst CLEAN row (err / scale and per-row mixed), i.e. the real arithmetic error of the
    kernels, next to the counts.  (tools/grad_budget.py splits that error further against a float64 evaluation.)"""
    got = np.asarray(got, np.float64).reshape(np.shape(want)[0], -1)
    want = np.asarray(want, np.float64).reshape(got.shape)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want).max(1)
    n = err.size
    assert len(direct) <= max(8, int(n * max_direct_frac)), f"{what}: too many fragile Gaussians ({len(direct)} of {n})"
    miss = err > tol * scale
    allowed = np.zeros(n, bool)
    allowed[direct] = True
    allowed[behind] = True
    stray = miss & ~allowed
    assert not stray.any(), (f"{what}: {int(stray.sum())} rows off the {tol:.0e} bar without a fragile evaluation nearby; "
                             f"max err {err[stray].max():.3e} (scale {scale:.3e}, row {int(np.argmax(np.where(stray, err, 0)))})")
    clean = ~allowed
    ctol = tol if clean_tol is None else clean_tol
    worst_clean = err[clean].max(initial=0)
    assert worst_clean <= ctol * scale, f"{what}: clean row off by {worst_clean:.3e} > {ctol:.0e} * scale ({scale:.3e})"
    row_mixed = err / np.maximum(1.0, np.abs(want).max(1))
    worst_row = row_mixed[clean].max(initial=0)
    if row_tol is not None:
        assert worst_row <= row_tol, f"{what}: clean row off by {worst_row:.3e} of max(1, |row|) > {row_tol:.0e}"
    is_direct = np.zeros(n, bool)
    is_direct[direct] = True
    bounded = miss & ~is_direct
    assert err[bounded].max(initial=0) <= 5e-3 * scale, f"{what}: {err[bounded].max():.3e} next to a fragile evaluation"
    n_miss = int(miss.sum())
    assert n - n_miss >= min_strict * n or n_miss <= 16, \
        f"{what}: only {n - n_miss} of {n} rows within the {tol:.0e} bar (< {min_strict:.0%})"
    _account("grad", what, n, n - n_miss, int(bounded.sum()), int((miss & is_direct).sum()), tol, scale, worst_clean)
    ACCOUNTING[-1].update(clean_rows=int(clean.sum()), worst_clean_row_mixed=float(worst_row), clean_tol=float(ctol),
                          row_tol=None if row_tol is None else float(row_tol))


def to_boundary(views, v, means3D, cov3D_precomp, opacities, shs, colors_precomp, features, feature_sh,
                shs_channel_major):
    """Host statement of what the kernels fuse: (scene-level inputs of view v) -> the tensors the
    reference hands to its rasterizer (scaled means, packed scaled covariance, (G,K,3) colour SH,
    evaluated latent features).  Pure torch, differentiable; used by the CPU stand-in below and by
    the gradient tests to chain oracle gradients back to scene-level inputs."""
    V = views.shape[0]
    # leading dim: one slice per view, or per scene (group of V / S consecutive views), or shared
    pv = lambda t, base: None if t is None else (t[v * t.shape[0] // V] if t.dim() == base + 1 else t)
    vw = views[v]
    scale = vw[40]
    means = pv(means3D, 2) * scale
    cov = cov3D_precomp
    full = cov.shape[-2:] == (3, 3)
    cov = pv(cov, 3 if full else 2)
    cov6 = (cs._pack_covariances(cov) if full else cov) * (scale * scale)   # same rounding as the kernel / reference
    sh = pv(shs, 3)
    if sh is not None and shs_channel_major:
        sh = sh.transpose(-1, -2)
    feats = pv(features, 2)
    if feature_sh is not None:
        fsh = pv(feature_sh, 3)
        from math import isqrt
        d = means - vw[32:35][None]
        d = d / d.norm(dim=-1, keepdim=True)
        feats = 0.5 + geometry.eval_sh(isqrt(fsh.shape[-1]) - 1, fsh, d)
    return means, cov6, pv(opacities, 2), sh, pv(colors_precomp, 2), feats


def oracle_rasterize_views(views, image_height, image_width, sh_degree, means3D, cov3D_precomp, opacities,
                           shs=None, colors_precomp=None, features=None, means2D=None, debug=False,
                           feature_sh=None, shs_channel_major=False):
    """CPU stand-in with the signature of latentsplat_amd.rasterizer.rasterize_views, served by the
    oracle.  TESTS ONLY: lets the not-gpu suite pin the host-side wrapper logic."""
    V = views.shape[0]
    n = lambda t: None if t is None else t.detach().cpu().float().contiguous().numpy()
    cols, feats, masks, depths, radii = [], [], [], [], []
    for v in range(V):
        vw = views[v].detach().cpu()
        view = orc.View(image_height, image_width, float(vw[35]), float(vw[36]), vw[37:40].numpy(),
                        vw[0:16].numpy().reshape(4, 4), vw[16:32].numpy().reshape(4, 4), vw[32:35].numpy(), sh_degree)
        m, c6, op, sh, cp, ft = to_boundary(views.detach().cpu(), v, means3D.detach().cpu(), cov3D_precomp.detach().cpu(),
                                            opacities.detach().cpu(), None if shs is None else shs.detach().cpu(),
                                            None if colors_precomp is None else colors_precomp.detach().cpu(),
                                            None if features is None else features.detach().cpu(),
                                            None if feature_sh is None else feature_sh.detach().cpu(), shs_channel_major)
        o = orc.forward(view, n(m), n(c6), n(op), n(sh), n(cp), n(ft), keep_intermediates=False)
        cols.append(o["color"]); feats.append(o["feature"]); masks.append(o["mask"]); depths.append(o["depth"])
        radii.append(o["radii"])
    st = lambda xs: None if xs[0] is None else torch.from_numpy(np.stack(xs))
    return st(cols), st(feats), st(masks), st(depths), st(radii)


# ---- frustum-edge scenes (tests/test_frustum_edges_*.py, tests/fuzz_parity.py mode "edges") ------------------------
# The projection has two geometric discontinuities the synthetic scenes above never reach: the clamp of the EWA
# Jacobian at |t.x / t.z| = 1.3 tanfov (t.y likewise) and the near cull t.z <= 0.2.  The builder below places Gaussians
# on and around both, with labels computed by float32 replicas of the forward's own expressions (lsr_project.h with
# FMA = false, raster_oracle.c): t = ((a0 b0 + a1 b1) + a2 b2) + b3, then the IEEE ratio t.x / t.z against 1.3f * tanfov.
EDGE_POPS = ("band", "outside", "near", "border", "wide", "wide_encoder")
NEAR_CULL = np.float32(0.2)
_F = np.float32


def f32_view_space(vm, p):
    """(G,3) view-space means of the forward: vm the (16,) view matrix in memory order, p (G,3) (scaled) means, all float32."""
    vm = np.asarray(vm, np.float32).reshape(16)
    p = np.asarray(p, np.float32)
    return np.stack([((vm[k] * p[:, 0] + vm[4 + k] * p[:, 1]) + vm[8 + k] * p[:, 2]) + vm[12 + k] for k in range(3)], -1)


def clamp_replica(bi: dict) -> dict:
    """Per (view, Gaussian) decisions of the forward for boundary inputs ``bi``: t (V,G,3); ratio = fl(t.x / t.z),
    fl(t.y / t.z) (V,G,2); lim = 1.3f * tanfov (V,2); clamped (V,G,2); clamped_rcp: the same decision taken on
    fl(t.x * fl(1 / t.z)) (a reciprocal formulation); clamped_f64: on the double ratio against 1.3 * (double)tanfov;
    culled (V,G): t.z <= 0.2."""
    c = bi["cams"]
    V = bi["V"]
    t = np.stack([f32_view_space(c.view_matrix[v].contiguous().numpy(), bi["means"][v].numpy()) for v in range(V)])
    tan = np.stack([c.tan_fov_x.numpy(), c.tan_fov_y.numpy()], -1).astype(np.float32)
    lim = _F(1.3) * tan
    with np.errstate(all="ignore"):
        ratio = t[..., :2] / t[..., 2:3]
        ratio_rcp = t[..., :2] * (_F(1.0) / t[..., 2:3])
        ratio64 = t[..., :2].astype(np.float64) / t[..., 2:3].astype(np.float64)
    L, L64 = lim[:, None, :], (1.3 * tan.astype(np.float64))[:, None, :]
    out = lambda r, l: (r < -l) | (r > l)
    return dict(t=t, ratio=ratio, lim=lim, clamped=out(ratio, L), clamped_rcp=out(ratio_rcp, L),
                clamped_f64=out(ratio64, L64), culled=~(t[..., 2] > NEAR_CULL))


def _rot(yaw, pitch, roll):
    cx, sx, cy, sy, cz, sz = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _edge_extrinsics(views, rng):
    """(V,4,4) camera-to-world float64: view 0 the identity, view 1 a fixed turned and shifted camera, further views random."""
    ext = np.tile(np.eye(4), (views, 1, 1))
    for v in range(1, views):
        if v == 1:
            ang, tr = (0.35, -0.2, 0.15), (0.3, -0.2, 0.1)
        else:
            ang, tr = rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.3, 0.3, 3)
        ext[v, :3, :3] = _rot(*ang)
        ext[v, :3, 3] = tr
    return ext


def _wide_extrinsics(views, rng, depth):
    """Target cameras of a wide baseline: turned by up to +-35 degrees (yaw, pitch; roll +-10) and moved by about half the
    scene depth ``depth``, mostly forwards into the cloud."""
    ext = np.tile(np.eye(4), (views, 1, 1))
    for v in range(views):
        a = np.radians(35.0)
        ext[v, :3, :3] = _rot(rng.uniform(-a, a), rng.uniform(-a, a), rng.uniform(-np.radians(10), np.radians(10)))
        ext[v, :3, 3] = depth * np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(0.35, 0.65)])
    return ext


def _edge_cameras(ext: np.ndarray):
    """The float32 view matrices / tangents boundary_inputs will hand to the rasterizer (near = 1: scene scale 1, so the
    world means ARE the rasterizer's means)."""
    V = ext.shape[0]
    e = torch.from_numpy(ext).float()
    intr = torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]]).repeat(V, 1, 1)
    near, far = torch.ones(V), torch.full((V,), 100.0)
    e2, nr, fr, _, _ = cs._scale_scene(e, near, far, torch.zeros(V, 1, 3), torch.zeros(V, 1, 3, 3))
    fov_x, fov_y = get_fov(intr).unbind(-1)
    return e, intr, near, far, cs._cameras(e2, nr, fr, fov_x, fov_y)


def _iso_cov(sig, rng, aniso=(0.5, 1.0)):
    """(G,3,3) float64 covariances with major standard deviation ``sig`` (G,), random orientation and axis ratios."""
    G = len(sig)
    q = rng.normal(size=(G, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(G, 3, 3)
    s = sig[:, None] * np.concatenate([np.ones((G, 1)), rng.uniform(*aniso, (G, 2))], 1)
    cov = R @ (s[:, :, None] ** 2 * np.eye(3)) @ R.transpose(0, 2, 1)
    return 0.5 * (cov + cov.transpose(0, 2, 1))


def _payload_sh(G, rng, color_sh_degree, feature_channels, feature_sh_degree):
    def att(deg):
        a = np.ones((deg + 1) ** 2)
        for d in range(1, deg + 1):
            a[d * d:(d + 1) ** 2] = 0.1 * 0.25 ** d
        return a
    csh = None if color_sh_degree is None else torch.from_numpy(rng.normal(size=(G, 3, (color_sh_degree + 1) ** 2)) * att(color_sh_degree)).float()
    fsh = None if not feature_channels else torch.from_numpy(
        0.3 * rng.normal(size=(G, feature_channels, (feature_sh_degree + 1) ** 2)) * att(feature_sh_degree)).float()
    return csh, fsh


def _band_means(cams, v, axis, sign, k, z, q, rng, n_cand=96):
    """World means (float32) of Gaussians whose forward ratio on ``axis`` in view v is exactly sign * (lim + k ulps),
    at depths ~z and perpendicular ratios ~q.  Among the hits, prefers the ones on which a reciprocal formulation
    (fl(t.x * fl(1 / t.z))) or a decision in double decides differently from the forward."""
    vm = cams.view_matrix[v].contiguous().numpy().reshape(16)
    tan = np.array([float(cams.tan_fov_x[v]), float(cams.tan_fov_y[v])], np.float32)
    lim = _F(1.3) * tan[axis]
    target = lim
    for _ in range(abs(k)):
        target = np.nextafter(target, _F(np.inf) if k > 0 else _F(0.0))
    target = _F(sign) * target
    c2w = np.linalg.inv(vm.astype(np.float64).reshape(4, 4).T)   # memory order is the transposed world-to-camera matrix
    picks = []
    for zi, qi in zip(z, q):
        zz = zi * (1.0 + 1e-3 * rng.uniform(-1, 1, n_cand))
        r = np.float64(target) * (1.0 + 2.0 ** -23 * rng.uniform(-3, 3, n_cand))
        cam = np.zeros((n_cand, 4))
        cam[:, axis], cam[:, 1 - axis], cam[:, 2], cam[:, 3] = r * zz, qi * tan[1 - axis] * zz, zz, 1.0
        w = (cam @ c2w.T)[:, :3].astype(np.float32)
        t = f32_view_space(vm, w)
        rat = t[:, axis] / t[:, 2]
        hit = rat.view(np.uint32) == np.asarray(target, np.float32).view(np.uint32)
        if not hit.any():
            continue
        out_f = np.abs(rat) > lim
        out_rcp = np.abs(t[:, axis] * (_F(1.0) / t[:, 2])) > lim
        out_64 = np.abs(t[:, axis].astype(np.float64) / t[:, 2].astype(np.float64)) > 1.3 * np.float64(tan[axis])
        score = np.where(hit, 1 + 2 * (out_rcp != out_f) + (out_64 != out_f), 0)
        picks.append(w[int(np.argmax(score))])
    return picks


def make_edge_scene(pop: str, H: int = 64, W: int = 64, views: int = 2, seed: int = 0, color_sh_degree=None,
                    feature_channels=4, feature_sh_degree: int = 0, filler: int = 200):
    """A Scene at the frustum edges plus its labels.  ``pop``:
      band    — for each side (+-x, +-y) of view 0 (identity: t = mean exactly) and view 1 (turned: t is rounded) and
                k = -4..4, a Gaussian whose forward ratio fl(t.x / t.z) is exactly sign * (fl(1.3f tanfov) + k ulps); footprints
                of tens of pixels reaching into the image, in front of everything else (`filler` Gaussians behind);
      outside — means at 1.3-3x tanfov off each side of views 0 and 1 (clamped Jacobian) whose footprints cover the border;
      near    — view-0 depths prev(0.2f), 0.2f, next(0.2f), 0.21, 0.25, 0.3, 0.5, on- and off-axis, footprints from a few
                pixels to several images;
      border  — view-0 centres off-screen whose tile rectangle reaches exactly one edge tile row / column, and footprints
                covering every tile;
      wide / wide_encoder — a make_scene cloud / an encoder-shaped cloud seen from wide-baseline targets (turned up to
                +-35 degrees, moved by half the scene depth): some Gaussians behind the camera, some clamped, some near the cull.
    Returns (scene, labels): labels = clamp_replica(...) of the scene's boundary inputs plus per-Gaussian `kind`
    ("filler" 0, "band" 1, "outside" 2, "near" 3, "border" 4, "cover" 5, "cloud" 6) and, for band Gaussians, band_view /
    band_axis / band_sign / band_k (-99 elsewhere)."""
    from latentsplat_amd.synthetic import make_encoder_scene
    assert pop in EDGE_POPS, pop
    rng = np.random.default_rng(seed)
    size = max(H, W)
    if pop in ("wide", "wide_encoder"):
        if pop == "wide":
            sc = make_scene(10 * max(filler, 100), image_size=size, views=1, color_sh_degree=color_sh_degree,
                            feature_channels=feature_channels, feature_sh_degree=feature_sh_degree, seed=seed)
        else:
            sc = make_encoder_scene(context_views=2, size=max(8, size // 4), samples=2, views=1, color_sh_degree=color_sh_degree,
                                    feature_channels=feature_channels, feature_sh_degree=feature_sh_degree, seed=seed)
        depth = float(np.median(sc.means[:, 2].numpy()))
        sc.extrinsics = torch.from_numpy(_wide_extrinsics(views, rng, depth)).float()
        sc.intrinsics = sc.intrinsics[:1].repeat(views, 1, 1)
        sc.near, sc.far = sc.near[:1].repeat(views), sc.far[:1].repeat(views)
        G = sc.means.shape[0]
        kind = np.full(G, 6, np.int32)
        lab = dict(kind=kind)
    else:
        views = max(views, 2 if pop in ("band", "outside") else 1)
        ext = _edge_extrinsics(views, rng)
        e, intr, near, far, cams = _edge_cameras(ext)
        c2w = [np.linalg.inv(cams.view_matrix[v].double().numpy().T) for v in range(views)]
        tan = np.stack([cams.tan_fov_x.numpy(), cams.tan_fov_y.numpy()], -1).astype(np.float64)
        focal = np.stack([W / (2 * tan[:, 0]), H / (2 * tan[:, 1])], -1)
        means, sig, opac, kind = [], [], [], []
        band = dict(band_view=[], band_axis=[], band_sign=[], band_k=[])

        def cam_to_world(v, cam):   # (n,3) camera space of view v -> float32 world
            c = np.concatenate([cam, np.ones((len(cam), 1))], 1)
            return (c @ c2w[v].T)[:, :3].astype(np.float32)

        if pop == "band":
            for v in (0, 1):
                for axis in (0, 1):
                    for sign in (1, -1):
                        for k in range(-4, 5):
                            z = rng.uniform(2.5, 4.0, 3)
                            w = _band_means(cams, v, axis, sign, k, z, rng.uniform(-0.6, 0.6, 3), rng)
                            assert w, f"band: no mean found for view {v} axis {axis} sign {sign} k {k}"
                            means.append(w[0][None])
                            zc = 3.25
                            sig.append([rng.uniform(0.12, 0.22) * size * zc / focal[v, axis]])
                            opac.append([rng.uniform(0.4, 0.8)])
                            kind.append([1])
                            for key, val in zip(band, (v, axis, sign, k)):
                                band[key].append(val)
        elif pop == "outside":
            for v in (0, 1):
                for axis in (0, 1):
                    for sign in (1, -1):
                        n = 5
                        z = rng.uniform(2.5, 4.0, n)
                        r = rng.uniform(1.3, 3.0, n) * tan[v, axis]
                        cam = np.zeros((n, 3))
                        cam[:, axis], cam[:, 1 - axis], cam[:, 2] = sign * r * z, rng.uniform(-0.6, 0.6, n) * tan[v, 1 - axis] * z, z
                        means.append(cam_to_world(v, cam))
                        d_px = (r / tan[v, axis] - 1.0) * (W if axis == 0 else H) / 2   # centre to image edge
                        sig.append((d_px + rng.uniform(0.05, 0.3, n) * size) / 3.0 * z / focal[v, axis])
                        opac.append(rng.uniform(0.2, 0.7, n))
                        kind.append(np.full(n, 2))
        elif pop == "near":
            zs = [np.nextafter(NEAR_CULL, _F(0)), NEAR_CULL, np.nextafter(NEAR_CULL, _F(1)), _F(0.21), _F(0.25), _F(0.3), _F(0.5)]
            for z in zs:
                for rx, ry in ((0.0, 0.0), (0.45, -0.3), (-0.7, 0.55), (1.1, 0.2)):
                    for s_px in (2.0, 8.0, 40.0, 200.0):
                        s_px *= size / 64
                        # the mean exactly: view 0 is the identity, so t = mean and t.z = z bit for bit
                        means.append(np.array([[_F(rx * tan[0, 0] * z), _F(ry * tan[0, 1] * z), z]], np.float32))
                        sig.append([s_px * float(z) / focal[0, 0]])
                        opac.append([rng.uniform(0.3, 0.8) if s_px < size else rng.uniform(0.03, 0.15)])
                        kind.append([3])
        else:   # border: candidates, kept by what the oracle's forward makes of them
            cand = []
            for side in range(4):   # left, right, top, bottom
                n = 48
                d = rng.uniform(0.3, 30.0, n)                  # centre this far outside the image, pixels
                r = d + rng.uniform(1.0, 15.0, n)              # radius aimed at one edge tile
                along = rng.uniform(0.2, 0.8, n) * (H if side < 2 else W)
                pxy = np.zeros((n, 2))
                if side < 2:
                    pxy[:, 0], pxy[:, 1] = (-d if side == 0 else W - 1 + d), along
                else:
                    pxy[:, 0], pxy[:, 1] = along, (-d if side == 2 else H - 1 + d)
                cand.append((pxy, r / 3.0, np.full(n, 4)))
            pxy = np.array([[-20.0, -30.0], [W + 25.0, -10.0], [-5.0, H + 40.0], [W + 60.0, H + 60.0]])
            cand.append((pxy, np.full(4, 1.2 * size), np.full(4, 5)))
            for pxy, s_px, kd in cand:
                z = rng.uniform(3.0, 5.0, len(pxy))
                cam = np.stack([((2 * pxy[:, 0] + 1) / W - 1) * tan[0, 0] * z, ((2 * pxy[:, 1] + 1) / H - 1) * tan[0, 1] * z, z], -1)
                means.append(cam_to_world(0, cam))
                sig.append(s_px * z / focal[0, 0])
                opac.append(rng.uniform(0.2, 0.7, len(pxy)))
                kind.append(kd)
        m_edge = np.concatenate(means).astype(np.float32)
        sig = np.concatenate([np.asarray(s, np.float64) for s in sig])
        n_edge = len(m_edge)
        # filler: an ordinary cloud behind the edge Gaussians (view-0 pixel uniform in [-0.1, 1.1]^2, depth 5-12)
        u, vv = rng.uniform(-0.1, 1.1, (2, filler))
        zf = rng.uniform(5.0, 12.0, filler)
        m_fill = cam_to_world(0, np.stack([(2 * u - 1) * tan[0, 0] * zf, (2 * vv - 1) * tan[0, 1] * zf, zf], -1))
        s_fill = rng.uniform(0.5, 4.0, filler) * size / 64 * zf / focal[0, 0]
        G = n_edge + filler
        cov = _iso_cov(np.concatenate([sig, s_fill]), rng)
        op = np.concatenate([np.concatenate([np.atleast_1d(o) for o in opac]), rng.uniform(0.05, 0.4, filler)])
        csh, fsh = _payload_sh(G, rng, color_sh_degree, feature_channels, feature_sh_degree)
        sc = Scene(torch.from_numpy(np.concatenate([m_edge, m_fill])), torch.from_numpy(cov).float(),
                   torch.from_numpy(op).float(), csh, fsh, e, intr, near, far)
        kind = np.concatenate([np.concatenate([np.atleast_1d(k) for k in kind]), np.zeros(filler)]).astype(np.int32)
        lab = dict(kind=kind)
        for key, val in band.items():
            a = np.full(G, -99, np.int32)
            a[:len(val)] = val
            lab[key] = a
        if pop == "border":   # keep the candidates whose rectangle does what they were made for (per-Gaussian results)
            o = oracle_forward(boundary_inputs(sc, H, W), 0)
            gx, gy = (W + 15) // 16, (H + 15) // 16
            rect, xy = o["rect"], o["xy"]
            one_col = ((rect[:, 2] - rect[:, 0]) == 1) & ((rect[:, 0] == 0) | (rect[:, 2] == gx))
            one_row = ((rect[:, 3] - rect[:, 1]) == 1) & ((rect[:, 1] == 0) | (rect[:, 3] == gy))
            off = (xy[:, 0] < -0.5) | (xy[:, 0] > W - 0.5) | (xy[:, 1] < -0.5) | (xy[:, 1] > H - 0.5)
            edge_ok = (o["radii"] > 0) & off & (one_col | one_row)
            cover_ok = (o["radii"] > 0) & off & (rect == np.array([0, 0, gx, gy])).all(1)
            keep = np.flatnonzero(((kind == 4) & edge_ok) | ((kind == 5) & cover_ok) | (kind == 0))
            sc = Scene(sc.means[keep], sc.covariances[keep], sc.opacities[keep], None if csh is None else csh[keep],
                       None if fsh is None else fsh[keep], e, intr, near, far)
            lab = {k: v[keep] for k, v in lab.items()}
    lab.update(clamp_replica(boundary_inputs(sc, H, W)))
    _check_edge_labels(pop, lab)
    return sc, lab


def _check_edge_labels(pop, lab):
    """What each population claims, on the float32 replicas (the builder asserts it; tests/test_frustum_edges_cpu.py too)."""
    kind = lab["kind"]
    if pop == "band":
        b = np.flatnonzero(kind == 1)
        v, ax, sg, k = (lab[n][b] for n in ("band_view", "band_axis", "band_sign", "band_k"))
        rat = lab["ratio"][v, b, ax]
        lim = lab["lim"][v, ax]
        steps = np.rint((np.abs(rat).astype(np.float64) - lim) / np.spacing(lim)).astype(int)
        assert (np.sign(rat) == sg).all() and (steps == k).all(), "band: ratio is not lim + k ulps"
        assert (lab["clamped"][v, b, ax] == (k > 0)).all() and not lab["culled"][v, b].any()
        assert (lab["clamped_rcp"][v, b, ax] != lab["clamped"][v, b, ax]).any(), \
            "band: no Gaussian on which fl(x / z) and fl(x fl(1 / z)) decide differently"
        for side in ((0, 0, 1), (0, 0, -1), (0, 1, 1), (0, 1, -1), (1, 0, 1), (1, 0, -1), (1, 1, 1), (1, 1, -1)):
            sel = (v == side[0]) & (ax == side[1]) & (sg == side[2])
            assert set(k[sel]) == set(range(-4, 5)), side
    elif pop == "outside":
        b = np.flatnonzero(kind == 2)
        assert lab["clamped"][:2, b].any(-1).any(0).all() and not lab["culled"][0, b].any()
    elif pop == "near":
        b = kind == 3
        z = lab["t"][0, :, 2]
        assert (lab["culled"][0, b] == (z[b] <= NEAR_CULL)).all()
        assert lab["culled"][0, b].any() and (~lab["culled"][0, b]).any()
        assert (z[b] == np.nextafter(NEAR_CULL, _F(1))).any() and (z[b] == NEAR_CULL).any()
    elif pop == "border":
        assert (kind == 4).sum() >= 4 and (kind == 5).sum() >= 1, "border: too few candidates kept"
    else:
        vis = ~lab["culled"]
        assert (lab["t"][..., 2] < 0).any(), f"{pop}: no Gaussian behind a camera"
        assert (lab["clamped"].any(-1) & vis).any(), f"{pop}: no clamped Gaussian in front of a camera"
        assert (vis & (lab["t"][..., 2] < 0.9)).any(), f"{pop}: no Gaussian in the band 0.2 < z < 0.9"
