"""Reference for the antialiased rasterization mode (``LSR_FWD_ANTIALIAS``): the opacity factor

    rho = sqrt(max(0.000025, det0 / det)),   det0 = a0 c0 - b^2,   det = (a0 + 0.3)(c0 + 0.3) - b^2

per (view, Gaussian), stated in torch from the view table, the means and the covariances — in float64 (the reference,
differentiable by autograd) and, the same composition, in float32 (the "stock" baseline: the error a float32 statement
of the same formula makes by itself).  (a0, b, c0) is the EWA projection of the 3D covariance, M S M^T with M = J W; the
clamp of the Jacobian follows the rasterizer's convention (``oracle.torch_oracle._clamp_mask``: the float32 decision of the
forward, and a clamped t.x / t.z is a constant).

The project's rule for a kernel against such a pair (tests/latent_ref.py): the kernel's error against float64 may be at most
``MARGIN`` = 4 x the stock composition's own worst error on the same case (and never needs to be below the float32 floor
given with each check).  ``WORST`` collects the measured ratios; the tests print them.

Also here: the C-ABI driver of the tests (:class:`Run`, tests/util.py ``HipRun`` over arbitrary dims), and the numpy replay
of the compositing rule for one isolated Gaussian.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.torch_oracle import _clamp_mask
from tests import util

LOWPASS = 0.3
FLOOR = 0.000025          # the published rasterizer's: rho >= 0.005
MARGIN = 4.0
WORST: dict = {}


def rho(views: torch.Tensor, means: torch.Tensor, cov: torch.Tensor, H: int, W: int, dtype=torch.float64,
        views_per_group: int = 0) -> torch.Tensor:
    """(V, G) opacity factors.  ``views`` (V, 44) table; ``means`` (G, 3) or (S, G, 3); ``cov`` (.., G, 6) packed or
    (.., G, 3, 3); S = V (per view) or V / views_per_group (per scene).  Everything is cast to ``dtype`` first (the clamp
    decision is always the forward's float32 one).  Differentiable in all three."""
    V = views.shape[0]
    out = []
    for v in range(V):
        s = v // views_per_group if views_per_group > 1 else v
        vw = views[v]
        m = means if means.dim() == 2 else means[s]
        full = cov.shape[-2:] == (3, 3)
        c = cov if cov.dim() == (3 if full else 2) else cov[s]
        # the float32 decision of the forward, on its float32 scaled means
        vm32 = vw[:16].detach().float().reshape(4, 4)
        inx, iny = _clamp_mask(vm32, m.detach().float() * vw[40].detach().float(), float(vw[35].detach()), float(vw[36].detach()))
        vwd, m, c = vw.to(dtype), m.to(dtype), c.to(dtype)
        vm = vwd[:16].reshape(4, 4)          # memory order: the transposed world-to-view matrix
        scale, tanx, tany = vwd[40], vwd[35], vwd[36]
        p = m * scale
        if full:
            S = c * (scale * scale)
        else:
            c = c * (scale * scale)
            S = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], -1).reshape(-1, 3, 3)
        t = p @ vm[:3, :3] + vm[3, :3]
        tz = t[:, 2]
        limx, limy = 1.3 * tanx.detach(), 1.3 * tany.detach()
        cx = (torch.minimum(limx, torch.maximum(-limx, t[:, 0] / tz)) * tz).detach()
        cy = (torch.minimum(limy, torch.maximum(-limy, t[:, 1] / tz)) * tz).detach()
        tx, ty = torch.where(inx, t[:, 0], cx), torch.where(iny, t[:, 1], cy)
        fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
        zero = torch.zeros_like(tz)
        J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], -1),
                         torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], -1)], 1)      # (G, 2, 3)
        M = J @ vm[:3, :3].T
        c2 = M @ S @ M.transpose(1, 2)
        a0, b, c0 = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
        det0 = a0 * c0 - b * b
        det = (a0 + LOWPASS) * (c0 + LOWPASS) - b * b
        out.append(torch.sqrt(torch.clamp_min(det0 / det, FLOOR)))
    return torch.stack(out)


def closed_form_isotropic(sigma2):
    """rho of a 2D covariance sigma^2 I."""
    return sigma2 / (sigma2 + LOWPASS)


def held(name: str, got, want, stock, floor: float, show: str = "") -> float:
    """max |got - want| <= max(MARGIN x max |stock - want|, floor); prints the three numbers and records the ratio."""
    got, want, stock = (np.asarray(x, np.float64) for x in (got, want, stock))
    assert np.isfinite(got).all(), (show, name, "non-finite values")
    err = float(np.abs(got - want).max(initial=0.0))
    err_stock = float(np.abs(stock - want).max(initial=0.0))
    bar = max(MARGIN * err_stock, floor)
    ratio = err / err_stock if err_stock > 0 else (0.0 if err == 0 else float("inf"))
    WORST[name] = max(WORST.get(name, 0.0), ratio if np.isfinite(ratio) else 0.0)
    print(f"{show:28s} {name:12s} kernel {err:.3e}  stock {err_stock:.3e}  ratio {ratio:.3f}  bar {bar:.3e}")
    assert err <= bar, (show, name, err, err_stock, bar)
    return ratio


class Run(util.HipRun):
    """``util.HipRun`` (prepare + render through the C ABI, workspaces kept) for arbitrary dims and device tensors."""

    def __init__(self, views, means, cov, opac, color, features, dims):
        self.views, self.means, self.cov6, self.opac, self.color, self.features = views, means, cov, opac, color, features
        self._forward(dims, views.device)

    def record_opacity(self) -> np.ndarray:
        """(V, G) slot 5 of the screen records."""
        return self.q()[1][:, :, 1].copy()

    def half_entries(self) -> list:
        """The valid part of every half-tile render list, as a list of uint32 arrays in (view, tile, half) order."""
        ts, hc, hl = self.tile_start(), self.half_count(), self.half_list()
        out = []
        for t in range(self.d.num_views * self.T):
            s0, n = ts[t], ts[t + 1] - ts[t]
            for h in range(2):
                out.append(hl[2 * s0 + h * n: 2 * s0 + h * n + hc[t, h]])
        return out


def assert_same_render(a: Run, b: Run, what: str) -> None:
    """Everything a forward leaves behind, bit for bit: images, radii, n_contrib, final_T, tile offsets, the canonical point
    list and the half-tile render lists."""
    eq = lambda x, y: (x is None and y is None) or torch.equal(x, y)
    assert eq(a.color_out, b.color_out), f"{what}: colour"
    assert eq(a.feat_out, b.feat_out), f"{what}: features"
    assert eq(a.mask_out, b.mask_out), f"{what}: mask"
    assert eq(a.depth_out, b.depth_out), f"{what}: depth"
    assert torch.equal(a.radii, b.radii), f"{what}: radii"
    assert a.P == b.P and a.maxtile == b.maxtile, f"{what}: pair counts {a.P, a.maxtile} vs {b.P, b.maxtile}"
    assert np.array_equal(a.n_contrib(), b.n_contrib()), f"{what}: n_contrib"
    assert np.array_equal(a.final_T().view(np.uint32), b.final_T().view(np.uint32)), f"{what}: final_T"
    assert np.array_equal(a.tile_start(), b.tile_start()), f"{what}: tile_start"
    assert np.array_equal(a.point_list(), b.point_list()), f"{what}: point list"
    assert np.array_equal(a.half_count(), b.half_count()), f"{what}: half-tile list lengths"
    ha, hb = a.half_entries(), b.half_entries()
    assert all(np.array_equal(x, y) for x, y in zip(ha, hb)), f"{what}: half-tile lists"


# ---- one isolated Gaussian: what the mode is for -------------------------------------------------------------------------
def isolated_draws(n: int, seed: int = 0) -> np.ndarray:
    """(n, 5): axis standard deviations s1, s2 in [0.2, 1.5] px (uniform), orientation in [0, pi), pixel-space mean in
    [24, 40)^2 of a 64 x 64 view (uniform: every sub-pixel phase)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.2, 1.5, n), rng.uniform(0.2, 1.5, n), rng.uniform(0.0, np.pi, n),
                     rng.uniform(24.0, 40.0, n), rng.uniform(24.0, 40.0, n)], -1)


def isolated_cov2d(draw):
    s1, s2, th = draw[..., 0], draw[..., 1], draw[..., 2]
    c, s = np.cos(th), np.sin(th)
    a0 = c * c * s1 * s1 + s * s * s2 * s2
    c0 = s * s * s1 * s1 + c * c * s2 * s2
    b = c * s * (s1 * s1 - s2 * s2)
    return a0, b, c0


def _isolated_alpha(draw, opacity: float, antialiasing: bool, size: int):
    a0, b, c0 = isolated_cov2d(draw)
    a, c = a0 + LOWPASS, c0 + LOWPASS
    det, det0 = a * c - b * b, a0 * c0 - b * b
    o = opacity * (np.sqrt(max(FLOOR, det0 / det)) if antialiasing else 1.0)
    A, B, C = c / det, -b / det, a / det
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float64)
    dx, dy = draw[3] - xs, draw[4] - ys
    power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
    alpha = np.minimum(0.99, o * np.exp(power))
    alpha[power > 0] = 0.0
    return alpha, o, (a, b, c)


def isolated_mask_sum(draw, opacity: float, antialiasing: bool, size: int = 64) -> float:
    """Numpy replay of the compositing rule for one Gaussian over a size x size view: alpha = min(0.99, o' G), dropped below
    1/255 (and where the exponent is positive); the mask of a single Gaussian is its alpha.  float64."""
    alpha = _isolated_alpha(draw, opacity, antialiasing, size)[0]
    return float(alpha[alpha >= 1.0 / 255.0].sum())


def isolated_expected_fraction(draw, opacity: float) -> float:
    """What the 1/255 cut leaves of the light, as an integral: a 2D Gaussian of peak o' holds the fraction t / o' of its mass
    below the level t, so the antialiased splat emits (1 - (1/255) / (o rho)) of 2 pi o sqrt(det0).  A sum over pixel centres
    at a uniformly random sub-pixel phase has exactly this integral as its expectation."""
    a0, b, c0 = isolated_cov2d(draw)
    rho = np.sqrt(max(FLOOR, (a0 * c0 - b * b) / ((a0 + LOWPASS) * (c0 + LOWPASS) - b * b)))
    return float(1.0 - (1.0 / 255.0) / (opacity * rho))


def isolated_sampling_bound(draw, opacity: float, size: int = 64) -> float:
    """A worst-case bound on |pixel sum / integral above the cut - 1| at ONE phase, relative to 2 pi o sqrt(det0), in two parts.
    The smooth part: by Poisson summation the sum of a Gaussian of covariance S over the unit lattice is its integral times
    (1 + sum_{k != 0} exp(-2 pi^2 k^T S k) cos(..)), so the sum over k != 0 of exp(-2 pi^2 k^T S k) bounds it at every phase
    (S has the 0.3 low-pass: below 0.5 %).  The cut: the level line alpha = 1/255 runs through the cells of the border pixels
    (those above the cut with a 4-neighbour below it, and the reverse); the replay takes such a pixel whole or not at all where
    the integral takes the part of its cell inside the line, so each is misstated by at most its own alpha.  The misstatements
    of neighbouring border pixels largely cancel, so the bound is loose — the measured deviations are a tenth of it — but
    it needs no assumption about the phase.  Near 0.2 x 0.2 px, where seven pixels carry the splat and all but one are border
    pixels, nothing tighter holds: a single pixel dropping under the cut moves the sum by several percent."""
    alpha, _, (a, b, c) = _isolated_alpha(draw, opacity, True, size)
    k = np.mgrid[-3:4, -3:4].reshape(2, -1).T
    k = k[(k != 0).any(1)]
    smooth = float(np.exp(-2.0 * np.pi ** 2 * (a * k[:, 0] ** 2 + 2.0 * b * k[:, 0] * k[:, 1] + c * k[:, 1] ** 2)).sum())
    above = alpha >= 1.0 / 255.0

    def near(m):
        p = np.pad(m, 1)
        return p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]

    border = (above & near(~above)) | (~above & near(above))
    return smooth + float(alpha[border].sum()) / isolated_want(draw, opacity)


def isolated_want(draw, opacity: float) -> float:
    """The light of the undilated Gaussian: 2 pi o sqrt(det0)."""
    a0, b, c0 = isolated_cov2d(draw)
    return float(2.0 * np.pi * opacity * np.sqrt(a0 * c0 - b * b))
