"""Antialiased rasterization (``LSR_FWD_ANTIALIAS``), what needs no GPU: the flag word's validation, the
settings tuple, the reference's closed forms and the replay of what the mode is for."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import Dims, Inputs
from tests import antialias_ref as ref


def _dims(**kw):
    base = dict(num_views=2, num_gaussians=1000, height=64, width=64, feat_channels=4, color_mode=0,
                sh_degree=0, sh_coeffs=0, vs_means=0, vs_cov=0, vs_opac=0, vs_color=0, vs_feat=0,
                cov_elems=6, feat_mode=0, feat_sh_degree=0, feat_sh_coeffs=0)
    base.update(kw)
    return Dims(**base)


def _prepare_rc(d):
    lib = _lib.load()
    npairs, maxtile = C.c_int64(0), C.c_int32(0)
    return lib.lsr_forward_prepare(C.byref(d), C.byref(Inputs()), None, None, C.byref(npairs), C.byref(maxtile), None)


def test_flag_value():
    assert _lib.FWD_ANTIALIAS == 32 and _lib.ABI_VERSION == 10


@pytest.mark.parametrize("flags", [32, 32 | 1, 32 | 2, 32 | 4, 32 | 8, 32 | 1 | 2 | 4 | 8])
def test_antialias_bit_is_accepted(flags):
    """Alone and with every existing bit: the dims pass validation (a size comes back, and prepare gets as far as its
    null-pointer check: LSR_ENULL, not LSR_EINVAL)."""
    lib = _lib.load()
    d = _dims(forward_flags=flags)
    assert lib.lsr_geom_workspace_bytes(C.byref(d)) == lib.lsr_geom_workspace_bytes(C.byref(_dims(forward_flags=flags & ~32))) > 0
    assert _prepare_rc(d) == -2


@pytest.mark.parametrize("flags", [64, 32 | 64, 16, 32 | 16])
def test_other_bits_stay_rejected(flags):
    lib = _lib.load()
    d = _dims(forward_flags=flags)
    assert lib.lsr_geom_workspace_bytes(C.byref(d)) == 0
    assert _prepare_rc(d) == -1


def test_settings_tuple_keeps_its_twelve_positional_fields():
    import diff_gaussian_rasterization as dgr
    from latentsplat_amd.rasterizer import GaussianRasterizationSettings
    assert dgr.GaussianRasterizationSettings is GaussianRasterizationSettings
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(64, 64, 0.6, 0.6, torch.zeros(3), 1.0, eye, eye, 0, torch.zeros(3), False, False)
    assert rs.antialiasing is False and len(rs) == 13 and rs._fields[-1] == "antialiasing"
    assert GaussianRasterizationSettings(64, 64, 0.6, 0.6, torch.zeros(3), 1.0, eye, eye, 0, torch.zeros(3), False, False,
                                         True).antialiasing is True
    assert rs._replace(antialiasing=True).antialiasing is True


def _identity_view(H=64, W=64, tan=0.625):
    """A (1, 44) table of the identity camera (the projection matrix plays no part in rho)."""
    v = torch.zeros(1, 44, dtype=torch.float64)
    v[0, :16] = torch.eye(4, dtype=torch.float64).reshape(-1)
    v[0, 16:32] = torch.eye(4, dtype=torch.float64).reshape(-1)
    v[0, 35], v[0, 36], v[0, 40] = tan, tan, 1.0
    return v


def test_closed_forms():
    """On the optical axis of the identity camera J = diag(f / z, f / z): a world covariance s^2 I projects to
    sigma^2 I with sigma = f s / z, and rho = sigma^2 / (sigma^2 + 0.3).  A zero covariance (det0 = 0) takes the floor:
    sqrt(0.000025) = 0.005, and so does a rank-1 covariance."""
    H = W = 64
    views = _identity_view(H, W)
    f = W / (2.0 * 0.625)
    z = torch.tensor([2.0, 3.0, 5.0, 9.0], dtype=torch.float64)
    sigma2 = torch.tensor([0.01, 0.3, 1.7, 40.0], dtype=torch.float64)
    s2 = sigma2 * (z / f) ** 2
    means = torch.stack([torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), z], -1)
    cov = torch.zeros(4, 6, dtype=torch.float64)
    cov[:, 0] = cov[:, 3] = cov[:, 5] = s2
    got = ref.rho(views, means, cov, H, W)[0]
    assert torch.allclose(got, ref.closed_form_isotropic(sigma2), rtol=1e-12, atol=0)
    got32 = ref.rho(views, means, cov, H, W, dtype=torch.float32)[0]
    assert got32.dtype == torch.float32 and torch.allclose(got32.double(), got, rtol=1e-5)
    zero = ref.rho(views, means, torch.zeros(4, 6, dtype=torch.float64), H, W)[0]
    assert torch.equal(zero, torch.full((4,), 0.000025, dtype=torch.float64).sqrt()) and abs(float(zero[0]) - 0.005) < 1e-15
    rank1 = torch.zeros(4, 6, dtype=torch.float64)
    rank1[:, 0] = s2
    assert torch.allclose(ref.rho(views, means, rank1, H, W)[0], zero)
    # 3 x 3 covariances and a scene scale s (means s x, covariances s^2 Sigma: the scaled scene is the same picture)
    full = torch.diag_embed(torch.stack([s2, s2, s2], -1))
    assert torch.allclose(ref.rho(views, means, full, H, W)[0], got, rtol=1e-12)
    scaled = views.clone()
    scaled[0, 40] = 0.5
    assert torch.allclose(ref.rho(scaled, 2.0 * means, 4.0 * cov, H, W)[0], got, rtol=1e-12)


def test_reference_is_differentiable_and_constant_at_the_floor():
    H = W = 64
    views = _identity_view(H, W).requires_grad_(True)
    means = torch.tensor([[0.3, -0.2, 3.0], [0.1, 0.4, 4.0], [4.0, 0.1, 3.0]], dtype=torch.float64, requires_grad=True)
    cov = torch.tensor([[2e-4, 1e-5, 0, 3e-4, 0, 2e-4], [0, 0, 0, 0, 0, 0], [3e-4, 0, 0, 2e-4, 0, 4e-4]], dtype=torch.float64,
                       requires_grad=True)
    r = ref.rho(views, means, cov, H, W)[0]
    r.sum().backward()
    assert all(torch.isfinite(t.grad).all() for t in (views, means, cov))
    assert cov.grad[0].abs().max() > 0 and means.grad[0].abs().max() > 0 and views.grad[0, :16].abs().max() > 0
    assert cov.grad[1].abs().max() == 0 and means.grad[1].abs().max() == 0      # the floor: a constant
    # Gaussian 2 is outside 1.3 tan(fov) in x: its clamped t.x / t.z is a constant, so rho does not depend on mean.x there
    g = torch.autograd.grad(ref.rho(views, means, cov, H, W)[0, 2], means)[0]
    assert g[2, 0] == 0 and g[2, 2] != 0


def test_replay_of_one_isolated_gaussian():
    """What the mode is for, on the compositing rule itself (numpy, float64; 1/255 cut, 0.99 clamp): one Gaussian of opacity 0.9
    with axes of 0.2-1.5 px, 2 000 seeded draws with uniform sub-pixel phases.  With the mode on, the summed alpha is the light
    of the UNDILATED Gaussian, 2 pi o sqrt(det0), less what the cut removes, (1/255) / (o rho) of it (0.5 % at 1.5 x 1.5 px,
    3.7 % at 0.2 x 0.2 px):
      * exactly so in the mean — the expectation of a sum over pixel centres at a uniform phase IS the integral, so the
        deviations of the draws are independent with mean zero: their average is held to 4 standard errors (2e-4);
      * at a single phase up to the worst-case sampling bound of tests/antialias_ref.py (smooth part by Poisson summation,
        border pixels of the cut misstated by at most their own alpha), draw by draw.
    The largest single deviation from 2 pi o sqrt(det0) itself depends on the draws — 4.1 %, 3.2 %, 3.9 %, 10.6 % for seeds
    0-3 (the last at 0.208 x 0.215 px, where a border pixel falls under the cut) — so no fixed percentage over 2 000 draws is
    a property of the mode, and none is asserted here; it is printed.  tests/test_antialias_gpu.py holds the kernels to 5 % at
    six fixed draws.  The classic mode misses by the factor 1 / rho."""
    draws = ref.isolated_draws(2000)
    want = np.array([ref.isolated_want(d, 0.9) for d in draws])
    on = np.array([ref.isolated_mask_sum(d, 0.9, True) for d in draws]) / want
    dev = on - np.array([ref.isolated_expected_fraction(d, 0.9) for d in draws])
    bound = np.array([ref.isolated_sampling_bound(d, 0.9) for d in draws])
    stderr = dev.std(ddof=1) / np.sqrt(len(dev))
    print(f"antialiased / expected: {on.min():.4f} .. {on.max():.4f}; deviation from the cut's integral: mean {dev.mean():.2e} "
          f"(standard error {stderr:.2e}), largest {np.abs(dev).max():.4f}, largest deviation / bound {np.abs(dev / bound).max():.3f}")
    assert abs(dev.mean()) <= 4.0 * stderr
    assert (np.abs(dev) <= bound).all()
    # 1 / rho >= 1.133 (both axes 1.5 px), and the cut takes less than 1 % of an opacity-0.9 splat
    off = np.array([ref.isolated_mask_sum(d, 0.9, False) for d in draws]) / want
    print(f"classic / expected: {off.min():.4f} .. {off.max():.4f}")
    assert (off >= 1.1).all()


# ---- the float64 oracle's statement of the mode (oracle/torch_oracle.py) against tests/antialias_ref.py --------------------
def _oracle_scene():
    """32 x 32, two views with scale slots 1 / 0.6 and 1 / 0.8 over the unscaled means of util.make_edge_scene("outside")
    (visible Gaussians beyond 1.3 tan(fov): clamped Jacobians), ten of the filler rows with a zero and ten with a rank-1
    covariance (det0 = 0: the floor).  float64 (views (2, 44), means, packed covariances)."""
    from latentsplat_amd.decoder import cuda_splatting as cs
    from tests import camera_grad_cases as cases
    from tests import util
    sc, lab = util.make_edge_scene("outside", 32, 32, views=2, seed=3, feature_channels=4)
    sc.near = torch.tensor([0.6, 0.8])
    views = cases.cams32(sc).double()
    means, cov = sc.means.double(), cs._pack_covariances(sc.covariances).double().clone()
    fill = np.nonzero(lab["kind"] == 0)[0][:20]
    cov[fill[:10]] = 0.0
    u = torch.randn(10, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    r1 = 1e-3 * u[:, :, None] * u[:, None, :]
    cov[fill[10:]] = torch.stack([r1[:, 0, 0], r1[:, 0, 1], r1[:, 0, 2], r1[:, 1, 1], r1[:, 1, 2], r1[:, 2, 2]], -1)
    return views, means, cov, torch.from_numpy(fill)


def _oracle_rho(rec, means, cov, H=32, W=32, dtype=None):
    """The oracle's factor of one view as the harness of tests/test_camera_grads_gpu.py calls it: scaled means and covariances"""
    from oracle import torch_oracle as TO
    s = rec[40]
    return TO.opacity_factor(H, W, rec[35], rec[36], rec[0:16], means * s, cov * s * s, dtype=dtype)


def test_oracle_factor_and_its_derivatives_equal_the_reference():
    """Two independent torch statements of one formula (oracle.torch_oracle.opacity_factor through the scaled scene, as the
    gradient harness composes it; tests/antialias_ref.rho from the table): the factor and its autograd derivatives w.r.t.
    means, packed covariances and the view record agree in float64 to 1e-10 of each tensor's maximum."""
    from oracle import torch_oracle as TO
    views, means, cov, floor_rows = _oracle_scene()
    G = means.shape[0]
    w = torch.randn(2, G, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    assert float((views[:, 40] - 1.0).abs().min()) > 0.2
    leaves = lambda: [t.clone().requires_grad_(True) for t in (views, means, cov)]
    a, b = leaves(), leaves()
    got = torch.stack([_oracle_rho(a[0][v], a[1], a[2]) for v in range(2)])
    want_g = ref.rho(b[0], b[1], b[2], 32, 32)
    want, got_g, got = want_g.detach(), got, got.detach()
    clamped = 0
    for v in range(2):
        inx, iny = TO._clamp_mask(views[v, :16].reshape(4, 4), means * views[v, 40], float(views[v, 35]), float(views[v, 36]))
        z = (torch.cat([means * views[v, 40], torch.ones(G, 1, dtype=torch.float64)], 1) @ views[v, :16].reshape(4, 4))[:, 2]
        clamped += int((~(inx & iny) & (z > 0.2)).sum())
    assert clamped >= 8, clamped
    assert bool((want[:, floor_rows] == 0.005).all()) and float(want.max()) > 0.5 and float(want.min()) == 0.005
    assert float((got - want).abs().max()) <= 1e-10 * float(want.max())
    (got_g * w).sum().backward()
    (want_g * w).sum().backward()
    for name, x, y in zip(("views", "means", "cov"), a, b):
        err, top = float((x.grad - y.grad).abs().max()), float(y.grad.abs().max())
        print(f"d rho / d{name}: max {top:.3e}, difference {err:.3e}")
        assert top > 0 and err <= 1e-10 * top, (name, err, top)
    assert float(a[1].grad[floor_rows].abs().max()) == 0.0 and float(a[2].grad[floor_rows].abs().max()) == 0.0
    # the record: rho depends on the rotation part of the view matrix, its translation, tan(fov) and the scale, nothing else
    used = torch.zeros(44, dtype=torch.bool)
    used[[4 * c + r for c in range(4) for r in range(3)] + [35, 36, 40]] = True
    assert float(a[0].grad[:, ~used].abs().max()) == 0.0 and bool((a[0].grad[:, used].abs() > 0).all())
    # the float32 statement: the same function to float32 rounding, and differentiable through the casts
    c = leaves()
    r32 = torch.stack([_oracle_rho(c[0][v], c[1], c[2], dtype=torch.float32) for v in range(2)])
    assert r32.dtype == torch.float32 and torch.equal(r32[:, floor_rows], torch.full((2, 20), 0.000025).sqrt())
    live = want > 0.0051
    assert float((r32.double() / want - 1.0)[live].abs().max()) < 1e-3
    (r32.double() * w).sum().backward()
    assert c[0].grad.dtype == torch.float64 and float((c[2].grad - b[2].grad).abs().max()) <= 1e-2 * float(b[2].grad.abs().max())


def test_oracle_rasterize_keywords():
    """rasterize(antialiasing=True) composites o rho: the same images as the classic call fed o rho, in every rho_dtype; the
    default is the function it was; "constant" has the values of the mode and the gradients of the classic call."""
    from oracle import torch_oracle as TO
    views, means, cov, _ = _oracle_scene()
    G = means.shape[0]
    gen = torch.Generator().manual_seed(1)
    o = 0.1 + 0.8 * torch.rand(G, 1, generator=gen, dtype=torch.float64)
    col = torch.rand(G, 3, generator=gen, dtype=torch.float64)
    rec = views[0]
    s = rec[40]

    def run(ms, cv, op, **kw):
        return TO.rasterize(32, 32, rec[35], rec[36], rec[37:40], rec[0:16], rec[16:32], rec[32:35], 0, ms, cv, op,
                            colors_precomp=col, **kw)

    ms, cv = means * s, cov * s * s
    plain, off = run(ms, cv, o), run(ms, cv, o, antialiasing=False, rho_dtype=torch.float32)
    assert all(torch.equal(x, y) for x, y in zip(plain[:1] + plain[2:], off[:1] + off[2:]))
    for dtype in (None, torch.float64, torch.float32, "constant"):
        rho = _oracle_rho(rec, means, cov, dtype=torch.float32 if dtype == torch.float32 else None).double()
        on, fed = run(ms, cv, o, antialiasing=True, rho_dtype=dtype), run(ms, cv, o * rho[:, None])
        assert all(torch.equal(x, y) for x, y in zip(on[:1] + on[2:], fed[:1] + fed[2:])), dtype
        assert not torch.equal(on[2], plain[2]) and torch.equal(on[4], plain[4])
    g = torch.Generator().manual_seed(3)
    wc = torch.randn(3, 32, 32, generator=g, dtype=torch.float64)
    grads = {}
    for dtype in (None, "constant"):
        cl = cv.clone().requires_grad_(True)
        (run(ms, cl, o, antialiasing=True, rho_dtype=dtype)[0] * wc).sum().backward()
        grads[dtype] = cl.grad
    cl = cv.clone().requires_grad_(True)
    with torch.no_grad():
        rho = _oracle_rho(rec, means, cov)
    (run(ms, cl, o * rho[:, None])[0] * wc).sum().backward()
    assert torch.allclose(grads["constant"], cl.grad, rtol=1e-12, atol=0)
    assert float((grads[None] - cl.grad).abs().max()) > 1e-3 * float(cl.grad.abs().max())


def test_oracle_factor_against_central_differences():
    """d (sum w rho) / dx of the oracle's float64 autograd against central differences, for the record slots rho depends on
    (the 12 view-matrix entries, both tan(fov), the scale) and for the means and covariances of twenty Gaussian rows.  The
    weights are zero on the rows with a clamped Jacobian: there the derivative is a convention (the clamped t.x / t.z is a
    constant), which no difference quotient sees.  Per coordinate, with D(h) = (f(x + h) - f(x - h)) / 2h:
    D(h) = f' + h^2 f''' / 6 + O(h^4), so (D(2h) - D(h)) / 3 estimates the truncation error of D(h); the rounding error of
    D(h) is at most 2 eps |f| / 2h with eps = 2^-53 per evaluation, taken 64-fold for the sums inside f.  The bar is twice the
    truncation estimate plus that rounding bound; h = 1e-4 of the coordinate's scale keeps both near 1e-8 of the derivative."""
    from oracle import torch_oracle as TO
    views, means, cov, floor_rows = _oracle_scene()
    G = means.shape[0]
    w = torch.randn(2, G, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    for v in range(2):
        inx, iny = TO._clamp_mask(views[v, :16].reshape(4, 4), means * views[v, 40], float(views[v, 35]), float(views[v, 36]))
        w[v][~(inx & iny)] = 0.0

    def f(vw, m, c):
        return float(sum((_oracle_rho(vw[v], m, c) * w[v]).sum() for v in range(2)))

    a = [t.clone().requires_grad_(True) for t in (views, means, cov)]
    sum((_oracle_rho(a[0][v], a[1], a[2]) * w[v]).sum() for v in range(2)).backward()
    f0 = abs(f(views, means, cov))
    with torch.no_grad():
        rho = torch.stack([_oracle_rho(views[v], means, cov) for v in range(2)])
    # twenty rows away from the floor and unclamped in a view, five of them the smallest factors there are
    ok = ((rho > 0.0051) & (w != 0)).any(0).nonzero()[:, 0]
    rows = torch.cat([ok[torch.argsort(rho[:, ok].min(0).values)[:5]], ok[5::max(1, len(ok) // 15)][:15]])
    assert len(rows) == 20
    slots = [4 * c + r for c in range(4) for r in range(3)] + [35, 36, 40]
    coords = [(0, (v, k), float(views[v, k].abs().clamp_min(0.1))) for v in range(2) for k in slots]
    coords += [(1, (int(g), k), float(means[g].abs().max())) for g in rows for k in range(3)]
    coords += [(2, (int(g), k), float(cov[g].abs().max())) for g in rows for k in range(6)]
    worst = 0.0
    for which, idx, scale in coords:
        h = 1e-4 * scale

        def D(step):
            hi, lo = [t.clone() for t in (views, means, cov)], [t.clone() for t in (views, means, cov)]
            hi[which][idx] += step
            lo[which][idx] -= step
            return (f(*hi) - f(*lo)) / (2.0 * step)

        d1, d2 = D(h), D(2.0 * h)
        bar = 2.0 * abs(d2 - d1) / 3.0 + 64.0 * 2.0 ** -53 * f0 / h
        got = float(a[which].grad[idx])
        worst = max(worst, abs(got - d1) / max(abs(d1), 1e-6 * float(a[which].grad.abs().max())))
        assert abs(got - d1) <= bar, (which, idx, got, d1, d2, bar)
        assert bar <= 1e-5 * max(abs(d1), float(a[which].grad.abs().max()) * 1e-3), (which, idx, d1, bar)
    print(f"{len(coords)} coordinates, worst |autograd - difference| / max(|difference|, 1e-6 of the tensor's largest) {worst:.2e}")
