"""SH coefficient rotation on the MI355X (csrc/sh_rotate.hip) against the float64 helper
(tests/sh_rotation_ref.py): the rotation tables, the fused forward / backward, ``rotate_sh``'s
broadcasting, and ``GaussianAdapter`` end to end with its default (fused, e3nn-free) path.

Bounds (fixed beforehand, from the arithmetic):
  tables    every entry within 1e-5 (entries are bounded by 1; float32 rounding of a double result
            plus the float32 input matrix's own 6e-8 departure from orthogonality, times l);
  forward   every element within 1e-5 * max(1, |masked input band|_2): rows of D have unit norm, so a
            9-term float32 dot product errs by at most 9 * 2^-24 |c| = 5.4e-7 |c|, plus the table error;
  backward  within 1e-5 of the gradient tensor's largest magnitude.
"""
import numpy as np
import pytest
import torch

from tests import sh_rotation_ref as ref

pytestmark = pytest.mark.gpu


def _f32_rotations(n, seed, special=False):
    R = ref.random_rotations(n, np.random.default_rng(seed))
    if special:
        R = np.concatenate([R, ref.special_rotations()])
    return R.astype(np.float32)          # what the device sees; the helper gets the same values in float64


def _adapter_mask(degree):
    m = np.ones((degree + 1) ** 2)
    for l in range(1, degree + 1):
        m[l * l:(l + 1) ** 2] = 0.1 * 0.25 ** l
    return m


def _reference(rows, R, S, Kc, C, Kf, cmask, fmask):
    """rows (cams, rays, W) float64 -> colour (cams, rays, S, 3, Kc), feature (cams, rays, S, C, Kf), and the
    per-element bound scale max(1, |masked input band|)."""
    cams, rays, _ = rows.shape
    out = []
    for lo, ch, K, mask in ((0, 3, Kc, cmask), (3 * Kc, C, Kf, fmask)):
        if K == 0:
            out += [None, None]
            continue
        deg = int(round(K ** 0.5)) - 1
        x = rows[..., lo:lo + ch * K].reshape(cams, rays, ch, K) * (mask if mask is not None else 1.0)
        y = np.stack([x[c] @ ref.full_matrix(deg, R[c].astype(np.float64)).T for c in range(cams)])
        scale = np.empty_like(x)
        for l in range(deg + 1):
            nrm = np.linalg.norm(x[..., l * l:(l + 1) ** 2], axis=-1, keepdims=True)
            scale[..., l * l:(l + 1) ** 2] = np.maximum(1.0, nrm)
        rep = lambda a: np.broadcast_to(a[:, :, None], (cams, rays, S, ch, K))
        out += [rep(y), rep(scale)]
    return out


def _run(dev, cams, rays, S, Kc, C, Kf, seed, strided=False, masks=True, grads="both", ext44=False):
    from latentsplat_amd.sh_rotate import rotate_harmonics
    rng = np.random.default_rng(seed)
    W = 3 * Kc + C * Kf
    R = _f32_rotations(cams, seed + 1)
    rows = (rng.normal(size=(cams, rays, W)) * np.exp(rng.normal(size=(cams, rays, 1)))).astype(np.float32)
    cmask = _adapter_mask(int(round(Kc ** 0.5)) - 1) if (masks and Kc) else None
    fmask = _adapter_mask(int(round(Kf ** 0.5)) - 1) if (masks and Kf) else None
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    if strided:       # the encoder's layout: the harmonics start 9 floats into a wider Linear output
        full = torch.zeros((cams, rays, W + 9), device=dev)
        full[..., 9:] = t(rows)
        full.requires_grad_()
        view = full[..., 9:]
    else:
        full = t(rows).requires_grad_()
        view = full
    if ext44:
        E = np.tile(np.eye(4, dtype=np.float32), (cams, 1, 1))
        E[:, :3, :3] = R
        E[:, :3, 3] = 7.0
        rot = t(E)
    else:
        rot = t(R)
    color, feature = rotate_harmonics(view, rot, S, Kc, C, Kf, t(cmask), t(fmask))
    want_c, scale_c, want_f, scale_f = _reference(rows.astype(np.float64), R, S, Kc, C, Kf, cmask, fmask)
    worst = 0.0
    for got, want, scale in ((color, want_c, scale_c), (feature, want_f, scale_f)):
        if want is None:
            assert got is None
            continue
        assert got.shape == want.shape and got.is_contiguous()
        err = float((np.abs(got.detach().cpu().numpy() - want) / scale).max())
        worst = max(worst, err)
    print(f"sh_rotate forward cams={cams} rays={rays} S={S} Kc={Kc} C={C} Kf={Kf} strided={strided}: "
          f"worst error / max(1, |band|) = {worst:.3e}")
    assert worst <= 1e-5
    if grads is None:
        return
    # backward against torch autograd through the float64 helper's matrices
    gc = rng.normal(size=(cams, rays, S, 3, Kc)) if (Kc and grads in ("both", "color")) else None
    gf = rng.normal(size=(cams, rays, S, C, Kf)) if (Kf and grads in ("both", "feature")) else None
    rows64 = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    loss64 = 0.0
    for lo, ch, K, mask, g in ((0, 3, Kc, cmask, gc), (3 * Kc, C, Kf, fmask, gf)):
        if g is None:
            continue
        deg = int(round(K ** 0.5)) - 1
        D = torch.tensor(np.stack([ref.full_matrix(deg, R[c].astype(np.float64)) for c in range(cams)]))
        x = rows64[..., lo:lo + ch * K].reshape(cams, rays, ch, K)
        if mask is not None:
            x = x * torch.tensor(mask)
        y = torch.einsum("cij,crhj->crhi", D, x)
        loss64 = loss64 + (y[:, :, None] * torch.tensor(g.astype(np.float32).astype(np.float64))).sum()
    loss64.backward()
    want = rows64.grad.numpy()

    def device_grad():
        full.grad = None
        c2, f2 = rotate_harmonics(view, rot, S, Kc, C, Kf, t(cmask), t(fmask))
        outs, ups = [], []
        if gc is not None:       # handed over NON-contiguous (for cams > 1): the op must not assume a layout
            outs.append(c2); ups.append(t(gc.swapaxes(0, 1)).transpose(0, 1))
        if gf is not None:
            outs.append(f2); ups.append(t(gf))
        torch.autograd.backward(outs, ups)
        return full.grad.clone()

    g1, g2 = device_grad(), device_grad()
    assert torch.equal(g1, g2)                                   # no atomics: bitwise reproducible
    if strided:
        assert float(g1[..., :9].abs().max()) == 0.0             # columns outside the harmonics: exactly zero
        g1 = g1[..., 9:]
    err = float(np.abs(g1.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"sh_rotate backward ({grads}): worst error / largest gradient = {err:.3e}")
    assert err <= 1e-5
    for K, lo, width, g in ((Kc, 0, 3 * Kc, gc), (Kf, 3 * Kc, C * Kf, gf)):
        if K and g is None:                                        # a NULL upstream gradient: written as zeros
            assert float(g1[..., lo:lo + width].abs().max()) == 0.0


def test_rotation_tables_match_the_helper(hip_device):
    from latentsplat_amd.sh_rotate import sh_rotation_matrices
    R = _f32_rotations(96, 21, special=True)
    assert len(R) >= 64 + 4 + 12
    worst = {}
    for degree in (4, 2, 0):
        got = sh_rotation_matrices(torch.tensor(R, device=hip_device), degree).cpu().numpy()
        want = np.stack([ref.packed_table(degree, r.astype(np.float64)) for r in R])
        assert got.shape == want.shape
        worst[degree] = float(np.abs(got - want).max())
    # the [cam][4][4] form reads the rotation corner in place
    E = np.zeros((len(R), 4, 4), dtype=np.float32)
    E[:, :3, :3] = R
    E[:, :3, 3] = 123.0
    E[:, 3] = (9.0, 9.0, 9.0, 1.0)
    got44 = sh_rotation_matrices(torch.tensor(E, device=hip_device), 4).cpu().numpy()
    assert np.array_equal(got44, sh_rotation_matrices(torch.tensor(R, device=hip_device), 4).cpu().numpy())
    print(f"sh rotation tables: worst entry error {worst}")
    assert max(worst.values()) <= 1e-5


@pytest.mark.parametrize("cams,rays,S,Kc,C,Kf,strided", [
    (2, 1000, 3, 25, 4, 9, True),        # the encoder's degrees (4, 2), strided view, rays not a multiple of 64
    (3, 257, 1, 16, 8, 4, False),        # degrees (3, 1), C = 8, S = 1
    (1, 77, 3, 1, 4, 1, True),           # degrees (0, 0)
    (2, 130, 3, 25, 0, 0, False),        # colour only
    (2, 131, 1, 0, 8, 9, True),          # feature only
    (1, 5, 40, 25, 32, 25, False),       # one row's samples exceed the staging budget: chunked path
    (5, 1, 2, 9, 1, 16, False),          # a single row per camera
])
def test_forward_and_backward_match_the_helper(cams, rays, S, Kc, C, Kf, strided, hip_device):
    _run(hip_device, cams, rays, S, Kc, C, Kf, seed=cams * 100 + rays, strided=strided)


@pytest.mark.parametrize("grads", ["color", "feature"])
def test_backward_with_one_upstream_gradient_absent(grads, hip_device):
    _run(hip_device, 2, 300, 3, 25, 4, 9, seed=9, strided=True, grads=grads)


def test_unit_masks_and_camera_table_input(hip_device):
    _run(hip_device, 2, 200, 2, 9, 4, 4, seed=3, masks=False, ext44=True)


def test_full_encoder_size(hip_device):
    """2 context views x 65 536 rays x 3 samples, colour degree 4, 4 latent channels of degree 2."""
    _run(hip_device, 2, 65536, 3, 25, 4, 9, seed=1, strided=True)


def test_rotate_sh_broadcasting(hip_device):
    from latentsplat_amd import rotate_sh
    rng = np.random.default_rng(17)
    dev = hip_device
    # the reference's call shape: c2w[..., None, :, :] against (b, v, r, srf, spp, c, n)
    b, v, r, srf, spp, c, n = 2, 2, 37, 1, 3, 4, 9
    R = _f32_rotations(b * v, 5).reshape(b, v, 3, 3)
    sh = rng.normal(size=(b, v, r, srf, spp, c, n)).astype(np.float32)
    c2w = torch.tensor(R, device=dev)[:, :, None, None, None]
    x = torch.tensor(sh, device=dev, requires_grad=True)
    out = rotate_sh(x, c2w[..., None, :, :])
    assert out.shape == sh.shape
    want = np.stack([np.stack([ref.rotate(sh[i, j], R[i, j]) for j in range(v)]) for i in range(b)])
    assert np.abs(out.detach().cpu().numpy() - want).max() <= 1e-5 * max(1.0, np.linalg.norm(sh, axis=-1).max())
    g = rng.normal(size=sh.shape).astype(np.float32)
    (out * torch.tensor(g, device=dev)).sum().backward()
    want_g = np.stack([np.stack([g[i, j].astype(np.float64) @ ref.full_matrix(2, R[i, j]) for j in range(v)]) for i in range(b)])
    assert np.abs(x.grad.cpu().numpy() - want_g).max() <= 1e-5 * np.abs(want_g).max()
    # one rotation per row
    N = 300
    Rn = _f32_rotations(N, 6)
    shn = rng.normal(size=(N, 25)).astype(np.float32)
    outn = rotate_sh(torch.tensor(shn, device=dev), torch.tensor(Rn, device=dev)).cpu().numpy()
    wantn = np.stack([ref.rotate(shn[i], Rn[i]) for i in range(N)])
    assert np.abs(outn - wantn).max() <= 1e-5 * max(1.0, np.linalg.norm(shn, axis=-1).max())
    # a rotation that varies over a middle dim only, coefficients broadcast over the leading one
    Rm = _f32_rotations(3, 7)
    shm = rng.normal(size=(1, 3, 50, 16)).astype(np.float32)
    outm = rotate_sh(torch.tensor(shm, device=dev), torch.tensor(Rm, device=dev)[None, :, None].expand(2, 3, 1, 3, 3))
    assert outm.shape == (2, 3, 50, 16)
    wantm = np.stack([ref.rotate(shm[0, j], Rm[j]) for j in range(3)])
    for i in range(2):
        assert np.abs(outm[i].cpu().numpy() - wantm).max() <= 1e-5 * max(1.0, np.linalg.norm(shm, axis=-1).max())
    # a single rotation, a single vector
    one = rotate_sh(torch.tensor(shn[0], device=dev), torch.tensor(Rn[0], device=dev)).cpu().numpy()
    assert one.shape == (25,) and np.abs(one - wantn[0]).max() <= 1e-5 * max(1.0, np.linalg.norm(shn[0]))


def test_gaussian_adapter_default_path_end_to_end(hip_device):
    """GaussianAdapter with NO rotate_sh=, called like encoder_epipolar.py:185-193: forward and backward run (before
    the HIP rotation existed this raised LsrError: e3nn missing); geometry is bit-equal to the adapter with an injected
    identity; harmonics are the helper's; raw_gaussians.grad is the sum of the geometry's and the harmonics' gradients."""
    from latentsplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    dev = hip_device
    rng = np.random.default_rng(23)
    b, v, r, srf, spp, C = 1, 2, 500, 1, 3, 4
    cfg = GaussianAdapterCfg(0.5, 15.0, 4, 2)
    fused = GaussianAdapter(cfg, C).to(dev)
    ident = GaussianAdapter(cfg, C, rotate_sh=lambda sh, rot: sh).to(dev)
    d_in = fused.d_in
    assert d_in == 118
    R = _f32_rotations(b * v, 31).reshape(b, v, 3, 3)
    E = np.tile(np.eye(4, dtype=np.float32), (b, v, 1, 1))
    E[..., :3, :3] = R
    E[..., :3, 3] = rng.normal(size=(b, v, 3))
    K = np.tile(np.eye(3, dtype=np.float32), (b, v, 1, 1))
    K[..., 0, 0] = K[..., 1, 1] = 0.9
    K[..., :2, 2] = 0.5
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    raw_np = rng.normal(size=(b, v, r, srf, d_in + 2)).astype(np.float32)
    coords = t(rng.random((b, v, r, srf, 2)))
    depths = t(0.5 + 20 * rng.random((b, v, r, srf, spp)))
    opac = t(rng.random((b, v, r, srf, spp)))
    g_names = ("means", "covariances", "scales", "color_harmonics", "feature_harmonics")
    g_up = {}

    def call(adapter):
        raw = t(raw_np).requires_grad_()
        g = adapter.forward(t(E)[:, :, None, None, None], t(K)[:, :, None, None, None], coords[..., None, :], depths,
                            opac, raw[..., None, 2:], (64, 48))
        return raw, g

    raw_f, gf = call(fused)
    raw_i, gi = call(ident)
    for name in ("means", "covariances", "scales", "rotations", "opacities"):
        assert torch.equal(getattr(gf, name), getattr(gi, name)), name
    assert gf.color_harmonics.shape == (b, v, r, srf, spp, 3, 25)
    assert gf.feature_harmonics.shape == (b, v, r, srf, spp, C, 9)
    # harmonics: helper-rotated masked coefficients (the identity adapter's harmonics ARE the masked coefficients)
    for name, deg in (("color_harmonics", 4), ("feature_harmonics", 2)):
        x = getattr(gi, name).detach().cpu().numpy().astype(np.float64)
        got = getattr(gf, name).detach().cpu().numpy()
        for i in range(b):
            for j in range(v):
                want = ref.rotate(x[i, j], R[i, j])
                band = np.concatenate([np.broadcast_to(np.linalg.norm(x[i, j][..., l * l:(l + 1) ** 2], axis=-1, keepdims=True),
                                                       x[i, j].shape[:-1] + (2 * l + 1,)) for l in range(deg + 1)], -1)
                assert (np.abs(got[i, j] - want) / np.maximum(1.0, band)).max() <= 1e-5, name
    for name in g_names:
        g_up[name] = t(rng.normal(size=tuple(getattr(gf, name).shape)))
    # fused: everything at once; identity adapter: geometry only; the harmonics' share in float64 through the helper
    sum((getattr(gf, n) * g_up[n]).sum() for n in g_names).backward()
    sum((getattr(gi, n) * g_up[n]).sum() for n in g_names[:3]).backward()
    got, geo = raw_f.grad.cpu().numpy(), raw_i.grad.cpu().numpy()
    assert np.abs(got[..., :2]).max() == 0.0
    assert np.array_equal(got[..., 2:9], geo[..., 2:9])
    raw64 = torch.tensor(raw_np, dtype=torch.float64, requires_grad=True)
    loss = 0.0
    for name, lo, ch, Kn, deg, mask in (("color_harmonics", 9, 3, 25, 4, fused.color_sh_mask),
                                        ("feature_harmonics", 9 + 75, C, 9, 2, fused.feature_sh_mask)):
        D = torch.tensor(np.stack([np.stack([ref.full_matrix(deg, R[i, j].astype(np.float64)) for j in range(v)]) for i in range(b)]))
        x = raw64[..., lo:lo + ch * Kn].reshape(b, v, r, srf, ch, Kn) * mask.cpu().double()
        y = torch.einsum("bvij,bvrshj->bvrshi", D, x)
        loss = loss + (y[:, :, :, :, None] * g_up[name].cpu().double()).sum()
    loss.backward()
    want = geo.astype(np.float64) + raw64.grad.numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
