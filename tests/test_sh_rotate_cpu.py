"""SH coefficient rotation, the parts that need no GPU: the float64 helper the GPU tests compare
against (tests/sh_rotation_ref.py) is itself checked against the defining equation's consequences,
the rotation is tied to the package's ``eval_sh``, the kernel's generated constant tables invert the
generator's basis, and the three C entry points validate their arguments on the host."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd.decoder import geometry
from tests import sh_rotation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rotations():
    return np.concatenate([ref.random_rotations(24, np.random.default_rng(5)), ref.special_rotations()])


def test_helper_fit_is_exact_and_orthogonal():
    for R in _rotations():
        assert abs(np.linalg.det(R) - 1) < 1e-12
        for l in range(5):
            D, residual = ref.band_matrix(l, R)
            n = 2 * l + 1
            assert residual < 1e-13, (l, residual)                       # Y_l(R x) = D_l Y_l(x) holds on all 400 directions
            assert np.abs(D @ D.T - np.eye(n)).max() < 1e-13, l
            if l == 0:
                assert abs(D[0, 0] - 1) < 1e-14
            if l == 1:
                assert np.abs(D - R).max() < 1e-14                        # e3nn's documented property


def test_helper_identity_and_homomorphism():
    assert np.abs(ref.full_matrix(4, np.eye(3)) - np.eye(25)).max() < 1e-14
    Rs = _rotations()
    for R1, R2 in zip(Rs[:12], Rs[12:24]):
        lhs = ref.full_matrix(4, R1 @ R2)
        assert np.abs(lhs - ref.full_matrix(4, R1) @ ref.full_matrix(4, R2)).max() < 1e-13
    table = ref.packed_table(4, Rs[0])
    assert table.shape == (165,) and _lib.sh_rotate_table_floats(4) == 165
    assert [_lib.sh_rotate_table_floats(l) for l in range(5)] == [1, 10, 35, 84, 165]
    assert np.array_equal(table[:35], ref.packed_table(2, Rs[0]))      # a lower degree's table is a prefix


def test_helper_basis_is_orthonormal_on_the_sphere():
    """Gram matrix of the helper's basis over the sphere (exact quadrature for degree 8) is the identity up to
    4 pi; with z in place of y at index 14 (the reference's eval_sh) band 3 is not."""
    nodes, weights = np.polynomial.legendre.leggauss(12)
    phi = 2 * np.pi * (np.arange(24) + 0.5) / 24
    ct, ph = np.meshgrid(nodes, phi, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    d = np.stack([st * np.cos(ph), ct, st * np.sin(ph)], -1).reshape(-1, 3)
    w = (weights[:, None] * np.full((1, 24), 2 * np.pi / 24)).reshape(-1)
    Y = ref.basis(4, d)
    assert np.abs((Y * w[:, None]).T @ Y - np.eye(25)).max() < 1e-12
    Yref = geometry.sh_basis_e3nn(4, torch.tensor(d)).numpy()
    gram = (Yref * w[:, None]).T @ Yref
    assert np.abs(gram[9:16, 9:16] - np.eye(7)).max() > 0.1
    keep = [i for i in range(25) if i != 14]
    assert np.abs(gram[np.ix_(keep, keep)] - np.eye(24)).max() < 1e-12


@pytest.mark.parametrize("band", [0, 1, 2, 4])
def test_rotated_coefficients_through_eval_sh(band):
    """What the rotation means for the package's own SH evaluation (the reference's, with its (-1)^m signs):
    eval_sh(D c, d) == eval_sh(c, P R^T P d), P = diag(-1, 1, -1) — for the bands where eval_sh is a harmonic basis."""
    rng = np.random.default_rng(band)
    lo, hi = band * band, (band + 1) ** 2
    worst = 0.0
    for R in _rotations()[:20]:
        c = np.zeros((3, 25))
        c[:, lo:hi] = rng.normal(size=(3, hi - lo))
        d = rng.normal(size=(16, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        lhs = geometry.eval_sh(4, torch.tensor(ref.rotate(c, R))[None], torch.tensor(d))
        rhs = geometry.eval_sh(4, torch.tensor(c)[None], torch.tensor(d @ (ref.P @ R.T @ ref.P).T))
        worst = max(worst, float((lhs - rhs).abs().max()))
        if band > 0:    # the naive reading is wrong by O(1)
            naive = geometry.eval_sh(4, torch.tensor(c)[None], torch.tensor(d @ R))
            assert float((lhs - naive).abs().max()) > 1e-3 or np.abs(R - ref.P @ R @ ref.P).max() < 1e-3
    assert worst <= 1e-12, worst


def test_generated_tables_invert_the_generators_basis():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sh_rotation_tables.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _dims(**kw):
    base = dict(num_cameras=2, rays=100, samples=3, color_coeffs=25, feat_channels=4, feat_coeffs=9,
                table_stride=165, reserved0=0, row_stride=120)
    base.update(kw)
    return _lib.ShRotateDims(**base)


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("lsr_sh_rotation_matrices", "lsr_sh_rotate_forward", "lsr_sh_rotate_backward"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert C.sizeof(_lib.ShRotateDims) == 40


@pytest.mark.parametrize("bad", [
    dict(color_coeffs=5), dict(color_coeffs=36), dict(feat_coeffs=2), dict(feat_coeffs=-1),
    dict(color_coeffs=0, feat_coeffs=0), dict(feat_channels=0), dict(feat_channels=33),
    dict(num_cameras=0), dict(rays=-1), dict(samples=0), dict(table_stride=164), dict(reserved0=1),
    dict(row_stride=110),
])
def test_invalid_dims_are_rejected_before_any_gpu_work(bad):
    lib = _lib.load()
    d = _dims(**bad)
    fake = C.c_void_p(256)     # never dereferenced: validation comes first
    assert lib.lsr_sh_rotate_forward(C.byref(d), fake, fake, None, None, fake, fake, None) == -1
    if "row_stride" not in bad:      # the backward writes dense rows: row_stride is not its business
        assert lib.lsr_sh_rotate_backward(C.byref(d), fake, fake, fake, None, None, fake, None) == -1


def test_absent_tensors_and_small_tables_are_valid_dims():
    """Kc = 0 or Kf = 0 (tensor absent; C is then ignored) and a table of the needed degree only: accepted — shown
    by the NULL-pointer code that follows validation."""
    lib = _lib.load()
    for kw in (dict(color_coeffs=0, row_stride=36, table_stride=35), dict(feat_coeffs=0, feat_channels=99, row_stride=75),
               dict(color_coeffs=16, feat_coeffs=4, table_stride=84, row_stride=64), dict(color_coeffs=1, feat_coeffs=1, table_stride=1, row_stride=7)):
        d = _dims(**kw)
        assert lib.lsr_sh_rotate_forward(C.byref(d), None, None, None, None, None, None, None) == -2
        assert lib.lsr_sh_rotate_backward(C.byref(d), None, None, None, None, None, None, None) == -2


def test_null_pointers():
    lib = _lib.load()
    d, fake = _dims(), C.c_void_p(256)
    assert lib.lsr_sh_rotate_forward(None, fake, fake, None, None, fake, fake, None) == -2
    assert lib.lsr_sh_rotate_backward(None, fake, fake, fake, None, None, fake, None) == -2
    assert lib.lsr_sh_rotate_forward(C.byref(d), None, fake, None, None, fake, fake, None) == -2     # tables
    assert lib.lsr_sh_rotate_forward(C.byref(d), fake, None, None, None, fake, fake, None) == -2     # rows
    assert lib.lsr_sh_rotate_forward(C.byref(d), fake, fake, None, None, None, fake, None) == -2     # colour out
    assert lib.lsr_sh_rotate_forward(C.byref(d), fake, fake, None, None, fake, None, None) == -2     # feature out
    assert lib.lsr_sh_rotate_backward(C.byref(d), None, fake, fake, None, None, fake, None) == -2    # tables
    assert lib.lsr_sh_rotate_backward(C.byref(d), fake, fake, fake, None, None, None, None) == -2    # d_rows
    assert lib.lsr_sh_rotation_matrices(3, None, 3, 9, 4, fake, None) == -2
    assert lib.lsr_sh_rotation_matrices(3, fake, 3, 9, 4, None, None) == -2
    assert b"NULL" in lib.lsr_error_string(-2) or b"null" in lib.lsr_error_string(-2).lower()


def test_rotation_matrices_arguments():
    lib = _lib.load()
    fake = C.c_void_p(256)
    for args in ((3, fake, 3, 9, 5, fake), (3, fake, 3, 9, -1, fake), (-1, fake, 3, 9, 4, fake),
                 (3, fake, 2, 9, 4, fake), (3, fake, 4, 10, 4, fake)):
        assert lib.lsr_sh_rotation_matrices(*args, None) == -1, args
    assert lib.lsr_sh_rotation_matrices(0, None, 3, 9, 4, None, None) == 0


def test_zero_rows_succeed_without_a_launch():
    lib = _lib.load()
    d = _dims(rays=0)
    assert lib.lsr_sh_rotate_forward(C.byref(d), None, None, None, None, None, None, None) == 0
    assert lib.lsr_sh_rotate_backward(C.byref(d), None, None, None, None, None, None, None) == 0


def test_python_entry_points_refuse_cpu_tensors():
    from latentsplat_amd import rotate_sh
    from latentsplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        rotate_sh(torch.zeros(5, 9), torch.eye(3))
    ad = GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, 4, 2), 4)
    assert ad._rotate_sh is None and ad.d_in == 7 + 75 + 36
    import latentsplat_amd.gaussian_adapter as ga
    assert "e3nn" not in {n for n in vars(ga)} and not hasattr(ga, "_e3nn_rotate_sh")
