"""Scene export without a GPU: the host writer (lsr_ply_write_scene_host) read back by the host reader, the SH
change-of-basis table (lsr_ply_sh_axes_matrix) against its defining equation, and the argument checks of pack_scene."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import PlyLayout
from tests import scene_export_ref as ref

EINVAL, ENULL = -1, -2


def _write(path, rows, n, K):
    ptr = rows.ctypes.data_as(C.c_void_p) if rows is not None else None
    return _lib.load().lsr_ply_write_scene_host(os.fsencode(str(path)), ptr, n, K)


@pytest.mark.parametrize("K", [1, 4, 9, 16, 25])
def test_host_writer_through_the_host_reader(tmp_path, K):
    from latentsplat_amd.ply_export import construct_list_of_attributes
    from latentsplat_amd.ply_import import layout_from_names
    lib = _lib.load()
    names = construct_list_of_attributes(3 * (K - 1))
    stride = len(names)
    assert stride == 14 + 3 * K == _lib.ply_scene_row_floats(K)
    for n in (0, 1, 1000):
        rows = np.random.default_rng(10 * K + n).standard_normal((n, stride)).astype(np.float32)
        path = tmp_path / f"w{n}.ply"
        assert _write(path, rows, n, K) == 0
        got, want = PlyLayout(), layout_from_names(names, n)
        assert lib.lsr_ply_read_header(os.fsencode(str(path)), C.byref(got)) == 0
        assert (got.n, got.stride, got.sh_coeffs) == (n, stride, K) == (want.n, want.stride, want.sh_coeffs)
        for field in ("xyz", "f_dc", "scale", "rot", "f_rest"):
            assert list(getattr(got, field)) == list(getattr(want, field)), field
        assert got.opacity == want.opacity
        header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" +
                  "".join(f"property float {p}\n" for p in names) + "end_header\n").encode()
        assert got.data_offset == len(header) and os.path.getsize(path) == len(header) + n * stride * 4
        raw = path.read_bytes()
        assert raw[:len(header)] == header and raw[len(header):] == rows.tobytes()
        back = np.full(n * stride + 2, np.float32(-77.0))
        assert lib.lsr_ply_read_rows(os.fsencode(str(path)), back.ctypes.data_as(C.c_void_p), back.size) == 0
        assert back[:n * stride].tobytes() == rows.tobytes() and (back[n * stride:] == -77).all()


def test_host_writer_rejections(tmp_path):
    rows = np.zeros((2, 89), np.float32)
    assert _write(tmp_path / "no" / "such" / "dir" / "x.ply", rows, 2, 1) == EINVAL       # cannot be created
    for K in (0, 2, 3, 26, -1):
        assert _write(tmp_path / "k.ply", rows, 2, K) == EINVAL
        assert not (tmp_path / "k.ply").exists()
    assert _write(tmp_path / "n.ply", rows, -1, 1) == EINVAL
    assert _write(tmp_path / "p.ply", None, 2, 1) == ENULL
    assert _lib.load().lsr_ply_write_scene_host(None, rows.ctypes.data_as(C.c_void_p), 2, 1) == ENULL
    assert _write(tmp_path / "empty.ply", None, 0, 4) == 0                                   # a header-only file needs no rows


def test_basis_change_table_satisfies_its_defining_equation():
    M = np.full(625, np.nan)
    assert _lib.load().lsr_ply_sh_axes_matrix(M.ctypes.data_as(C.c_void_p)) == 0
    assert _lib.load().lsr_ply_sh_axes_matrix(None) == ENULL
    M = M.reshape(25, 25)
    d = ref.unit_directions(1000, 4)
    residual = np.abs(ref.basis(d) @ M - ref.reference_view(d)).max()
    orth = np.abs(M @ M.T - np.eye(25)).max()
    print(f"residual {residual:.2e}, |M M^T - I| {orth:.2e}")
    assert residual <= 1e-12 and orth <= 1e-12
    block = np.zeros((25, 25), bool)
    for l in range(5):
        block[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = True
    assert (M[~block] == 0.0).all()
    assert [int(np.count_nonzero(M[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2])) for l in range(5)] == [1, 3, 7, 13, 21]
    assert np.abs(M - ref.axes_matrix()).max() <= 1e-12          # (the restatement the GPU tests use solves the same equation)
    # what the matrix is for: coefficients c under "reference" and M c under "3dgs" give the same colour
    c = np.random.default_rng(5).standard_normal(25)
    assert np.abs(ref.basis(d) @ (M @ c) - ref.reference_view(d) @ c).max() <= 1e-11


def test_generated_header_is_current():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import gen_sh_axes_table
    finally:
        sys.path.pop(0)
    assert gen_sh_axes_table.check()


def test_argument_checks():
    from latentsplat_amd.ply_export import pack_scene, save_gaussians, save_ply
    from latentsplat_amd.decoder.types import Gaussians
    n = 5
    means, opac, shs = torch.zeros(n, 3), torch.full((n,), 0.5), torch.zeros(n, 4, 3)
    cov, scales, rot = torch.eye(3).expand(n, 3, 3), torch.ones(n, 3), torch.ones(n, 4)
    with pytest.raises(_lib.LsrError, match="ROCm"):                        # CPU tensors: no fallback
        pack_scene(means, opac, shs, covariances=cov)
    with pytest.raises(_lib.LsrError, match="ROCm"):
        pack_scene(means, opac, shs, scales=scales, rotations=rot)
    with pytest.raises(_lib.LsrError, match="ROCm"):
        save_ply("unused.ply", means, opac, shs, covariances=cov)
    for kw in (dict(), dict(covariances=cov, scales=scales, rotations=rot), dict(scales=scales), dict(rotations=rot),
               dict(covariances=cov, scales=scales)):
        with pytest.raises(_lib.LsrError, match="exactly one"):
            pack_scene(means, opac, shs, **kw)
    with pytest.raises(_lib.LsrError, match="ambiguous"):
        pack_scene(means, opac, torch.zeros(n, 3, 3), covariances=cov)
    with pytest.raises(_lib.LsrError, match="expected 1, 4, 9, 16 or 25"):     # ... and K = 3 is no SH size either way
        pack_scene(means, opac, torch.zeros(n, 3, 3), covariances=cov, channel_major=True)
    with pytest.raises(_lib.LsrError, match="shs must be"):
        pack_scene(means, opac, torch.zeros(n, 4, 4), covariances=cov)
    with pytest.raises(_lib.LsrError, match="convention"):
        pack_scene(means, opac, shs, covariances=cov, convention="opengl")
    g = Gaussians(means[None], cov[None], opac[None], None, None)
    with pytest.raises(_lib.LsrError, match="color_harmonics"):
        save_gaussians("unused.ply", g)
    assert not os.path.exists("unused.ply")


def test_pack_scene_abi_rejections():
    """lsr_ply_pack_scene validates before it touches the device: these calls return without a GPU."""
    lib = _lib.load()
    one = C.c_void_p(16)                                                      # never dereferenced: every call is rejected
    def call(n=4, K_in=4, K_out=4, conv=0, major=0, ce=6, cov=one, scales=None, rot=None, means=one, rows=one, r_in=0, r_opt=0):
        inp = _lib.PlySceneInputs(means, one, one, cov, scales, rot, K_in, major, ce, r_in)
        opts = _lib.PlySceneOpts(conv, K_out, r_opt, 0)
        return lib.lsr_ply_pack_scene(n, C.byref(inp), C.byref(opts), rows, None)
    assert call(n=-1) == EINVAL
    assert call(K_in=3) == EINVAL and call(K_out=5) == EINVAL and call(K_in=4, K_out=9) == EINVAL
    assert call(conv=2) == EINVAL and call(major=2) == EINVAL and call(ce=7) == EINVAL
    assert call(r_in=1) == EINVAL and call(r_opt=1) == EINVAL
    assert call(means=None) == ENULL and call(rows=None) == ENULL
    assert call(cov=None) == ENULL and call(cov=None, scales=one) == ENULL
    assert lib.lsr_ply_pack_scene(4, None, None, one, None) == ENULL
    assert call(n=0, means=None, rows=None) == 0                              # nothing to do, nothing launched
