"""The codebook compression without a GPU: the exported names, the host side of lsr_vq_* (sizing, every argument check:
all of them return before any GPU work), the refusal of CPU tensors, QuantizedScene's file and gathers on CPU tensors, and
the float64 reference of tests/vq_ref.py against its own bars (a bar is a condition: the reference has to meet it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import vq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_names_are_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsr_vq.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lsr_[a-z_0-9]+)\s*\(", text)))
    assert names == ["lsr_vq_assign", "lsr_vq_update", "lsr_vq_workspace_bytes"]
    lib = _lib.load()
    assert all(hasattr(lib, n) and n in _lib.EXPORTS for n in names)
    assert lib.lsr_abi_version() == 10
    for macro, value in (("MAX_DIM", _lib.VQ_MAX_DIM), ("MAX_CODES", _lib.VQ_MAX_CODES), ("ROWS", _lib.VQ_ROWS), ("CODES", _lib.VQ_CODES),
                         ("KSTEP", _lib.VQ_KSTEP)):
        assert int(re.search(rf"#define LSR_VQ_{macro} (\d+)", text).group(1)) == value
    assert (ref.ROWS, ref.CODES, ref.KSTEP) == (_lib.VQ_ROWS, _lib.VQ_CODES, _lib.VQ_KSTEP)
    assert C.sizeof(_lib.VqDims) == 24


def test_workspace_bytes():
    lib = _lib.load()
    f = lib.lsr_vq_workspace_bytes
    assert f(3_000_000, 4096, 45) == f(3_000_000, 4096, 45) > 3_000_000 * 12
    for d in (0, 97, -1):
        assert f(1000, 64, d) == 0
    for k in (0, 65537, -1):
        assert f(1000, k, 7) == 0
    assert f(-1, 64, 7) == 0 and f(-(1 << 40), 64, 7) == 0 and f(_lib.VQ_MAX_ROWS + 1, 64, 7) == 0
    for d in (1, 7, 45, 96):
        by_n = [f(n, 4096, d) for n in ref.NS + [3_000_000]]
        by_k = [f(20_011, k, d) for k in ref.KS + [65536]]
        assert all(s > 0 for s in by_n + by_k) and by_n == sorted(by_n) and by_k == sorted(by_k)


@pytest.mark.parametrize("n, k, d, r0, on, code", [
    (-1, 4, 4, 0, 1, -1), (10, 0, 4, 0, 1, -1), (10, 65537, 4, 0, 1, -1), (10, 4, 0, 0, 1, -1), (10, 4, 97, 0, 1, -1),
    (_lib.VQ_MAX_ROWS + 1, 4, 4, 0, 1, -1), (10, 4, 4, 1, 1, -1),
    (10, 4, 4, 0, 0, -2),
    (0, 4, 4, 0, 0, 0),                                    # n == 0: nothing to do, nothing needed
])
def test_arguments_are_checked_before_any_gpu_work(n, k, d, r0, on, code):
    """Dummy pointers: a call that got past the checks would have to touch them (and a device this machine lacks)."""
    lib = _lib.load()
    dims = _lib.VqDims(n=n, k=k, d=d, reserved0=r0)
    p = C.c_void_p(0x1000 if on else None)
    assert lib.lsr_vq_assign(C.byref(dims), p, p, p, None, p, None) == code
    assert lib.lsr_vq_update(C.byref(dims), p, p, None, p, p, p, p, None) == code
    assert lib.lsr_vq_assign(None, p, p, p, None, p, None) == -2 and lib.lsr_vq_update(None, p, p, None, p, p, p, p, None) == -2
    if code == -2:                                         # each required pointer on its own
        q = C.c_void_p(0x1000)
        for hole in range(4):
            args = [q, q, q, q]
            args[hole] = None
            assert lib.lsr_vq_assign(C.byref(dims), args[0], args[1], args[2], None, args[3], None) == -2
        for hole in range(6):
            args = [q] * 6
            args[hole] = None
            assert lib.lsr_vq_update(C.byref(dims), args[0], args[1], None, args[2], args[3], args[4], args[5], None) == -2


def test_lazy_names_resolve():
    import latentsplat_amd
    from latentsplat_amd import vq
    for name in ("vq_assign", "vq_update", "kmeans", "quantize_scene", "QuantizedScene", "contribution_weights"):
        assert latentsplat_amd._LAZY[name] == "vq" and getattr(latentsplat_amd, name) is getattr(vq, name)
    assert "``vq``" in latentsplat_amd.__doc__
    assert callable(latentsplat_amd.GaussianScene.quantize)


def _cpu_scene(n=50, degree=1, seed=0):
    from latentsplat_amd import GaussianScene
    g = torch.Generator().manual_seed(seed)
    K = (degree + 1) ** 2
    r = lambda *s: torch.randn(*s, generator=g)
    return GaussianScene(r(n, 3), r(n, 1, 3), r(n, K - 1, 3), r(n, 1), r(n, 3), r(n, 4))


def test_cpu_tensors_are_refused():
    from latentsplat_amd import kmeans, quantize_scene, vq_assign, vq_update
    x, c = (torch.from_numpy(a.copy()) for a in ref.case("normal", 64, 17, 4))
    idx = torch.zeros(64, dtype=torch.int32)
    for call in (lambda: vq_assign(x, c), lambda: vq_assign(x, c, want_dist=True), lambda: vq_update(x, idx, c),
                 lambda: kmeans(x, 17), lambda: kmeans(x, 17, init=c), lambda: quantize_scene(_cpu_scene()),
                 lambda: _cpu_scene().quantize(rest_codes=4)):
        with pytest.raises(_lib.LsrError, match="no CPU fallback"):
            call()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("degree", [0, 1, 3])
def test_quantized_scene_file_and_gathers_on_cpu(tmp_path, degree):
    from latentsplat_amd import QuantizedScene
    n, k_r, k_s = 300, 70, 40
    g = torch.Generator().manual_seed(degree)
    r = lambda *s: torch.randn(*s, generator=g)
    K = (degree + 1) ** 2
    q = QuantizedScene(xyz=r(n, 3), features_dc=r(n, 1, 3), opacity=r(n, 1),
                       rest_codebook=r(k_r, K - 1, 3) if degree else None,
                       rest_idx=torch.randint(0, k_r, (n,), generator=g, dtype=torch.int32) if degree else None,
                       shape_codebook=r(k_s, 7), shape_idx=torch.randint(0, k_s, (n,), generator=g, dtype=torch.int32),
                       max_sh_degree=degree, active_sh_degree=min(degree, 1))
    path = tmp_path / "scene.npz"
    q.save(path)
    with np.load(path) as z:
        assert z["shape_idx"].dtype == np.uint16 and z["xyz"].dtype == np.float32
        assert ("rest_idx" in z.files) == bool(degree) and (not degree or z["rest_idx"].dtype == np.uint16)
    back = QuantizedScene.load(path, "cpu")
    for name in ("xyz", "features_dc", "opacity", "rest_codebook", "rest_idx", "shape_codebook", "shape_idx"):
        a, b = getattr(q, name), getattr(back, name)
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), name
    assert (back.max_sh_degree, back.active_sh_degree) == (degree, min(degree, 1))
    scene = back.dequantize()
    assert scene.num_gaussians == n and scene.max_sh_degree == degree and scene.active_sh_degree == min(degree, 1)
    shape = torch.stack([q.shape_codebook[int(j)] for j in q.shape_idx])
    assert torch.equal(_bits(scene._scaling), _bits(shape[:, :3])) and torch.equal(_bits(scene._rotation), _bits(shape[:, 3:]))
    assert torch.equal(_bits(scene._xyz), _bits(q.xyz)) and torch.equal(_bits(scene._features_dc), _bits(q.features_dc))
    assert torch.equal(_bits(scene._opacity), _bits(q.opacity))
    if degree:
        rest = torch.stack([q.rest_codebook[int(j)] for j in q.rest_idx])
        assert torch.equal(_bits(scene._features_rest), _bits(rest))
    else:
        assert tuple(scene._features_rest.shape) == (n, 0, 3)
    floats = n * 7 + k_s * 7 + (k_r * (K - 1) * 3 if degree else 0)
    assert q.nbytes == 4 * floats + 2 * n * (2 if degree else 1)


def test_shape_rows_fix_the_sign():
    from latentsplat_amd.vq import shape_rows
    q = torch.tensor([[0.5, -0.5, 0.5, -0.5], [-0.5, 0.5, 0.5, 0.5], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, -2.0], [0.0, 0.0, 3.0, -4.0],
                      [0.0, 0.0, 0.0, 0.0]])
    s = torch.arange(18.0).reshape(6, 3)
    rows = shape_rows(s, q)
    want = torch.tensor([[0.5, -0.5, 0.5, -0.5], [0.5, -0.5, -0.5, -0.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.6, -0.8],
                         [0.0, 0.0, 0.0, 0.0]])
    assert torch.equal(rows[:, :3], s) and torch.allclose(rows[:, 3:], want, atol=1e-7)
    assert torch.equal(_bits(rows[:4, 3:]), _bits(want[:4]))          # unit quaternions with exact norms keep their bits; no -0.0
    assert torch.equal(_bits(shape_rows(s, -q)), _bits(rows))


@pytest.mark.parametrize("name", ref.NAMES + ("lattice",))
def test_the_reference_meets_its_own_bars(name):
    """Every generated case, the largest included: the reference picks its code from |x|^2 - 2 x.c + |c|^2; a direct float64
    search over the summed squared differences (tests/vq_ref.py assign_direct, sharing nothing with it but the inputs) must
    find no code nearer than the reference's choice by more than 1e-9 of the gap bar (float64 rounding of the two routes),
    and on the integer lattices, where both are exact, the same lowest index."""
    for n, k, d in ref.SHAPES:
        x, c = ref.case(name, n, k, d)
        idx, _ = ref.assign_ref(x, c)
        assert idx.shape == (n,) and (idx >= 0).all() and (idx < k).all(), (n, k, d)
        nearest, lowest = ref.assign_direct(x, c)
        gap = ref.chosen_dist2(x, c, idx) - nearest
        assert (gap <= 1e-9 * ref.gap_bar(x, c)).all(), (n, k, d, float(gap.max()))
        if name == "lattice":
            assert np.array_equal(idx, lowest), (n, k, d)
            assert np.array_equal(ref.chosen_dist2(x, c, idx), nearest), (n, k, d)


def test_the_shape_list():
    assert set(n for n, _, _ in ref.SHAPES) == set(ref.NS) and set(k for _, k, _ in ref.SHAPES) == set(ref.KS)
    assert set(d for _, _, d in ref.SHAPES) == set(ref.DS) and len(set(ref.SHAPES)) == len(ref.SHAPES) == 40
    for must in ((20_011, 4096, 72), (1, 1, 1), (65, 17, 5)):
        assert must in ref.SHAPES
    assert any(n < k for n, k, _ in ref.SHAPES)
    for centre, values in ((ref.ROWS, ref.NS), (ref.CODES, ref.KS), (ref.KSTEP, ref.DS)):
        assert all(centre + o in values for o in (-1, 0, 1))


def test_update_reference_and_planted_clusters():
    x, label, first = ref.planted(64, 2000, 45)
    assert len(set(label[first])) == 64 and (np.bincount(label, minlength=64) > 0).all()
    idx, _ = ref.assign_ref(x, x[first])
    assert np.array_equal(label[first][idx], label)
    prev = np.full((66, 45), 7.0)
    w = np.linspace(0.5, 2.0, 2000)
    code, mass, absmean = ref.update_ref(x, label, 66, prev, w)
    assert (code[64:] == 7.0).all() and (mass[64:] == 0).all() and (absmean[64:] == 0).all()
    j = 5
    rows = label == j
    assert np.allclose(code[j], (w[rows, None] * x[rows]).sum(0) / w[rows].sum(), rtol=1e-12)
    assert np.isclose(mass[j], w[rows].sum(), rtol=1e-12)
    skipped = label.copy()
    skipped[::2] = -1
    skipped[1::4] = 66
    code2, mass2, _ = ref.update_ref(x, skipped, 66, prev, w)
    keep = (skipped >= 0) & (skipped < 66)
    assert np.isclose(mass2.sum(), w[keep].sum(), rtol=1e-12)
