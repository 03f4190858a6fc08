"""Similarity transforms of a GaussianScene without a GPU: the float64 restatement of tests/transform_ref.py is consistent
with itself (composition, orthogonality, band 1 against R, the adjoint identity), the module's surface, the matrix helpers,
the similarity check of transform_records on CPU tensors, every documented LSR_EINVAL / LSR_ENULL case of
lsr_scene_transform and lsr_transform_records (each returns before any GPU work), the refusal of CPU tensors, the camera
map against a float64 restatement, the generated basis table and the tool's exit without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import sh_rotation_ref as shref
from tests import transform_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENULL = 0, -1, -2
P = C.c_void_p(0x1000)       # a non-NULL, 16-byte aligned pointer that is never dereferenced: every call below is refused


# ---- the restatement against itself ----

def test_reference_band_matrices_compose_and_are_orthogonal():
    rng = np.random.default_rng(3)
    R1, R2 = shref.random_rotations(2, rng)
    for l in range(1, 5):
        T1, r1 = ref.band_matrix(l, R1)
        T2, r2 = ref.band_matrix(l, R2)
        T12, r12 = ref.band_matrix(l, R1 @ R2)
        assert max(r1, r2, r12) < ref.FIT_RESIDUAL
        assert np.abs(T12 - T1 @ T2).max() < 1e-12
        assert np.abs(T1 @ T1.T - np.eye(2 * l + 1)).max() < 1e-12
        assert np.abs(ref.band_matrix(l, np.eye(3))[0] - np.eye(2 * l + 1)).max() < 1e-12
    # band 1 of the "3dgs" basis is (-y, z, -x) up to a factor: T_1 is a signed permutation of R
    S = np.array([[0, -1.0, 0], [0, 0, 1.0], [-1.0, 0, 0]])
    assert np.abs(ref.band_matrix(1, R1)[0] - S @ R1 @ S.T).max() < 1e-12


def test_reference_adjoint_identity_and_quaternion():
    rng = np.random.default_rng(5)
    M = ref.random_similarity(rng)
    c = ref.Constants(M, 4)
    x = ref.f64(ref.random_scene(9, 25, 1))
    y = ref.f64(ref.random_scene(9, 25, 2))
    zero = [torch.zeros_like(t) for t in x]
    linear = [a - b for a, b in zip(ref.forward(c, *x), ref.forward(c, *zero))]
    lhs = sum(float((a * b).sum()) for a, b in zip(y, linear))
    rhs = sum(float((a * b).sum()) for a, b in zip(ref.adjoint(c, *y), x))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # autograd of the forward is the adjoint
    xs = [t.clone().requires_grad_(True) for t in x]
    torch.autograd.backward(ref.forward(c, *xs), list(y))
    for got, want in zip((t.grad for t in xs), ref.adjoint(c, *y)):
        assert float((got - want).abs().max()) < 1e-12
    # q_R (x) q is the quaternion of R R(q), and R is a rotation with s R the matrix's linear part to float32 rounding
    from tests import scene_export_ref as sref
    q = x[3][:1].numpy()
    moved = (x[3][:1] @ c.L.T).numpy()
    assert np.abs(sref.rotation_matrices(moved)[0] - c.R @ sref.rotation_matrices(q)[0]).max() < 1e-12
    assert np.abs(c.R @ c.R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(c.R) > 0
    assert np.abs(c.s * c.R - M[:3, :3].astype(np.float64)).max() < 4 * ref.U * c.s
    assert abs(np.linalg.norm(moved) - np.linalg.norm(q)) < 1e-12


# ---- the module's surface ----

def test_new_symbols_are_exported_and_listed():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsr_transform.h")).read()
    for name in ("lsr_transform_records", "lsr_scene_transform"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in header, name
    import latentsplat_amd
    for name in ("similarity_matrix", "invert_similarity", "transform_records", "transform_scene", "transform_cameras"):
        assert latentsplat_amd._LAZY[name] == "transform" and callable(getattr(latentsplat_amd, name))
    assert lib.lsr_abi_version() == 10
    assert C.sizeof(_lib.TransformDims) == 24 and C.sizeof(_lib.TransformIn) == 32 and C.sizeof(_lib.TransformOut) == 32
    assert [_lib.transform_record_floats(d) for d in range(5)] == [20, 29, 54, 103, 184]
    assert "#define LSR_TRANSFORM_HEADER_FLOATS 20" in header
    from latentsplat_amd.scene_model import GaussianScene
    assert callable(GaussianScene.transform_) and callable(GaussianScene.merge)


def test_similarity_matrix_and_inverse_compose_to_the_identity():
    from latentsplat_amd.transform import invert_similarity, quaternion_matrix, similarity_matrix
    rng = np.random.default_rng(11)
    for _ in range(5):
        q = rng.normal(size=4)
        t, s = rng.normal(size=3) * 100, float(np.exp(rng.uniform(-2, 2)))
        M = similarity_matrix(q, t, s)
        assert M.dtype == torch.float64 and tuple(M.shape) == (4, 4)
        R = quaternion_matrix(q)
        assert torch.equal(M[:3, :3], R * s) and M[3].tolist() == [0, 0, 0, 1]
        assert torch.equal(similarity_matrix(R.numpy(), t, s), M)
        eye = invert_similarity(M) @ M
        assert float((eye - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-12
        both = invert_similarity(torch.stack([M, M]))
        assert torch.allclose(both[0], invert_similarity(M), rtol=1e-13, atol=0) and torch.equal(both[1], both[0])
    assert torch.equal(similarity_matrix(), torch.eye(4, dtype=torch.float64))
    with pytest.raises(_lib.LsrError, match="3x3 matrix or a w,x,y,z quaternion"):
        similarity_matrix(np.zeros(5))


def _good():
    from latentsplat_amd.transform import similarity_matrix
    return similarity_matrix([0.3, -0.5, 0.2, 0.7], [1.0, -2.0, 3.0], 1.7)


@pytest.mark.parametrize("what,match", [
    ("reflection", "determinant"), ("shear", "shear or non-uniform scale"), ("nonuniform", "shear or non-uniform scale"),
    ("last_row", "last row"), ("nan", "non-finite"), ("singular", "determinant"), ("second_of_two", "transform 1")])
def test_transform_records_refuses_what_is_not_a_similarity(what, match):
    """On CPU tensors: the check is one host read that comes before any GPU work."""
    from latentsplat_amd.transform import transform_records
    M = _good()
    if what == "reflection":
        M[:3, 0] *= -1
    elif what == "shear":
        M[0, 1] += 1e-3
    elif what == "nonuniform":
        M[:3, 2] *= 1.001
    elif what == "last_row":
        M[3, 0] = 0.1
    elif what == "nan":
        M[1, 3] = float("nan")
    elif what == "singular":
        M[:3, :3] = 0
    elif what == "second_of_two":
        bad = M.clone()
        bad[:3, 1] *= 2
        M = torch.stack([M, bad])
    with pytest.raises(_lib.LsrError, match=match):
        transform_records(M, 3)
    with pytest.raises(_lib.LsrError, match=match):
        transform_records(M.to(torch.float32), 3)


def test_transform_records_accepts_float32_rotations_and_needs_a_device():
    from latentsplat_amd.transform import check_similarity, transform_records
    rng = np.random.default_rng(2)
    for _ in range(20):      # float32 roundings of a rotation are far inside the 1e-5 bound
        check_similarity(torch.from_numpy(ref.random_similarity(rng))[None])
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        transform_records(_good(), 3)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        transform_records(_good(), 3, check=False)
    with pytest.raises(_lib.LsrError, match="degree"):
        transform_records(_good(), 5)
    with pytest.raises(_lib.LsrError, match=r"\(4, 4\) or \(T, 4, 4\)"):
        transform_records(torch.eye(3), 1)


def test_transform_scene_refuses_cpu_tensors():
    from latentsplat_amd.scene_model import GaussianScene
    from latentsplat_amd.transform import transform_scene
    sc = ref.random_scene(4, 16, 0)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        transform_scene(sc["xyz"], sc["features_rest"], sc["scaling"], sc["rotation"], _good())
    scene = GaussianScene(sc["xyz"], torch.zeros(4, 1, 3), sc["features_rest"], torch.zeros(4, 1), sc["scaling"], sc["rotation"])
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.transform_(_good())
    with pytest.raises(_lib.LsrError, match="filter_3d"):
        scene.render(torch.zeros(1, 44), 16, 16, transforms=_good(), filter_3d=torch.zeros(4))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.render(torch.zeros(1, 44), 16, 16, transforms=_good())


# ---- the C ABI's argument checks ----

def _dims(**kw):
    base = dict(n=100, sh_coeffs=16, num_transforms=2, reserved0=0, reserved1=0)
    base.update(kw)
    return _lib.TransformDims(**base)


def _io(K=16, **holes):
    rest = P if K > 1 else None
    tin = dict(xyz=P, features_rest=rest, scaling=P, rotation=P)
    tout = dict(xyz=P, features_rest=rest, scaling=P, rotation=P)
    for k, v in holes.items():
        (tin if k.startswith("in_") else tout)[k.split("_", 1)[1]] = v
    return _lib.TransformIn(**tin), _lib.TransformOut(**tout)


def _call(d, records=P, idx=P, K=16, **holes):
    tin, tout = _io(K, **holes)
    return _lib.load().lsr_scene_transform(C.byref(d), records, idx, C.byref(tin), C.byref(tout), None)


def test_scene_transform_argument_checks():
    lib = _lib.load()
    tin, tout = _io()
    assert lib.lsr_scene_transform(None, P, P, C.byref(tin), C.byref(tout), None) == ENULL
    assert lib.lsr_scene_transform(C.byref(_dims()), P, P, None, C.byref(tout), None) == ENULL
    assert lib.lsr_scene_transform(C.byref(_dims()), P, P, C.byref(tin), None, None) == ENULL
    assert _call(_dims(n=-1)) == EINVAL
    for K in (0, 2, 3, 5, 15, 17, 26, 36, -1):
        assert _call(_dims(sh_coeffs=K)) == EINVAL, K
    assert _call(_dims(num_transforms=0)) == EINVAL and _call(_dims(num_transforms=-3)) == EINVAL
    assert _call(_dims(reserved0=1)) == EINVAL and _call(_dims(reserved1=1)) == EINVAL
    # features_rest against K
    assert _call(_dims(sh_coeffs=1), K=1, in_features_rest=P) == EINVAL
    assert _call(_dims(sh_coeffs=1), K=1, out_features_rest=P) == EINVAL
    assert _call(_dims(), in_features_rest=None) == EINVAL
    # a rotation pointer that is not 16-byte aligned
    assert _call(_dims(), in_rotation=C.c_void_p(0x1008)) == EINVAL
    assert _call(_dims(), out_rotation=C.c_void_p(0x1004)) == EINVAL
    # with n > 0: NULL records, a wanted output without its input
    assert _call(_dims(), records=None) == ENULL
    for name in ("xyz", "scaling", "rotation"):
        assert _call(_dims(), **{"in_" + name: None}) == ENULL, name
    # n == 0 is fine whatever the pointers; so is a call that wants nothing
    assert _call(_dims(n=0), records=None, idx=None) == OK
    assert _call(_dims(n=0, sh_coeffs=1), records=None, K=1) == OK
    assert _call(_dims(), out_xyz=None, out_features_rest=None, out_scaling=None, out_rotation=None) == OK
    # the checks come first also with n == 0
    assert _call(_dims(n=0, sh_coeffs=7)) == EINVAL and _call(_dims(n=0, reserved0=2)) == EINVAL


def test_transform_records_argument_checks():
    lib = _lib.load()
    assert lib.lsr_transform_records(-1, P, 3, 0, P, None) == EINVAL
    assert lib.lsr_transform_records(1, P, 5, 0, P, None) == EINVAL and lib.lsr_transform_records(1, P, -1, 0, P, None) == EINVAL
    assert lib.lsr_transform_records(1, P, 3, 2, P, None) == EINVAL
    assert lib.lsr_transform_records(0, None, 3, 0, None, None) == OK
    assert lib.lsr_transform_records(1, None, 3, 0, P, None) == ENULL and lib.lsr_transform_records(1, P, 3, 1, None, None) == ENULL


# ---- cameras ----

def test_transform_cameras_against_a_float64_restatement():
    """The world point a camera sees at pixel (u, v) and depth z maps to M times that point, seen by the moved camera at
    the same pixel and depth s z."""
    from latentsplat_amd.transform import transform_cameras
    rng = np.random.default_rng(21)
    M = np.eye(4)                                            # float64 throughout: a similarity to 1e-16
    M[:3, :3] = 2.5 * shref.random_rotations(1, rng)[0]
    M[:3, 3] = rng.normal(size=3) * 10
    M = torch.from_numpy(M)
    s, R, t = ref.split(M.numpy())
    V = 3
    ext = np.tile(np.eye(4), (V, 1, 1))
    ext[:, :3, :3] = shref.random_rotations(V, rng)
    ext[:, :3, 3] = rng.normal(size=(V, 3)) * 5
    near, far = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64), torch.tensor([10.0, 20.0, 30.0], dtype=torch.float64)
    ext2, near2, far2 = transform_cameras(torch.from_numpy(ext), near, far, M)
    assert ext2.dtype == torch.float64 and tuple(ext2.shape) == (V, 4, 4)
    assert torch.allclose(near2, near * s, rtol=1e-14) and torch.allclose(far2, far * s, rtol=1e-14)
    Kinv = np.linalg.inv(np.array([[0.8, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1.0]]))
    for v in range(V):
        for _ in range(4):
            u, w, z = rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.5, 8)
            p_cam = Kinv @ np.array([u, w, 1.0]) * z
            world = ext[v, :3, :3] @ p_cam + ext[v, :3, 3]
            moved = M.numpy()[:3, :3] @ world + M.numpy()[:3, 3]
            seen = ext2[v, :3, :3].numpy() @ (p_cam * s) + ext2[v, :3, 3].numpy()
            assert np.abs(seen - moved).max() < 1e-11 * max(1.0, np.abs(moved).max())
    assert np.abs(ext2[:, :3, :3].numpy() - R @ ext[:, :3, :3]).max() < 1e-14
    assert ext2[:, 3].tolist() == [[0, 0, 0, 1]] * V
    f32 = transform_cameras(torch.from_numpy(ext).float(), near.float(), far.float(), M)
    assert f32[0].dtype == torch.float32 and f32[1].dtype == torch.float32
    assert float((f32[0].double() - ext2).abs().max()) < 1e-5 * float(ext2.abs().max())


# ---- the generated table and the tools ----

def test_basis_table_generator_check():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sh_basis_table.py"), "--check"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "non-zeros [1, 3, 7, 13, 21]" in r.stdout            # 45 in all


@pytest.mark.parametrize("tool,args", [("transform_ply.py", ["in.ply", "out.ply", "--scale", "2"]),
                                       ("bench_scene_transform.py", [])])
def test_tools_need_a_device(tool, args):
    """In a child process that sees no ROCm device (the visibility variables hide any there is)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *args], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode != 0 and "needs an MI355X" in r.stderr, r.stdout + r.stderr
