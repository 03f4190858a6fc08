"""Pose gradients of a GaussianScene's rigid parts without a GPU: the module's surface, every documented LSR_EINVAL /
LSR_ENULL / LSR_EUNSUPPORTED return of lsr_pose_matrices, lsr_pose_grad_workspace_bytes and lsr_scene_pose_grad (each
returns before any GPU work), the workspace size as a pure monotone function, the generated generator table, the analytic
twist formulas (numpy, with the committed table) against autograd of tests/pose_grad_ref.py, and the refusals of the
Python layer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import pose_grad_ref as pref
from tests import transform_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENULL, EUNSUPPORTED = 0, -1, -2, -5
P = C.c_void_p(0x1000)       # a non-NULL, 16-byte aligned pointer that is never dereferenced: every call below is refused
NAMES = ("lsr_pose_matrices", "lsr_pose_grad_workspace_bytes", "lsr_scene_pose_grad")


def test_new_symbols_are_exported_and_listed():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsr_pose.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in header, name
    assert lib.lsr_abi_version() == 10
    assert "#define LSR_POSE_MAX_TRANSFORMS 256" in header and _lib.POSE_MAX_TRANSFORMS == 256
    assert C.sizeof(_lib.PoseGradIn) == 56
    import latentsplat_amd
    for name in ("pose_matrices", "pose_scene", "PartPoses"):
        assert latentsplat_amd._LAZY[name] == "pose" and callable(getattr(latentsplat_amd, name))


# ---- the C ABI's argument checks ----

def _dims(**kw):
    base = dict(n=100, sh_coeffs=16, num_transforms=2, reserved0=0, reserved1=0)
    base.update(kw)
    return _lib.TransformDims(**base)


def _call(d, records=P, idx=P, quats=P, ws=P, ws_bytes=1 << 30, gq=P, gt=P, gl=P, K=16, **holes):
    rest = P if K > 1 else None
    fields = dict(xyz=P, rotation=P, features_rest=rest, g_xyz=P, g_features_rest=rest, g_scaling=P, g_rotation=P)
    fields.update(holes)
    gin = _lib.PoseGradIn(**fields)
    return _lib.load().lsr_scene_pose_grad(C.byref(d), records, idx, quats, C.byref(gin), ws, ws_bytes, gq, gt, gl, None)


def test_scene_pose_grad_argument_checks():
    lib = _lib.load()
    gin = _lib.PoseGradIn()
    assert lib.lsr_scene_pose_grad(None, P, P, P, C.byref(gin), P, 1 << 30, P, P, P, None) == ENULL
    assert lib.lsr_scene_pose_grad(C.byref(_dims()), P, P, P, None, P, 1 << 30, P, P, P, None) == ENULL
    assert _call(_dims(n=-1)) == EINVAL
    for K in (0, 2, 3, 5, 15, 17, 26, 36, -1):
        assert _call(_dims(sh_coeffs=K)) == EINVAL, K
    assert _call(_dims(num_transforms=-1)) == EINVAL
    assert _call(_dims(reserved0=1)) == EINVAL and _call(_dims(reserved1=1)) == EINVAL
    # features_rest against K
    assert _call(_dims(sh_coeffs=1), K=1, features_rest=P) == EINVAL
    assert _call(_dims(sh_coeffs=1), K=1, g_features_rest=P) == EINVAL
    # a quaternion pointer that is not 16-byte aligned
    assert _call(_dims(), rotation=C.c_void_p(0x1008)) == EINVAL
    assert _call(_dims(), g_rotation=C.c_void_p(0x1004)) == EINVAL
    # more transforms than the LDS tables hold: unsupported, whatever else is given
    assert _call(_dims(num_transforms=_lib.POSE_MAX_TRANSFORMS + 1)) == EUNSUPPORTED
    assert _call(_dims(num_transforms=1 << 20, n=0)) == EUNSUPPORTED
    # a workspace that is too small
    need = lib.lsr_pose_grad_workspace_bytes(100, 16, 2)
    assert need > 0 and _call(_dims(), ws_bytes=need - 1) == EINVAL
    # NULL pointers that are needed
    assert _call(_dims(), quats=None) == ENULL
    assert _call(_dims(), records=None) == ENULL and _call(_dims(), ws=None) == ENULL
    for g, companion in (("g_xyz", "xyz"), ("g_rotation", "rotation"), ("g_features_rest", "features_rest")):
        assert _call(_dims(), **{companion: None}) == ENULL, companion
    # nothing to do: no transforms, or no output wanted (the checks above still come first)
    assert _call(_dims(num_transforms=0), records=None, quats=None, ws=None, ws_bytes=0) == OK
    assert _call(_dims(), gq=None, gt=None, gl=None, records=None, ws=None) == OK
    assert _call(_dims(num_transforms=0, sh_coeffs=7)) == EINVAL and _call(_dims(num_transforms=0, reserved0=2)) == EINVAL
    # without grad_quaternion the quaternions are not asked for: the next check (records) answers
    assert _call(_dims(), quats=None, gq=None, records=None) == ENULL


def test_pose_matrices_argument_checks():
    lib = _lib.load()
    assert lib.lsr_pose_matrices(-1, P, P, P, P, None) == EINVAL
    assert lib.lsr_pose_matrices(0, None, None, None, None, None) == OK
    assert lib.lsr_pose_matrices(1, None, P, P, P, None) == ENULL
    assert lib.lsr_pose_matrices(1, P, None, P, P, None) == ENULL
    assert lib.lsr_pose_matrices(1, P, P, None, None, None) == ENULL


def test_workspace_bytes_is_a_pure_monotone_function():
    lib = _lib.load()
    f = lib.lsr_pose_grad_workspace_bytes
    assert f(1000, 16, 3) == f(1000, 16, 3) > 0
    assert f(-1, 16, 3) == 0 and f(10, 7, 3) == 0 and f(10, 16, -1) == 0 and f(10, 16, _lib.POSE_MAX_TRANSFORMS + 1) == 0
    assert f(0, 16, 3) == 0 and f(10, 16, 0) == 0
    ns = (0, 1, 63, 64, 65, 128, 129, 10_000, 131_072, 131_073, 262_144, 262_145, 3_000_000, 1 << 31)
    for K in (1, 4, 9, 16, 25):
        for T in (1, 3, 64, 256):
            sizes = [f(n, K, T) for n in ns]
            assert sizes == sorted(sizes), (K, T)
            assert sizes[-1] <= 2048 * T * 56                       # the grid cap keeps the partial table small
    for n in ns:
        for K in (1, 4, 9, 16, 25):
            sizes = [f(n, K, T) for T in (0, 1, 2, 64, 255, 256)]
            assert sizes == sorted(sizes), (n, K)
        for T in (1, 256):
            sizes = [f(n, K, T) for K in (1, 4, 9, 16, 25)]
            assert sizes == sorted(sizes), (n, T)
    assert f(100, 16, 2) == 2 * 2 * 56                              # two 64-Gaussian chunks of two transforms' 7 doubles


# ---- the generated table ----

def test_generator_table_check_and_committed_header():
    tool = os.path.join(ROOT, "tools", "gen_sh_generator_table.py")
    r = subprocess.run([sys.executable, tool, "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pairs [[0, 1, 3, 5, 7], [0, 1, 3, 5, 7], [0, 1, 2, 3, 4]]" in r.stdout             # 42 in all
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_sh_generator_table as gen
    finally:
        sys.path.pop(0)
    assert open(gen.HEADER).read() == gen.render()


def _table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_sh_generator_table as gen
    finally:
        sys.path.pop(0)
    return gen.parse(open(gen.HEADER).read())[0]


def test_generator_table_equals_the_references_generators():
    J, own = _table(), pref.generators()
    for a in range(3):
        for l in range(1, 5):
            assert np.abs(J[a][l] - own[a][l].numpy()).max() < 1e-12, (a, l)


def test_twist_formulas_equal_autograd_of_the_reference():
    """The per-Gaussian contributions of include/lsr_pose.h, in numpy with the committed table, summed per transform and
    pushed through dL/dp = (2 / |p|) (0, G_w) (x) p / |p|: equal to autograd of the float64 map to 1e-10, at degree 4, with
    non-unit quaternions, out-of-range rows and a transform that owns nothing."""
    J = _table()
    n, K, T = 40, 25, 4
    scene = tref.f64(tref.random_scene(n, K, 5))
    p, t, ls = (v.double() for v in pref.random_poses(T, 9))
    idx = torch.from_numpy(np.random.default_rng(4).integers(-1, 3, size=n))       # -1 .. 2 with T = 4: 3 owns nothing
    gen = torch.Generator().manual_seed(2)
    grads = [torch.randn(s.shape, generator=gen, dtype=torch.float64) for s in scene]
    signs = torch.tensor([1.0, -1.0, 1.0, 1.0], dtype=torch.float64)
    want_p, want_t, want_l = pref.pose_grads(scene, p, t, ls, idx, grads, signs)
    with torch.no_grad():
        out = [o.numpy() for o in pref.forward(*scene, p, t, ls, idx, signs)]
    gx, gc, gs, gq = (g.numpy() for g in grads)
    x = scene[0].numpy()
    for k in range(T):
        rows = np.nonzero(idx.numpy() == k)[0]
        Gw, Gt, Gl = np.zeros(3), np.zeros(3), 0.0
        A = float(ls[k].exp()) * pref.rotation(p[k]).numpy()
        for r in rows:
            y = A @ x[r]
            Gw += np.cross(y, gx[r])
            Gt += gx[r]
            Gl += gx[r] @ y + gs[r].sum()
            w, v, gw, gv = out[3][r, 0], out[3][r, 1:], gq[r, 0], gq[r, 1:]
            Gw += 0.5 * (w * gv - gw * v + np.cross(v, gv))
            for l in range(1, 5):
                sl = slice(l * l - 1, (l + 1) ** 2 - 1)
                for a in range(3):
                    Gw[a] += np.einsum("ic,ij,jc->", gc[r, sl], J[a][l], out[1][r, sl])
        got_p = pref.twist_to_quaternion(Gw, p[k].numpy())
        scale = max(1.0, float(want_p.abs().max()))
        assert np.abs(got_p - want_p[k].numpy()).max() < 1e-10 * scale, k
        assert np.abs(Gt - want_t[k].numpy()).max() < 1e-10 * scale and abs(Gl - float(want_l[k])) < 1e-10 * scale, k
        assert abs(got_p @ p[k].numpy()) < 1e-10 * scale                   # orthogonal to p: no projection needed
        if k == 3:
            assert not rows.size and not np.any(got_p) and not np.any(Gt) and Gl == 0.0


def test_reference_forward_is_the_transform_reference():
    """The differentiable restatement agrees with transform_ref's (numpy least squares, SVD split) on a similarity."""
    p, t, ls = (v.double() for v in pref.random_poses(1, 3))
    R = pref.rotation(p[0]).numpy()
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = float(ls[0].exp()) * R, t[0].numpy()
    scene = tref.f64(tref.random_scene(7, 25, 1))
    c = tref.Constants(M, 4, like_q=(p[0] / p[0].norm()).numpy())
    for a, b in zip(pref.forward(*scene, p, t, ls), tref.forward(c, *scene)):
        assert float((a - b).abs().max()) < 1e-11


# ---- the Python layer ----

def test_pose_scene_and_part_poses_refuse_cpu_tensors():
    from latentsplat_amd.pose import PartPoses, pose_matrices, pose_scene
    from latentsplat_amd.scene_model import GaussianScene
    sc = tref.random_scene(4, 16, 0)
    p, t, ls = pref.random_poses(2, 1)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        pose_scene(sc["xyz"], sc["features_rest"], sc["scaling"], sc["rotation"], p, t, ls)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        pose_matrices(p, t, ls)
    poses = PartPoses(2, learn_scale=True)
    assert [k for k, _ in poses.named_parameters()] == ["rotation", "translation", "log_scale"]
    assert [k for k, _ in PartPoses(3).named_parameters()] == ["rotation", "translation"]
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        poses.matrices()
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        poses(sc["xyz"], sc["features_rest"], sc["scaling"], sc["rotation"])
    assert torch.equal(poses.as_matrices(), torch.eye(4, dtype=torch.float64).expand(2, 4, 4))
    with pytest.raises(_lib.LsrError, match="LSR_POSE_MAX_TRANSFORMS"):
        PartPoses(_lib.POSE_MAX_TRANSFORMS + 1)
    scene = GaussianScene(sc["xyz"], torch.zeros(4, 1, 3), sc["features_rest"], torch.zeros(4, 1), sc["scaling"], sc["rotation"])
    with pytest.raises(_lib.LsrError, match="poses together with transforms"):
        scene.render(torch.zeros(1, 44), 16, 16, poses=poses, transforms=torch.eye(4))
    with pytest.raises(_lib.LsrError, match="poses together with transforms"):
        scene.activated(poses=poses, transforms=torch.eye(4))
    with pytest.raises(_lib.LsrError, match="filter_3d"):
        scene.render(torch.zeros(1, 44), 16, 16, poses=poses, filter_3d=torch.zeros(4))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.render(torch.zeros(1, 44), 16, 16, poses=poses)


def test_part_poses_from_matrices_round_trips():
    from latentsplat_amd.pose import PartPoses
    from latentsplat_amd.transform import similarity_matrix
    M = torch.stack([similarity_matrix([0.3, -0.5, 0.2, 0.7], [1.0, -2.0, 3.0], 1.7),
                     similarity_matrix([-0.1, 0.9, 0.1, 0.2], [0.0, 5.0, -1.0], 0.6)])
    poses = PartPoses.from_matrices(M)
    assert poses.log_scale is not None and poses.num == 2
    assert float((poses.as_matrices() - M).abs().max()) < 1e-6          # float32 parameters
    rigid = PartPoses.from_matrices(similarity_matrix([0.3, -0.5, 0.2, 0.7], [1.0, -2.0, 3.0]))
    assert rigid.log_scale is None and rigid.num == 1
    with pytest.raises(_lib.LsrError, match="learn_scale"):
        PartPoses.from_matrices(M, learn_scale=False)


def test_tools_need_a_device():
    """In a child process that sees no ROCm device (the visibility variables hide any there is)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    for tool, args in (("align_ply.py", ["moving.ply", "--to", "fixed.ply", "--out", "out"]), ("bench_pose_grad.py", [])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *args], capture_output=True, text=True,
                           timeout=120, env=env)
        assert r.returncode != 0 and "needs an MI355X" in r.stderr, r.stdout + r.stderr
