"""The 3DGS activation map without a GPU: the float64 restatement against the import's, the host-side validation of
lsr_scene_activate_forward / _backward, the refusal of CPU tensors, and the scene-file row assembly."""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import SceneDims, SceneInGrads, SceneOutGrads, SceneOutputs, SceneParams
from tests import ply_import_ref as ref
from tests import scene_params_ref as sref

OK, EINVAL, ENULL = 0, -1, -2
A = 0x10000                   # a 16-byte aligned address that is never dereferenced: every case returns before any launch


@pytest.mark.parametrize("K", [1, 4, 16, 25])
def test_restatement_forward_is_the_imports(K):
    names = ref.standard_names(K)
    table = ref.make_table(500, names, seed=40 + K)
    p = sref.split_table(table, names)
    want, got = ref.expected(table, names), sref.expected(p)
    assert np.array_equal(p["xyz"], want["means"])
    for k in ("shs", "opacities", "scales", "rotations", "cov3D"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k]), k
    ref.assert_matches(got, want)
    half = sref.expected(p, 0.5)
    np.testing.assert_allclose(half["scales"], 0.5 * want["scales"], rtol=1e-6)
    np.testing.assert_allclose(half["cov3D"], 0.25 * want["cov3D"], rtol=1e-5, atol=1e-30)


def test_restatement_gradients_against_finite_differences():
    p = sref.make_params(6, 4, seed=2)
    up = sref.make_upstream(6, 4, seed=3)
    g = sref.gradients(p, up, 0.5)
    up64 = {k: torch.from_numpy(v.astype(np.float64)) for k, v in up.items()}

    def loss(q):
        out = sref.forward64({k: torch.from_numpy(q[k]) for k in sref.PARAMS}, 0.5)
        return float(sum((out[k] * up64[k]).sum() for k in up64))

    base = {k: p[k].astype(np.float64) for k in sref.PARAMS}
    rng = np.random.default_rng(0)
    for k in sref.PARAMS:
        d = rng.standard_normal(base[k].shape)
        h = 1e-6
        plus, minus = dict(base), dict(base)
        plus[k], minus[k] = base[k] + h * d, base[k] - h * d
        fd = (loss(plus) - loss(minus)) / (2 * h)
        assert abs(fd - float((g[k] * d).sum())) <= 1e-6 * max(1.0, abs(fd)), k


def _call(fn, dims, params, a, b=None):
    lib = _lib.load()
    r = lambda s: None if s is None else C.byref(s)
    if fn == "forward":
        return lib.lsr_scene_activate_forward(r(dims), r(params), r(a), None)
    return lib.lsr_scene_activate_backward(r(dims), r(params), r(a), r(b), None)


def _dims(n=100, K=4, m=1.0, r0=0, r1=0):
    return SceneDims(n=n, sh_coeffs=K, scale_modifier=m, reserved0=r0, reserved1=r1)


def _params(K=4, **kw):
    base = dict(features_dc=A, features_rest=A if K > 1 else None, opacity=A, scaling=A, rotation=A)
    base.update(kw)
    return SceneParams(**base)


BOTH = [("forward", lambda: (SceneOutputs(shs=A, opacities=A, cov3D=A, scales=A, rotations=A),)),
        ("backward", lambda: (SceneOutGrads(shs=A, opacities=A, cov3D=A),
                              SceneInGrads(features_dc=A, features_rest=A, opacity=A, scaling=A, rotation=A)))]


@pytest.mark.parametrize("fn,rest", BOTH, ids=["forward", "backward"])
def test_validation_before_any_gpu_work(fn, rest):
    # NULL structs
    assert _call(fn, None, _params(), *rest()) == ENULL
    assert _call(fn, _dims(), None, *rest()) == ENULL
    assert _call(fn, _dims(), _params(), *[None for _ in rest()]) == ENULL
    # invalid dims and combinations, each before anything is launched (no device is needed to be told so)
    for bad in (_dims(n=-1), _dims(K=0), _dims(K=2), _dims(K=36), _dims(m=0.0), _dims(m=-1.0), _dims(m=float("inf")),
                _dims(m=float("nan")), _dims(r0=1), _dims(r1=1)):
        assert _call(fn, bad, _params(), *rest()) == EINVAL
    for K in (1, 4, 9, 16, 25):
        assert _call(fn, _dims(n=0, K=K), _params(K), *rest()) == OK
    assert _call(fn, _dims(K=1), _params(4), *rest()) == EINVAL            # features_rest given with K == 1
    assert _call(fn, _dims(K=4), _params(1), *rest()) == EINVAL            # ... missing with K > 1
    assert _call(fn, _dims(n=0, K=4), _params(1), *rest()) == EINVAL       # (checked before the empty-scene return)
    # n == 0 launches nothing, whatever the tensors
    assert _call(fn, _dims(n=0), SceneParams(features_rest=A), *rest()) == OK
    # NULL required tensors with n > 0
    required = ("features_dc", "opacity", "scaling", "rotation") if fn == "forward" else ("opacity", "scaling", "rotation")
    for name in required:
        assert _call(fn, _dims(), _params(**{name: None}), *rest()) == ENULL, name
    # misaligned quads
    assert _call(fn, _dims(), _params(rotation=A + 4), *rest()) == EINVAL
    if fn == "forward":
        assert _call(fn, _dims(), _params(), SceneOutputs(shs=A, rotations=A + 8)) == EINVAL
    else:
        assert _call(fn, _dims(), _params(), rest()[0], SceneInGrads(rotation=A + 12)) == EINVAL


def test_cpu_tensors_are_refused():
    from latentsplat_amd import GaussianScene, activate_scene
    p = {k: torch.from_numpy(v) for k, v in sref.make_params(10, 4, seed=1).items()}
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        activate_scene(p["features_dc"], p["features_rest"], p["opacity"], p["scaling"], p["rotation"])
    scene = GaussianScene.from_tensors(**p)
    assert scene.max_sh_degree == 1 and scene.active_sh_degree == 1 and scene.num_gaussians == 10
    assert [k for k, _ in scene.named_parameters()] == ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.render(torch.zeros(1, 44), 16, 16)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        scene.activated()
    with pytest.raises(_lib.LsrError):
        GaussianScene.from_tensors(**dict(p, features_rest=p["features_rest"][:, :2]))      # K = 3


@pytest.mark.parametrize("K,shuffled", [(1, False), (4, False), (16, False), (25, False), (9, True)])
def test_scene_file_rows_round_trip_bit_for_bit(tmp_path, K, shuffled):
    """from_ply then save_ply, on the host: the parameters are the file's columns (f_rest transposed from the file's
    channel-major order) and the saved rows are the loaded ones in the published order, bit for bit."""
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.ply_import import read_header
    names = ref.shuffled_names(K, extra=3, seed=7) if shuffled else ref.standard_names(K)
    table = ref.make_table(300, names, seed=K)
    if not shuffled:
        table[:, 3:6] = 0.0                                                 # normals, as trainers write them
    ref.write_ply(tmp_path / "in.ply", names, table)
    scene = GaussianScene.from_ply(tmp_path / "in.ply", "cpu")
    p = sref.split_table(table, names)
    for k, v in p.items():
        assert np.array_equal(getattr(scene, "_" + k).detach().numpy(), v), k
    assert scene.max_sh_degree == {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}[K]
    scene.save_ply(tmp_path / "out" / "point_cloud.ply")
    layout = read_header(tmp_path / "out" / "point_cloud.ply")
    assert (layout.n, layout.stride, layout.sh_coeffs) == (300, 14 + 3 * K, K)
    saved = np.fromfile(tmp_path / "out" / "point_cloud.ply", "<f4", offset=layout.data_offset).reshape(300, -1)
    assert np.array_equal(saved, sref.expected_rows(p))
    if not shuffled:
        assert np.array_equal(saved, table)                                 # the file itself, normals (zero) included
        assert (tmp_path / "out" / "point_cloud.ply").read_bytes()[layout.data_offset:] == \
            (tmp_path / "in.ply").read_bytes()[read_header(tmp_path / "in.ply").data_offset:]


def test_probability_files_are_refused(tmp_path):
    from latentsplat_amd import GaussianScene
    names = ref.standard_names(1)
    table = ref.make_table(50, names, seed=3)
    table[:, names.index("opacity")] = np.random.default_rng(0).uniform(0.0, 1.0, 50).astype(np.float32)
    ref.write_ply(tmp_path / "viewer.ply", names, table)
    with pytest.raises(_lib.LsrError, match=r'load_ply\(path, device, opacity="raw"\)'):
        GaussianScene.from_ply(tmp_path / "viewer.ply", "cpu")
    assert GaussianScene.from_ply(tmp_path / "viewer.ply", "cpu", check_opacity=False).num_gaussians == 50
