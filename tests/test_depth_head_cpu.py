"""Fused depth head without a GPU: the float64 restatement (tests/depth_head_ref.py) reproduces the vectors
the reference's DepthPredictorMonocular generated (tests/golden/make_golden_depth_head.py); the C ABI of
include/lsr_depth_head.h is exported and validates its arguments on the host; the Python surface."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import depth_head_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "depth_head_*.npz")))
case_id = lambda p: os.path.basename(p)[len("depth_head_"):-4]


def flat_case(path):
    """The golden arrays with (b, v) merged into cameras, and the keyword arguments of the restatement."""
    z = np.load(path)
    b, v, rays, F, k = z["depth"].shape
    c = {n: z[n].reshape((b * v, rays) + z[n].shape[3:]) for n in
         ("logits", "uniforms", "depth", "opacity", "index", "g_depth", "g_opacity", "d_logits")}
    c["near"], c["far"] = z["near"].reshape(-1), z["far"].reshape(-1)
    kw = dict(uniforms=c["uniforms"], deterministic=bool(z["deterministic"]), samples=k,
              transmittance=bool(z["transmittance"]), exponent=float(z["opacity_exponent"]),
              scale=float(z["opacity_scale"]))
    return z, c, int(z["surfaces"]), kw


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(1e-6, np.abs(want).max()))


def test_the_golden_cases_are_the_issue_s():
    shapes = {case_id(p): np.load(p)["depth"].shape + (np.load(p)["logits"].shape[-1],) for p in GOLDEN}
    assert shapes == {"stochastic": (2, 2, 48, 1, 3, 64), "deterministic_two_surfaces": (1, 3, 25, 2, 1, 128),
                      "transmittance": (1, 2, 40, 1, 3, 16), "ragged_three_surfaces": (1, 2, 30, 3, 2, 72),
                      "wide_64": (2, 2, 48, 1, 3, 128), "opacity_map_sqrt2": (1, 2, 40, 1, 3, 64),
                      "opacity_map_half": (1, 2, 40, 2, 3, 64)}


@pytest.mark.parametrize("path", GOLDEN, ids=case_id)
def test_restatement_reproduces_the_reference_vectors(path):
    z, c, F, kw = flat_case(path)
    assert float(z["margin"]) >= 1e-5          # the maker's seed condition: exact indices, no exclusions
    assert all(np.isfinite(c[n]).all() for n in ("depth", "opacity", "d_logits"))
    depth, opacity, index, d_logits = ref.forward_backward(c["logits"], c["near"], c["far"], F, c["g_depth"],
                                                           c["g_opacity"], **kw)
    assert np.array_equal(index, c["index"])
    np.testing.assert_allclose(depth, c["depth"], rtol=2e-5)
    np.testing.assert_allclose(opacity, c["opacity"], rtol=2e-5)
    assert rel_err(d_logits, c["d_logits"]) <= 1e-4


def test_exponent_one_returns_the_sampled_pdf():
    z, c, F, kw = flat_case([p for p in GOLDEN if case_id(p) == "stochastic"][0])
    lg = torch.tensor(c["logits"], dtype=torch.float64)
    _, opacity, index = ref.forward(lg, torch.tensor(c["near"]).double(), torch.tensor(c["far"]).double(), F,
                                    uniforms=torch.tensor(c["uniforms"]))
    n = ref.distribution(lg, F)[2]
    assert torch.allclose(opacity, n.gather(-1, index), rtol=1e-12, atol=0)


def _declared():
    text = open(os.path.join(ROOT, "include", "lsr_depth_head.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lsr_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported():
    lib = _lib.load()
    names = _declared()
    assert names == ["lsr_depth_head_backward", "lsr_depth_head_forward"]
    assert all(hasattr(lib, n) and n in _lib.EXPORTS for n in names)
    # the ctypes mirror has the size the header's struct has: 6 int32, 2 float, 2 int64
    assert C.sizeof(_lib.DepthHeadDims) == 48


def _dims(**kw):
    base = dict(num_cameras=2, rays=10, buckets=32, surfaces=1, samples=3, flags=0, opacity_exponent=1.0,
                opacity_scale=1.0, row_stride=64, grad_row_stride=64)
    base.update(kw)
    return _lib.DepthHeadDims(**base)


def _call(lib, d, ptr):
    p = C.c_void_p(ptr) if ptr else None
    return (lib.lsr_depth_head_forward(C.byref(d), p, p, p, p, p, p, p, None),
            lib.lsr_depth_head_backward(C.byref(d), p, p, p, p, p, p, p, None))


EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5


@pytest.mark.parametrize("bad,code", [
    (dict(buckets=0), EINVAL), (dict(buckets=65, row_stride=130, grad_row_stride=130), EINVAL),
    (dict(samples=9), EINVAL), (dict(samples=0), EINVAL), (dict(row_stride=63), EINVAL), (dict(surfaces=0), EINVAL),
    (dict(num_cameras=0), EINVAL), (dict(rays=-1), EINVAL), (dict(flags=4), EINVAL),
    (dict(flags=1, buckets=2, samples=3, row_stride=4, grad_row_stride=4), EINVAL),      # top-3 of two buckets
    (dict(opacity_exponent=0.0), EINVAL), (dict(opacity_exponent=float("nan")), EINVAL),
    (dict(opacity_scale=float("inf")), EINVAL),
    (dict(buckets=64, surfaces=33, row_stride=4224, grad_row_stride=4224), EUNSUPPORTED),   # 4224 floats per row
])
def test_invalid_dims_are_rejected_before_any_device_call(bad, code):
    """The pointers are bogus host addresses (non-NULL): a launch would fault, the validation must come first."""
    lib = _lib.load()
    assert _call(lib, _dims(**bad), 0x1000) == (code, code)
    assert _call(lib, _dims(**bad), 0) == (code, code)


def test_backward_checks_its_own_stride():
    lib = _lib.load()
    fwd, bwd = _call(lib, _dims(grad_row_stride=63), 0)
    assert (fwd, bwd) == (ENULL, EINVAL)          # the forward ignores grad_row_stride


def test_null_pointers_are_rejected_before_any_device_call():
    lib = _lib.load()
    assert _call(lib, _dims(), 0) == (ENULL, ENULL)
    assert lib.lsr_depth_head_forward(None, None, None, None, None, None, None, None, None) == ENULL
    assert lib.lsr_depth_head_backward(None, None, None, None, None, None, None, None, None) == ENULL
    assert _call(lib, _dims(rays=0), 0) == (0, 0)          # nothing to do: LSR_OK, nothing launched
    # the 4096-float row itself is supported (NULL pointers are what is wrong with this call)
    assert _call(lib, _dims(buckets=64, surfaces=32, row_stride=4096, grad_row_stride=4096), 0) == (ENULL, ENULL)


def test_mirror_has_the_reference_s_parameters():
    from latentsplat_amd.depth_head import DepthPredictorMonocular
    for path in GOLDEN:
        z = np.load(path)
        S = z["logits"].shape[-1] // (2 * int(z["surfaces"]))
        m = DepthPredictorMonocular(z["features"].shape[-1], S, int(z["surfaces"]), bool(z["transmittance"]))
        assert sorted(m.state_dict().keys()) == list(z["state_dict_keys"])
        m.load_state_dict({"projection.1.weight": torch.tensor(z["weight"]), "projection.1.bias": torch.tensor(z["bias"])})
        # the projection is the reference's: ReLU, then the Linear (float32 matmul summation order aside)
        logits = m.projection(torch.tensor(z["features"])).detach().numpy()
        np.testing.assert_allclose(logits, z["logits"], rtol=1e-4, atol=1e-5)
    assert isinstance(m.to_pdf, torch.nn.Softmax) and isinstance(m.to_offset, torch.nn.Sigmoid)


def test_package_exports():
    import latentsplat_amd
    from latentsplat_amd import depth_head
    assert latentsplat_amd.DepthPredictorMonocular is depth_head.DepthPredictorMonocular
    assert latentsplat_amd.opacity_exponent is depth_head.opacity_exponent
    assert callable(depth_head.depth_head)


def test_opacity_exponent_follows_the_warm_up_rule():
    from latentsplat_amd.depth_head import opacity_exponent
    # x = initial + min(step / warm_up, 1) (final - initial); exponent = 2 ** x
    assert opacity_exponent(0.0, 0.01, 50_000, 0) == 1.0
    assert opacity_exponent(-2.0, 3.0, 1000, 500) == pytest.approx(2 ** 0.5, rel=1e-15)
    assert opacity_exponent(-2.0, 3.0, 1000, 1000) == 8.0
    assert opacity_exponent(-2.0, 3.0, 1000, 10 ** 9) == 8.0
    assert opacity_exponent(1.0, -1.0, 4, 1) == pytest.approx(2 ** 0.5, rel=1e-15)


def test_cpu_tensors_are_refused():
    from latentsplat_amd.depth_head import DepthPredictorMonocular, depth_head
    logits, near, far = torch.zeros(1, 4, 64), torch.ones(1), 2 * torch.ones(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_head(logits, near, far, num_surfaces=1, uniforms=torch.rand(1, 4, 1, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_head(logits, near, far, num_surfaces=1, num_samples=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_head(logits, near, far, num_surfaces=1, deterministic=True, num_samples=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DepthPredictorMonocular(8, 32, 1, False)(torch.zeros(1, 1, 4, 8), torch.ones(1, 1), 2 * torch.ones(1, 1), False, 3)


def test_near_far_that_require_grad_are_refused():
    from latentsplat_amd.depth_head import depth_head
    near = torch.ones(1, requires_grad=True)
    with pytest.raises(RuntimeError, match="constants"):
        depth_head(torch.zeros(1, 4, 64), near, 2 * torch.ones(1), num_surfaces=1, num_samples=3)


def test_encoder_size_exclusions_stay_under_the_cap():
    """The GPU test at encoder size leaves out the samples whose float64 gap to the nearest cumulative-sum
    edge is below 1e-6; for its seed that share is under the 5e-4 cap (expected 6.4e-5) on the restatement alone."""
    _, close = ref.encoder_case()
    assert close.shape == (2, 65536, 1, 3)
    assert close.mean() <= ref.ENCODER_MAX_SHARE
