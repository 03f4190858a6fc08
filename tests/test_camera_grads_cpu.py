"""Camera gradients, CPU tier: the C ABI additions (lsr_view_grad_workspace_bytes / lsr_backward_views) and the
differentiable camera-table path that carries dL/d(view record) back to extrinsics, intrinsics, near, far and background."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import Dims
from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.rasterizer import _straight_through, make_view_table
from latentsplat_amd.synthetic import make_scene
from tests import camera_grad_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dims(V, G):
    return Dims(num_views=V, num_gaussians=G, height=64, width=64, feat_channels=4, color_mode=1, sh_degree=2,
                sh_coeffs=9, cov_elems=6)


def test_new_symbols_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsr_rasterizer.h")).read()
    for name in ("lsr_view_grad_workspace_bytes", "lsr_backward_views"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", header)
    assert lib.lsr_abi_version() == 10


def test_view_grad_workspace_is_host_only_and_monotone():
    lib = _lib.load()
    size = lambda V, G: lib.lsr_view_grad_workspace_bytes(C.byref(_dims(V, G)))
    assert size(1, 0) > 0                      # the background term needs its second-level records even without Gaussians
    for V in (1, 2, 4, 16):
        prev = 0
        for G in (0, 1, 63, 64, 65, 1000, 300_000):
            s = size(V, G)
            assert s >= prev and s >= V * ((G + 63) // 64) * 32 * 4
            prev = s
    for G in (0, 1000, 300_000):
        assert all(size(V, G) <= size(V + 1, G) for V in (1, 2, 3, 8, 15))
    assert lib.lsr_view_grad_workspace_bytes(C.byref(_dims(0, 10))) == 0   # invalid dims


def test_backward_views_rejects_null_workspace():
    # every other argument present (non-null placeholders; the checks run before anything is dereferenced or launched):
    # only the missing view-gradient workspace makes the call fail
    lib = _lib.load()
    d = _dims(1, 10)
    fake = lambda k: C.c_void_p(4096 * k)
    inp = _lib.Inputs(fake(1), fake(2), fake(3), fake(4), fake(5), fake(6))
    fwd = _lib.Outputs(fake(7), fake(8), None, fake(9), None, None)
    gout = _lib.OutGrads(None, None, None, None)
    gin = _lib.InGrads(fake(10), fake(11), fake(12), fake(13), fake(14), None)
    rc = lib.lsr_backward_views(C.byref(d), C.byref(inp), fake(15), fake(16), fake(17), 0, fake(18), C.byref(fwd),
                                C.byref(gout), fake(19), C.byref(gin), fake(20), None, None)
    assert rc == -2   # LSR_ENULL


def _cameras(dtype=torch.float64, V=3):
    sc = make_scene(16, image_size=32, views=V)
    ext = sc.extrinsics.to(dtype).clone()
    ext[:, :3, 3] += torch.tensor([0.05, -0.02, 0.1], dtype=dtype)
    return ext, sc.intrinsics.to(dtype), sc.near.to(dtype) * 1.3, sc.far.to(dtype), torch.tensor([0.1, 0.2, 0.3], dtype=dtype)


def test_differentiable_table_gradcheck_float64():
    """The statement of the camera table whose gradient build_view_table carries (_scaled_cameras + make_view_table),
    in float64: autograd against finite differences for all five camera inputs, scale-invariant and not."""
    ext, intr, near, far, bg = _cameras()

    for si in (True, False):
        def table(e, k, n, f, b):
            cams, scale = cs._scaled_cameras(e, k, n, f, si)
            return make_view_table(cams.view_matrix, cams.full_projection, cams.campos, cams.tan_fov_x, cams.tan_fov_y,
                                   b, scale, dtype=torch.float64)

        args = tuple(t.clone().requires_grad_(True) for t in (ext, intr, near, far, bg))
        assert torch.autograd.gradcheck(table, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_straight_through_keeps_values_and_moves_gradient():
    values = torch.randn(4, 44)
    values[0, 0] = -0.0
    x = torch.randn(4, 44, requires_grad=True)
    carrier = 3.0 * x
    out = _straight_through(values, carrier)
    assert torch.equal(out, values) and torch.signbit(out[0, 0])
    g = torch.randn(4, 44)
    out.backward(g)
    assert torch.equal(x.grad, 3.0 * g)


def test_host_view_table_gradient_reaches_every_camera_input():
    ext, intr, near, far, bg = (t.float().requires_grad_(True) for t in _cameras())
    views = cs._view_table(ext, intr, near, far, bg, True)
    g = torch.randn(views.shape, generator=torch.Generator().manual_seed(0))
    (views * g).sum().backward()
    for t in (ext, intr, near, far, bg):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0


# what each A case of tests/camera_grad_cases.py is about: (parts of launch_preprocess_backward, nv of k_sh_bwd's view chunks)
VIEW_PARALLEL = {"A1": (4, [4]), "A2": (4, [4, 1]), "A2-contraction": (4, [4, 1]), "A2-depth": (4, [4, 1]), "A3": (4, [4, 3]),
                 "A4": (4, [4, 1]), "A4-depth": (4, [4, 1]), "A5": (4, [1] * 5), "A6": (4, [4] * 4)}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_cases_are_fragile_free_and_reach_their_structure(name):
    """The cases test_camera_grads_gpu.py compares with the float64 oracle: no fragile evaluation in any view (the seeds),
    and the kernel instance / reduction loop each is about, restated from the constants in the sources."""
    c = cases.case(name)
    fw = c.forwards()
    assert cases.fragile_counts(None, c.H, c.W, None, None, None, None, forwards=fw) == [0] * c.V
    if name in VIEW_PARALLEL:
        assert cases.view_parallel_shape(c) == VIEW_PARALLEL[name]
        return
    radii64, masks = cases.oracle64_forward(c)
    radii32 = torch.from_numpy(np.stack([f["radii"] for f in fw]))
    for radii in (radii64, radii32):
        cases.assert_reduction_structure(name, c, radii)
    if name == "B4":
        cases.assert_background_mask(masks[0])


def test_a6_needs_the_big_lds_instance():
    """sh.hip sh_backward: (64 * 75 + 64 * 117 + 4 * 64 * 17) * 4 bytes with 13 latent channels; 12 stay within 64 KB"""
    assert cases.sh_backward_lds_bytes(4, cases.A6_CHANNELS, 2) == 66560 > 65536
    assert cases.sh_backward_lds_bytes(4, cases.A6_CHANNELS - 1, 2) <= 65536
    c = cases.case("A6")
    assert c.kw["feature_sh"].shape[1:] == (cases.A6_CHANNELS, 9) and c.kw["sh_degree"] == 4 and c.V == 16
