"""Absolute view-space gradients (AbsGS), CPU tier: the preconditions of every case of tests/absgrad_ref.py — the float64
restatement is the oracle, magnitudes dominate, no fragile evaluation, the two mutants (|signed sum|, magnitude after the
lane's pixel pair) can be told — and the C ABI addition ``lsr_backward_absgrad``: exported, declared, ABI version unchanged, and
its argument checks answer before any GPU work (placeholder pointers, no device here)."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

from latentsplat_amd import _lib
from latentsplat_amd._lib import Dims
from tests import absgrad_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSR_EINVAL, LSR_ENULL, LSR_EUNSUPPORTED = -1, -2, -5


@pytest.mark.parametrize("name", A.NAMES)
def test_case_preconditions(name):
    away = A.preconditions(A.case(name))
    assert away >= A.SEPARATION


def test_one_pixel_case_preconditions():
    assert A.preconditions(A.case("onepix")) is None


def test_symbol_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsr_rasterizer.h")).read()
    assert "lsr_backward_absgrad" in _lib.EXPORTS and "lsr_backward_absgrad" in _lib.PROTOTYPES
    assert hasattr(lib, "lsr_backward_absgrad")
    assert re.search(r"\blsr_backward_absgrad\s*\(", header)
    assert lib.lsr_abi_version() == 10
    assert re.search(r"#define\s+LSR_ABI_VERSION\s+10\b", header)
    # lsr_in_grads is the struct it was: six pointers
    assert C.sizeof(_lib.InGrads) == 6 * C.sizeof(C.c_void_p)


def _dims(V=2, G=10, feat=0, color_mode=1, **kw):
    return Dims(num_views=V, num_gaussians=G, height=32, width=32, feat_channels=feat, color_mode=color_mode, sh_degree=0,
                sh_coeffs=1, cov_elems=6, **kw)


fake = lambda k: C.c_void_p(4096 * k)


def _call(d, abs_ptr=fake(21), grad_views=None, view_ws=None, geom=fake(15)):
    """Every pointer a placeholder: an answer other than the expected code would mean the library went on to launch."""
    lib = _lib.load()
    inp = _lib.Inputs(fake(1), fake(2), fake(3), fake(4), fake(5), fake(6))
    fwd = _lib.Outputs(fake(7), fake(8), None, fake(9), None, None)
    gout = _lib.OutGrads(None, None, None, None)
    gin = _lib.InGrads(fake(10), fake(11), fake(12), fake(13), fake(14), None)
    return lib.lsr_backward_absgrad(C.byref(d), C.byref(inp), geom, fake(16), fake(17), 0, fake(18), C.byref(fwd),
                                    C.byref(gout), fake(19), C.byref(gin), grad_views, view_ws, abs_ptr, None)


def test_null_arguments():
    assert _call(_dims(), abs_ptr=None) == LSR_ENULL                      # the output itself
    assert _call(_dims(), geom=None) == LSR_ENULL
    assert _call(_dims(), grad_views=fake(22), view_ws=None) == LSR_ENULL   # a camera gradient needs its workspace


def test_bad_dims():
    assert _call(_dims(V=0)) == LSR_EINVAL
    assert _call(_dims(G=-1)) == LSR_EINVAL
    assert _call(_dims(forward_flags=1 << 4)) == LSR_EINVAL               # the reserved flag bit


@pytest.mark.parametrize("feat,color_mode", [(2, 1), (5, 0), (6, 1), (32, 0)])
def test_more_than_four_channels_unsupported(feat, color_mode):
    """3 colour + 2 features, 5 features, ...: record slots 14 / 15 are taken (or the record is wider)"""
    assert _call(_dims(feat=feat, color_mode=color_mode)) == LSR_EUNSUPPORTED


def test_python_constant_matches_the_source():
    src = open(os.path.join(ROOT, "latentsplat_amd", "csrc", "lsr_internal.h")).read()
    assert int(re.search(r"constexpr int kAbsGradMaxChannels\s*=\s*(\d+)", src).group(1)) == _lib.ABSGRAD_MAX_CHANNELS == 4
