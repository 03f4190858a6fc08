"""Adaptive density control without a GPU: the C ABI's exports and argument checks (every documented LSR_EINVAL /
LSR_ENULL case returns its code before any GPU work, n == 0 returns LSR_OK), the two formulations of the reference
(tests/density_ref.py) against each other, and the fitting tool's flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import density_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENULL = 0, -1, -2
NEW = ("lsr_density_accumulate", "lsr_densify_workspace_bytes", "lsr_densify_plan", "lsr_densify_apply")
P = C.c_void_p(0x1000)       # a non-NULL pointer that is never dereferenced: every call below returns before any GPU work


def test_new_symbols_are_exported_and_listed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "lsr_density.h")).read()
    for name in NEW:
        assert name in header
    import latentsplat_amd
    for name in ("accumulate_density_stats", "plan_densify", "apply_densify", "DensityControl"):
        assert callable(getattr(latentsplat_amd, name))
    assert lib.lsr_abi_version() == 10


def test_header_constants_match_the_binding():
    header = open(os.path.join(ROOT, "include", "lsr_density.h")).read()
    for text in ("LSR_DENSIFY_MAX_SPLIT 8", "LSR_DENSIFY_MAX_TABLES 24", "LSR_DENSIFY_MAX_WIDTH 4096", "LSR_DENSIFY_KIND_SHIFT 28",
                 "LSR_DENSIFY_COPY = 0", "LSR_DENSIFY_ZERO_NEW = 1", "LSR_DENSIFY_XYZ = 2", "LSR_DENSIFY_SCALING = 3"):
        assert text in header, text
    assert (_lib.DENSIFY_MAX_SPLIT, _lib.DENSIFY_MAX_TABLES, _lib.DENSIFY_MAX_WIDTH, _lib.DENSIFY_KIND_SHIFT) == (8, 24, 4096, 28)
    assert (_lib.DENSIFY_COPY, _lib.DENSIFY_ZERO_NEW, _lib.DENSIFY_XYZ, _lib.DENSIFY_SCALING) == (0, 1, 2, 3)
    assert ref.KIND_SHIFT == _lib.DENSIFY_KIND_SHIFT and C.sizeof(_lib.DensifyParams) == 32 and C.sizeof(_lib.DensifyTable) == 24


def test_accumulate_argument_checks():
    lib = _lib.load()
    assert lib.lsr_density_accumulate(-1, 10, P, P, P, P, P, None) == EINVAL
    assert lib.lsr_density_accumulate(2, -1, P, P, P, P, P, None) == EINVAL
    for hole in range(5):
        args = [P] * 5
        args[hole] = None
        assert lib.lsr_density_accumulate(2, 10, *args, None) == ENULL
    assert lib.lsr_density_accumulate(2, 0, None, None, None, None, None, None) == OK
    assert lib.lsr_density_accumulate(0, 10, None, None, None, None, None, None) == OK


def _params(**kw):
    base = dict(grad_threshold=0.25, dense_extent=1.0, min_opacity=0.005, max_screen_size=0.0, world_limit=10.0, n_split=2,
                reserved0=0, reserved1=0)
    base.update(kw)
    return _lib.DensifyParams(**base)


def _plan(n=100, params=None, capacity=None, holes=(), pass_params=True):
    lib = _lib.load()
    p = params if params is not None else _params()
    ptrs = [None if i in holes else P for i in range(8)]     # opacity scaling grad_accum denom max_radii | map counts workspace
    most = max(2, p.n_split)
    return lib.lsr_densify_plan(n, *ptrs[:5], C.byref(p) if pass_params else None, ptrs[5],
                                n * most if capacity is None else capacity, ptrs[6], ptrs[7], None)


@pytest.mark.parametrize("bad", [dict(n_split=0), dict(n_split=9), dict(n_split=-1), dict(grad_threshold=float("inf")),
                                 dict(grad_threshold=float("nan")), dict(dense_extent=float("inf")), dict(min_opacity=float("nan")),
                                 dict(max_screen_size=float("inf")), dict(max_screen_size=20.0, world_limit=float("nan")),
                                 dict(reserved0=1), dict(reserved1=1)])
def test_plan_rejects_invalid_parameters(bad):
    assert _plan(params=_params(**bad)) == EINVAL


def test_plan_argument_checks():
    assert _plan(n=-1, capacity=0) == EINVAL
    # n * max(2, N) must stay below 2^28
    assert _plan(n=1 << 27) == EINVAL and _plan(n=(1 << 27) - 1, holes=(0,)) == ENULL
    assert _plan(n=(1 << 28) // 3 + 1, params=_params(n_split=3)) == EINVAL
    assert _plan(n=(1 << 28) // 3, params=_params(n_split=3), holes=(0,)) == ENULL      # 3 n = 2^28 - 1: passes the size check
    assert _plan(n=1 << 25, params=_params(n_split=8)) == EINVAL
    # capacity
    assert _plan(n=100, capacity=199) == EINVAL and _plan(n=100, params=_params(n_split=3), capacity=299) == EINVAL
    assert _plan(n=100, params=_params(n_split=1), capacity=199) == EINVAL               # max(2, N): a clone beside every original
    # a world limit that is not read may be anything
    assert _plan(n=100, params=_params(world_limit=float("nan")), holes=(0,)) == ENULL
    # NULL
    assert _plan(pass_params=False) == ENULL
    for hole in range(8):
        assert _plan(holes=(hole,)) == ENULL
    # n == 0: nothing to do, whatever the pointers
    assert _plan(n=0, holes=tuple(range(8))) == OK
    lib = _lib.load()
    assert lib.lsr_densify_workspace_bytes(0) == 0 and lib.lsr_densify_workspace_bytes(-5) == 0
    assert lib.lsr_densify_workspace_bytes(1000) >= 1000


def _apply(n=100, n_out=150, n_split=2, tables=((3, _lib.DENSIFY_COPY),), map_=P, counts=P, scaling=P, rotation=P, eps=P,
           eps_rows=10, null_tables=False, src=P, dst=P, num_tables=None):
    lib = _lib.load()
    desc = (_lib.DensifyTable * max(1, len(tables)))(*[_lib.DensifyTable(src, dst, w, r) for w, r in tables])
    return lib.lsr_densify_apply(n, n_out, map_, counts, n_split, None if null_tables else desc,
                                 len(tables) if num_tables is None else num_tables, scaling, rotation, eps, eps_rows, None)


def test_apply_argument_checks():
    L = _lib
    assert _apply(n=-1) == EINVAL and _apply(n_out=-1) == EINVAL and _apply(n_out=1 << 28) == EINVAL
    assert _apply(n=0, n_out=5) == EINVAL
    assert _apply(n_split=0) == EINVAL and _apply(n_split=9) == EINVAL
    assert _apply(num_tables=-1) == EINVAL and _apply(num_tables=25) == EINVAL
    assert _apply(eps_rows=-1) == EINVAL
    for table in ((0, L.DENSIFY_COPY), (4097, L.DENSIFY_COPY), (3, 4), (3, -1), (4, L.DENSIFY_XYZ), (1, L.DENSIFY_SCALING)):
        assert _apply(tables=(table,)) == EINVAL, table
    assert _apply(map_=None) == ENULL and _apply(counts=None) == ENULL and _apply(null_tables=True) == ENULL
    assert _apply(src=None) == ENULL and _apply(dst=None) == ENULL
    xyz, scal = ((3, L.DENSIFY_XYZ),), ((3, L.DENSIFY_SCALING),)
    assert _apply(tables=xyz, scaling=None) == ENULL and _apply(tables=xyz, rotation=None) == ENULL
    assert _apply(tables=xyz, eps=None) == ENULL and _apply(tables=scal, scaling=None) == ENULL
    # the extras are required only with the tables that read them
    assert _apply(n_out=0, scaling=None, rotation=None, eps=None) == OK
    assert _apply(n=0, n_out=0, map_=None, counts=None, src=None, dst=None) == OK
    assert _apply(tables=(), map_=None, counts=None) == OK


@pytest.mark.parametrize("size_pruning", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_the_two_formulations_agree(N, size_pruning):
    """The published sequence, written literally, keeps exactly the rows the header's rules name, in the pinned order."""
    thr = ref.thresholds(size_pruning)
    for n, seed in ((1, 1), (7, 2), (64, 3), (257, 4), (3000, 5)):
        inp = ref.make_inputs(n, seed, sh_rest=3)
        want_map, want_counts = ref.direct_map(inp, thr, N)
        rng = np.random.default_rng(seed)
        eps = rng.normal(size=(N * int(want_counts[2]), 3))
        moments = {k: dict(exp_avg=rng.normal(size=inp[k].shape), exp_avg_sq=rng.uniform(size=inp[k].shape)) for k in ref.PARAMS}
        tensors, new_moments, got_map, max_radii = ref.literal_sequence(inp, thr, N, eps, torch.float64, "cpu", moments)
        assert got_map.dtype == np.uint32 and np.array_equal(got_map, want_map), (n, N)
        assert int(want_counts[3]) == len(want_map) == int(want_counts[0] + want_counts[1] + N * want_counts[2])
        rows = ref.direct_rows(inp, want_map, want_counts, N, eps)
        parent, kind = want_map & ((1 << ref.KIND_SHIFT) - 1), want_map >> ref.KIND_SHIFT
        for k in ref.PARAMS:
            got = tensors[k].numpy()
            assert got.shape == rows[k].shape
            if k in ("xyz", "scaling"):
                assert np.array_equal(got[kind < 2], rows[k][kind < 2])
                assert np.allclose(got, rows[k], rtol=1e-12, atol=1e-12)
            else:
                assert np.array_equal(got, rows[k])
            for m in ("exp_avg", "exp_avg_sq"):
                want = np.where((kind == 0).reshape((-1,) + (1,) * (inp[k].ndim - 1)), moments[k][m][parent], 0.0)
                assert np.array_equal(new_moments[k][m].numpy(), want)
        assert np.array_equal(max_radii.numpy(), np.where(kind == 0, inp["max_radii"][parent], 0.0))
        if n >= 3000:
            seen = ref.outcomes(want_map, n)
            assert min(seen.values()) > 0, seen
            # pruned by opacity and pruned by size both occur
            o = 1 / (1 + np.exp(-inp["opacity"].astype(np.float64)[:, 0]))
            assert (o < thr["min_opacity"]).any()
            if size_pruning:
                assert len(want_map) < len(ref.direct_map(inp, ref.thresholds(False), N)[0])


def test_hand_made_rows_sit_on_their_thresholds():
    """The four rows make_inputs appends: avg == threshold is selected (>=) and cloned; smax == dense_extent is cloned, not
    split (<=); 0 / 0 is not selected; a radius equal to the limit is kept (>)."""
    n = 64
    inp = ref.make_inputs(n, 9)
    for N in (1, 2, 3):
        map_, _ = ref.direct_map(inp, ref.thresholds(True), N)
        entries = {g: sorted((map_[(map_ & ((1 << 28) - 1)) == g] >> 28).tolist()) for g in range(n - 4, n)}
        assert entries == {n - 4: [0, 1], n - 3: [0, 1], n - 2: [0], n - 1: [0]}


def test_accumulate_formulations_agree():
    rng = np.random.default_rng(0)
    V, n = 4, 300
    grad = rng.normal(size=(V, n, 3)).astype(np.float32)
    radii = rng.integers(-1, 30, (V, n)).astype(np.int32)
    start = [rng.uniform(size=n).astype(np.float32), rng.integers(0, 5, n).astype(np.float32), rng.integers(0, 20, n).astype(np.float32)]
    want, got = ref.accumulate_direct(grad, radii, *start), ref.accumulate_literal(grad, radii, *start)
    assert np.allclose(got[0], want[0], rtol=1e-5) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_fit_tool_lists_the_new_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fit_ply.py"), "--help"], capture_output=True, text=True,
                         check=True).stdout
    for flag in ("--drop", "--densify-interval", "--densify-from", "--densify-until", "--densify-grad-threshold", "--min-opacity",
                 "--opacity-reset-interval"):
        assert flag in out, flag


def test_refuses_cpu_tensors():
    from latentsplat_amd import DensityControl, accumulate_density_stats
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        accumulate_density_stats(torch.zeros(2, 4, 3), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(4), torch.zeros(4), torch.zeros(4))
    assert DensityControl.update.__doc__ and "(V, n, 3)" in DensityControl.update.__doc__
