"""Bilateral-grid appearance compensation without a GPU: the C ABI's exports and argument checks (every documented
LSR_EINVAL / LSR_ENULL / LSR_EUNSUPPORTED case returns its code before any GPU work), the kernel path of every case of the
GPU tests, the two references of tests/bilagrid_ref.py against each other, the module's surface and the fitting tool's flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import bilagrid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENULL, EUNSUPPORTED = 0, -1, -2, -5
NEW = ("lsr_bilagrid_slice_path", "lsr_bilagrid_slice_forward", "lsr_bilagrid_slice_backward", "lsr_bilagrid_tv_workspace_bytes",
       "lsr_bilagrid_tv_forward", "lsr_bilagrid_tv_backward")
P = C.c_void_p(0x1000)       # a non-NULL pointer that is never dereferenced: every call below returns before any GPU work


def _dims(**kw):
    base = dict(num_views=2, height=48, width=64, num_grids=3, grid_l=8, grid_y=16, grid_x=16, reserved0=0)
    base.update(kw)
    return _lib.BilagridDims(**base)


POINTERS = dict(slice_forward=4, slice_backward=6, tv_forward=3, tv_backward=3)      # pointers after dims, stream excluded
REQUIRED = dict(POINTERS, slice_backward=5)     # its last pointer, grad_grids, may be NULL: the grid gradient is not wanted
SLICE, TV = ("slice_forward", "slice_backward"), ("tv_forward", "tv_backward")


def _calls(d, which, holes=()):
    """The return codes of the entry points named in `which` for dims `d`, with pointer number `hole` of each call NULL
    ("dims": the dims themselves).  Every call made here must be one the library refuses: the pointers are fake, so the
    caller passes either dims that the entry point refuses or a hole among the pointers it takes."""
    lib = _lib.load()
    ref_d = None if "dims" in holes else C.byref(d)
    got = {}
    for name in which:
        fn = getattr(lib, "lsr_bilagrid_" + name)
        got[name] = fn(ref_d, *[None if i in holes else P for i in range(POINTERS[name])], None)
        assert got[name] in (EINVAL, ENULL, EUNSUPPORTED), (name, got[name])
    return got


def test_new_symbols_are_exported_and_listed():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsr_bilagrid.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS and name in header, name
    import latentsplat_amd
    for name in ("bilagrid_slice", "bilagrid_tv", "BilateralGrid"):
        assert latentsplat_amd._LAZY[name] == "bilagrid" and callable(getattr(latentsplat_amd, name))
    assert lib.lsr_abi_version() == 10 and "#define LSR_ABI_VERSION 10" in open(os.path.join(ROOT, "include", "lsr_rasterizer.h")).read()
    assert C.sizeof(_lib.BilagridDims) == 32
    assert "LSR_BILAGRID_MAX_XY 64" in header and "LSR_BILAGRID_MAX_L 16" in header
    assert (_lib.BILAGRID_MAX_XY, _lib.BILAGRID_MAX_L) == (64, 16)


@pytest.mark.parametrize("bad", [dict(num_grids=0), dict(grid_l=0), dict(grid_y=0), dict(grid_x=0), dict(grid_x=-3), dict(reserved0=1),
                                 dict(reserved0=1, grid_x=65)])
def test_invalid_grid_dims_are_refused_by_every_call(bad):
    assert set(_calls(_dims(**bad), SLICE + TV).values()) == {EINVAL}
    lib = _lib.load()
    assert lib.lsr_bilagrid_tv_workspace_bytes(C.byref(_dims(**bad))) == 0 and lib.lsr_bilagrid_slice_path(C.byref(_dims(**bad))) == EINVAL


@pytest.mark.parametrize("bad", [dict(num_views=0), dict(height=0), dict(width=0), dict(width=-1)])
def test_invalid_image_dims_are_refused_by_the_slice_calls(bad):
    """The tv calls do not read the image sizes: with these dims they pass the size checks, which a NULL grids shows."""
    assert set(_calls(_dims(**bad), SLICE).values()) == {EINVAL}
    assert _lib.load().lsr_bilagrid_slice_path(C.byref(_dims(**bad))) == EINVAL
    assert set(_calls(_dims(**bad), TV, holes=(0,)).values()) == {ENULL}


@pytest.mark.parametrize("big", [dict(grid_x=65), dict(grid_y=65), dict(grid_l=17),
                                 dict(num_grids=2731, grid_l=16, grid_y=64, grid_x=64)])       # N 12 L Y X = 2^31 + 262144
def test_unsupported_grids_are_refused_by_every_call(big):
    assert set(_calls(_dims(**big), SLICE + TV).values()) == {EUNSUPPORTED}
    lib = _lib.load()
    assert lib.lsr_bilagrid_tv_workspace_bytes(C.byref(_dims(**big))) == 0 and lib.lsr_bilagrid_slice_path(C.byref(_dims(**big))) == EUNSUPPORTED


def test_the_limits_themselves_are_supported():
    """Dims just inside the limits pass the size checks: the calls get as far as the NULL grids."""
    lib = _lib.load()
    edge = _dims(num_grids=2730, grid_l=16, grid_y=64, grid_x=64)      # N 12 L Y X = 2^31 - 524288
    assert set(_calls(edge, SLICE + TV, holes=(0,)).values()) == {ENULL}
    assert lib.lsr_bilagrid_tv_workspace_bytes(C.byref(edge)) >= 3 * 8 and lib.lsr_bilagrid_slice_path(C.byref(edge)) >= 0
    images = _dims(num_views=1, height=1 << 14, width=43690)           # V 3 H W = 2^31 - 32768
    assert set(_calls(images, SLICE, holes=(0,)).values()) == {ENULL} and lib.lsr_bilagrid_slice_path(C.byref(images)) >= 0


def test_unsupported_images_are_refused_by_the_slice_calls():
    lib = _lib.load()
    for d in (_dims(num_views=1, height=1 << 14, width=43691),         # V 3 H W = 2^31 + 16384
              _dims(num_views=1 << 30, height=1, width=1)):
        assert set(_calls(d, SLICE).values()) == {EUNSUPPORTED} and lib.lsr_bilagrid_slice_path(C.byref(d)) == EUNSUPPORTED


def test_null_pointers_are_refused_before_the_dims_are_read():
    for name, n in REQUIRED.items():
        for hole in range(n):
            assert _calls(_dims(), (name,), holes=(hole,))[name] == ENULL, (name, hole)
            # ahead of the dims' own faults
            assert _calls(_dims(grid_x=0), (name,), holes=(hole,))[name] == ENULL, (name, hole)
    assert set(_calls(_dims(), SLICE + TV, holes=("dims",)).values()) == {ENULL}
    lib = _lib.load()
    assert lib.lsr_bilagrid_slice_path(None) == ENULL and lib.lsr_bilagrid_tv_workspace_bytes(None) == 0


def test_tv_workspace_is_pure_and_its_alignment_is_checked():
    lib = _lib.load()
    d = _dims()
    n = lib.lsr_bilagrid_tv_workspace_bytes(C.byref(d))
    assert n == lib.lsr_bilagrid_tv_workspace_bytes(C.byref(d)) and n >= 3 * 8
    assert n == lib.lsr_bilagrid_tv_workspace_bytes(C.byref(_dims(num_views=0, height=-1, width=0)))     # not read
    assert lib.lsr_bilagrid_tv_workspace_bytes(C.byref(_dims(num_grids=200))) <= 1024 * 24 + 256          # bounded
    assert lib.lsr_bilagrid_tv_forward(C.byref(d), P, C.c_void_p(0x1004), P, None) == EINVAL


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_kernel_path_of_every_gpu_case(name):
    """The table of tests/bilagrid_ref.py names the path each case is there for; the library agrees."""
    (L, Y, X), (H, W), V, N, _, path = ref.CASES[name]
    d = _dims(num_views=V, height=H, width=W, num_grids=N, grid_l=L, grid_y=Y, grid_x=X)
    assert _lib.load().lsr_bilagrid_slice_path(C.byref(d)) == path
    assert {c[5] for c in ref.CASES.values()} == {32, 16, 0}


def test_published_shapes_stage_their_footprint():
    lib = _lib.load()
    for H, W, want in ((256, 256, 32), (1024, 1024, 32), (64, 64, 16)):
        assert lib.lsr_bilagrid_slice_path(C.byref(_dims(height=H, width=W))) == want
    assert lib.lsr_bilagrid_slice_path(C.byref(_dims(height=256, width=256, grid_l=16, grid_y=64, grid_x=64))) == 16
    assert lib.lsr_bilagrid_slice_path(C.byref(_dims(height=7, width=9, grid_l=1, grid_y=1, grid_x=1))) == 32


def _axis_bound(T, extent, size):
    """csrc/bilagrid.hip bg_axis_nodes restated: the most nodes a tile of edge T is taken to reach along one axis."""
    if size == 1:
        return 1
    span = (min(T, extent) - 1) * (size - 1) / extent
    return min(int(span + 1e-4) + 3, size)


def _axis_reached(T, extent, size):
    """The most nodes a tile of edge T does reach along one axis, by the kernel's own float32 arithmetic (bg_coord, bg_lower,
    bg_tile) over every tile of the axis."""
    f32 = np.float32
    u = np.minimum((np.arange(extent).astype(f32) + f32(0.5)) * f32(size - 1) / f32(extent), f32(size - 1))
    lower = np.minimum(u.astype(np.int64), max(size - 2, 0))
    assert u.dtype == f32 and (np.diff(lower) >= 0).all()
    first = np.arange(0, extent, T)
    last = np.minimum(first + T, extent) - 1
    return int((np.minimum(lower[last] + 1, size - 1) - lower[first] + 1).max())


def test_no_tile_reaches_more_nodes_than_its_lds_holds():
    """The LDS of the slice kernels is sized by a host-side bound per axis; a tile that reached more nodes than that would
    write past it.  Every extent up to 300 and some larger ones, every grid size, both tile edges: the float32 arithmetic of
    the kernels never reaches more nodes than the bound, and sometimes exactly as many."""
    rng = np.random.default_rng(0)
    extents = list(range(1, 301)) + [int(e) for e in rng.integers(301, 5000, 100)]
    tight = 0
    for size in range(1, 65):
        for extent in extents:
            for T in (32, 16):
                reached, bound = _axis_reached(T, extent, size), _axis_bound(T, extent, size)
                assert 1 <= reached <= bound, (T, extent, size, reached, bound)
                tight += reached == bound
    assert tight > 0


def test_the_restated_bound_is_the_librarys():
    """lsr_bilagrid_slice_path takes the largest tile whose bound is at most 640 nodes: the restatement above picks the same
    path for random dims, so it is the bound the library sizes its LDS by."""
    lib = _lib.load()
    rng = np.random.default_rng(1)
    seen = set()
    for _ in range(4000):
        H, W = (int(v) for v in rng.integers(1, 700, 2))
        L, Y, X = int(rng.integers(1, 17)), int(rng.integers(1, 65)), int(rng.integers(1, 65))
        want = next((T for T in (32, 16) if _axis_bound(T, W, X) * _axis_bound(T, H, Y) * L <= 640), 0)
        assert lib.lsr_bilagrid_slice_path(C.byref(_dims(height=H, width=W, grid_l=L, grid_y=Y, grid_x=X))) == want, (H, W, L, Y, X)
        seen.add(want)
    assert seen == {32, 16, 0}


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_restatement_equals_the_stock_composition_in_float64(name):
    c = ref.make_case(name)
    mine = ref.restate(c["grids"], c["image"], c["grid_idx"], c["grad_out"])
    theirs = ref.stock(c["grids"], c["image"], c["grid_idx"], c["grad_out"], torch.float64)
    for k in ("out", "grad_image", "grad_grids"):
        err = float((mine[k] - theirs[k]).abs().max())
        print(name, k, err)
        assert mine[k].shape == theirs[k].shape and err <= 1e-12, (name, k, err)
    tv_mine, tv_theirs = ref.restate_tv(c["grids"], 1.7), ref.stock_tv(c["grids"], 1.7, torch.float64)
    for k in ("tv", "grad"):
        assert float((tv_mine[k] - tv_theirs[k]).abs().max()) <= 1e-12, (name, k)
    (L, Y, X) = ref.CASES[name][0]
    if (L, Y, X) == (1, 1, 1):
        assert float(tv_mine["tv"]) == 0.0 and not tv_mine["grad"].any()
    # both luminance clamps occur wherever there are enough pixels for it
    if L > 1 and c["image"].shape[2] * c["image"].shape[3] >= 35:
        u = ref.luma_coordinate(c["image"], L)
        assert (u < 0).any() and (u > L - 1).any() and ((u > 0) & (u < L - 1)).any()


def test_views_without_a_grid_pass_through_the_references():
    c = ref.make_case("default_33x65")
    for res in (ref.restate(c["grids"], c["image"], c["grid_idx"], c["grad_out"]),
                ref.stock(c["grids"], c["image"], c["grid_idx"], c["grad_out"], torch.float32)):
        assert torch.equal(res["out"][1], c["image"][1].double()) and torch.equal(res["grad_image"][1], c["grad_out"][1].double())
        assert not res["grad_grids"][1].any() and res["grad_grids"][0].any() and res["grad_grids"][2].any()


def test_a_single_cell_is_the_affine():
    c = ref.make_case("affine_5x7")
    A = c["grids"].double().reshape(2, 3, 4)[c["grid_idx"].long()]
    want = torch.einsum("vrk,vkhw->vrhw", A[:, :, :3], c["image"].double()) + A[:, :, 3, None, None]
    assert float((ref.restate(c["grids"], c["image"], c["grid_idx"])["out"] - want).abs().max()) <= 1e-15


def test_module_surface():
    from latentsplat_amd import BilateralGrid
    m = BilateralGrid(5)
    assert list(m.state_dict()) == ["grids"] and m.grids.shape == (5, 12, 8, 16, 16) and m.grids.dtype == torch.float32
    m = BilateralGrid(3, grid_x=4, grid_y=2, grid_l=6)
    assert m.grids.shape == (3, 12, 6, 2, 4) and m.grids.requires_grad
    # identity in every cell: the references map an image to itself, and the total variation is 0
    eye = torch.eye(3, 4).reshape(12)
    assert torch.equal(m.grids.detach().permute(0, 2, 3, 4, 1).reshape(-1, 12), eye.expand(3 * 6 * 2 * 4, 12))
    image = torch.rand(2, 3, 9, 11) * 1.4 - 0.2
    out = ref.restate(m.grids.detach(), image, torch.tensor([2, 0], dtype=torch.int32))["out"]
    assert float((out - image.double()).abs().max()) <= 1e-15
    assert float(ref.restate_tv(m.grids.detach())["tv"]) == 0.0
    with pytest.raises(_lib.LsrError, match="1 x 1 x 1"):
        m.affine()
    one = BilateralGrid(4, 1, 1, 1)
    assert one.affine().shape == (4, 3, 4) and torch.equal(one.affine()[2].detach(), torch.eye(3, 4))
    for bad in (dict(num=0), dict(num=1, grid_x=65), dict(num=1, grid_y=0), dict(num=1, grid_l=17)):
        with pytest.raises(_lib.LsrError):
            BilateralGrid(**bad)


def test_refuses_cpu_tensors_and_other_shapes():
    from latentsplat_amd import BilateralGrid, bilagrid_slice, bilagrid_tv
    grids, image, idx = torch.zeros(2, 12, 2, 3, 4), torch.zeros(2, 3, 5, 6), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        bilagrid_slice(grids, image, idx)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        bilagrid_tv(grids)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        BilateralGrid(2, 1, 1, 1)(image, idx)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        BilateralGrid(2, 1, 1, 1).tv_loss()
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        bilagrid_tv(grids.double())


def test_fit_tool_lists_the_new_flags():
    tool = os.path.join(ROOT, "tools", "fit_ply.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--bilateral-grid", "--bilateral-grid-lr", "--tv-weight", "--target-jitter"):
        assert flag in out, flag
    bad = subprocess.run([sys.executable, tool, "scene.ply", "--out", "nowhere", "--bilateral-grid", "16", "16"], capture_output=True, text=True)
    assert bad.returncode == 2 and "expected 3 arguments" in bad.stderr
