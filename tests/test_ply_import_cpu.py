"""Host reader of 3DGS scene files (lsr_ply_read_header / lsr_ply_read_rows, include/lsr_ply.h) through ctypes:
layouts of well-formed headers, and one malformed file per documented rejection."""
import ctypes as C
import os

import numpy as np
import pytest

from latentsplat_amd import _lib
from latentsplat_amd._lib import PlyLayout
from tests import ply_import_ref as ref
from tests.test_ply_cpu import GOLDEN

EINVAL, EUNSUPPORTED = -1, -5


def _header(path):
    layout = PlyLayout()
    rc = _lib.load().lsr_ply_read_header(os.fsencode(str(path)), C.byref(layout))
    return rc, layout


def _rows(path, floats):
    buf = np.full(floats, np.float32(-77.0))
    rc = _lib.load().lsr_ply_read_rows(os.fsencode(str(path)), buf.ctypes.data_as(C.c_void_p), floats)
    return rc, buf


def _check_layout(layout, names, n):
    K = sum(1 for x in names if x.startswith("f_rest_")) // 3 + 1
    assert (layout.n, layout.stride, layout.sh_coeffs) == (n, len(names), K)
    at = names.index
    assert list(layout.xyz) == [at(k) for k in "xyz"]
    assert list(layout.f_dc) == [at(f"f_dc_{i}") for i in range(3)]
    assert layout.opacity == at("opacity")
    assert list(layout.scale) == [at(f"scale_{i}") for i in range(3)]
    assert list(layout.rot) == [at(f"rot_{i}") for i in range(4)]
    assert list(layout.f_rest)[:3 * (K - 1)] == [at(f"f_rest_{i}") for i in range(3 * (K - 1))]


@pytest.mark.parametrize("K", [1, 4, 9, 16, 25])
def test_standard_and_shuffled_headers(tmp_path, K):
    names = ref.standard_names(K)
    assert len(names) == {1: 17, 4: 26, 9: 41, 16: 62, 25: 89}[K]
    table = ref.make_table(5, names, seed=K)
    ref.write_ply(tmp_path / "std.ply", names, table)
    rc, layout = _header(tmp_path / "std.ply")
    assert rc == 0
    _check_layout(layout, names, 5)
    assert layout.data_offset == os.path.getsize(tmp_path / "std.ply") - table.nbytes
    rc, buf = _rows(tmp_path / "std.ply", table.size)
    assert rc == 0 and np.array_equal(buf.reshape(table.shape), table)

    mixed = ref.shuffled_names(K, extra=2, seed=100 + K)
    assert len(mixed) == len(names) - 3 + 2
    table = ref.make_table(7, mixed, seed=K)
    ref.write_ply(tmp_path / "mix.ply", mixed, table, comments=("written by a test", "element face 3", ""))
    with open(tmp_path / "mix.ply", "rb") as f:
        raw = f.read().replace(b"element vertex", b"obj_info property uchar x\nelement vertex")
    (tmp_path / "mix.ply").write_bytes(raw)
    rc, layout = _header(tmp_path / "mix.ply")
    assert rc == 0
    _check_layout(layout, mixed, 7)
    rc, buf = _rows(tmp_path / "mix.ply", table.size + 3)                 # (a larger buffer is fine)
    assert rc == 0 and np.array_equal(buf[:table.size].reshape(table.shape), table) and (buf[table.size:] == -77).all()


def test_own_export_layout_parses(tmp_path):
    z = np.load(GOLDEN)
    table = np.ascontiguousarray(z["vertices"], np.float32)
    path = tmp_path / "g.ply"
    assert _lib.load().lsr_ply_write_host(os.fsencode(str(path)), table.ctypes.data_as(C.c_void_p), table.shape[0]) == 0
    rc, layout = _header(path)
    assert rc == 0 and (layout.n, layout.stride, layout.sh_coeffs) == (table.shape[0], 17, 1)
    _check_layout(layout, list(z["names"]), table.shape[0])
    rc, buf = _rows(path, table.size)
    assert rc == 0 and np.array_equal(buf.view(np.uint32), table.reshape(-1).view(np.uint32))
    # an empty scene is a valid file
    assert _lib.load().lsr_ply_write_host(os.fsencode(str(tmp_path / "e.ply")), None, 0) == 0
    rc, layout = _header(tmp_path / "e.ply")
    assert rc == 0 and (layout.n, layout.stride) == (0, 17)
    assert _lib.load().lsr_ply_read_rows(os.fsencode(str(tmp_path / "e.ply")), None, 0) == 0


def _bad_file(tmp_path, case):
    """(path, documented return code) of one malformed file."""
    names = ref.standard_names(4)
    table = ref.make_table(3, names, seed=1)
    path = tmp_path / f"{case}.ply"
    kw, code, edit = {}, EINVAL, None
    if case == "ascii":
        kw, code = dict(fmt="ascii"), EUNSUPPORTED
    elif case == "big_endian":
        kw, code = dict(fmt="binary_big_endian"), EUNSUPPORTED
    elif case == "uchar":
        code, edit = EUNSUPPORTED, lambda h: h.replace(b"property float nx", b"property uchar nx")
    elif case == "list":
        code, edit = EUNSUPPORTED, lambda h: h.replace(b"property float nx", b"property list uchar int nx")
    elif case == "second_element":
        code, edit = EUNSUPPORTED, lambda h: h.replace(b"end_header", b"element face 0\nend_header")
    elif case == "f_rest_5":
        names = [n for n in names if not n.startswith("f_rest_") or int(n[7:]) < 5]
        table, code = ref.make_table(3, names, seed=1), EUNSUPPORTED
    elif case == "missing_opacity":
        names = [n for n in names if n != "opacity"]
        table = ref.make_table(3, names, seed=1)
    elif case == "duplicate_x":
        edit = lambda h: h.replace(b"property float nx", b"property float x")
    elif case == "no_end_header":
        edit = lambda h: h.replace(b"end_header\n", b"")
    elif case == "count_minus_1":
        kw = dict(count=-1)
    elif case == "count_2_62":
        kw = dict(count=2 ** 62)
    elif case == "overlong_line":
        edit = lambda h: h.replace(b"element vertex", b"comment " + b"a" * 300 + b"\nelement vertex")
    elif case == "malformed_line":
        edit = lambda h: h.replace(b"property float nx", b"property float")
    elif case != "truncated":
        raise AssertionError(case)
    ref.write_ply(path, names, table, **kw)
    raw = path.read_bytes()
    if edit:
        cut = raw.index(b"end_header\n") + len(b"end_header\n")
        edited = edit(raw[:cut])
        assert edited != raw[:cut]
        raw = edited + raw[cut:]
    if case == "truncated":
        raw = raw[:-1]
    path.write_bytes(raw)
    return path, code, table.size


@pytest.mark.parametrize("case", ["ascii", "big_endian", "uchar", "list", "second_element", "f_rest_5", "missing_opacity",
                                  "duplicate_x", "no_end_header", "count_minus_1", "count_2_62", "truncated",
                                  "overlong_line", "malformed_line"])
def test_malformed_files_are_rejected(tmp_path, case):
    path, code, floats = _bad_file(tmp_path, case)
    layout = PlyLayout()
    before = bytes(layout)
    rc = _lib.load().lsr_ply_read_header(os.fsencode(str(path)), C.byref(layout))
    assert rc == code and bytes(layout) == before                          # nothing written
    rc, buf = _rows(path, floats)
    assert rc == code and (buf == -77).all()


def test_host_buffer_one_float_short(tmp_path):
    names = ref.standard_names(1)
    table = ref.make_table(9, names, seed=2)
    ref.write_ply(tmp_path / "s.ply", names, table)
    assert _header(tmp_path / "s.ply")[0] == 0
    rc, buf = _rows(tmp_path / "s.ply", table.size - 1)
    assert rc == EINVAL and (buf == -77).all()
    lib = _lib.load()
    assert lib.lsr_ply_read_rows(os.fsencode(str(tmp_path / "s.ply")), None, table.size) == -2
    assert lib.lsr_ply_read_header(os.fsencode(str(tmp_path / "absent.ply")), C.byref(PlyLayout())) == EINVAL


def test_layout_from_names_matches_the_reader(tmp_path):
    from latentsplat_amd.ply_import import layout_from_names
    names = ref.shuffled_names(9, extra=3, seed=5)
    ref.write_ply(tmp_path / "m.ply", names, ref.make_table(4, names, seed=3))
    rc, layout = _header(tmp_path / "m.ply")
    mine = layout_from_names(names, 4)
    mine.data_offset = layout.data_offset
    assert rc == 0 and bytes(mine) == bytes(layout)
    for bad in (names + ["x"], [n for n in names if n != "rot_2"], [n for n in names if n != "f_rest_3"]):
        with pytest.raises(_lib.LsrError):
            layout_from_names(bad, 4)


def test_no_cpu_fallback(tmp_path):
    import torch
    import latentsplat_amd
    from latentsplat_amd.ply_import import load_ply, unpack_vertices
    assert latentsplat_amd.load_ply is load_ply and latentsplat_amd.Scene3DGS.__name__ == "Scene3DGS"
    names = ref.standard_names(1)
    ref.write_ply(tmp_path / "s.ply", names, ref.make_table(2, names, seed=0))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        load_ply(tmp_path / "s.ply", "cpu")
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        unpack_vertices(torch.zeros(2, 17), names)
