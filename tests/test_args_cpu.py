"""The argument helpers every wrapper shares (latentsplat_amd/_args.py): null pointers, the 16-byte quad rule and the
sentences of the float32 / int32 checks.  No GPU: the checks refuse before anything is launched."""
import ctypes as C

import pytest
import torch

from latentsplat_amd import _args
from latentsplat_amd._lib import LsrError


def test_ptr_is_null_for_nothing_and_the_address_otherwise():
    assert _args.ptr(None) is None                                    # (ctypes' own NULL)
    for t in (torch.empty(0), torch.zeros(5)[5:], torch.zeros(3, 0)):
        assert _args.ptr(t).value is None                             # (how ctypes reads address 0 back)
    holder = C.c_void_p * 3
    assert list(holder(_args.ptr(None), _args.ptr(torch.empty(0)), None)) == [None, None, None]
    t = torch.zeros(9)
    assert _args.ptr(t).value == t.data_ptr() != 0
    assert _args.ptr(t[2:]).value == t.data_ptr() + 8


def test_quad_keeps_aligned_tensors_and_clones_the_others():
    base = torch.arange(9, dtype=torch.float32)
    assert base.data_ptr() % 16 == 0
    aligned, off = base[4:8], base[1:5]
    assert _args.quad(aligned) is aligned
    q = _args.quad(off)
    assert q is not off and q.data_ptr() % 16 == 0 and torch.equal(q, off)


@pytest.mark.parametrize("check, good, other", [(_args.f32, torch.float32, torch.float64), (_args.i32, torch.int32, torch.int64)])
def test_typed_checks_name_the_caller_and_the_tensor(check, good, other):
    who = "the tested module"
    bad = {"a CPU tensor": torch.zeros(4, 3, dtype=good), "another dtype": torch.zeros(4, 3, dtype=other), "no tensor": [1, 2]}
    for t in bad.values():
        with pytest.raises(LsrError, match=rf"^{who} needs \w+32 ROCm tensors \(no CPU fallback\): rows is not one$"):
            check(who, "rows", t, (4, 3))
    # a tensor of the right kind that is not on a ROCm device is still refused first, whatever its shape
    with pytest.raises(LsrError, match="no CPU fallback"):
        check(who, "rows", torch.zeros(5, 3, dtype=good), (4, 3))


def test_typed_checks_report_shape_device_and_contiguity():
    """The later checks, on CPU tensors made to pass for device tensors (``is_cuda`` is all the first check reads)."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    t = torch.zeros(4, 3).as_subclass(OnDevice)
    assert _args.f32("w", "rows", t, (4, 3), t.device, contiguous=True) is t
    with pytest.raises(LsrError, match=r"^rows must have shape \(4, 2\), got \(4, 3\)$"):
        _args.f32("w", "rows", t, (4, 2))
    with pytest.raises(LsrError, match=r"^rows must be on meta$"):
        _args.f32("w", "rows", t, (4, 3), torch.device("meta"))
    with pytest.raises(LsrError, match=r"^rows is updated in place and must be contiguous \(it is not copied\)$"):
        _args.f32("w", "rows", t.t(), contiguous=True)
    assert _args.f32("w", "rows", t.t()).shape == (3, 4)             # (contiguity is asked for, not assumed)
    i = torch.zeros(4, dtype=torch.int32).as_subclass(OnDevice)
    with pytest.raises(LsrError, match=r"^idx must have shape \(5,\), got \(4,\)$"):
        _args.i32("w", "idx", i, (5,))
