"""The fused image losses give the bits they gave before their fixed-order sums moved into csrc/lsr_wave.h (``block_sum``)
and csrc/lsr_image_sum.h: every output of tests/golden/loss_sum_bits.npz, bit for bit, no tolerance.

The fixture was recorded by tests/golden/make_golden_loss_sum_bits.py on an MI355X from the library as it stood BEFORE that
change (the expectation is the earlier code's, not the code under test), on the seeded inputs of tests/loss_sum_cases.py,
whose docstring says which loops each shape reaches and why the planted pairs make a changed order visible in float32."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import loss_sum_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_sum_bits.npz")


@functools.lru_cache(maxsize=None)
def _golden() -> dict:
    with np.load(GOLDEN, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _compare(case: str, got: dict) -> None:
    golden = _golden()
    want = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "/")}
    assert want and sorted(got) == sorted(want), (sorted(got), sorted(want))
    recorded = f"(fixture recorded with: {str(golden['hipcc_version']).splitlines()[0]})"
    for k in sorted(want):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype == np.uint32 and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, (f"{case}/{k}: {bad.size} of {g.size} values differ, first at {bad[0]}: "
                               f"{g.reshape(-1)[bad[0]]:#010x} ({g.view(np.float32).reshape(-1)[bad[0]]!r}), recorded "
                               f"{w.reshape(-1)[bad[0]]:#010x} ({w.view(np.float32).reshape(-1)[bad[0]]!r}) {recorded}")


@pytest.mark.parametrize("case", sorted(cases.IMAGE_CASES))
def test_image_losses_keep_their_bits(case):
    _compare(case, cases.image_outputs(case, torch.device("cuda:0")))


def test_bilagrid_tv_keeps_its_bits():
    _compare("bilagrid", cases.bilagrid_outputs(torch.device("cuda:0")))
