"""The antialiased gradient cases (tests/antialias_grad_cases.py), what needs no GPU: every case is free of fragile
evaluations under the mode, reaches the instance it is about, and can tell a backward without rho's term from one with it —
the float64 oracle with the factor detached lies at least 10 bars from the oracle proper (tests/test_antialias_grads_gpu.py
holds the kernels to those bars)."""
import pytest
import torch

from tests import antialias_grad_cases as ag


@pytest.mark.parametrize("name", [n for n in ag.NAMES if not n.endswith("-contraction")])
def test_case_preconditions(name):
    """(The -contraction variants are the same scenes and the same oracle: the knob changes the kernels' rounding only.)"""
    c = ag.case(name)
    assert ag.preconditions(c) >= ag.SEPARATION
    want, stock, const = ag.references(name)
    assert set(want) == {"views", "means", "cov", "opac"} | {k for k, v in c.kw.items() if torch.is_tensor(v)}
    assert want["means"].shape == c.means.shape and want["cov"].shape == c.cov.shape and want["opac"].shape == c.opac.shape
    if c.mode is not None:      # near and far are blocks too
        assert bool((want["views"][:, 42:44].abs() > 0).all())


def test_cases_cover_the_twelve_instances_and_the_layouts():
    """parts 1, 2 and 4, each with the contraction off and on (with the camera launch next to the plain one: all twelve
    k_preprocess_bwd<PARTS, FMA, CAM, AA = true>), and per layout what the issue lists"""
    from tests import camera_grad_cases as cases
    seen = {(cases.view_parallel_shape(ag.case(n))[0], ag.case(n).contraction) for n in ag.INSTANCES}
    assert seen == {(p, f) for p in (1, 2, 4) for f in (False, True)}
    a2, a4, a5 = ag.case("A2"), ag.case("A4"), ag.case("A5")
    assert a2.cov.shape[-2:] == (3, 3) and "feature_sh" in a2.kw and a2.V == 5
    assert a4.scenes == 2 and a4.V == 10 and a4.means.dim() == 3
    assert a5.scenes == a5.V == 5 and a5.opac.shape[0] == 5
    assert ag.case("A2-contraction").contraction and ag.case("A2-depth").mode == ag.case("A4-depth").mode == "relative_disparity"
    assert float((ag.case("A2-depth").views[:, 41] != 0).all())
