"""Antialiased gradients (``LSR_FWD_ANTIALIAS``) on the MI355X against autograd through the float64 oracle
(oracle/torch_oracle.py ``rasterize(antialiasing=True)``), for every ``k_preprocess_bwd<PARTS, FMA, CAM, AA = true>``
instance and every input layout: cases, seeds, bars and their CPU-only preconditions in tests/antialias_grad_cases.py.

One forward and backward per case with every input a leaf: the plain instances store dL/d(means, cov, opacities, payload),
the camera instances the partial records of dL/d(view record).  The printed ratios (-s) are quoted in DESIGN.md §2.21."""
import pytest
import torch

from tests import antialias_grad_cases as ag
from tests import camera_grad_cases as cases
from tests.test_camera_grads_gpu import _kernel_and_oracle_grads

pytestmark = pytest.mark.gpu


def _run(name):
    c = ag.case(name)
    refs = ag.references(name)
    ag.preconditions(c, refs, show=False)
    got, _, radii = _kernel_and_oracle_grads(c.views, c.H, c.W, c.means, c.cov, c.opac, c.kw, c.C, scenes=c.scenes,
                                             contraction=c.contraction, antialiasing=True, rho_dtypes=())
    ag.hold(c, got, refs)
    return c, got, refs, radii


@pytest.mark.parametrize("name", ag.INSTANCES)
def test_instances(hip_device, name):
    """V = 1, 3, 5 shared views of sub-pixel splats (median rho < 0.5), contraction off and on: parts = 1, 2, 4 x FMA x
    {plain, camera} = the twelve AA instances"""
    c, _, _, _ = _run(name)
    assert cases.view_parallel_shape(c)[0] == {"1": 1, "3": 2, "5": 4}[name[1]]


@pytest.mark.parametrize("name", ag.LAYOUTS)
def test_layouts(hip_device, name):
    """A1 (colour SH 2), A2 (colour SH 1 + latent SH 2, 3 x 3 covariances; with the contraction; with a depth mode), A4 (2 scenes
    x 5 views: blockIdx.y = 1; with a depth mode), A5 (per-view everything: the per-view stores) of tests/camera_grad_cases.py
    under the mode"""
    c, got, refs, _ = _run(name)
    assert cases.view_parallel_shape(c)[0] == 4
    if c.mode is not None:
        assert bool((refs[0]["views"][:, 42:44].abs() > 0).all())
    if c.cov.shape[-2:] == (3, 3):      # the nine-value store: the upper triangle carries the gradient, the lower is zero
        low = torch.tril(torch.ones(3, 3, dtype=torch.bool), -1)
        assert float(got["cov"][..., low].abs().max()) == 0.0 and float(refs[0]["cov"][..., low].abs().max()) == 0.0


def test_scale_slot(hip_device):
    """Scale slots 2 ... 1.25 over unscaled means, cameras off the origin: the scale block at its own bar in every view (hold),
    10 bars from the oracle without rho's term (preconditions)"""
    c, got, refs, _ = _run("scale")
    assert ("views", 0, "scale") in ag.separation_keys(c)


def test_either_side_of_the_floor(hip_device):
    """Needles a factor 2.5 below and above det0 / det = 0.000025: below, the kernel's rows of dL/dcov are those of the oracle
    WITHOUT rho's term within the tensor's bar; above, they are not (and at the bar against the oracle proper: hold)."""
    c, got, (want, stock, const), _ = _run("floor")
    below, above = ag.floor_rows()
    bar = ag.bars(c, want, stock)[("cov",)][0]
    reach = want["opac"][:, 0] != 0
    d = (got["cov"] - const["cov"]).abs().amax(-1)
    print(f"floor: dL/dcov rows against the oracle without rho's term: below {float(d[below].max()):.3e}, above "
          f"{float(d[above][reach[above]].min()):.3e} ... {float(d[above].max()):.3e}; bar {bar:.3e}")
    assert float(d[below].max()) <= bar
    assert bool((d[above][reach[above]] > ag.SEPARATION * bar).all())
    assert bool(torch.isfinite(got["means"]).all()) and float(got["opac"][below].abs().max()) > 0


def test_clamped_jacobians(hip_device):
    """util.make_edge_scene("outside"), V = 2 (parts = 2): the clamped t.x / t.z is a constant of rho as well"""
    c, _, _, _ = _run("clamped")
    assert cases.view_parallel_shape(c)[0] == 2

