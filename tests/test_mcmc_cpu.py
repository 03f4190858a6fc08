"""The MCMC strategy without a GPU: the references of tests/mcmc_ref.py are held to what they claim (the sampling rule to
its distribution, the closed form of D to the published loop, the relocation values to the paper's conservation
claims), and the host side of include/lsr_mcmc.h refuses what it documents before any GPU work."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from latentsplat_amd import _lib
from tests import mcmc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lsr_mcmc_workspace_bytes", "lsr_mcmc_classify", "lsr_mcmc_sample", "lsr_mcmc_apply", "lsr_mcmc_noise")


def test_sampling_reference_follows_its_distribution():
    """8 weights over three decades, 200 000 draws: every frequency within 5 binomial standard deviations of q / total."""
    w = np.array([1.0, 0.5, 0.2, 0.1, 0.03, 0.01, 0.003, 0.001], np.float32)
    m = 200_000
    u = np.random.default_rng(2024).random(m)
    idx, count, total = ref.sample(w, u)
    q = ref.quanta(w)
    assert total == int(q.sum()) and count.sum() == m and np.array_equal(np.bincount(idx, minlength=8), count)
    p = q.astype(np.float64) / total
    sd = np.sqrt(m * p * (1 - p))
    z = (count - m * p) / sd
    print("z scores:", np.round(z, 2))
    assert (np.abs(z) <= 5.0).all()


def test_sampling_reference_edges():
    rng = np.random.default_rng(1)
    w = rng.random(1000).astype(np.float32)
    w[rng.random(1000) < 0.3] = 0.0
    w[:4] = [np.nan, -1.0, 2.0 ** -31, 0.0]                     # NaN, negative and sub-quantum weights are never drawn
    u = np.concatenate([rng.random(5000), [0.0, 1.0 - 2.0 ** -53, np.nan, -0.5, 1.5]])
    idx, count, total = ref.sample(w, u)
    assert (ref.quanta(w)[idx] > 0).all() and not count[ref.quanta(w) == 0].any()
    first, last = np.nonzero(ref.quanta(w))[0][[0, -1]]
    assert idx[5000] == first and idx[5001] == last and idx[5002] == first and idx[5003] == first and idx[5004] == last
    # a weight above 1 counts as 1
    assert ref.quanta(np.array([7.0], np.float32))[0] == 1 << 30
    # total == 0: every draw is -1
    idx, count, total = ref.sample(np.zeros(10, np.float32), rng.random(7))
    assert total == 0 and (idx == -1).all() and not count.any()


def test_hockey_stick_form_equals_the_published_loop():
    op = np.concatenate([np.linspace(1e-6, 1 - 1e-6, 41), [0.005, 0.5, 0.9]])
    for N in range(1, 51):
        a, b = ref.D_double_loop(op, N), ref.D_hockey_stick(op, N)
        # the terms reach C(N, N/2) op^(N/2): the sums agree to that many ulps and no closer
        terms = max(math.comb(N, k + 1) for k in range(N))
        assert np.abs(a - b).max() <= 64 * np.finfo(np.float64).eps * max(1.0, terms), N


@pytest.mark.parametrize("N", [1, 2, 5, 20, 50])
def test_relocation_values_conserve_peak_and_integral(N):
    """N co-located copies at (o', s') composite to 1 - (1 - o' g(x))^N: the peak is the original opacity and the
    integral along a line is the original's o s sqrt(2 pi) (by quadrature, not by the series that defines D)."""
    o = np.array([0.01, 0.3, 0.9, 0.999])
    s = np.array([[0.5], [2.0], [0.01], [1.0]])
    op, sp = ref.new_values(o, s, N)
    assert np.allclose(-np.expm1(N * np.log1p(-op)), o, rtol=1e-13, atol=0)      # 1 - (1 - o')^N, without cancellation
    for i in range(len(o)):
        x = np.linspace(-14.0 * sp[i, 0], 14.0 * sp[i, 0], 40001)
        composite = 1.0 - (1.0 - op[i] * np.exp(-0.5 * (x / sp[i, 0]) ** 2)) ** N
        integral = composite.sum() * (x[1] - x[0])           # trapezoid of a function that vanishes at both ends
        assert abs(integral - o[i] * s[i, 0] * math.sqrt(2 * math.pi)) <= 1e-9 * integral, (N, o[i])


def test_relocation_reference_copies_unsampled_rows_and_clamps():
    rng = np.random.default_rng(0)
    x, s = rng.uniform(-5, 16, (64, 1)).astype(np.float32), rng.normal(size=(64, 3)).astype(np.float32)
    count = np.tile([0, 1, 49, 500], 16)
    got_o, got_s = ref.relocation_values(x, s, count)
    assert np.array_equal(got_o[count == 0], x[count == 0].astype(np.float64)) and np.array_equal(got_s[count == 0], s[count == 0].astype(np.float64))
    assert np.array_equal(ref.ratio([0, 1, 48, 49, 50, 500]), [1, 2, 49, 50, 50, 50])
    floor = math.log(0.005 / 0.995)
    assert (got_o[count > 0] >= floor - 1e-6).all() and (got_o[count > 0] < x[count > 0]).all()
    x[1] = -5.2                                              # sigmoid 0.0055 split in two: below the floor, clamped to it
    assert abs(ref.relocation_values(x, s, count)[0][1, 0] - floor) < 1e-6


def test_symbols_are_exported():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "lsr_mcmc.h")).read()
    for name in NAMES:
        assert name in header
    assert lib.lsr_abi_version() == 10


def test_host_side_refusals():
    lib = _lib.load()
    big = 1 << 28
    one = C.c_void_p(64)                                     # never dereferenced: every call below returns before any GPU work
    table = (_lib.McmcTable * 2)(_lib.McmcTable(64, 1, _lib.MCMC_OPACITY), _lib.McmcTable(64, 3, _lib.MCMC_SCALING))
    # n >= 2^28
    assert lib.lsr_mcmc_classify(big, one, 0.0, one, one, one, one, None) == -1
    assert lib.lsr_mcmc_sample(big, one, 1, one, one, one, one, one, None) == -1
    assert lib.lsr_mcmc_noise(big, one, one, one, one, one, 1.0, None) == -1
    assert lib.lsr_mcmc_apply(big - 5, 5, one, one, None, table, 2, 0.005, one, None) == -1
    # other bad arguments
    assert lib.lsr_mcmc_classify(10, one, float("nan"), one, one, one, one, None) == -1
    assert lib.lsr_mcmc_classify(10, one, 0.0, one, one, None, one, None) == -1          # dead without counts
    assert lib.lsr_mcmc_sample(-1, one, 1, one, one, one, one, one, None) == -1
    assert lib.lsr_mcmc_sample(0, one, 1, one, one, one, one, one, None) == -1
    assert lib.lsr_mcmc_noise(10, one, one, one, one, one, float("inf"), None) == -1
    assert lib.lsr_mcmc_apply(10, 1, one, one, None, table, 2, 1.0, one, None) == -1      # min_opacity
    assert lib.lsr_mcmc_apply(10, 1, one, one, None, table, 1, 0.005, one, None) == -1    # no SCALING table
    bad = (_lib.McmcTable * 2)(_lib.McmcTable(64, 2, _lib.MCMC_OPACITY), _lib.McmcTable(64, 3, _lib.MCMC_SCALING))
    assert lib.lsr_mcmc_apply(10, 1, one, one, None, bad, 2, 0.005, one, None) == -1
    # a NULL required pointer
    assert lib.lsr_mcmc_classify(10, None, 0.0, one, one, one, one, None) == -2
    assert lib.lsr_mcmc_classify(10, one, 0.0, one, one, one, None, None) == -2
    assert lib.lsr_mcmc_sample(10, one, 1, None, one, one, one, one, None) == -2
    assert lib.lsr_mcmc_sample(10, one, 1, one, one, one, one, None, None) == -2
    assert lib.lsr_mcmc_noise(10, one, one, one, one, None, 1.0, None) == -2
    assert lib.lsr_mcmc_apply(10, 1, None, one, None, table, 2, 0.005, one, None) == -2
    null = (_lib.McmcTable * 2)(_lib.McmcTable(None, 1, _lib.MCMC_OPACITY), _lib.McmcTable(64, 3, _lib.MCMC_SCALING))
    assert lib.lsr_mcmc_apply(10, 1, one, one, None, null, 2, 0.005, one, None) == -2
    # nothing to do
    assert lib.lsr_mcmc_noise(0, None, None, None, None, None, 1.0, None) == 0
    assert lib.lsr_mcmc_sample(0, None, 0, None, None, None, None, None, None) == 0
    assert lib.lsr_mcmc_workspace_bytes(0, 10) == 0 and lib.lsr_mcmc_workspace_bytes(1000, 50) >= 16 * 1000


def test_wrappers_refuse_cpu_tensors():
    import torch
    from latentsplat_amd import MCMCControl, GaussianScene, inject_noise, relocation_values, sample_by_weight
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        sample_by_weight(torch.ones(4), torch.rand(2, dtype=torch.float64))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        relocation_values(torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        inject_noise(torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3), torch.ones(4, 4), torch.zeros(4, 3), 1.0)
    scene = GaussianScene.from_tensors(torch.zeros(4, 3), torch.zeros(4, 1, 3), torch.zeros(4, 0, 3), torch.zeros(4, 1),
                                       torch.zeros(4, 3), torch.ones(4, 4))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        MCMCControl(scene, cap_max=100)


def test_dead_logit_is_the_rounded_double():
    from latentsplat_amd.mcmc import dead_logit
    assert dead_logit(0.005) == float(ref.dead_logit(0.005)) == float(np.float32(math.log(0.005 / 0.995)))
    assert dead_logit(0.0) == -math.inf


def test_fit_tool_lists_the_new_flags():
    tool = os.path.join(ROOT, "tools", "fit_ply.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--strategy", "adc", "mcmc", "--cap-max", "--noise-lr", "--opacity-reg", "--scale-reg"):
        assert flag in out, flag
    bad = subprocess.run([sys.executable, tool, "scene.ply", "--out", "x", "--strategy", "random"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--strategy" in bad.stderr
