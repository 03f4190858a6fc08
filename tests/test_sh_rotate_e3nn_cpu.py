"""The e3nn-free SH rotation pinned to e3nn itself: the float64 helper every SH-rotation test compares against
(tests/sh_rotation_ref.py, built from the defining equation Y(R x) = D(R) Y(x)) must give what e3nn's Wigner-D route
(the reference's rotate_sh, src/misc/sh_utils.py:100-120) gives.

Two sources, both optional in the build image: tests/golden/e3nn_rotate_sh.npz (written by
`python tools/dump_fork_vectors.py --only e3nn_rotate_sh` on a machine where e3nn imports) and e3nn itself when it is
importable.  With neither, the test skips with a loud reason — the only test of the SH rotation that may.

Bound: 1e-6 on float64 data.  Generic rotations agree to ~1e-12; within 1e-6 of the gimbal lock of e3nn's Y-X-Y angles the
two outer angles are determined only to eps / sin(beta) ~ 1e-16 * 1e6, which the product D(alpha) D(beta) D(gamma) inherits."""
import os

import numpy as np
import pytest

from tests import sh_rotation_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e3nn_rotate_sh.npz")

try:
    import e3nn  # noqa: F401
    HAVE_E3NN = True
except ImportError:
    HAVE_E3NN = False

SKIP_REASON = ("NO e3nn VECTORS: tests/golden/e3nn_rotate_sh.npz is absent and e3nn does not import here, so the SH rotation "
               "is checked against its defining equation only (tests/test_sh_rotate_cpu.py), not against e3nn's own output.  "
               "Run `python tools/dump_fork_vectors.py --only e3nn_rotate_sh` on a machine with e3nn and commit the file.")


@pytest.mark.skipif(not (os.path.exists(GOLDEN) or HAVE_E3NN), reason=SKIP_REASON)
def test_helper_matches_e3nn():
    checked = 0
    if os.path.exists(GOLDEN):
        z = np.load(GOLDEN)
        for R, c, want in zip(z["rotations"], z["coefficients"], z["rotated"]):
            assert np.abs(ref.rotate(c, R) - want).max() <= 1e-6
            checked += 1
    if HAVE_E3NN:
        import torch
        from e3nn.o3 import matrix_to_angles, wigner_D
        Rs = np.concatenate([ref.random_rotations(32, np.random.default_rng(8)), ref.special_rotations()])
        angles = matrix_to_angles(torch.tensor(Rs))
        for degree in range(5):
            D = wigner_D(degree, *angles).to(torch.float64).numpy()
            for i, R in enumerate(Rs):
                assert np.abs(D[i] - ref.band_matrix(degree, R)[0]).max() <= 1e-6, (degree, i)
                checked += 1
    assert checked > 0
