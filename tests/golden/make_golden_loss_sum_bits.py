#!/usr/bin/env python
"""Record tests/golden/loss_sum_bits.npz: the outputs of the five fused image losses (photometric, normal consistency,
distortion, inverse depth, bilagrid total variation) on the seeded inputs of tests/loss_sum_cases.py, as raw uint32 bit
patterns, plus the `hipcc --version` string of the build that produced them (for assertion messages only).

Run it on an MI355X with the library built from the commit whose summation order is to be pinned, BEFORE changing the
kernels: the recorded bits are the expectation of tests/test_loss_sum_bits_gpu.py, so they must come from the library as
it was, never from the code under test.

usage: python tests/golden/make_golden_loss_sum_bits.py [output.npz]
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(path: str) -> None:
    from tests import loss_sum_cases as cases
    dev = torch.device("cuda:0")
    data = {}
    for name in cases.IMAGE_CASES:
        data.update({f"{name}/{k}": v for k, v in cases.image_outputs(name, dev).items()})
    data.update({f"bilagrid/{k}": v for k, v in cases.bilagrid_outputs(dev).items()})
    hollow = []
    for k, v in data.items():
        f = v.view(np.float32)
        print(f"{k}: {f.reshape(-1)[:4]}{' ...' if f.size > 4 else ''}")
        if not (np.isfinite(f).all() and (f != 0).any()):
            hollow.append(k)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    data["hipcc_version"] = np.array(subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip())
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {len(data) - 1} outputs")
    if hollow:
        raise SystemExit(f"not finite, or all zero (such a fixture pins nothing): {hollow}")


if __name__ == "__main__":
    if len(sys.argv) > 2:
        raise SystemExit(__doc__)
    main(sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "tests", "golden", "loss_sum_bits.npz"))
