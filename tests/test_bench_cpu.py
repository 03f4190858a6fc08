"""bench.py --dump-outputs: what the last timed step returned, as float32 .npy files, within the size budget."""
import os

import numpy as np
import torch

import bench


def _outputs():
    g = torch.Generator().manual_seed(0)
    return dict(color=None, feature=torch.rand(4, 4, 32, 32, generator=g), mask=torch.rand(4, 32, 32, generator=g),
                radii=torch.randint(0, 100, (4, 1000), dtype=torch.int32, generator=g))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_output_as_float32(tmp_path):
    named = _outputs()
    assert bench.dump_outputs(str(tmp_path), named) == ["feature", "mask", "radii"]      # None (no colour) writes nothing
    got = _load(tmp_path)
    assert set(got) == {"feature", "mask", "radii"}
    for k, a in got.items():
        assert a.dtype == np.float32 and np.array_equal(a, named[k].float().numpy()), k


def test_dump_over_budget_is_a_fixed_sample(tmp_path):
    named, budget = _outputs(), 20_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named, budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= budget
    assert all(np.array_equal(a[k], b[k]) for k in a)                                   # the same sample every run
    for k, x in a.items():
        assert np.isin(x, named[k].float().numpy().reshape(-1)).all(), k
