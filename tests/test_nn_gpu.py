"""The exact cross-cloud nearest-neighbour query on the MI355X (lsr_nn_build / lsr_nn_query, csrc/nn.hip) against the
float32 brute force of tests/nn_ref.py, run on the card.

The bar: ``dist2`` equals the reference BIT FOR BIT and ``index`` is EQUAL, on every case, nothing exempt.  The reference
evaluates ``(dx*dx + dy*dy) + dz*dz`` in float32 with every operation a separate rounded array operation, which is what
the kernel computes (the unit is built with -ffp-contract=off), and takes the lowest index among the minima.

Sizes (queries m <- reference n): the constants are those of csrc/lsr_morton.h: 64 queries per wavefront, 128 sorted
points per chunk, 64 chunks per group, groups tested in blocks of 64.  (1, 1) is a one-point reference; 63 / 64 / 65
straddle a wavefront of queries and half a chunk of the reference; 127 / 128 / 129 a chunk; 1000 is eight chunks in one
group; 70 001 is 547 chunks in nine groups (more chunks than a ballot has lanes) and, as queries, 1094 waves with the last
one partial.  Only beyond 128 * 64 * 64 = 524 288 reference points is there a second block of groups: the 90^3 lattice
and the 600 001-point clustered reference walk it."""
import functools

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import knn_ref
from tests import nn_ref as ref

pytestmark = pytest.mark.gpu

QUERIES, CHUNK, GROUP = 64, 128, 64
BIG = 70_001
CASES = [(1, 1), (5, 2), (64, 63), (65, 64), (63, 65), (1000, 127), (129, 128), (128, 129), (257, 1000), (5000, BIG), (BIG, 1000)]
LATTICE_SIDE, SAMPLED = 90, 600_001
assert BIG > 4 * CHUNK * GROUP and BIG % CHUNK != 0 and BIG % QUERIES != 0
assert min(LATTICE_SIDE ** 3, SAMPLED) > CHUNK * GROUP * 64


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)


def _query(queries, reference, dev=None):
    """(dist2, index) of the kernel as numpy arrays."""
    from latentsplat_amd import nearest
    dev = dev or torch.device("cuda:0")
    d, i = nearest(_dev(queries, dev), _dev(reference, dev))
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (len(queries),)
    return d.cpu().numpy(), i.cpu().numpy()


def _same(got, want, what):
    """The bar: the distances bit for bit, the indices equal."""
    (d, i), (want_d, want_i) = got, want
    bad_d, bad_i = int((_bits(d) != _bits(want_d)).sum()), int((i != want_i).sum())
    print(f"{what}: {d.size} queries, {bad_d} distances differ in bits, {bad_i} indices differ")
    assert bad_d == 0 and bad_i == 0, what


@pytest.mark.parametrize("m, n", CASES)
@pytest.mark.parametrize("name", knn_ref.NAMES)
def test_against_the_brute_force(hip_device, name, m, n):
    got = _query(ref.cloud(name, m), ref.cloud(name, n), hip_device)
    assert (got[1] >= 0).all() and (got[1] < n).all()
    _same(got, ref.reference(name, m, n, hip_device), f"{name} {m} <- {n}")


@pytest.mark.parametrize("n", [1000, BIG])
@pytest.mark.parametrize("name", knn_ref.NAMES)
def test_self(hip_device, name, n):
    """The queries are a copy of the reference: every distance is an exact 0 and the index is the lowest among the
    coincident points (``dup`` and ``same`` make that non-trivial)."""
    cloud = ref.cloud(name, n)
    d, i = _query(cloud, cloud, hip_device)
    _, inverse = np.unique(cloud, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    lowest = np.full(inverse.max() + 1, n, np.int64)
    np.minimum.at(lowest, inverse, np.arange(n))
    assert not d.any() and np.array_equal(_bits(d), np.zeros(n, np.uint32))
    assert np.array_equal(i, lowest[inverse])
    if name in ("dup", "same"):
        assert (i != np.arange(n)).sum() >= n // 2


@pytest.mark.parametrize("m, n", [(5000, BIG), (BIG, 1000), (257, 129)])
def test_far_queries(hip_device, m, n):
    """Every query lies outside the reference's box (shifted by 10^3 on every axis): all of them clamp to one corner cell
    of the reference's grid and the seed is useless.  The answer may not depend on it."""
    reference = ref.cloud("normal", n)
    queries = ref.cloud("normal", m) + np.float32(1000.0)
    assert (queries.min(axis=0) > reference.max(axis=0)).all()
    _same(_query(queries, reference, hip_device), ref.nn_ref_torch(queries, reference, hip_device), f"far {m} <- {n}")


def test_far_queries_on_every_side(hip_device):
    """Shifts of +-10^3 along single axes and diagonals: queries clamped to different faces of the grid in one call."""
    reference = ref.cloud("clusters", BIG)
    queries = np.array(ref.cloud("normal", 4096))
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float32) * np.float32(1000.0)
    queries += shifts[np.arange(4096) % 27]
    _same(_query(queries, reference, hip_device), ref.nn_ref_torch(queries, reference, hip_device), "far on every side")


def test_sparse_halo_around_a_core(hip_device):
    """The ``outlier`` reference (one point at 10^6 coarsens the grid: the core falls into few cells) against a halo of
    queries thirty times as wide as the core, and a core-and-halo reference against core queries."""
    reference = ref.cloud("outlier", BIG)
    halo = ref.cloud("normal", 5000) * np.float32(30.0)
    _same(_query(halo, reference, hip_device), ref.nn_ref_torch(halo, reference, hip_device), "halo <- outlier")
    both = np.concatenate([ref.cloud("normal", 60_000) * np.float32(0.01), ref.cloud("normal", 10_001) * np.float32(100.0)])
    both = both[np.random.default_rng(5).permutation(len(both))]
    queries = np.concatenate([ref.cloud("normal", 3000), ref.cloud("outlier", 2001)])
    _same(_query(queries, both, hip_device), ref.nn_ref_torch(queries, both, hip_device), "normal + outlier <- core and halo")


def test_ties_at_lattice_cell_centres(hip_device):
    """Queries at the centres of the cells of an integer lattice: eight equidistant corners at dist2 == 0.75 exactly; the
    lowest-indexed corner must win, whatever order the chunks are visited in."""
    cloud = ref.lattice(12, 12)
    queries, want = ref.lattice_cell_centres(cloud, (0, 0, 0), 11)
    d, i = _query(queries, cloud, hip_device)
    assert (d == np.float32(0.75)).all() and np.array_equal(i, want)
    _same((d, i), ref.nn_ref_torch(queries, cloud, hip_device), "lattice ties")


def test_lattice_beyond_one_block_of_groups(hip_device):
    """729 000 shuffled lattice sites (more than 524 288: a second block of groups) against the 40^3 cell centres of a
    sub-block; the exact answer costs O(m) from a site -> index grid."""
    cloud = ref.lattice(LATTICE_SIDE, LATTICE_SIDE)
    queries, want = ref.lattice_cell_centres(cloud, (25, 30, 35), 40)
    d, i = _query(queries, cloud, hip_device)
    assert d.shape == (64_000,) and (d == np.float32(0.75)).all() and np.array_equal(i, want)


def test_sampled_queries_beyond_one_block_of_groups(hip_device):
    """A 600 001-point clustered reference against 4096 queries: half ``clusters`` of another size, half shifted
    ``normal``.  Brute force on the card in query chunks of 256."""
    reference = ref.cloud("clusters", SAMPLED)
    queries = np.concatenate([ref.cloud("clusters", 2048), ref.cloud("normal", 2048) + np.float32(1000.0)])
    queries = queries[np.random.default_rng(9).permutation(4096)]
    _same(_query(queries, reference, hip_device), ref.nn_ref_torch(queries, reference, hip_device, chunk=256), "600 001 clusters")


def _pair(index, q):
    return index._run(q, True, True)


@pytest.mark.parametrize("name, m, n", [("clusters", BIG, BIG), ("lattice", 1000, BIG), ("dup", 1000, 1000), ("normal", 5, 2)])
def test_two_calls_give_the_same_bits(hip_device, name, m, n):
    from latentsplat_amd import NearestIndex
    q, r = _dev(ref.cloud(name, m), hip_device), _dev(ref.cloud(name, n), hip_device)
    first, second = _pair(NearestIndex(r), q), _pair(NearestIndex(r), q)
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name, m, n", [("clusters", BIG, 1000), ("lattice", 1000, BIG), ("outlier", 257, 129)])
def test_each_output_alone(hip_device, name, m, n):
    from latentsplat_amd import NearestIndex
    index = NearestIndex(_dev(ref.cloud(name, n), hip_device))
    q = _dev(ref.cloud(name, m), hip_device)
    full = _pair(index, q)
    for k in range(2):
        want = [False] * 2
        want[k] = True
        alone = index._run(q, *want)
        assert [t is not None for t in alone] == want
        assert np.array_equal(_bits(alone[k]), _bits(full[k]))


def test_side_stream(hip_device):
    from latentsplat_amd import NearestIndex
    dev = hip_device
    q, r = _dev(ref.cloud("clusters", 5000), dev), _dev(ref.cloud("clusters", BIG), dev)
    index = NearestIndex(r)
    main = _pair(index, q)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        built_there = NearestIndex(r)
        other, third = _pair(index, q), _pair(built_there, q)
    side.synchronize()
    for a, b, c in zip(main, other, third):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


def test_non_contiguous_input(hip_device):
    from latentsplat_amd import nearest
    dev = hip_device
    wide_q, wide_r = torch.zeros((5000, 4), device=dev), torch.zeros((BIG, 5), device=dev)
    wide_q[:, 1:] = _dev(ref.cloud("clusters", 5000), dev)
    wide_r[:, :3] = _dev(ref.cloud("clusters", BIG), dev)
    q, r = wide_q[:, 1:], wide_r[:, :3]
    assert not q.is_contiguous() and not r.is_contiguous()
    got, want = nearest(q, r), nearest(q.contiguous(), r.contiguous())
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
    _same((got[0].cpu().numpy(), got[1].cpu().numpy()), ref.reference("clusters", 5000, BIG, dev), "non-contiguous")


def test_index_is_not_consumed(hip_device):
    """One index, two different query sets, then the first again; the reference tensor is gone by then."""
    from latentsplat_amd import NearestIndex
    dev = hip_device
    r = _dev(ref.cloud("clusters", BIG), dev)
    index = NearestIndex(r)
    assert index.num_points == BIG
    r.fill_(float("nan"))                                           # the index holds its own copy of the points
    del r
    first = _pair(index, _dev(ref.cloud("clusters", 5000), dev))
    second = _pair(index, _dev(ref.cloud("normal", 1000) * np.float32(3.0), dev))
    again = _pair(index, _dev(ref.cloud("clusters", 5000), dev))
    _same(tuple(t.cpu().numpy() for t in first), ref.reference("clusters", 5000, BIG, dev), "first query set")
    _same(tuple(t.cpu().numpy() for t in second),
          ref.nn_ref_torch(ref.cloud("normal", 1000) * np.float32(3.0), ref.cloud("clusters", BIG), dev), "second query set")
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))


def test_wrappers_refuse_what_they_cannot_take(hip_device):
    from latentsplat_amd import NearestIndex, nearest
    dev = hip_device
    good = _dev(ref.cloud("normal", 100), dev)
    for bad in (torch.zeros((10, 2), device=dev), torch.zeros((10, 3), device=dev, dtype=torch.float64),
                torch.zeros((10, 3), device=dev, dtype=torch.int32), torch.zeros((3,), device=dev), torch.zeros((10, 3))):
        with pytest.raises(_lib.LsrError):
            NearestIndex(bad)
        with pytest.raises(_lib.LsrError):
            nearest(bad, good)
    with pytest.raises(_lib.LsrError, match="empty"):
        NearestIndex(torch.zeros((0, 3), device=dev))
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        NearestIndex(good).query(good.cpu())                        # a query on another device
    d, i = nearest(torch.zeros((0, 3), device=dev), good)
    assert tuple(d.shape) == (0,) and tuple(i.shape) == (0,) and d.dtype == torch.float32 and i.dtype == torch.int32 and d.is_cuda
