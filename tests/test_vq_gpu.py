"""The codebook compression on the MI355X (csrc/vq.hip, latentsplat_amd/vq.py) against the float64 restatements of
tests/vq_ref.py, whose docstring derives every bar used here (the large brute force runs on the card in chunks).

Assignment: for every row, |x - c_chosen|^2 - min_j |x - c_j|^2 <= 4 (D + 2) u (|x| + C)^2 in float64; nothing is
exempt.  On integer lattices the index must EQUAL the reference's lowest-index nearest code and dist2 the integer distance.
dist2: |got - want| <= 2 (D + 3) u want against the float64 distance to the code the kernel chose.
Update: every centroid coordinate within 4 u (sum w |x_d| / sum w) of float64, the mass within 4 u relative, empty codes
bit for bit the previous codebook, the same bits on every call.

Sizes (tests/vq_ref.py SHAPES): the kernel's tile constants are ROWS = 128 rows per workgroup, CODES = 64 codes per LDS
tile and KSTEP = 4 floats of a row per trip of the inner loop (rows are zero-padded to it); the list straddles each by
-1 / 0 / +1, and 20 011 x 4096 x 72 is 157 workgroups by 64 tiles by 18 trips.  The update's blocks are 256 sorted rows: 1000
rows are four, 20 011 rows with k = 1 are 79 blocks of one code (the chunked sum of block sums)."""
import functools

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import util
from tests import vq_ref as ref

pytestmark = pytest.mark.gpu

ROWS, CODES, KSTEP = 128, 64, 4
assert (ROWS, CODES, KSTEP) == (_lib.VQ_ROWS, _lib.VQ_CODES, _lib.VQ_KSTEP) == (ref.ROWS, ref.CODES, ref.KSTEP)
assert all(ROWS + o in ref.NS and CODES + o in ref.KS and KSTEP + o in ref.DS for o in (-1, 0, 1))
assert all(any(n == ROWS + o for n, _, _ in ref.SHAPES) and any(k == CODES + o for _, k, _ in ref.SHAPES)
           and any(d == KSTEP + o for _, _, d in ref.SHAPES) for o in (-1, 0, 1))
assert ref.BIG in ref.SHAPES and (1, 1, 1) in ref.SHAPES and (65, 17, 5) in ref.SHAPES and any(n < k for n, k, _ in ref.SHAPES)
DEV = "cuda:0"


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, dev=DEV):
    return torch.from_numpy(np.array(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _kernel(name, n, k, d):
    """(idx, dist2) of the kernel as numpy arrays, once per case."""
    from latentsplat_amd import vq_assign
    x, c = ref.case(name, n, k, d)
    idx, dist2 = vq_assign(_dev(x), _dev(c), want_dist=True)
    return idx.cpu().numpy(), dist2.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(name, n, k, d):
    x, c = ref.case(name, n, k, d)
    return ref.assign_ref(x, c, torch.device(DEV))


@pytest.mark.parametrize("n, k, d", ref.SHAPES)
@pytest.mark.parametrize("name", ref.NAMES)
def test_assignment(hip_device, name, n, k, d):
    x, c = ref.case(name, n, k, d)
    idx, dist2 = _kernel(name, n, k, d)
    _, best = _reference(name, n, k, d)
    assert idx.shape == (n,) and idx.dtype == np.int32 and dist2.shape == (n,) and dist2.dtype == np.float32
    assert (idx >= 0).all() and (idx < k).all()
    chosen = ref.chosen_dist2(x, c, idx)
    gap, bar = chosen - best, ref.gap_bar(x, c)
    rel = np.abs(dist2.astype(np.float64) - chosen) / np.maximum(chosen, 1e-300) / (2.0 * (d + 3) * ref.U)
    print(f"{name} {n}x{k}x{d}: worst gap / bar {float((gap / bar).max()):.4f}, worst dist2 error / bar {float(rel.max()):.3f}, "
          f"{int((gap > 0).sum())} rows off the float64 nearest")
    assert (gap <= bar).all()
    assert ref.dist2_within_bar(dist2, chosen, d).all()


@pytest.mark.parametrize("n, k, d", ref.SHAPES)
def test_lattice_is_exact(hip_device, n, k, d):
    """|v| <= 8 integers: every product and sum is exact in float32, so the index is the lowest-index nearest code (ties
    abound: 17^D lattice points for up to 4096 codes) and dist2 the integer distance."""
    idx, dist2 = _kernel("lattice", n, k, d)
    want_idx, want_d = _reference("lattice", n, k, d)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dist2.astype(np.float64), want_d)


@pytest.mark.parametrize("n, k, d", [(1000, 64, 9), (1000, 258, 45), (129, 4096, 48), (65, 2, 5)])
def test_repeated_codes_go_to_the_lowest_index(hip_device, n, k, d):
    from latentsplat_amd import vq_assign
    x, c = ref.case("normal", n, k // 2, d)
    both = np.concatenate([c, c])
    idx = vq_assign(_dev(x), _dev(both)).cpu().numpy()
    assert (idx < k // 2).all()
    assert np.array_equal(idx, vq_assign(_dev(x), _dev(c)).cpu().numpy())
    same = np.repeat(c[:1], k, 0)
    idx, dist2 = vq_assign(_dev(x), _dev(same), want_dist=True)
    assert not idx.any() and ref.dist2_within_bar(dist2.cpu().numpy(), ref.chosen_dist2(x, same, idx.cpu().numpy()), d).all()


@pytest.mark.parametrize("name, n, k, d", [("normal", 1000, 1000, 45), ("normal", 257, 257, 7), ("clusters", 4096, 4096, 96)])
def test_rows_equal_to_codes(hip_device, name, n, k, d):
    from latentsplat_amd import vq_assign
    _, c = ref.case(name, 1, k, d)
    rows = np.random.default_rng(k).permutation(k)[:n]
    idx, dist2 = vq_assign(_dev(c[rows]), _dev(c), want_dist=True)
    assert (dist2 == 0.0).all()
    assert np.array_equal(c[idx.cpu().numpy()], c[rows])


def test_non_finite_rows_stay_in_range(hip_device):
    from latentsplat_amd import vq_assign
    x, c = (np.array(a) for a in ref.case("normal", 1000, 257, 45))
    x[3, 7], x[64, 0], x[999, 44], x[500, :] = np.nan, np.inf, -np.inf, np.nan
    c[200, 3] = np.nan
    idx, dist2 = vq_assign(_dev(x), _dev(c), want_dist=True)
    idx = idx.cpu().numpy()
    assert (idx >= 0).all() and (idx < 257).all()
    clean = np.ones(1000, bool)
    clean[[3, 64, 999, 500]] = False
    c[200] = 1e6                                    # a code with a NaN never wins a finite row
    assert (idx[clean] != 200).all()
    want, _ = ref.assign_ref(x[clean], c, torch.device(DEV))
    assert (ref.chosen_dist2(x[clean], c, idx[clean]) - ref.chosen_dist2(x[clean], c, want) <= ref.gap_bar(x[clean], np.delete(c, 200, 0))).all()


# ---- update ----

def _update_case(n, k, d, seed=0):
    rng = np.random.default_rng([5, n, k, d, seed])
    x, c = ref.case("clusters", n, k, d)
    idx = rng.integers(0, k, n).astype(np.int32)
    w = rng.uniform(0.25, 4.0, n).astype(np.float32)
    return x, c, idx, w


def _check_update(got, mass, x, idx, k, prev, w, what):
    want, want_mass, absmean = ref.update_ref(x, idx, k, prev, w)
    got, mass = got.cpu().numpy(), mass.cpu().numpy()
    live = want_mass > 0
    err = np.abs(got.astype(np.float64) - want)
    bar = ref.update_bar(absmean)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))[live]
    merr = np.abs(mass.astype(np.float64) - want_mass)[live] / want_mass[live] / (4.0 * ref.U)
    print(f"{what}: worst centroid error / bar {float(ratio.max()) if ratio.size else 0.0:.4f}, worst mass error / bar "
          f"{float(merr.max()) if merr.size else 0.0:.4f}, {int(live.sum())} live codes of {k}")
    assert (err[live] <= bar[live]).all()
    assert (merr <= 1.0).all()
    assert np.array_equal(_bits(got[~live]), _bits(np.asarray(prev, np.float32)[~live])) and not mass[~live].any()


@pytest.mark.parametrize("n, k, d", ref.SHAPES)
def test_update(hip_device, n, k, d):
    from latentsplat_amd import vq_update
    x, c, idx, w = _update_case(n, k, d)
    got, mass = vq_update(_dev(x), _dev(idx), _dev(c), _dev(w))
    _check_update(got, mass, x, idx, k, c, w, f"weighted {n}x{k}x{d}")
    again = vq_update(_dev(x), _dev(idx), _dev(c), _dev(w))
    assert np.array_equal(_bits(got), _bits(again[0])) and np.array_equal(_bits(mass), _bits(again[1]))
    plain, pmass = vq_update(_dev(x), _dev(idx), _dev(c))
    _check_update(plain, pmass, x, idx, k, c, None, f"unweighted {n}x{k}x{d}")


def test_update_of_one_large_code(hip_device):
    """k = 1: 20 011 rows in one code, summed in 79 blocks and eight chunks of blocks; offset data, where naive float32
    accumulation is wrong in the fourth digit."""
    from latentsplat_amd import vq_update
    n, d = 20_011, 45
    x, _ = ref.case("offset", n, 1, d)
    idx = np.zeros(n, np.int32)
    prev = np.zeros((1, d), np.float32)
    got, mass = vq_update(_dev(x), _dev(idx), _dev(prev))
    _check_update(got, mass, x, idx, 1, prev, None, "k = 1")
    assert float(mass[0]) == n


def test_update_skips_and_keeps(hip_device):
    from latentsplat_amd import vq_update
    n, k, d = 5000, 257, 45
    x, c, idx, w = _update_case(n, k, d, seed=1)
    idx = np.where(idx % 5 == 0, 3, idx)                 # codes 0, 5, 10, ... are empty
    idx[::7], idx[1::7] = -1, k                          # skipped rows
    idx[2::7] = np.where(idx[2::7] == 3, 3, -(1 << 31))
    w[idx == 11] = 0.0                                   # a code whose rows all weigh nothing
    w[::3] = 0.0
    got, mass = vq_update(_dev(x), _dev(idx), _dev(c), _dev(w))
    _check_update(got, mass, x, idx, k, c, w, "skips, empty codes, zero weights")
    gm = mass.cpu().numpy()
    assert not gm[0::5][gm[0::5] != 0].size and gm[11] == 0.0 and np.array_equal(_bits(got[11]), _bits(c[11]))
    nothing = vq_update(_dev(x), _dev(np.full(n, -1, np.int32)), _dev(c))
    assert np.array_equal(_bits(nothing[0]), _bits(c)) and not nothing[1].any()


@pytest.mark.parametrize("n, k, d", [(20_011, 17, 96), (1000, 257, 45), (20_011, 1, 7)])
def test_update_of_permuted_rows(hip_device, n, k, d):
    from latentsplat_amd import vq_update
    x, c, idx, w = _update_case(n, k, d, seed=2)
    p = np.random.default_rng(n).permutation(n)
    got, mass = vq_update(_dev(x[p]), _dev(idx[p]), _dev(c), _dev(w[p]))
    _check_update(got, mass, x, idx, k, c, w, f"permuted {n}x{k}x{d}")


def test_wrappers_refuse_what_they_cannot_take(hip_device):
    from latentsplat_amd import kmeans, vq_assign, vq_update
    dev = hip_device
    x, c = torch.zeros((10, 4), device=dev), torch.zeros((3, 4), device=dev)
    idx = torch.zeros(10, dtype=torch.int32, device=dev)
    for call in (lambda: vq_assign(x, torch.zeros((3, 5), device=dev)), lambda: vq_assign(x.double(), c), lambda: vq_assign(torch.zeros((10, 97), device=dev), torch.zeros((3, 97), device=dev)),
                 lambda: vq_assign(x, torch.zeros((0, 4), device=dev)), lambda: vq_update(x, idx.long(), c), lambda: vq_update(x, idx[:9], c),
                 lambda: vq_update(x, idx, c, torch.zeros(9, device=dev)), lambda: kmeans(x, 0), lambda: kmeans(x, 3, init=torch.zeros((4, 4), device=dev))):
        with pytest.raises(_lib.LsrError):
            call()
    empty = torch.zeros((0, 4), device=dev)
    assert tuple(vq_assign(empty, c).shape) == (0,)
    code, mass = vq_update(empty, idx[:0], c + 1.0)
    assert torch.equal(code, c + 1.0) and not mass.any()
    wide = torch.randn((100, 8), device=dev, generator=torch.Generator(dev).manual_seed(0))
    assert torch.equal(vq_assign(wide[:, 1:6], wide[:17, 1:6]), vq_assign(wide[:, 1:6].contiguous(), wide[:17, 1:6].contiguous()))


# ---- kmeans ----

@pytest.mark.parametrize("k", [3, 64])
def test_planted_clusters(hip_device, k):
    from latentsplat_amd import kmeans
    n, d = 3000, 45
    x, label, first = ref.planted(k, n, d)
    code, idx = kmeans(_dev(x), k, iters=1, init=_dev(x[first]))
    idx = idx.cpu().numpy()
    assert np.array_equal(label[first][idx], label)      # code j started from a row of cluster label[first[j]]
    want, _, absmean = ref.update_ref(x, idx, k, x[first])
    assert (np.abs(code.cpu().numpy().astype(np.float64) - want) <= ref.update_bar(absmean)).all()


def test_lloyd_iterations_do_not_raise_the_inertia(hip_device):
    from latentsplat_amd import vq_assign, vq_update
    n, k, d = 5000, 64, 45
    x, _ = ref.case("clusters", n, k, d)
    w = np.random.default_rng(9).uniform(0.5, 2.0, n).astype(np.float32)
    X, W = _dev(x), _dev(w)
    code = X[:k].clone()
    idx = vq_assign(X, code)
    last = ref.inertia(x, code.cpu().numpy(), idx.cpu().numpy(), w)
    slack = lambda v: 1e-12 * abs(v)                     # the float64 evaluation itself
    for it in range(5):
        code, mass = vq_update(X, idx, code, W)
        c = code.cpu().numpy()
        _, _, absmean = ref.update_ref(x, idx.cpu().numpy(), k, c, w)
        now = ref.inertia(x, c, idx.cpu().numpy(), w)
        allowed = ref.update_allowance(mass.cpu().numpy(), absmean)
        print(f"iteration {it}: update {last:.6f} -> {now:.6f} (allowance {allowed:.3e})")
        assert now <= last + allowed + slack(last)
        last = now
        idx = vq_assign(X, code)
        now = ref.inertia(x, c, idx.cpu().numpy(), w)
        allowed = ref.assign_allowance(x, c, w)
        print(f"iteration {it}: assign {last:.6f} -> {now:.6f} (allowance {allowed:.3e})")
        assert now <= last + allowed + slack(last)
        last = now


def test_kmeans_is_reproducible(hip_device):
    from latentsplat_amd import kmeans, vq_assign
    x, _ = ref.case("clusters", 20_011, 257, 45)
    X = _dev(x)
    w = torch.rand(20_011, device=hip_device, generator=torch.Generator(hip_device).manual_seed(1)) + 0.5
    runs = [kmeans(X, 257, iters=4, weights=w, generator=torch.Generator().manual_seed(5)) for _ in range(2)]
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    assert tuple(runs[0][0].shape) == (257, 45) and runs[0][1].dtype == torch.int32
    assert torch.equal(runs[0][1], vq_assign(X, runs[0][0]))      # idx is the assignment against the codebook
    other = kmeans(X, 257, iters=4, weights=w, generator=torch.Generator().manual_seed(6))
    assert not np.array_equal(_bits(runs[0][0]), _bits(other[0]))
    few = kmeans(X[:100], 257, iters=2, generator=torch.Generator().manual_seed(5))      # n < k: the drawn rows wrap around
    assert tuple(few[0].shape) == (257, 45) and int(few[1].max()) < 257


# ---- scenes ----

N, W, VIEWS = 3000, 64, 2
UNIT_QUATS = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]] +
                      [[0.5, a, b, c] for a in (0.5, -0.5) for b in (0.5, -0.5) for c in (0.5, -0.5)], np.float32)


def _scene(degree, dev, n=N, views=VIEWS, size=W, seed=0, lossless=True):
    """A scene in front of `views` cameras.  lossless: f_rest rows drawn from 50 distinct rows and shape rows from 40 (unit
    quaternions whose norm is exactly 1 in float32, w >= 0, or w == 0 and the first non-zero component positive)."""
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.rasterizer import build_view_table
    sc = util.make_scene(n, image_size=size, views=views, color_sh_degree=0, feature_channels=None, seed=seed + 1)
    table = build_view_table(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                             torch.tensor([0.1, 0.2, 0.3], device=dev), scale_invariant=False).detach()
    rng = np.random.default_rng([21, degree, n, seed])
    K = (degree + 1) ** 2
    sigma = float(torch.sqrt(torch.diagonal(sc.covariances, dim1=1, dim2=2).mean()))
    rest_pool = (0.1 * rng.standard_normal((50, K - 1, 3))).astype(np.float32)
    shape_pool = np.concatenate([np.log(sigma * rng.uniform(0.5, 2.0, (40, 3))), UNIT_QUATS[rng.integers(0, len(UNIT_QUATS), 40)]], 1).astype(np.float32)
    if lossless:
        rest, shape = rest_pool[rng.integers(0, 50, n)], shape_pool[rng.integers(0, 40, n)]
    else:
        rest = (0.1 * rng.standard_normal((n, K - 1, 3))).astype(np.float32)
        shape = np.concatenate([np.log(sigma * rng.uniform(0.5, 2.0, (n, 3))), rng.standard_normal((n, 4))], 1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    scene = GaussianScene(sc.means.float().to(dev), t(rng.standard_normal((n, 1, 3))), t(rest), t(rng.standard_normal((n, 1))),
                          t(shape[:, :3]), t(shape[:, 3:]))
    pad = lambda pool, rows: t(np.concatenate([pool.reshape(len(pool), -1), 1.0 + 0.1 * rng.standard_normal((rows, pool.reshape(len(pool), -1).shape[1]))]))
    return scene, table, pad(rest_pool, 14), pad(shape_pool, 24)


PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.mark.parametrize("degree", [1, 3])
def test_lossless_scene(hip_device, degree):
    scene, views, rest_init, shape_init = _scene(degree, hip_device)
    q = scene.quantize(rest_codes=64, shape_codes=64, rest_init=rest_init, shape_init=shape_init)
    assert tuple(q.rest_codebook.shape) == (64, (degree + 1) ** 2 - 1, 3) and tuple(q.shape_codebook.shape) == (64, 7)
    assert q.rest_idx.dtype == q.shape_idx.dtype == torch.int32 and int(q.rest_idx.max()) < 50 and int(q.shape_idx.max()) < 40
    back = q.dequantize()
    assert back.max_sh_degree == degree and back.active_sh_degree == scene.active_sh_degree
    for name in PARAMS:
        assert np.array_equal(_bits(getattr(back, name)), _bits(getattr(scene, name))), name
    with torch.no_grad():
        a, b = scene.render(views, W, W), back.render(views, W, W)
    assert float(a[0].std()) > 0
    for i in (0, 2, 3, 4):
        assert torch.equal(a[i], b[i])
    full = 4 * sum(getattr(scene, name).numel() for name in PARAMS)
    assert q.nbytes < full and q.nbytes == 4 * (N * 7 + 64 * 7 + 64 * 3 * ((degree + 1) ** 2 - 1)) + 4 * N


def test_degree_zero_scene(hip_device, tmp_path):
    from latentsplat_amd import QuantizedScene, quantize_scene
    scene, views, _, shape_init = _scene(0, hip_device)
    q = quantize_scene(scene, rest_codes=64, shape_codes=64, shape_init=shape_init)
    assert q.rest_codebook is None and q.rest_idx is None and q.max_sh_degree == 0
    q.save(tmp_path / "q.npz")
    back = QuantizedScene.load(tmp_path / "q.npz", hip_device).dequantize()
    for name in PARAMS:
        assert np.array_equal(_bits(getattr(back, name)), _bits(getattr(scene, name))), name
    with torch.no_grad():
        assert torch.equal(scene.render(views, W, W)[0], back.render(views, W, W)[0])


def test_quantised_scene_round_trips_on_the_card(hip_device, tmp_path):
    from latentsplat_amd import QuantizedScene
    scene, _, _, _ = _scene(3, hip_device, lossless=False)
    q = scene.quantize(rest_codes=257, shape_codes=65, iters=3, generator=torch.Generator().manual_seed(2))
    q.save(tmp_path / "q.npz")
    with np.load(tmp_path / "q.npz") as z:
        assert z["rest_idx"].dtype == np.uint16 and z["shape_idx"].dtype == np.uint16
    back = QuantizedScene.load(tmp_path / "q.npz", hip_device)
    for name in ("xyz", "features_dc", "opacity", "rest_codebook", "rest_idx", "shape_codebook", "shape_idx"):
        a, b = getattr(q, name), getattr(back, name)
        assert a.device == b.device and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), name
    a, b = q.dequantize(), back.dequantize()
    for name in PARAMS:
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    # lossy, and still a scene: a mean of unit quaternions of one sign (no longer than 1, and not 0), every row one of the codes
    norms = a._rotation.detach().norm(dim=1)
    assert float(norms.min()) > 0.1 and float(norms.max()) <= 1.0 + 1e-6
    assert int(q.rest_idx.max()) < 257 and int(q.shape_idx.max()) < 65 and int(q.rest_idx.min()) >= 0


def test_negated_quaternions_quantise_alike(hip_device):
    scene, _, _, _ = _scene(1, hip_device, lossless=False)
    kw = dict(rest_codes=64, shape_codes=64, iters=3)
    q = scene.quantize(generator=torch.Generator().manual_seed(4), **kw)
    with torch.no_grad():
        scene._rotation[::3] *= -1.0
    flipped = scene.quantize(generator=torch.Generator().manual_seed(4), **kw)
    assert torch.equal(q.shape_idx, flipped.shape_idx) and torch.equal(q.rest_idx, flipped.rest_idx)
    assert np.array_equal(_bits(q.shape_codebook), _bits(flipped.shape_codebook))
    assert (q.shape_codebook[q.shape_idx.long().unique(), 3] >= -1e-6).all()


def test_contribution_weights(hip_device):
    """Against the forward-only route: a one-hot feature channel for each of 8 Gaussians; the sum of channel c's image is
    the sum over pixels of alpha T of its Gaussian.  The tolerance of tests/test_parity_gpu.py for feature images against
    gradients: 1e-4 of the tensor's scale."""
    from latentsplat_amd import contribution_weights
    scene, views, _, _ = _scene(1, hip_device, n=64, views=1, size=32, lossless=False)
    weights = contribution_weights(scene, views, 32, 32)
    assert tuple(weights.shape) == (64,) and weights.dtype == torch.float32 and not weights.requires_grad
    assert all(p.grad is None for p in scene.parameters())
    order = torch.argsort(weights, descending=True).cpu()
    chosen = torch.cat([order[:4], order[-4:]])
    onehot = torch.zeros((64, 8), device=hip_device)
    onehot[chosen.to(hip_device), torch.arange(8, device=hip_device)] = 1.0
    with torch.no_grad():
        feature = scene.render(views, 32, 32, features=onehot)[1]
    want = feature.sum(dim=(0, 2, 3)).cpu().numpy()
    got = weights.cpu().numpy()[chosen.numpy()]
    scale = float(weights.abs().max())
    print(f"contribution weights: scale {scale:.4f}, worst difference {float(np.abs(got - want).max()):.3e}")
    assert scale > 0 and (weights >= 0).all() and np.abs(got - want).max() <= 1e-4 * scale


def test_compress_tool(hip_device, tmp_path):
    import os
    import sys
    from latentsplat_amd import GaussianScene, QuantizedScene
    from tests import scene_params_ref as sref
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        import compress_ply
    finally:
        sys.path.pop(0)
    src, dst, dec = tmp_path / "point_cloud.ply", tmp_path / "scene.npz", tmp_path / "decoded.ply"
    sref.write_scene_file(src, 2000, W, VIEWS)
    args = [str(src), str(dst), "--rest-codes", "64", "--shape-codes", "65", "--iters", "2", "--seed", "3"]
    res = compress_ply.main(args + ["--decode", str(dec)])
    assert res["gaussians"] == 2000 and res["bytes_in"] == os.path.getsize(src) and res["bytes_out"] == os.path.getsize(dst)
    assert res["ratio"] > 1.0 and res["rest_codes"] == 64 and res["shape_codes"] == 65
    q = QuantizedScene.load(dst, hip_device)
    decoded, direct = GaussianScene.from_ply(dec, hip_device), q.dequantize()
    assert decoded.num_gaussians == 2000
    for name in PARAMS:
        assert np.array_equal(_bits(getattr(decoded, name)), _bits(getattr(direct, name))), name
    first = dst.read_bytes()
    compress_ply.main(args)
    assert dst.read_bytes() == first                      # the same seed, the same file
