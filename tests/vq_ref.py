"""float64 restatements of the vector quantisation (include/lsr_vq.h, latentsplat_amd/vq.py), the case generators of
tests/test_vq_cpu.py and tests/test_vq_gpu.py, and the bars with their derivations.

Notation: u = 2^-24 (the unit roundoff of float32), D the row width, C = max_j |c_j|.

GAP BAR (assignment).  The kernel picks the largest float32 score  s_j = x . c_j - |c_j|^2 / 2 ; a squared distance is
|x|^2 - 2 s_j.  A length-D float32 dot product (one rounding per fused step, D steps), the bias (D steps and one rounded
multiplication by a power of two, which is exact) seeding it: the computed score errs by at most
(D + 2) u (|x| |c_j| + |c_j|^2 / 2) <= (D + 2) u (|x| + C)^2 / 2.  Two scores are compared, so the chosen code's true score
is within (D + 2) u (|x| + C)^2 of the best one, and a distance gap is twice a score gap:
    |x - c_chosen|^2 - min_j |x - c_j|^2  <=  2 (D + 2) u (|x| + C)^2.
The bar is twice that: 4 (D + 2) u (|x| + C)^2.  Nothing is exempt; a near-tie passes because either code is within it.

DIST2 BAR.  Each float32 difference is rounded once (relative u), squaring doubles it (2 u), D non-negative terms are
added with one rounding each (at most D u more): (D + 3) u relative in all.  The bar is twice that:
|got - want| <= 2 (D + 3) u want.  An exact zero must be exact.

UPDATE BAR.  The sums are float64 (relative error about n 2^-53, nothing next to u), the quotient is rounded to float32
once: |got - want| <= u |want| <= u (sum w |x_d| / sum w).  The bar is 4 u (sum w |x_d| / sum w) per coordinate: room for a
compensated float32 scheme, none for naive float32 accumulation (whose error grows with the cluster).  The mass: 4 u
relative.

MONOTONICITY (a Lloyd iteration driven by hand, inertia I = sum_i w_i |x_i - c_idx(i)|^2 in float64).
  assignment half-step: every row moves to a code within its gap bar g_i of its nearest, and its nearest is no farther
  than the code it had: I_new <= I_old + sum_i w_i g_i.
  update half-step: with mu_j the exact weighted mean, sum_{i in j} w_i |x_i - c|^2 = sum_{i in j} w_i |x_i - mu_j|^2 +
  m_j |c - mu_j|^2, and the exact mean minimises the first term over c; the computed centroid is within the update bar
  b_jd of mu_j in every coordinate, so I_new <= I_old + sum_j m_j D (max_d b_jd)^2.  Codes of zero mass do not move.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
ROWS, CODES, KSTEP = 128, 64, 4         # the tile constants of csrc/vq.hip (LSR_VQ_ROWS, LSR_VQ_CODES, LSR_VQ_KSTEP)
BIG = (20_011, 4096, 72)

# (n, k, D): a chosen list, not the product.  n straddles a wave's 32 columns twice over (63 / 64 / 65) and the workgroup's
# ROWS (127 / 128 / 129); k the 16-code register groups (15 / 16 / 17), the CODES of a tile (63 / 64 / 65) and several tiles
# (257, 4096); D the KSTEP (3 / 4 / 5), odd widths whose rows are not 16-byte aligned, and the widths of a scene (45: the
# rest rows of degree 3, 7: the shape rows, 24, 72, 96: degrees 2 and 4 and the limit).
SHAPES = [
    (1, 1, 1), (1, 2, 3), (1, 15, 4), (63, 1, 1), (63, 16, 3), (64, 17, 4), (65, 17, 5), (64, 63, 7), (65, 64, 9), (63, 65, 24),
    (127, 1, 45), (127, 64, 48), (128, 65, 72), (129, 63, 96), (128, 257, 5), (129, 257, 45), (127, 4096, 7), (129, 4096, 48),
    (64, 257, 1), (65, 15, 96),
    (1000, 2, 1), (1000, 15, 3), (1000, 16, 4), (1000, 17, 5), (1000, 63, 7), (1000, 64, 9), (1000, 65, 24), (1000, 257, 45),
    (1000, 257, 48), (1000, 64, 72), (1000, 65, 96), (1000, 4096, 45),
    (20_011, 1, 7), (20_011, 2, 45), (20_011, 17, 96), (20_011, 64, 3), (20_011, 65, 4), (20_011, 257, 9), (20_011, 4096, 5),
    BIG,
]
NS = [1, 63, 64, 65, 127, 128, 129, 1000, 20_011]
KS = [1, 2, 15, 16, 17, 63, 64, 65, 257, 4096]
DS = [1, 3, 4, 5, 7, 9, 24, 45, 48, 72, 96]
NAMES = ("normal", "clusters", "offset")


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@functools.lru_cache(maxsize=None)
def case(name, n, k, d):
    """(x (n, d), codebook (k, d)) float32, seeded.  The arrays are shared: do not write to them.
    normal    unit Gaussians, both;
    clusters  codes 3 N(0, 1), rows a random code plus 0.1 N(0, 1);
    offset    both near 100 with spread 1: the scores cancel to a 10^-4 of their size, which the bar's (|x| + C)^2 allows;
    lattice   integers in [-8, 8]: every product and every sum of the kernel is exact in float32."""
    rng = _rng(NAMES.index(name) if name in NAMES else 7, n, k, d)
    if name == "normal":
        x, c = rng.standard_normal((n, d)), rng.standard_normal((k, d))
    elif name == "clusters":
        c = 3.0 * rng.standard_normal((k, d))
        x = c[rng.integers(0, k, n)] + 0.1 * rng.standard_normal((n, d))
    elif name == "offset":
        x, c = 100.0 + rng.standard_normal((n, d)), 100.0 + rng.standard_normal((k, d))
    elif name == "lattice":
        x, c = rng.integers(-8, 9, (n, d)), rng.integers(-8, 9, (k, d))
    else:
        raise KeyError(name)
    x, c = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)
    x.setflags(write=False); c.setflags(write=False)
    return x, c


def assign_ref(x, c, device=None, chunk=4096):
    """(idx (n,) int64: the LOWEST index among the nearest codes, dist2 (n,) float64: its squared distance), in float64:
    |x|^2 - 2 x . c + |c|^2 picks the code (its rounding, 1e-16 of the squares, is nothing next to the bars, and integers
    stay exact), the distance itself is summed from the differences.  Chunked over rows; on `device` when given."""
    dev = torch.device("cpu") if device is None else device
    X, Cb = torch.from_numpy(np.array(x)).to(dev).double(), torch.from_numpy(np.array(c)).to(dev).double()
    k = Cb.shape[0]
    c2 = (Cb * Cb).sum(1)
    codes = torch.arange(k, device=dev)
    idx, dist2 = [], []
    for a in range(0, X.shape[0], chunk):
        xb = X[a:a + chunk]
        d2 = (xb * xb).sum(1, keepdim=True) - 2.0 * (xb @ Cb.T) + c2[None, :]
        low = torch.where(d2 == d2.min(1, keepdim=True).values, codes[None, :], k).min(1).values
        idx.append(low)
        dist2.append(((xb - Cb[low]) ** 2).sum(1))
    if not idx:
        return np.zeros((0,), np.int64), np.zeros((0,), np.float64)
    return torch.cat(idx).cpu().numpy(), torch.cat(dist2).cpu().numpy()


def assign_direct(x, c, budget=1 << 23):
    """(nearest (n,) float64, lowest (n,) int64): the smallest sum over d of (x_d - c_d)^2 and the lowest index that
    attains it, accumulated coordinate by coordinate from the differences, in row chunks of `budget` distances.  The check
    of assign_ref: no expansion, no matrix product."""
    X, Cb = torch.from_numpy(np.array(x)).double(), torch.from_numpy(np.array(c)).double()
    (n, d), k = X.shape, Cb.shape[0]
    Ct, codes = Cb.T.contiguous(), torch.arange(k)
    nearest, lowest = [], []
    for a in range(0, n, max(1, budget // k)):
        xb = X[a:a + max(1, budget // k)]
        acc = torch.zeros((xb.shape[0], k), dtype=torch.float64)
        diff = torch.empty_like(acc)
        for e in range(d):
            torch.sub(xb[:, e:e + 1], Ct[e][None, :], out=diff)
            acc.addcmul_(diff, diff)
        m = acc.min(1).values
        nearest.append(m)
        lowest.append(torch.where(acc == m[:, None], codes[None, :], k).min(1).values)
    return torch.cat(nearest).numpy(), torch.cat(lowest).numpy()


def chosen_dist2(x, c, idx):
    """float64 squared distance of every row to the code idx names, from the differences."""
    diff = np.asarray(x, np.float64) - np.asarray(c, np.float64)[np.asarray(idx, np.int64)]
    return (diff * diff).sum(1)


def gap_bar(x, c):
    """Per row: 4 (D + 2) u (|x| + C)^2 (the module docstring)."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    C = np.sqrt((c * c).sum(1)).max()
    return 4.0 * (x.shape[1] + 2) * U * (np.sqrt((x * x).sum(1)) + C) ** 2


def dist2_within_bar(got, want, d):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) <= 2.0 * (d + 3) * U * want


def update_ref(x, idx, k, prev, weights=None):
    """(codebook (k, d) float64, mass (k,) float64, absmean (k, d) float64 = sum w |x_d| / sum w, 0 for an empty code), rows
    with idx outside [0, k) skipped; codes of zero mass hold prev."""
    x, idx = np.asarray(x, np.float64), np.asarray(idx, np.int64)
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, np.float64)
    ok = (idx >= 0) & (idx < k)
    x, idx, w = x[ok], idx[ok], w[ok]
    mass = np.bincount(idx, weights=w, minlength=k)
    d = x.shape[1]
    sums = np.stack([np.bincount(idx, weights=w * x[:, e], minlength=k) for e in range(d)], 1) if d else np.zeros((k, 0))
    absum = np.stack([np.bincount(idx, weights=w * np.abs(x[:, e]), minlength=k) for e in range(d)], 1) if d else np.zeros((k, 0))
    live = mass > 0
    safe = np.where(live, mass, 1.0)[:, None]
    code = np.where(live[:, None], sums / safe, np.asarray(prev, np.float64))
    return code, mass, np.where(live[:, None], absum / safe, 0.0)


def update_bar(absmean):
    return 4.0 * U * absmean


def inertia(x, c, idx, weights=None):
    d2 = chosen_dist2(x, c, idx)
    return float(d2.sum() if weights is None else (np.asarray(weights, np.float64) * d2).sum())


def assign_allowance(x, c, weights=None):
    g = gap_bar(x, c)
    return float(g.sum() if weights is None else (np.asarray(weights, np.float64) * g).sum())


def update_allowance(mass, absmean):
    return float((np.asarray(mass, np.float64) * absmean.shape[1] * update_bar(absmean).max(1) ** 2).sum())


def planted(k, n, d, seed=0):
    """k clusters of spread 1 whose centres are at least 100 apart (a lattice of pitch 100 along the first axes), n rows
    in all, every cluster at least one row: (x (n, d) float32, label (n,), one row index per cluster)."""
    rng = _rng(11, k, n, d, seed)
    label = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    label = label[rng.permutation(n)]
    centres = np.zeros((k, d))
    side = int(np.ceil(k ** (1.0 / min(d, 3))))
    for a in range(min(d, 3)):
        centres[:, a] = 100.0 * ((np.arange(k) // side ** a) % side)
    x = (centres[label] + np.clip(rng.standard_normal((n, d)), -3.0, 3.0) / np.sqrt(d)).astype(np.float32)
    first = np.array([int(np.nonzero(label == j)[0][0]) for j in range(k)])
    return x, label, first
