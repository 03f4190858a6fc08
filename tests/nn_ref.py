"""Reference of the cross-cloud nearest-neighbour query (include/lsr_nn.h).

A brute force in FLOAT32 IN THE KERNEL'S OWN OPERATION ORDER: three rounded differences, three rounded squares and
``(dx*dx + dy*dy) + dz*dz``, each operation a separate rounded array operation (numpy never fuses two of them, eager
torch runs one kernel per operation), so the kernel's ``dist2`` has to equal it BIT FOR BIT and its ``index`` has to be
equal.  The index is the lowest among the minima, taken explicitly: no reliance on ``argmin``'s tie order.

:func:`nn_ref_numpy` runs on the host, :func:`nn_ref_torch` on any device (the large cases run it on the card),
:func:`nn_ref_f64` is the float64 difference form the float32 one is bounded against.  Clouds come from
``tests.knn_ref.cloud`` (seeded per ``(name, n)``: two sizes give independent samples)."""
import numpy as np
import torch

from tests import knn_ref

BOUND = 8.0 * 2.0 ** -24        # |float32 form - float64 form| <= BOUND * float64 form (derived in include/lsr_knn.h)


def cloud(name: str, n: int) -> np.ndarray:
    """``knn_ref.cloud``; below 4 points its ``dup`` takes an index modulo 0, which numpy answers with 0 and a warning."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return knn_ref.cloud(name, n)


def nn_ref_numpy(queries, reference, chunk: int = 256):
    """``(dist2 (m,) float32, index (m,) int64)``."""
    q, r = np.ascontiguousarray(queries, np.float32), np.ascontiguousarray(reference, np.float32)
    m, n = q.shape[0], r.shape[0]
    every = np.arange(n, dtype=np.int64)
    dist2, index = np.empty(m, np.float32), np.empty(m, np.int64)
    for lo in range(0, m, chunk):
        c = q[lo:lo + chunk]
        dx = c[:, None, 0] - r[None, :, 0]
        dy = c[:, None, 1] - r[None, :, 1]
        dz = c[:, None, 2] - r[None, :, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        d = xx + yy
        d = d + zz
        assert d.dtype == np.float32
        best = d.min(axis=1)
        dist2[lo:lo + chunk] = best
        index[lo:lo + chunk] = np.where(d == best[:, None], every[None, :], n).min(axis=1)      # the lowest index that has it
    return dist2, index


def nn_ref_torch(queries, reference, device="cpu", chunk: int = 256):
    """The same in eager torch on ``device``; numpy arrays in and out."""
    q = torch.from_numpy(np.array(queries, dtype=np.float32)).to(device)      # (a copy: the clouds are read-only)
    r = torch.from_numpy(np.array(reference, dtype=np.float32)).to(device)
    m, n = q.shape[0], r.shape[0]
    every = torch.arange(n, device=q.device)
    dist2 = torch.empty(m, dtype=torch.float32, device=q.device)
    index = torch.empty(m, dtype=torch.int64, device=q.device)
    for lo in range(0, m, chunk):
        c = q[lo:lo + chunk]
        dx = torch.sub(c[:, None, 0], r[None, :, 0])
        dy = torch.sub(c[:, None, 1], r[None, :, 1])
        dz = torch.sub(c[:, None, 2], r[None, :, 2])
        xx = torch.mul(dx, dx)
        yy = torch.mul(dy, dy)
        zz = torch.mul(dz, dz)
        d = torch.add(xx, yy)
        d = torch.add(d, zz)
        best = d.min(dim=1).values
        dist2[lo:lo + chunk] = best
        index[lo:lo + chunk] = torch.where(d == best[:, None], every[None, :], n).min(dim=1).values
    return dist2.cpu().numpy(), index.cpu().numpy()


def nn_ref_f64(queries, reference, chunk: int = 256):
    """``(dist2 (m,) float64, index (m,) int64)`` of the float64 difference form of the float32 coordinates."""
    q, r = np.asarray(queries, np.float32).astype(np.float64), np.asarray(reference, np.float32).astype(np.float64)
    m, n = q.shape[0], r.shape[0]
    every = np.arange(n, dtype=np.int64)
    dist2, index = np.empty(m, np.float64), np.empty(m, np.int64)
    for lo in range(0, m, chunk):
        d = ((q[lo:lo + chunk, None, :] - r[None, :, :]) ** 2).sum(-1)
        best = d.min(axis=1)
        dist2[lo:lo + chunk] = best
        index[lo:lo + chunk] = np.where(d == best[:, None], every[None, :], n).min(axis=1)
    return dist2, index


def pair_dist2_f32(queries, reference, index) -> np.ndarray:
    """The float32 squared distance, in the kernel's operation order, from query i to ``reference[index[i]]``."""
    q, r = np.asarray(queries, np.float32), np.asarray(reference, np.float32)[np.asarray(index, np.int64)]
    dx, dy, dz = q[:, 0] - r[:, 0], q[:, 1] - r[:, 1], q[:, 2] - r[:, 2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    d = xx + yy
    return d + zz


_CACHE = {}


def reference(name: str, m: int, n: int, device="cpu"):
    """``nn_ref_torch(cloud(name, m), cloud(name, n))``, once per case and shared (read-only)."""
    key = (name, m, n)
    if key not in _CACHE:
        out = nn_ref_torch(cloud(name, m), cloud(name, n), device, chunk=256 if n > 4096 else 8192)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def lattice(side: int, seed: int) -> np.ndarray:
    """The ``side^3`` sites of an integer lattice as float32, shuffled."""
    i = np.arange(side ** 3)
    sites = np.stack([i % side, (i // side) % side, i // side ** 2], 1)
    return sites[np.random.default_rng(seed).permutation(side ** 3)].astype(np.float32)


def lattice_cell_centres(points, lo, count: int):
    """Queries at the centres of the ``count^3`` cells whose low corner is ``lo + (0..count-1)^3`` of the full integer
    lattice ``points`` (any order), and their exact answer in O(m) from a site -> index grid: ``dist2 == 0.75`` and the
    lowest index among the eight corners.  Returns ``(queries (m, 3) float32, index (m,) int64)``."""
    p = np.asarray(points).astype(np.int64)
    n, side = p.shape[0], int(p.max()) + 1
    assert side ** 3 == n
    at = np.empty((side,) * 3, np.int64)
    at[p[:, 0], p[:, 1], p[:, 2]] = np.arange(n)
    g = np.arange(count)
    cx, cy, cz = (a.reshape(-1) for a in np.meshgrid(g + lo[0], g + lo[1], g + lo[2], indexing="ij"))
    assert max(cx.max(), cy.max(), cz.max()) + 1 < side
    corners = np.stack([at[cx + a, cy + b, cz + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], 1)
    queries = (np.stack([cx, cy, cz], 1) + 0.5).astype(np.float32)
    return queries, corners.min(axis=1)
