"""References for adaptive density control (include/lsr_density.h), shared by tests/test_density_cpu.py and
tests/test_density_gpu.py.

  * :func:`literal_sequence`: the published trainer's ``densify_and_clone -> densify_and_split -> prune_points`` written
    literally in torch — boolean masks, ``cat``, ``repeat``, ``prune_points`` and the optimizer-state surgery
    (``cat_tensors_to_optimizer`` / ``_prune_optimizer``) — for any device and dtype.  Two points are pinned by the C ABI
    rather than by one published revision: ``max_radii2D`` travels with its row and new rows start at 0, and the
    children's offsets are the caller's standard normals for the parents whose children survive, in child-major order
    (the shape and order of the published draw restricted to those parents).  An id column travels through the same
    masks and ``cat``s, so the sequence also yields the row map.
  * :func:`direct_map` / :func:`direct_rows`: the map, the counts and every row constructed in float64 straight from the
    rules of the header, with no sequence at all.
  * :func:`accumulate_literal` / :func:`accumulate_direct`: the per-view statistics update.
  * :func:`make_inputs`: scenes and statistics with all five outcomes present and no decision within relative 1e-5 of
    its threshold, plus hand-made rows that sit exactly on a threshold where float32 is exact.
"""
from __future__ import annotations

import numpy as np
import torch

KIND_SHIFT = 28
PARAMS = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
THRESHOLDS = dict(grad_threshold=0.25, dense_extent=1.0, min_opacity=0.005, max_screen_size=20.0, world_limit=10.0)
GUARD = 1e-5
HAND_MADE = 4       # rows appended by make_inputs when n >= MIN_HAND_MADE
MIN_HAND_MADE = 8


def thresholds(size_pruning: bool) -> dict:
    t = dict(THRESHOLDS)
    if not size_pruning:
        t["max_screen_size"] = 0.0
    return t


def _draw(rng, m):
    avg = np.exp(rng.uniform(np.log(0.02), np.log(1.5), m))
    denom = rng.integers(1, 17, m).astype(np.float32)
    grad_accum = (avg * denom).astype(np.float32)
    smax = np.exp(rng.uniform(np.log(0.05), np.log(60.0), m))
    scaling = np.log(smax)[:, None] + np.log(rng.uniform(0.2, 1.0, (m, 3)))
    scaling[np.arange(m), rng.integers(0, 3, m)] = np.log(smax)
    opacity = rng.normal(0.0, 3.5, (m, 1))
    radii = rng.integers(0, 40, m)
    radii[radii >= 20] += 1                                  # never the threshold itself
    return dict(grad_accum=grad_accum, denom=denom, scaling=scaling.astype(np.float32), opacity=opacity.astype(np.float32),
                max_radii=radii.astype(np.float32))


def _near(x, t):
    return np.abs(x - t) <= GUARD * abs(t)


def near_a_threshold(inp) -> np.ndarray:
    """Rows one of whose decisions (for any N in 1..8) lies within relative GUARD of its threshold, in float64."""
    t = THRESHOLDS
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(inp["grad_accum"].astype(np.float64) / inp["denom"].astype(np.float64), nan=0.0)
    smax = np.exp(inp["scaling"].astype(np.float64)).max(1)
    o = 1.0 / (1.0 + np.exp(-inp["opacity"].astype(np.float64)[:, 0]))
    bad = _near(avg, t["grad_threshold"]) | _near(smax, t["dense_extent"]) | _near(smax, t["world_limit"])
    bad |= _near(o, t["min_opacity"]) | _near(inp["max_radii"].astype(np.float64), t["max_screen_size"])
    for N in range(1, 9):
        bad |= _near(smax / (0.8 * N), t["world_limit"])
    return bad


def make_inputs(n: int, seed: int = 0, sh_rest: int = 15) -> dict:
    """float32 numpy arrays: the six parameters, the three statistics.  The thresholds are THRESHOLDS."""
    rng = np.random.default_rng(seed)
    m = n - HAND_MADE if n >= MIN_HAND_MADE else n
    inp = _draw(rng, m)
    for _ in range(100):
        bad = near_a_threshold(inp)
        if not bad.any():
            break
        again = _draw(rng, int(bad.sum()))
        for k in inp:
            inp[k][bad] = again[k]
    assert not near_a_threshold(inp).any()
    if n >= MIN_HAND_MADE:
        low = np.full(3, -1.0, np.float32)
        hand = dict(
            #            avg == threshold: selected   smax == dense_extent: cloned   0 / 0: NaN -> not selected   radius == limit: kept
            grad_accum=np.array([0.5, 1.0, 0.0, 0.0], np.float32), denom=np.array([2.0, 2.0, 0.0, 1.0], np.float32),
            scaling=np.stack([low, np.array([0.0, -1.0, -1.0], np.float32), low, low]),
            opacity=np.full((4, 1), 2.0, np.float32), max_radii=np.array([0.0, 0.0, 0.0, 20.0], np.float32))
        inp = {k: np.concatenate([inp[k], hand[k]]) for k in inp}
    inp["xyz"] = rng.normal(0.0, 5.0, (n, 3)).astype(np.float32)
    inp["features_dc"] = rng.normal(0.0, 1.0, (n, 1, 3)).astype(np.float32)
    inp["features_rest"] = rng.normal(0.0, 0.2, (n, sh_rest, 3)).astype(np.float32)
    inp["rotation"] = (rng.normal(0.0, 1.0, (n, 4)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    return inp


def outcomes(map_: np.ndarray, n: int) -> dict:
    """How many Gaussians were kept / cloned / split / dropped altogether."""
    parent, kind = map_ & ((1 << KIND_SHIFT) - 1), map_ >> KIND_SHIFT
    seen = np.zeros(n, bool)
    seen[parent] = True
    return dict(kept=int((kind == 0).sum()), cloned=int((kind == 1).sum()), split=int((kind == 2).sum()),
                dropped=int((~seen).sum()))


# ---- straight from the rules, float64 ----

def direct_map(inp, thr, N):
    """(map uint32 [n_out], counts uint32 [4]) from the rules of include/lsr_density.h, evaluated in float64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(inp["grad_accum"].astype(np.float64).reshape(-1) / inp["denom"].astype(np.float64).reshape(-1), nan=0.0)
    smax = np.exp(inp["scaling"].astype(np.float64)).max(1) if len(avg) else np.zeros(0)
    o = 1.0 / (1.0 + np.exp(-inp["opacity"].astype(np.float64).reshape(-1)))
    big = thr["max_screen_size"] > 0
    selected = avg >= thr["grad_threshold"]
    clone, split = selected & (smax <= thr["dense_extent"]), selected & (smax > thr["dense_extent"])
    faint = o < thr["min_opacity"]
    radii = inp["max_radii"].astype(np.float64).reshape(-1)
    kept = ~split & ~faint & ~(big & ((radii > thr["max_screen_size"]) | (smax > thr["world_limit"])))
    clones = clone & ~faint & ~(big & (smax > thr["world_limit"]))
    children = split & ~faint & ~(big & (smax / (0.8 * N) > thr["world_limit"]))
    ik, ic, ip = (np.nonzero(m)[0].astype(np.uint32) for m in (kept, clones, children))
    parts = [ik, ic | np.uint32(1 << KIND_SHIFT)] + [ip | np.uint32((2 + c) << KIND_SHIFT) for c in range(N)]
    map_ = np.concatenate(parts).astype(np.uint32)
    return map_, np.array([len(ik), len(ic), len(ip), len(map_)], np.uint32)


def rotation_matrices(q):
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def direct_rows(inp, map_, counts, N, eps):
    """The six new parameter tables in float64: gathers, and for the children the header's formulas."""
    parent = (map_ & np.uint32((1 << KIND_SHIFT) - 1)).astype(np.int64)
    out = {k: inp[k].astype(np.float64)[parent] for k in PARAMS}
    first = int(counts[0] + counts[1])
    p = parent[first:]
    s = np.exp(inp["scaling"].astype(np.float64)[p])
    R = rotation_matrices(inp["rotation"].astype(np.float64)[p])
    out["xyz"][first:] += np.einsum("nij,nj->ni", R, s * np.asarray(eps, np.float64))
    out["scaling"][first:] = np.log(s / (0.8 * N))
    return out


# ---- the published sequence, literally ----

def _build_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r_, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r_ * z)
    R[:, 0, 2] = 2 * (x * z + r_ * y)
    R[:, 1, 0] = 2 * (x * y + r_ * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r_ * x)
    R[:, 2, 0] = 2 * (x * z - r_ * y)
    R[:, 2, 1] = 2 * (y * z + r_ * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class _Model:
    """The part of the published GaussianModel the sequence touches: tensors, statistics, Adam moments, the id column."""

    def __init__(self, tensors, stats, moments, dtype, device):
        cast = lambda a: torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype).clone()
        self.t = {k: cast(tensors[k]) for k in PARAMS}
        self.grad_accum, self.denom = cast(stats["grad_accum"]).reshape(-1, 1), cast(stats["denom"]).reshape(-1, 1)
        self.max_radii = cast(stats["max_radii"]).reshape(-1)
        self.moments = None if moments is None else {k: {m: cast(v) for m, v in moments[k].items()} for k in moments}
        self.ids = torch.arange(self.t["xyz"].shape[0], dtype=torch.int64, device=device)

    get_scaling = property(lambda self: torch.exp(self.t["scaling"]))
    get_opacity = property(lambda self: torch.sigmoid(self.t["opacity"]))

    def densification_postfix(self, new, new_ids):          # cat_tensors_to_optimizer and the rest of the postfix
        for k in PARAMS:
            if self.moments is not None and k in self.moments:
                for m in self.moments[k]:
                    self.moments[k][m] = torch.cat((self.moments[k][m], torch.zeros_like(new[k])), dim=0)
            self.t[k] = torch.cat((self.t[k], new[k]), dim=0)
        self.ids = torch.cat((self.ids, new_ids))
        self.max_radii = torch.cat((self.max_radii, torch.zeros(new_ids.shape[0], dtype=self.max_radii.dtype, device=self.ids.device)))

    def prune_points(self, mask):                           # _prune_optimizer and the rest of prune_points
        valid = ~mask
        for k in PARAMS:
            if self.moments is not None and k in self.moments:
                for m in self.moments[k]:
                    self.moments[k][m] = self.moments[k][m][valid]
            self.t[k] = self.t[k][valid]
        self.ids, self.max_radii = self.ids[valid], self.max_radii[valid]

    def densify_and_clone(self, grads, grad_threshold, dense_extent):
        selected = torch.where(torch.norm(grads, dim=-1) >= grad_threshold, True, False)
        selected = torch.logical_and(selected, torch.max(self.get_scaling, dim=1).values <= dense_extent)
        self.densification_postfix({k: self.t[k][selected] for k in PARAMS}, self.ids[selected] | (1 << KIND_SHIFT))

    def densify_and_split(self, grads, grad_threshold, dense_extent, N, samples_unit):
        n_init = self.t["xyz"].shape[0]
        padded = torch.zeros(n_init, dtype=grads.dtype, device=grads.device)
        padded[:grads.shape[0]] = grads.squeeze(-1)
        selected = torch.where(padded >= grad_threshold, True, False)
        selected = torch.logical_and(selected, torch.max(self.get_scaling, dim=1).values > dense_extent)
        stds = self.get_scaling[selected].repeat(N, 1)
        samples = stds * samples_unit(stds.shape[0])        # normal(mean=0, std=stds) from the caller's standard normals
        rots = _build_rotation(self.t["rotation"][selected]).repeat(N, 1, 1)
        new = {k: self.t[k][selected].repeat(N, *([1] * (self.t[k].dim() - 1))) for k in PARAMS}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.t["xyz"][selected].repeat(N, 1)
        new["scaling"] = torch.log(self.get_scaling[selected].repeat(N, 1) / (0.8 * N))
        kinds = torch.arange(N, device=self.ids.device).repeat_interleave(int(selected.sum())) + 2
        self.densification_postfix(new, self.ids[selected].repeat(N) | (kinds << KIND_SHIFT))
        count = N * int(selected.sum())
        self.prune_points(torch.cat((selected, torch.zeros(count, device=selected.device, dtype=torch.bool))))
        return count

    def densify_and_prune(self, thr, N, samples_unit):
        grads = self.grad_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, thr["grad_threshold"], thr["dense_extent"])
        count = self.densify_and_split(grads, thr["grad_threshold"], thr["dense_extent"], N, samples_unit)
        prune = (self.get_opacity < thr["min_opacity"]).squeeze(-1)
        if thr["max_screen_size"]:
            big_vs = self.max_radii > thr["max_screen_size"]
            big_ws = self.get_scaling.max(dim=1).values > thr["world_limit"]
            prune = torch.logical_or(torch.logical_or(prune, big_vs), big_ws)
        survivors = ~prune[prune.shape[0] - count:]          # of the children, child-major
        self.prune_points(prune)
        return survivors


def literal_sequence(inp, thr, N, eps=None, dtype=torch.float64, device="cpu", moments=None):
    """The published sequence on copies.  ``eps`` are the standard normals of the surviving children in their final
    order (``None``: zeros); a first pass finds which children survive (that does not depend on the draw), the second
    places ``eps`` at their positions of the full published draw.  Returns ``(tensors, moments, map uint32, max_radii)``."""
    stats = {k: inp[k] for k in ("grad_accum", "denom", "max_radii")}
    probe = _Model(inp, stats, None, dtype, device)
    survivors = probe.densify_and_prune(thr, N, lambda m: torch.zeros((m, 3), dtype=dtype, device=device))

    def samples_unit(m):
        full = torch.zeros((m, 3), dtype=dtype, device=device)
        if eps is not None and m:
            full[survivors] = torch.as_tensor(np.asarray(eps)).to(device=device, dtype=dtype)
        return full

    model = _Model(inp, stats, moments, dtype, device)
    model.densify_and_prune(thr, N, samples_unit)
    return model.t, model.moments, model.ids.cpu().numpy().astype(np.uint32), model.max_radii


# ---- the statistics ----

def accumulate_direct(grad, radii, grad_accum, denom, max_radii):
    """float64: the update of lsr_density_accumulate."""
    g = np.asarray(grad, np.float64)
    vis = np.asarray(radii) > 0
    norm = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2)
    acc = np.asarray(grad_accum, np.float64).reshape(-1) + np.where(vis, norm, 0.0).sum(0)
    den = np.asarray(denom, np.float64).reshape(-1) + vis.sum(0)
    mr = np.maximum(np.asarray(max_radii, np.float64).reshape(-1), np.where(vis, radii, 0).max(0, initial=0))
    return acc, den, mr


def accumulate_literal(grad, radii, grad_accum, denom, max_radii):
    """The published per-view update in float32 torch (CPU), view after view."""
    g, r = torch.as_tensor(np.asarray(grad, np.float32)), torch.as_tensor(np.asarray(radii))
    acc = torch.as_tensor(np.asarray(grad_accum, np.float32)).clone().reshape(-1, 1)
    den = torch.as_tensor(np.asarray(denom, np.float32)).clone().reshape(-1, 1)
    mr = torch.as_tensor(np.asarray(max_radii, np.float32)).clone().reshape(-1)
    for v in range(g.shape[0]):
        vis = r[v] > 0
        mr[vis] = torch.max(mr[vis], r[v][vis].to(torch.float32))
        acc[vis] += torch.norm(g[v][vis, :2], dim=-1, keepdim=True)
        den[vis] += 1
    return acc.numpy().reshape(-1), den.numpy().reshape(-1), mr.numpy()
