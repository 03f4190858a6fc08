"""References for the MCMC strategy (include/lsr_mcmc.h): float64 numpy restatements of the header's formulas, with exact
``math.comb`` binomials and the published double loop for D, and the float32 torch-CPU "stock composition" of the
published sequence (compute_relocation's float32 loop, build_scaling_rotation -> L L^T -> bmm for the noise)."""
import math

import numpy as np
import torch

WEIGHT_BITS = 30
MAX_RATIO = 50
OPACITY_MAX = 1.0 - 1.1920929e-7
MIN_OPACITY = 0.005


# ---- sampling ----

def quanta(weights) -> np.ndarray:
    """uint64 [n]: trunc(clamp(w, 0, 1) * 2^30), NaN -> 0, of the float32 weights."""
    w = np.asarray(weights, np.float32).astype(np.float64)
    w = np.where(np.isnan(w), 0.0, np.clip(w, 0.0, 1.0))
    return np.floor(w * float(1 << WEIGHT_BITS)).astype(np.uint64)


def sample(weights, uniforms):
    """(idx int32 [m], count uint32 [n], total): the header's inverse-CDF rule."""
    q = quanta(weights)
    n, u = q.shape[0], np.asarray(uniforms, np.float64)
    cum = np.cumsum(q, dtype=np.uint64)
    total = int(cum[-1]) if n else 0
    if total == 0:
        return np.full(u.shape[0], -1, np.int32), np.zeros(n, np.uint32), 0
    u = np.where(np.isnan(u), 0.0, np.clip(u, 0.0, 1.0 - 2.0 ** -53))
    t = np.minimum((u * np.float64(total)).astype(np.uint64), np.uint64(total - 1))
    idx = np.searchsorted(cum, t, side="right").astype(np.int32)       # the smallest g with cum[g] > t
    return idx, np.bincount(idx, minlength=n).astype(np.uint32), total


# ---- classification ----

def dead_logit(min_opacity: float) -> np.float32:
    return np.float32(math.log(min_opacity / (1.0 - min_opacity)))


def classify(opacity, threshold):
    """(weights float64 [n], dead indices, counts) with dead = logit <= threshold, compared as float32."""
    o = np.asarray(opacity, np.float32).reshape(-1)
    dead = o <= np.float32(threshold)
    with np.errstate(over="ignore"):
        w = np.where(dead, 0.0, 1.0 / (1.0 + np.exp(-o.astype(np.float64))))
    return w, np.nonzero(dead)[0].astype(np.int32), np.array([dead.sum(), (~dead).sum()], np.uint32)


# ---- relocation values ----

def D_double_loop(op, N: int):
    """The published loop: sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k op^(k+1) / sqrt(k+1), float64."""
    op = np.asarray(op, np.float64)
    total = np.zeros_like(op)
    for i in range(1, N + 1):
        for k in range(i):
            total = total + math.comb(i - 1, k) * ((-1.0) ** k / math.sqrt(k + 1)) * op ** (k + 1)
    return total


def D_hockey_stick(op, N: int):
    """sum_{k=0..N-1} C(N, k+1) (-1)^k op^(k+1) / sqrt(k+1), float64."""
    op = np.asarray(op, np.float64)
    total = np.zeros_like(op)
    for k in range(N):
        total = total + math.comb(N, k + 1) * ((-1.0) ** k / math.sqrt(k + 1)) * op ** (k + 1)
    return total


def ratio(count):
    return np.minimum(np.asarray(count, np.int64) + 1, MAX_RATIO)


def new_values(o, scale, N: int):
    """(o', scale') in the activated domain for N copies, float64: o' = 1 - (1 - o)^(1/N), scale' = o / D scale."""
    o = np.asarray(o, np.float64)
    op = -np.expm1(np.log1p(-o) / N)
    return op, (o / D_double_loop(op, N))[..., None] * np.asarray(scale, np.float64)


def relocation_values(opacity, scaling, count, min_opacity=MIN_OPACITY):
    """float64 (logit', log-scale') for every row; rows with count 0 are the inputs."""
    x = np.asarray(opacity, np.float64).reshape(-1)
    s = np.asarray(scaling, np.float64)
    N = ratio(count)
    out_o, out_s = x.copy(), s.copy()
    for n_copies in np.unique(N[np.asarray(count) > 0]):
        rows = (N == n_copies) & (np.asarray(count) > 0)
        o = 1.0 / (1.0 + np.exp(-x[rows]))
        one_minus_o = 1.0 / (1.0 + np.exp(x[rows]))
        op = -np.expm1(np.log(one_minus_o) / n_copies)
        D = D_double_loop(op, int(n_copies))
        out_s[rows] = np.log((o / D)[:, None] * np.exp(s[rows]))
        oc = np.clip(op, float(np.float32(min_opacity)), OPACITY_MAX)
        out_o[rows] = np.log(oc) - np.log1p(-oc)
    return out_o.reshape(np.shape(opacity)), out_s


def relocation_values_stock(opacity, scaling, count, min_opacity=MIN_OPACITY):
    """The published sequence in float32 torch (CPU): sigmoid / exp activations, compute_relocation's float32 double
    loop over a float32 binomial table, clamp, inverse_sigmoid and log."""
    x = torch.as_tensor(np.asarray(opacity, np.float32)).reshape(-1)
    s = torch.as_tensor(np.asarray(scaling, np.float32))
    cnt = np.asarray(count)
    N = torch.as_tensor(ratio(cnt))
    binoms = torch.zeros((MAX_RATIO + 1, MAX_RATIO + 1), dtype=torch.float32)
    for n in range(MAX_RATIO + 1):
        for k in range(n + 1):
            binoms[n, k] = math.comb(n, k)
    o_old, scale_old = torch.sigmoid(x), torch.exp(s)
    new_o = 1.0 - torch.pow(1.0 - o_old, 1.0 / N.to(torch.float32))
    denom = torch.ones_like(o_old)
    for copies in np.unique(ratio(cnt)[cnt > 0]):           # (the rows of one N together; the powers once per k)
        rows = torch.as_tensor((ratio(cnt) == copies) & (cnt > 0))
        terms = [torch.tensor((-1.0) ** k / math.sqrt(k + 1), dtype=torch.float32) * torch.pow(new_o[rows], k + 1) for k in range(copies)]
        total = torch.zeros_like(terms[0])
        for i in range(1, int(copies) + 1):
            for k in range(i):
                total = total + binoms[i - 1, k] * terms[k]
        denom[rows] = total
    new_scale = (o_old / denom)[:, None] * scale_old
    new_o = torch.clamp(new_o, max=1.0 - torch.finfo(torch.float32).eps, min=float(min_opacity))
    out_o, out_s = torch.log(new_o / (1.0 - new_o)), torch.log(new_scale)
    keep = torch.as_tensor(cnt == 0)
    out_o = torch.where(keep, x, out_o)
    out_s = torch.where(keep[:, None], s, out_s)
    return out_o.numpy().reshape(np.shape(opacity)), out_s.numpy()


# ---- noise ----

def rotation_matrices(q):
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def noise_increment(opacity, scaling, rotation, eps, step_scale):
    """float64 [n][3]: Sigma (eps f)."""
    o = np.asarray(opacity, np.float64).reshape(-1)
    R = rotation_matrices(np.asarray(rotation, np.float64))
    L = R * np.exp(np.asarray(scaling, np.float64))[:, None, :]
    cov = L @ L.transpose(0, 2, 1)
    one_minus_o = 1.0 / (1.0 + np.exp(o))
    with np.errstate(over="ignore"):
        f = float(np.float32(step_scale)) / (1.0 + np.exp(-100.0 * (one_minus_o - 0.995)))
    return (cov @ (np.asarray(eps, np.float64) * f[:, None])[:, :, None])[:, :, 0]


def _build_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def noise_increment_stock(opacity, scaling, rotation, eps, step_scale, dtype=torch.float32, device="cpu"):
    """The published per-step noise as stock PyTorch composes it (about a dozen launches and (n, 3, 3) temporaries):
    build_scaling_rotation, L L^T, op_sigmoid, bmm."""
    o = torch.as_tensor(np.asarray(opacity)).to(device, dtype).reshape(-1, 1)
    s = torch.exp(torch.as_tensor(np.asarray(scaling)).to(device, dtype))
    R = _build_rotation(torch.as_tensor(np.asarray(rotation)).to("cpu", dtype)).to(device)
    L = R @ torch.diag_embed(s)
    cov = L @ L.transpose(1, 2)
    f = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - torch.sigmoid(o)) - 0.995)))
    noise = torch.as_tensor(np.asarray(eps)).to(device, dtype) * f * step_scale
    return torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)


def noise_inputs(n: int, seed: int = 0):
    """Opacity logits across the factor's whole transition, unnormalised quaternions, log-scales over four decades."""
    rng = np.random.default_rng(seed)
    return dict(xyz=rng.normal(size=(n, 3)).astype(np.float32), opacity=rng.uniform(-8.0, 6.0, (n, 1)).astype(np.float32),
                scaling=rng.uniform(np.log(1e-3), np.log(10.0), (n, 3)).astype(np.float32),
                rotation=(rng.normal(size=(n, 4)) * np.exp(rng.uniform(-2, 2, (n, 1)))).astype(np.float32),
                eps=rng.normal(size=(n, 3)).astype(np.float32))


# ---- whole tables ----

PARAMS = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
ROLES = dict(xyz="copy", features_dc="copy", features_rest="copy", opacity="opacity", scaling="scaling", rotation="copy")
MOMENTS = ("exp_avg", "exp_avg_sq")


def scene_inputs(n: int, seed: int = 0, sh_rest: int = 15, dead_fraction: float = 0.2):
    """The six raw parameter tables (float32) with opacities from 0.006 to 1 - 1e-7 (uniform in the logit), about
    ``dead_fraction`` of them moved below logit(0.005), and two Adam moments per table."""
    rng = np.random.default_rng(seed)
    lo, hi = math.log(0.006 / 0.994), math.log((1 - 1e-7) / 1e-7)
    opacity = rng.uniform(lo, hi, (n, 1)).astype(np.float32)
    dead = rng.random(n) < dead_fraction
    opacity[dead, 0] = rng.uniform(-9.0, -5.5, int(dead.sum())).astype(np.float32)
    inp = dict(xyz=rng.normal(size=(n, 3)).astype(np.float32), features_dc=rng.normal(size=(n, 1, 3)).astype(np.float32),
               features_rest=rng.normal(size=(n, sh_rest, 3)).astype(np.float32), opacity=opacity,
               scaling=rng.uniform(np.log(1e-3), np.log(10.0), (n, 3)).astype(np.float32),
               rotation=rng.normal(size=(n, 4)).astype(np.float32))
    moments = {k: dict(exp_avg=rng.normal(size=inp[k].shape).astype(np.float32),
                       exp_avg_sq=rng.uniform(0.1, 1.0, size=inp[k].shape).astype(np.float32)) for k in PARAMS}
    return inp, moments
