"""Restatement of the fused depth head's contract (include/lsr_depth_head.h) with stock PyTorch ops, any
dtype (the tests use float64), forward and autograd backward.  Test infrastructure: it is what the
golden files (made by the reference's own module) and the HIP kernels are both held against."""
import numpy as np
import torch

F32_EPS = float(np.finfo(np.float32).eps)


def split(logits, surfaces):
    """(..., 2 S F) with channel (bucket F + surface) 2 + c  ->  pdf logits, offset logits (..., F, S)."""
    x = logits.reshape(*logits.shape[:-1], -1, surfaces, 2)
    return x[..., 0].transpose(-1, -2), x[..., 1].transpose(-1, -2)


def distribution(logits, surfaces):
    """p, o, n, cdf, each (..., F, S)."""
    pdf_raw, off_raw = split(logits, surfaces)
    p = torch.softmax(pdf_raw, dim=-1)
    o = torch.sigmoid(off_raw)
    n = p / (F32_EPS + p.sum(-1, keepdim=True))
    return p, o, n, n.cumsum(-1)


def sample_indices(cdf, uniforms):
    """#{ i : cdf_i <= u } clipped to S - 1; cdf (..., S), uniforms (..., k) -> int64 (..., k)."""
    count = (cdf[..., None, :] <= uniforms[..., :, None]).sum(-1)
    return count.clamp(max=cdf.shape[-1] - 1)


def edge_gap(cdf, uniforms):
    """Distance of every uniform to the nearest cumulative-sum edge it could cross, (..., k): the last
    edge cannot change a clipped index and is left out."""
    edges = cdf[..., :-1]
    if edges.shape[-1] == 0:
        return torch.full_like(uniforms, float("inf"))
    return (edges[..., None, :] - uniforms[..., :, None]).abs().amin(-1)


def forward(logits, near, far, surfaces, uniforms=None, deterministic=False, samples=None, transmittance=False,
            exponent=1.0, scale=1.0, index=None):
    """logits (cams, rays, 2 S F), near / far (cams,), uniforms (cams, rays, F, k) ->
    depth, opacity, index (cams, rays, F, k).  `index` overrides the sampling (gradient checks)."""
    p, o, n, cdf = distribution(logits, surfaces)
    S = p.shape[-1]
    if index is None:
        if deterministic:
            index = p.topk(samples, dim=-1).indices
        else:
            index = sample_indices(cdf.detach(), uniforms.to(cdf.dtype))
    index = index.long()
    rd = (index + o.gather(-1, index)) / S
    nr, fr = near.reshape(-1, 1, 1, 1), far.reshape(-1, 1, 1, 1)
    dn, df = 1 / (nr + 1e-10), 1 / (fr + 1e-10)
    depth = 1 / ((1 - rd) * (dn - df) + df + 1e-10)
    if transmittance:
        partial = p.cumsum(-1)
        partial = torch.cat((torch.zeros_like(partial[..., :1]), partial[..., :-1]), -1)
        x = (p / (1 - partial + 1e-10)).gather(-1, index)
    else:
        x = n.gather(-1, index)
    opacity = scale * 0.5 * (1 - (1 - x) ** exponent + x ** (1 / exponent))
    return depth, opacity, index


def forward_backward(logits, near, far, surfaces, g_depth, g_opacity, dtype=torch.float64, **kw):
    """numpy in, numpy out: depth, opacity, index, dL/dlogits for L = sum(depth g_depth + opacity g_opacity)."""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    lg = t(logits).requires_grad_()
    if kw.get("uniforms") is not None:
        kw["uniforms"] = t(kw["uniforms"])
    if kw.get("index") is not None:
        kw["index"] = torch.as_tensor(np.asarray(kw["index"]))
    depth, opacity, index = forward(lg, t(near), t(far), surfaces, **kw)
    ((depth * t(g_depth)).sum() + (opacity * t(g_opacity)).sum()).backward()
    return depth.detach().numpy(), opacity.detach().numpy(), index.numpy(), lg.grad.numpy()


def random_case(cams, rays, S, F, k, seed, deterministic=False, min_gap=1e-5, logit_scale=2.0):
    """Seeded inputs (float32 numpy) whose float64 indices cannot be moved by float32 rounding: every uniform
    at least `min_gap` from the edges that matter (deterministic: consecutive probabilities among the k + 1
    largest `min_gap` apart), as the golden maker demands; another seed is drawn otherwise.  min_gap=None:
    the first draw, unconditioned."""
    while True:
        rng = np.random.default_rng(seed)
        c = dict(logits=(logit_scale * rng.normal(size=(cams, rays, 2 * S * F))).astype(np.float32),
                 near=(0.5 + rng.random(cams)).astype(np.float32), uniforms=rng.random((cams, rays, F, k), dtype=np.float32),
                 g_depth=rng.normal(size=(cams, rays, F, k)).astype(np.float32),
                 g_opacity=rng.normal(size=(cams, rays, F, k)).astype(np.float32))
        c["far"] = (c["near"] + 2.0 + 5.0 * rng.random(cams)).astype(np.float32)
        if min_gap is None:
            return c
        p, _, _, cdf = distribution(torch.tensor(c["logits"]).double(), F)
        if deterministic:
            top = p.topk(min(k + 1, S), dim=-1).values
            margin = float((top[..., :-1] - top[..., 1:]).min()) if S > 1 else 1.0
        else:
            margin = float(edge_gap(cdf, torch.tensor(c["uniforms"]).double()).min())
        if margin >= min_gap:
            return c
        seed += 1000


ENCODER_SHAPE = (2, 65536, 32, 1, 3)      # cameras, rays, S, F, k: one scene of the reference's training shape
ENCODER_SEED = 5
ENCODER_GAP = 1e-6                        # float32 cumulative-sum rounding: samples closer to an edge are left out
ENCODER_MAX_SHARE = 5e-4                  # (expected for uniform draws: 2 * 1e-6 * 32 = 6.4e-5)


def encoder_case():
    """The encoder-size inputs and the mask (cams, rays, F, k) of samples within ENCODER_GAP of an edge."""
    c = random_case(*ENCODER_SHAPE, seed=ENCODER_SEED, min_gap=None)
    cdf = distribution(torch.tensor(c["logits"]).double(), ENCODER_SHAPE[3])[3]
    close = edge_gap(cdf, torch.tensor(c["uniforms"]).double()) < ENCODER_GAP
    return c, close.numpy()
