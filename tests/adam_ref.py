"""Reference of the fused Adam step (include/lsr_optim.h): the header's three formulas in float64 numpy on the CPU, from
float32 inputs and the float32 scalars the C ABI takes, with the visibility mask; and the error bounds the GPU tests
hold the kernel to.

Per element and step, with g, m, v, p in float64 and the seven scalars the float32 values of the table (``1 - beta`` is
the table's ``one_minus_beta``: ``float32(1 - beta)`` of the double beta, not ``1 - float32(beta)``)::

    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)

Rows whose mask byte is 0 are left as they are.

The bounds (after T steps from identical float32 inputs; each of m and v takes three float32 roundings per step, the
update about ten, and the subtraction from p one rounding of p itself)::

    |m - m_ref| <= 4 T 2^-24 max_t max(|m_ref,t|, |g_t|)
    |v - v_ref| <= 4 T 2^-24 max_t max(v_ref,t, g_t^2)
    |p - p_ref| <= T 2^-23 max_t |p_ref,t| + 32 2^-24 sum_t |dp_ref,t|

all per element, the maxima and the sum over the steps in which the element's row was updated (and the inputs)."""
import math

import numpy as np

WIDTHS = (3, 3, 45, 1, 3, 4)      # a degree-3 scene: xyz, f_dc, f_rest, opacity, scaling, rotation
SHAPES = lambda n, rest=15: [(n, 3), (n, 1, 3), (n, rest, 3), (n, 1), (n, 3), (n, 4)]
# one set per table: the scene's rates, and betas / eps that differ so that a mixed-up descriptor shows
HYPER = (dict(lr=1.6e-4, betas=(0.9, 0.999), eps=1e-15), dict(lr=2.5e-3, betas=(0.8, 0.99), eps=1e-15),
         dict(lr=1.25e-4, betas=(0.9, 0.999), eps=1e-8), dict(lr=5e-2, betas=(0.5, 0.9), eps=1e-15),
         dict(lr=5e-3, betas=(0.0, 0.999), eps=0.0), dict(lr=1e-3, betas=(0.95, 0.5), eps=1e-15))


def scalars(lr, betas, eps, step, bias_correction=True):
    """The seven float32 scalars of lsr_adam_table for step ``step`` (1 for the first): beta1, beta2, 1 - beta1,
    1 - beta2, eps, step_size, inv_sqrt_bc2, each computed in double and rounded once."""
    b1, b2 = float(betas[0]), float(betas[1])
    step_size = lr / (1.0 - b1 ** step) if bias_correction else lr
    inv_sqrt_bc2 = 1.0 / math.sqrt(1.0 - b2 ** step) if bias_correction else 1.0
    return tuple(float(np.float32(x)) for x in (b1, b2, 1.0 - b1, 1.0 - b2, eps, step_size, inv_sqrt_bc2))


def step(p, g, m, v, sc, visible=None):
    """One step in float64; ``sc`` from :func:`scalars`; ``visible`` a ``(rows,)`` array or None.  Returns new p, m, v
    and the update |dp| (0 on rows that are not updated)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    beta1, beta2, c1, c2, eps, step_size, inv_sqrt_bc2 = sc
    m1 = beta1 * m + c1 * g
    v1 = beta2 * v + c2 * g * g
    dp = step_size * m1 / (np.sqrt(v1) * inv_sqrt_bc2 + eps)
    p1 = p - dp
    if visible is not None:
        on = (np.asarray(visible) != 0).reshape((-1,) + (1,) * (p.ndim - 1))
        p1, m1, v1, dp = np.where(on, p1, p), np.where(on, m1, m), np.where(on, v1, v), np.where(on, dp, 0.0)
    return p1, m1, v1, np.abs(dp)


def run(p0, grads, hyper, bias_correction=True, masks=None, m0=None, v0=None, first_step=1):
    """``len(grads)`` steps from float32 ``p0`` (and moments, default 0).  Returns a dict: ``p``, ``m``, ``v`` in
    float64 and the three bounds of the module's docstring as arrays."""
    p = np.asarray(p0, np.float64)
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, np.float64)
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, np.float64)
    T = len(grads)
    m_scale, v_scale, p_scale, dp_sum = np.abs(m), v.copy(), np.abs(p), np.zeros_like(p)
    for t, g in enumerate(grads):
        g = np.asarray(g, np.float64)
        vis = None if masks is None else masks[t]
        sc = scalars(hyper["lr"], hyper["betas"], hyper["eps"], first_step + t, bias_correction)
        p, m, v, dp = step(p, g, m, v, sc, vis)
        on = True if vis is None else (np.asarray(vis) != 0).reshape((-1,) + (1,) * (p.ndim - 1))
        m_scale = np.maximum(m_scale, np.where(on, np.maximum(np.abs(m), np.abs(g)), 0.0))
        v_scale = np.maximum(v_scale, np.where(on, np.maximum(v, g * g), 0.0))
        p_scale = np.maximum(p_scale, np.abs(p))
        dp_sum += dp
    return dict(p=p, m=m, v=v, bound_m=4 * T * 2.0 ** -24 * m_scale, bound_v=4 * T * 2.0 ** -24 * v_scale,
                bound_p=T * 2.0 ** -23 * p_scale + 32 * 2.0 ** -24 * dp_sum)


def draw_grad(rng, shape):
    """|g| log-uniform in [1e-3, 1] with a random sign: sqrt(v) dominates eps and nothing cancels behind the bounds."""
    return (np.exp(rng.uniform(np.log(1e-3), 0.0, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def within(name, got, ref, show=""):
    """The worst error / bound ratio of each of ``got = dict(p, m, v)`` (printed): within the bounds when <= 1."""
    worst = {}
    for k in ("m", "v", "p"):
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        bound = ref["bound_" + k]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        worst[k] = float(ratio.max()) if ratio.size else 0.0
    print(f"{show} {name:8s} error / bound: m {worst['m']:.3f}  v {worst['v']:.3f}  p {worst['p']:.3f}")
    return worst
