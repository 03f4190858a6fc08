"""Float64 restatement of the latent epilogue (csrc/latent_epilogue.hip, include/lsr_latent.h) with an explicit output
size, the same composition in float32 ("stock": the error yardstick), the kernel's path predicates restated, and the
case table of tests/test_latent_paths_{cpu,gpu}.py with seeded inputs.  CPU only; torch ops and autograd, nothing else.

The bars (every element is on them):
  * resize-only quantities: error against float64 <= max(4 x stock error, 2^-20 x max |want|)  -- the margin and the
    floor of tests/test_photometric_gpu.py;
  * the full epilogue (the kernel uses __expf / __logf / __fsqrt_rn): per quantity max(project tolerance, 4 x stock
    error), the project tolerance being that of tests/test_latent_gpu.py: |err| <= 2e-5 + 2e-5 |want| per element for
    sample, skip, z and logvar, 1e-4 x max |want| for gradients."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

THREADS = 256           # kLatentThreads
MAX_COLS = 4            # kLatentMaxCols: width <= 1024
BWD_ROWS = 16           # kBwdRows
NOZ_ROWS = 8            # rows per forward band when z is not wanted
DEFAULT_INTERVAL = (-30.0, 20.0)
NARROW_INTERVAL = (-10.0, 2.0)
MARGIN = 4.0
FLOOR = 2.0 ** -20
VALUE_TOL = 2e-5        # rtol = atol of sample / skip / z / logvar
GRAD_TOL = 1e-4         # x max |want|

# case -> (V, C, H, W, out_h, out_w)
CASES = {
    1: (2, 3, 48, 64, 36, 48),        # scale 4/3, float4 path
    2: (1, 2, 45, 30, 30, 20),        # scale 3/2, scalar path, scalar colour copy
    3: (1, 1, 40, 1024, 15, 384),     # scale 8/3, float4 path with one row lane, the width limit
    4: (1, 2, 17, 4, 17, 1),          # 256 row lanes for 17 rows, vertical identity, H = 16 + 1
    5: (1, 1, 33, 1023, 11, 341),     # scalar path, four columns per thread, odd width
    6: (1, 1, 16, 1021, 1, 1),        # one output, window = whole image
    7: (1, 1, 1024, 4, 1, 1),         # the same, vertically
    8: (1, 2, 30, 260, 10, 65),       # sy = 3, sx = 4; W % 4 == 0 off the float4 path
    9: (1, 2, 7, 12, 7, 4),           # H < 8, W = 12
    10: (1, 1, 100, 100, 33, 33),     # scale 100/33 (the CPU weight test's ratio)
    11: (1, 1, 9, 257, 3, 257),       # the second column held by one thread
    12: (1, 1, 9, 768, 3, 256),       # exactly three columns per thread
}
VARIATIONAL_CASES = (1, 2, 5, 8)
ABI_CASES = (2, 4)
GRAD_MODES = ("z", "skip", "both")


def uses_float4_path(W: int) -> bool:
    """The forward's vector-path predicate: 16-byte accesses, a whole number of row lanes in the block."""
    return W % 4 == 0 and 256 % (W // 4) == 0


def row_lanes(W: int) -> int:
    """Rows in flight on the float4 path."""
    assert uses_float4_path(W)
    return THREADS // (W // 4)


def columns_per_thread(W: int) -> int:
    """Columns the busiest thread (thread 0) holds on the scalar path."""
    return -(-W // THREADS)


def forward_bands(H: int, out_h: int, want_z: bool = True) -> int:
    return out_h if want_z else -(-H // NOZ_ROWS)


def backward_bands(H: int) -> int:
    return -(-H // BWD_ROWS)


def is_isotropic(case: int) -> bool:
    """One scale for both axes: expressible through the public rescale / sample_rescale_skip."""
    _, _, H, W, oh, ow = CASES[case]
    return H * ow == W * oh


def clamp_plants(interval) -> np.ndarray:
    """Both ends of the interval and their float32 neighbours on both sides."""
    lo, hi = np.float32(interval[0]), np.float32(interval[1])
    inf = np.float32(np.inf)
    return np.array([lo, hi, np.nextafter(lo, -inf), np.nextafter(lo, inf), np.nextafter(hi, -inf), np.nextafter(hi, inf)],
                    np.float32)


@functools.lru_cache(maxsize=None)
def make_inputs(case: int, variational: bool = False, interval=DEFAULT_INTERVAL) -> dict:
    """Seeded float32 inputs of one case.  Shared between tests: never modify them.
    mask = rand ** 0.2 with exact 0 and 1 planted; variational: logvar half = 15 randn with the interval's ends and
    their float32 neighbours planted (8 copies each) and 12 % of the elements moved outside the interval on each side."""
    V, C, H, W, oh, ow = CASES[case]
    g = torch.Generator().manual_seed(7919 * case + (1 if variational else 0) + (2 if tuple(interval) != DEFAULT_INTERVAL else 0))
    features = torch.randn(V, 2 * C if variational else C, H, W, generator=g)
    if variational:
        lv = 15.0 * torch.randn(V * C * H * W, generator=g)
        perm = torch.randperm(lv.numel(), generator=g)
        plants = torch.from_numpy(clamp_plants(interval)).repeat(8)
        n_out = (12 * lv.numel() + 99) // 100
        a, b, c = plants.numel(), plants.numel() + n_out, plants.numel() + 2 * n_out
        assert c <= lv.numel()
        lv[perm[:a]] = plants
        lv[perm[a:b]] = interval[0] - 0.5 - 30.0 * torch.rand(n_out, generator=g)
        lv[perm[b:c]] = interval[1] + 0.5 + 30.0 * torch.rand(n_out, generator=g)
        features[:, C:] = lv.reshape(V, C, H, W)
    mask = torch.rand(V * H * W, generator=g) ** 0.2
    perm = torch.randperm(mask.numel(), generator=g)
    k = max(1, mask.numel() // 16)
    mask[perm[:k]] = 0.0
    mask[perm[k:2 * k]] = 1.0
    return dict(features=features, mask=mask.reshape(V, H, W), noise=torch.randn(V, C, H, W, generator=g),
                color=torch.rand(V, 3, H, W, generator=g), g_z=torch.randn(V, C, oh, ow, generator=g),
                g_skip=torch.randn(V, 3 + C, H, W, generator=g), size=(oh, ow), variational=variational,
                interval=tuple(interval))


def compose(inp: dict, dtype, noise: bool = True, color: bool = True, modes=GRAD_MODES) -> dict:
    """The epilogue as a composition of torch CPU operators in `dtype`, the gradient of sum(z g_z) ("z"), sum(skip g_skip)
    ("skip") or their sum ("both") with respect to `features` by autograd.  Everything comes back as float64 numpy."""
    to = lambda t: t.to(dtype)
    f = to(inp["features"]).clone().requires_grad_(bool(modes))
    if inp["variational"]:
        mean, logvar = f.chunk(2, dim=-3)
    else:
        mean, logvar = f, (1 - to(inp["mask"]).unsqueeze(-3)).log()
    logvar = torch.clamp(logvar, *inp["interval"])
    sample = mean + torch.exp(logvar / 2) * to(inp["noise"]) if noise else mean
    z = F.interpolate(sample, size=inp["size"], mode="bilinear", align_corners=False, antialias=True)
    skip = torch.cat((to(inp["color"]), sample), dim=-3) if color else sample
    g_z, g_skip = to(inp["g_z"]), to(inp["g_skip"] if color else inp["g_skip"][:, 3:])
    loss = dict(z=lambda: (z * g_z).sum(), skip=lambda: (skip * g_skip).sum(), both=lambda: (z * g_z).sum() + (skip * g_skip).sum())
    out = dict(sample=sample, z=z, skip=skip, logvar=logvar)
    for m in modes:
        out["grad_" + m], = torch.autograd.grad(loss[m](), f, retain_graph=True)
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def epilogue_pair(case: int, variational: bool = False, interval=DEFAULT_INTERVAL, noise: bool = True, color: bool = True):
    """(float64 restatement, stock float32 composition) of one configuration, computed once."""
    inp = make_inputs(case, variational, interval)
    return compose(inp, torch.float64, noise, color), compose(inp, torch.float32, noise, color)


def resize(x: torch.Tensor, size, g: torch.Tensor, dtype) -> dict:
    leaf = x.to(dtype).clone().requires_grad_(True)
    z = F.interpolate(leaf, size=tuple(size), mode="bilinear", align_corners=False, antialias=True)
    grad, = torch.autograd.grad((z * g.to(dtype)).sum(), leaf)
    return dict(z=z.detach().to(torch.float64).numpy(), grad=grad.to(torch.float64).numpy())


@functools.lru_cache(maxsize=None)
def resize_pair(case: int):
    """(float64, stock float32) of the resize alone: z of the case's mean features and its gradient under g_z."""
    inp = make_inputs(case)
    return tuple(resize(inp["features"], inp["size"], inp["g_z"], dt) for dt in (torch.float64, torch.float32))


WORST = {}          # quantity -> worst kernel error / stock error seen


def held(name: str, got, want: np.ndarray, stock: np.ndarray, kind: str, show: str = "") -> None:
    """Assert every element of `got` on the bar of its kind: "resize", "value" (sample / skip / z / logvar of the full
    epilogue) or "grad" (its gradients).  Prints kernel error, stock error and their ratio."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (show, name, got.shape, want.shape)
    assert np.isfinite(want).all() and np.isfinite(got).all(), (show, name, "not finite")
    diff = np.abs(got - want)
    err, err_stock = float(diff.max()), float(np.abs(stock - want).max())
    scale = float(np.abs(want).max())
    if kind == "resize":
        bar = max(MARGIN * err_stock, FLOOR * scale)
    elif kind == "value":
        bar = np.maximum(VALUE_TOL + VALUE_TOL * np.abs(want), MARGIN * err_stock)
    else:
        assert kind == "grad"
        bar = max(GRAD_TOL * scale, MARGIN * err_stock)
    ratio = err / err_stock if err_stock > 0 else (0.0 if err == 0 else float("inf"))
    if np.isfinite(ratio):
        WORST[name] = max(WORST.get(name, 0.0), ratio)
    over = diff > bar
    print(f"{show} {name:12s} kernel {err:.3e}  stock {err_stock:.3e}  ratio {ratio:.3f}  scale {scale:.3e}  over the bar {int(over.sum())}")
    assert not over.any(), (show, name, err, err_stock, float(np.max(diff - bar)))
