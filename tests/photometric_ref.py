"""The photometric loss of include/lsr_loss.h restated in float64 numpy: the SSIM map through the separable 11-tap Gaussian
window with zero padding, the per-image means, the loss and its analytic gradient; and, for the tests' bars, the stock
PyTorch composition of the same loss (grouped ``conv2d`` + autograd) in any dtype, plus the tests' seeded inputs."""
import math

import numpy as np

R = 5
TAPS = 2 * R + 1
C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE = 32            # kPhTile of csrc/photometric.hip: output pixels per tile, each way
WAVE = 64            # lanes of a wave: k_photo_finish adds the slots of an image WAVE at a time ...
FINISH_WAVES = 16    # ... and its 1024 lanes are 16 waves, wave w taking the images w, w + 16, ...


def photo_shift(H: int, W: int) -> float:
    """photo_shift of csrc/photometric.hip: the constant both kernels subtract from the images, 0.5 times the image's share
    of its zero-padded extent, to the nearest eighth."""
    share = H * W / ((H + 2.0 * R) * (W + 2.0 * R))
    return math.floor(4.0 * share + 0.5) / 8.0


def tile_grid(H: int, W: int):
    """(tiles_y, tiles_x) of one plane."""
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def slots_per_image(shape) -> int:
    """Workspace slots k_photo_finish adds per image of a ``(V, C, H, W)`` call: one per tile of every plane."""
    ty, tx = tile_grid(*shape[2:])
    return shape[1] * ty * tx


def window() -> np.ndarray:
    g = np.array([math.exp(-(k - R) ** 2 / (2 * 1.5 ** 2)) for k in range(TAPS)], dtype=np.float64)
    return g / g.sum()


def blur(a: np.ndarray) -> np.ndarray:
    """``w * a`` with ``w = g g^T`` over the last two axes, zero outside the image."""
    g = window()
    H, W = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(R, R), (R, R)])
    h = sum(g[k] * p[..., :, k:k + W] for k in range(TAPS))
    return sum(g[k] * h[..., k:k + H, :] for k in range(TAPS))


def _terms(x, y, cov_norm):
    mu1, mu2 = blur(x), blur(y)
    s1 = cov_norm * (blur(x * x) - mu1 * mu1)
    s2 = cov_norm * (blur(y * y) - mu2 * mu2)
    s12 = cov_norm * (blur(x * y) - mu1 * mu2)
    return mu1, mu2, 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2


def ssim_map(x: np.ndarray, y: np.ndarray, cov_norm: float = 1.0) -> np.ndarray:
    _, _, A1, A2, B1, B2 = _terms(x.astype(np.float64), y.astype(np.float64), cov_norm)
    return A1 * A2 / (B1 * B2)


def results(x: np.ndarray, y: np.ndarray, lam: float = 0.2, cov_norm: float = 1.0, crop: int = 0) -> dict:
    """``loss``, ``l1 (V,)``, ``ssim (V,)`` and the ``map`` for ``(V, C, H, W)`` images."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    S = ssim_map(x, y, cov_norm)
    H, W = x.shape[-2:]
    inner = S[..., crop:H - crop, crop:W - crop]
    ssim = inner.reshape(x.shape[0], -1).mean(1)
    l1 = np.abs(x - y).reshape(x.shape[0], -1).mean(1)
    return dict(loss=(1 - lam) * l1.mean() + lam * (1 - ssim.mean()), l1=l1, ssim=ssim, map=S)


def gradient(x: np.ndarray, y: np.ndarray, lam: float = 0.2) -> np.ndarray:
    """d loss / d x, analytically (cov_norm 1, crop 0)."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    mu1, mu2, A1, A2, B1, B2 = _terms(x, y, 1.0)
    dS1 = -A1 * A2 / (B1 * B2 * B2)
    dS12 = 2 * A1 / (B1 * B2)
    Dmu = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * A1 * A2 / (B1 * B1 * B2) - 2 * mu1 * dS1 - mu2 * dS12
    dmean = (blur(Dmu) + 2 * x * blur(dS1) + y * blur(dS12)) / x.size
    return (1 - lam) * np.sign(x - y) / x.size - lam * dmean


# ---- the stock composition (what a trainer writes in PyTorch), any dtype ----

def stock_map(x, y, cov_norm: float = 1.0):
    import torch
    import torch.nn.functional as F
    C = x.shape[1]
    g = torch.from_numpy(window()).to(x.dtype)
    w = (g[:, None] * g[None, :]).expand(C, 1, TAPS, TAPS).contiguous()
    f = lambda t: F.conv2d(t, w, padding=R, groups=C)
    mu1, mu2 = f(x), f(y)
    s1, s2, s12 = cov_norm * (f(x * x) - mu1 * mu1), cov_norm * (f(y * y) - mu2 * mu2), cov_norm * (f(x * y) - mu1 * mu2)
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def stock_results(x, y, lam: float = 0.2, cov_norm: float = 1.0, crop: int = 0, grad: bool = True) -> dict:
    """The same quantities as :func:`results` (and ``grad`` through autograd) from torch CPU tensors of one dtype, as float64
    numpy."""
    import torch
    x = x.clone().requires_grad_(grad)
    S = stock_map(x, y, cov_norm)
    H, W = x.shape[-2:]
    ssim = S[..., crop:H - crop, crop:W - crop].reshape(x.shape[0], -1).mean(1)
    l1 = (x - y).abs().reshape(x.shape[0], -1).mean(1)
    loss = (1 - lam) * l1.mean() + lam * (1 - ssim.mean())
    out = dict(loss=loss, l1=l1, ssim=ssim, map=S)
    if grad:
        out["grad"], = torch.autograd.grad(loss, x)
    return {k: v.detach().double().numpy() for k, v in out.items()}


# ---- inputs ----

def smooth(V: int, C: int, H: int, W: int) -> np.ndarray:
    """Smooth sinusoids with a flat 0.9 patch over the top-left (H // 3, W // 2): where ``w*x^2 - mu^2`` cancels worst."""
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    im = np.stack([0.5 + 0.5 * np.sin(6 * xx * (c + 1) + 3 * yy * (v + 1)) for v in range(V) for c in range(C)]).reshape(V, C, H, W)
    im[:, :, :H // 3, :W // 2] = 0.9
    return im


def make_pair(shape, kind: str, seed: int):
    """``(image, target)`` as float32 arrays: the target is uniform noise or :func:`smooth`, the image the target plus 0.05
    Gaussian noise, clamped to [0, 1]."""
    rng = np.random.default_rng(seed)
    y = rng.random(shape) if kind == "noise" else smooth(*shape)
    x = np.clip(y + 0.05 * rng.standard_normal(shape), 0.0, 1.0)
    return x.astype(np.float32), y.astype(np.float32)
