"""The cases of tests/test_loss_sum_bits_gpu.py and of tests/golden/make_golden_loss_sum_bits.py: seeded host inputs for the
five fused image losses, and one function that runs their forwards and returns every compared output as raw bits.

What is pinned is the ORDER of the double sums behind the losses (csrc/lsr_wave.h ``block_sum``, csrc/lsr_image_sum.h):
a lane's pixels, the wave butterfly, the waves of a workgroup in order, a lane's slots, the butterfly again, the waves of
the finish in order.  A sum of doubles rounds only when its terms differ in magnitude by more than the 29 bits a double
has over a float32 product, so every input is drawn log-uniformly over dozens of binades: a changed order then changes
low bits of the double totals.  Those bits reach a float32 result only where the sum cancels, so the three losses whose
terms have a sign carry PLANTED PAIRS as well (:func:`_pairs`): two pixels of one image whose terms are +K and -K with K
up to 2^50, thousands of them per image.  Their partial sums round at 2^50 x 2^-53 while the image's total is that of the
small terms, a few units: another order of the same terms moves the float32 result by thousands of ulps.
  distortion   alpha M2 - M1^2 = +q^2 from (alpha, M2, M1) = (1, q^2, 0) and -q^2 from (M2, M1) = (0, q); q has 12
               significant bits, so q^2 is a float32; the two pixels share their weight.
  normals      the surface is the plane depth / alpha = 4, whose normal is (0, 0, +-1) up to a rounding, and the rendered
               normal's z is +K and -K at two valid pixels.
  depth, fit   the two pixels share depth, alpha and target and weigh +K and -K: all six moments cancel.
               NEGATIVE WEIGHTS ARE OUTSIDE THE LOSS'S CONTRACT: a weight below 0 means nothing, and the kernels merely do
               not refuse it.  The six moments have no in-contract term with a sign, so this is the one way to make their
               order visible; if weights >= 0 are ever validated, this configuration needs new inputs and a new recording.
The photometric sums, the depth loss's |r| and the total variation add terms of one sign: for them the fixture pins the
bits, and only a larger change of order than a rounding of the double would show.

Shapes: the smallest that reach every loop of the shared bodies.
  many_images  V = 17, 5 x 7: one more image than the 16 waves of a finish; 35 pixels: a ragged group of 4, a single slot.
  many_chunks  V = 2, 275 x 477 = 131 175 pixels: 65 chunks of 2048, one more than a wave has lanes (distortion, depth).
  many_tiles   V = 2, 131 x 389: 5 x 13 = 65 tiles of 32 x 32, ragged on both edges (photometric with C = 1, normals).
  bilagrid     3 grids of 12 x 8 x 43 x 43 = 532 512 entries: 261 workgroups of 2048, past the 256 lanes of the TV finish."""
import numpy as np

from tests import normals_ref

SEED = 20261021
LAMBDA = 0.2
NC_ALPHA_MIN = 2.0 ** -10
DEPTH_CONFIGS = (("fit", "pixels", True), ("given", "weights", False))
IMAGE_CASES = {
    # name: (V, H, W, photometric channels or None, normals, chunked losses)
    "many_images": (17, 5, 7, 3, True, True),
    "many_chunks": (2, 275, 477, None, False, True),
    "many_tiles": (2, 131, 389, 1, True, False),
}
GRIDS_SHAPE = (3, 12, 8, 43, 43)


def _log_uniform(rng, shape, lo: float, hi: float, signed: bool = False) -> np.ndarray:
    """float32 values 2^u, u uniform in [lo, hi); ``signed``: with a random sign."""
    v = np.exp2(rng.uniform(lo, hi, shape))
    if signed:
        v = v * rng.choice([-1.0, 1.0], shape)
    return v.astype(np.float32)


def _coarse(rng, shape, lo: int, hi: int) -> np.ndarray:
    """float32 values 2^e (1 + j / 2048), e in [lo, hi): 12 significant bits, so the square is a float32 too."""
    return np.ldexp(1.0 + rng.integers(0, 2048, shape) / 2048.0, rng.integers(lo, hi, shape)).astype(np.float32)


def _pairs(rng, candidates: np.ndarray, share: float):
    """Two disjoint index arrays of one length out of ``candidates`` (flat pixel indices), ``share`` of them in all."""
    pick = rng.permutation(candidates)[:2 * (int(len(candidates) * share) // 2)]
    return pick[0::2], pick[1::2]


def image_inputs(name: str) -> dict:
    """The host inputs of one image case, float32 numpy, from ``default_rng``: the same arrays every call."""
    V, H, W, channels, normals, chunked = IMAGE_CASES[name]
    rng = np.random.default_rng([SEED, sorted(IMAGE_CASES).index(name)])
    x = {}
    if channels:
        x["image"] = _log_uniform(rng, (V, channels, H, W), -24, 0)
        x["target"] = _log_uniform(rng, (V, channels, H, W), -24, 0)
    if normals:
        alpha = _log_uniform(rng, (V, H, W), -12, 0)               # some below NC_ALPHA_MIN: invalid stencils
        x["nc_views"] = normals_ref.make_views(V, seed=5, offcentre=True)
        x["nc_alpha"] = alpha
        x["nc_depth"] = 4.0 * alpha                                 # (exact: depth / alpha is 4 everywhere)
        nmap = (rng.standard_normal((V, 3, H, W)) * _log_uniform(rng, (V, 1, H, W), -20, 0)).astype(np.float32)
        ok = np.pad(alpha > NC_ALPHA_MIN, ((0, 0), (1, 1), (1, 1)))
        valid = ok[:, 1:-1, 1:-1] & ok[:, 1:-1, :-2] & ok[:, 1:-1, 2:] & ok[:, :-2, 1:-1] & ok[:, 2:, 1:-1]
        valid[:, [0, -1], :] = False
        valid[:, :, [0, -1]] = False
        for v in range(V):
            pos, neg = _pairs(rng, np.flatnonzero(valid[v]), 0.5)
            K = _coarse(rng, len(pos), 20, 45)
            nmap[v, 2].reshape(-1)[pos] = K
            nmap[v, 2].reshape(-1)[neg] = -K
        x["normal_map"] = nmap
    if chunked:
        x["moment_map"] = np.stack([_log_uniform(rng, (V, H, W), -16, 4, signed=True), _log_uniform(rng, (V, H, W), -30, 8)], axis=1)
        x["dist_alpha"] = _log_uniform(rng, (V, H, W), -12, 0)
        x["dist_weight"] = _log_uniform(rng, (V, H, W), -10, 2)
        for v in range(V):
            pos, neg = _pairs(rng, np.arange(H * W), 0.5)
            q = _coarse(rng, len(pos), 10, 25)
            m1, m2, al, wt = (a[v].reshape(-1) for a in (x["moment_map"][:, 0], x["moment_map"][:, 1], x["dist_alpha"], x["dist_weight"]))
            al[pos], m2[pos], m1[pos] = 1.0, q * q, 0.0
            m2[neg], m1[neg], wt[neg] = 0.0, q, wt[pos]
        views = rng.standard_normal((V, normals_ref.VIEW_FLOATS)).astype(np.float32)
        views[:, 40] = np.array([(0.5, 1.0, 2.5)[v % 3] for v in range(V)], np.float32)
        x["dl_views"] = views
        x["dl_alpha"] = _log_uniform(rng, (V, H, W), -8, 0)         # some below the gate of 0.01
        x["dl_depth"] = _log_uniform(rng, (V, H, W), -6, 6)
        sparse = _log_uniform(rng, (V, H, W), -10, 4)
        sparse[rng.random((V, H, W)) < 0.3] = 0.0                   # unweighted: target > 0 is the mask
        x["dl_target_sparse"] = sparse
        x["dl_target"] = _log_uniform(rng, (V, H, W), -10, 4)
        weight = _log_uniform(rng, (V, H, W), -12, 2)
        weight[rng.random((V, H, W)) < 0.25] = 0.0
        for v in range(V):
            pos, neg = _pairs(rng, np.arange(H * W), 0.5)
            K = _coarse(rng, len(pos), 25, 40)
            for key in ("dl_depth", "dl_alpha", "dl_target"):
                x[key][v].reshape(-1)[neg] = x[key][v].reshape(-1)[pos]
            weight[v].reshape(-1)[pos] = K
            weight[v].reshape(-1)[neg] = -K
        x["dl_weight"] = weight
        x["dl_affine"] = np.stack([rng.uniform(0.5, 2.0, V), rng.uniform(-0.05, 0.1, V)], axis=1).astype(np.float32)
    return x


def grids_input() -> np.ndarray:
    return _log_uniform(np.random.default_rng([SEED, 99]), GRIDS_SHAPE, -12, 2, signed=True)


def _bits(prefix: str, out: dict, names) -> dict:
    return {f"{prefix}.{k}": out[k].detach().cpu().contiguous().numpy().view(np.uint32).copy() for k in names}


def image_outputs(name: str, dev) -> dict:
    """``{"<loss>.<output>": uint32 bits}`` of every compared output of one image case, computed on ``dev``."""
    import torch
    from latentsplat_amd.depth_sup import inverse_depth_forward
    from latentsplat_amd.distortion import distortion_loss_forward
    from latentsplat_amd.losses import photometric_forward
    from latentsplat_amd.normals import normal_consistency_forward
    x = {k: torch.from_numpy(v).to(dev) for k, v in image_inputs(name).items()}
    got = {}
    if "image" in x:
        got.update(_bits("photometric", photometric_forward(x["image"], x["target"], LAMBDA), ("loss", "l1", "ssim")))
    if "normal_map" in x:
        out = normal_consistency_forward(x["normal_map"], x["nc_depth"], x["nc_alpha"], x["nc_views"], NC_ALPHA_MIN,
                                         want=("loss", "per_view"))
        got.update(_bits("normals", out, ("loss", "per_view")))
    if "moment_map" in x:
        for tag, weight in (("distortion", None), ("distortion_weighted", x["dist_weight"])):
            out = distortion_loss_forward(x["moment_map"], x["dist_alpha"], weight, want=("loss", "per_view"))
            got.update(_bits(tag, out, ("loss", "per_view")))
        for align, normalize, weighted in DEPTH_CONFIGS:
            out = inverse_depth_forward(x["dl_depth"], x["dl_alpha"], x["dl_views"], x["dl_target" if weighted else "dl_target_sparse"],
                                        x["dl_weight"] if weighted else None, x["dl_affine"] if align == "given" else None,
                                        align=align, normalize=normalize, want=("loss", "per_view", "affine"))
            got.update(_bits(f"depth_{align}_{normalize}", out, ("loss", "per_view", "affine")))
    return got


def bilagrid_outputs(dev) -> dict:
    import torch
    from latentsplat_amd.bilagrid import tv_forward
    return _bits("bilagrid", {"tv": tv_forward(torch.from_numpy(grids_input()).to(dev))}, ("tv",))
