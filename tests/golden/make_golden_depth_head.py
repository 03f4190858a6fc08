#!/usr/bin/env python
"""Generate tests/golden/depth_head_*.npz by IMPORTING the reference's DepthPredictorMonocular
(src/model/encoder/epipolar/depth_predictor_monocular.py) and running it — forward and autograd
backward — on seeded inputs.  Only arrays travel; nothing of the reference is copied.

usage: python tests/golden/make_golden_depth_head.py /path/to/reference

Stubs: jaxtyping / e3nn placeholders and namespace packages as in tests/golden/make_golden.py, plus
package shims for src.model.encoder.common as in make_golden_adapter.py.

The uniforms.  The reference draws them inside forward with one torch.rand((b, v, r, srf, spp)); the
maker seeds the generator right before forward (`forward_seed`) and replays the same call under the same
seed to record them.

Seed condition, ASSERTED per case (another seed is taken otherwise): every uniform lies at least 1e-5
from every cumulative-sum edge that can change its index, and in the deterministic cases consecutive
probabilities among each row's k + 1 largest differ by at least 1e-5.  Under that condition float32
summation order cannot move an index, so the tests demand exact index equality with no exclusions.

The opacity-map cases get their expected opacity from the reference encoder's own map_pdf_to_opacity
(encoder_epipolar.py:113-126) divided by gaussians_per_pixel when that module imports under the stubs;
otherwise (`opacity_map_source` = "restatement") from the same formula evaluated in float64.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

D_IN = 16
MIN_GAP = 1e-5
CASES = {
    # name: (b, v, rays, S, F, k, deterministic, transmittance, opacity x_cfg or None, gaussians_per_pixel divisor)
    "stochastic": (2, 2, 48, 32, 1, 3, False, False, None, 1),
    "deterministic_two_surfaces": (1, 3, 25, 32, 2, 1, True, False, None, 1),
    "transmittance": (1, 2, 40, 8, 1, 3, False, True, None, 1),
    "ragged_three_surfaces": (1, 2, 30, 12, 3, 2, False, False, None, 1),
    "wide_64": (2, 2, 48, 64, 1, 3, False, False, None, 1),
    "opacity_map_sqrt2": (1, 2, 40, 32, 1, 3, False, False, 0.5, 3),
    # (no transmittance with an exponent below 1: the last bucket's quotient is 1 and the map's slope is infinite there)
    "opacity_map_half": (1, 2, 40, 16, 2, 3, False, False, -1.0, 3),
}


def import_reference(ref):
    import make_golden
    make_golden.REF = ref
    make_golden._install_stubs(make_golden._recording_module())
    common = types.ModuleType("src.model.encoder.common")
    common.__path__ = [os.path.join(ref, "src/model/encoder/common")]
    sys.modules["src.model.encoder.common"] = common
    dpm = importlib.import_module("src.model.encoder.epipolar.depth_predictor_monocular")
    try:
        enc = importlib.import_module("src.model.encoder.encoder_epipolar")
        opacity_map = enc.EncoderEpipolar.map_pdf_to_opacity
    except Exception as e:      # heavy imports (datasets, backbones) are not available under the stubs
        print("encoder_epipolar does not import under the stubs:", type(e).__name__, e)
        opacity_map = None
    return dpm.DepthPredictorMonocular, opacity_map


def run_case(Module, opacity_map, spec, seed):
    from tests import depth_head_ref as ref
    b, v, rays, S, F, k, det, trans, x_cfg, gpp = spec
    torch.manual_seed(seed)
    module = Module(D_IN, S, F, trans)
    with torch.no_grad():
        module.projection[1].weight.mul_(4.0)      # logits a few units apart: peaked and flat rows both occur
    features = torch.randn(b, v, rays, D_IN)
    near = 0.5 + torch.rand(b, v)
    far = near + 2.0 + 5.0 * torch.rand(b, v)
    logits = module.projection(features).detach().clone().requires_grad_()
    tail = torch.nn.Sequential()                   # forward() behind its projection: feed the recorded logits
    original, module.projection = module.projection, tail
    seen = {}
    sample = module.sampler.sample

    def recording_sample(pdf, deterministic, num_samples):      # the reference's own indices
        seen["index"], densities = sample(pdf, deterministic, num_samples)
        return seen["index"], densities

    module.sampler.sample = recording_sample
    forward_seed = seed + 1000
    torch.manual_seed(forward_seed)
    depth, density = module.forward(logits, near, far, det, k)
    torch.manual_seed(forward_seed)
    uniforms = torch.rand((b, v, rays, F, k))
    module.projection = original

    # the seed condition
    p, o, n, cdf = ref.distribution(logits.detach().reshape(b * v, rays, -1), F)
    index = (ref.forward(logits.detach().reshape(b * v, rays, -1), near.reshape(-1), far.reshape(-1), F,
                         uniforms=uniforms.reshape(b * v, rays, F, k), deterministic=det, samples=k)[2])
    if det:
        top = p.topk(min(k + 1, S), dim=-1).values
        margin = float((top[..., :-1] - top[..., 1:]).min())
    else:
        margin = float(ref.edge_gap(cdf, uniforms.reshape(b * v, rays, F, k)).min())
    if margin < MIN_GAP:
        return None, margin
    assert torch.equal(index.reshape(b, v, rays, F, k), seen["index"]), "the restated rule disagrees with the reference"

    source = "none"
    if x_cfg is None:
        opacity, exponent, scale = density, 1.0, 1.0
    else:
        exponent, scale = 2.0 ** x_cfg, 1.0 / gpp
        if opacity_map is not None:
            fake = types.SimpleNamespace(cfg=types.SimpleNamespace(
                opacity_mapping=types.SimpleNamespace(initial=x_cfg, final=x_cfg, warm_up=1)))
            opacity = opacity_map(fake, density, 0) / gpp
            source = "reference"
        else:
            x = density.double()
            opacity = (0.5 * (1 - (1 - x) ** exponent + x ** (1 / exponent)) / gpp).float()
            source = "restatement"
    gen = torch.Generator().manual_seed(seed + 2000)
    g_depth = torch.randn(depth.shape, generator=gen)
    g_opacity = torch.randn(opacity.shape, generator=gen)
    ((depth * g_depth).sum() + (opacity * g_opacity).sum()).backward()
    a = lambda t: t.detach().numpy()
    state = module.state_dict()
    return dict(
        features=a(features), weight=a(state["projection.1.weight"]), bias=a(state["projection.1.bias"]),
        logits=a(logits), near=a(near), far=a(far), uniforms=a(uniforms), depth=a(depth), opacity=a(opacity),
        index=index.reshape(b, v, rays, F, k).numpy().astype(np.int32), g_depth=a(g_depth), g_opacity=a(g_opacity),
        d_logits=a(logits.grad), state_dict_keys=np.array(sorted(state.keys())),
        surfaces=np.int32(F), deterministic=np.bool_(det), transmittance=np.bool_(trans),
        opacity_exponent=np.float64(exponent), opacity_scale=np.float64(scale), opacity_map_source=np.array(source),
        seed=np.int32(seed), forward_seed=np.int32(forward_seed), margin=np.float64(margin)), margin


def main(ref):
    Module, opacity_map = import_reference(ref)
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, spec in CASES.items():
        seed = 11
        while True:
            data, margin = run_case(Module, opacity_map, spec, seed)
            if data is not None:
                break
            print(f"{name}: seed {seed} gives a margin of {margin:.2e} < {MIN_GAP:.0e}, trying the next")
            seed += 1
        assert data["margin"] >= MIN_GAP
        np.savez_compressed(os.path.join(out_dir, f"depth_head_{name}.npz"), **data)
        print(f"{name}: seed {seed}, margin {margin:.2e}, depth {data['depth'].shape}, "
              f"opacity map from {data['opacity_map_source']}")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    main(sys.argv[1])
