#!/usr/bin/env python
"""bench.py — headline measurement of the rasterizer hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full [--full-json PATH]]

A *step* is one pass of the hot path (preprocess -> bin -> per-tile sort -> composite) over one
batch of synthetic input: ``--views`` target views (default 16) of one seeded random-init scene of
``--gaussians`` latent Gaussians (default 300 000; 4 feature channels + opacity, no colour) at
256x256 — BASELINE.json configs[1].  Inputs are resident in HBM before the timed region; the scene
is shared by the views (scene-level inputs, per-view cameras), as in the decoder's training use.
``value`` = views rendered per second by the whole job (all ranks).  With N > 1 every rank renders
its own scene (disjoint seeds), there is no data-path collective: weak scaling.

A plain run sets up, warms up, times exactly K steps and prints one JSON line (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` = milliseconds of one timed step, ...).  ``--dump-outputs DIR`` then also
writes what the last timed step returned (rank 0: color / feature / mask / depth / radii, whichever exist) as
``DIR/<name>.npy`` in float32; the inputs are seeded, so two builds can be compared output for output.

With ``--full`` the same JSON line also carries
  * ``fwdbwd``   : configs[2] (forward + backward) timed the same way right after the headline run;
  * ``roofline`` : the dominant kernel (k_render_fwd) against the HBM roofline — algorithmic bytes
                   of that kernel per launch / its mean duration measured live with hipEvents
                   on the launch stream (lsr_profile_* hook), see DESIGN.md §Measurement;
  * ``cpu_baseline`` : the CPU oracle (oracle/raster_oracle.c, OpenMP) timed on this box's host
                   cores on a bounded sample of the same workload (rank 0, N = 1 only);
and the decoder / adapter / latent / chained-path, pipelined and latency legs and the parity gate below; the whole
dictionary goes to ``--full-json`` (default ``bench_out/bench_full.json``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


def build_inputs(G, V, size, device, seed, **scene_kw):
    """Scene-level inputs of one scene / V views, resident on the device: shared means (G,3),
    3x3 covariances, opacities and 4-channel latent features; per-view cameras in the (V,44) view
    table (built by the library's own kernel, scene scale 1/near included)."""
    from latentsplat_amd.rasterizer import build_view_table
    from latentsplat_amd.synthetic import make_scene
    sc = make_scene(G, image_size=size, views=V, color_sh_degree=None, feature_channels=4,
                    feature_sh_degree=0, seed=seed, **scene_kw).to(device)
    views = build_view_table(sc.extrinsics, sc.intrinsics, sc.near, sc.far, torch.zeros(3, device=device), True)
    features = (0.5 + 0.28209479177387814 * sc.feature_sh[..., 0]).contiguous()   # degree-0 latent SH
    return dict(views=views, means=sc.means.contiguous(), cov=sc.covariances.contiguous(),
                opac=sc.opacities[:, None].contiguous(), features=features)


def cpu_baseline(G, size, seed, budget_s=12.0):
    """Oracle (port) on the host cores: whole forward of single views of the same workload."""
    from oracle import oracle as orc
    from tests import util
    from latentsplat_amd.synthetic import make_scene
    sc = make_scene(G, image_size=size, views=1, color_sh_degree=None, feature_channels=4, seed=seed)
    bi = util.boundary_inputs(sc, size, size)
    util.oracle_forward(bi, 0)  # warm-up (page in, build)
    n, t0 = 0, time.perf_counter()
    while True:
        util.oracle_forward(bi, 0)
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s or n >= 50:
            break
    # forward + backward of the same view (configs[2]'s CPU side): few repetitions, the backward's
    # scatter of per-Gaussian gradients is the slow part of the port
    import numpy as np
    o = util.oracle_forward(bi, 0)
    gf = np.random.default_rng(7).normal(size=(4, size, size)).astype(np.float32)
    nb, t1 = 0, time.perf_counter()
    while nb < 3 and (nb == 0 or time.perf_counter() - t1 < 8.0):
        util.oracle_backward(bi, 0, util.oracle_forward(bi, 0), None, gf)
        nb += 1
    el_b = time.perf_counter() - t1
    return dict(value=n / el, unit="views/s", cores=os.cpu_count(), kind="port",
                sample=f"{n} forward renders of the same {G}-Gaussian {size}x{size} view "
                       f"(oracle/raster_oracle.c, gcc -O2 -fopenmp, {os.cpu_count()} threads)",
                fwdbwd_value=nb / el_b, fwdbwd_sample=f"{nb} forward+backward passes of that view")


def kernel_source_hash():
    """First 16 hex digits of sha256(render_forward.hip + lsr_blend.h): what profiles/traffic_render_forward.json is tied to."""
    import hashlib
    h = hashlib.sha256()
    for f in ("render_forward.hip", "lsr_blend.h"):
        with open(os.path.join(ROOT, "latentsplat_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def parity_gate(G, V, size, seed, dev):
    """"parity gates reported next to every timing".  OUTSIDE every timed region (part of the
    cpu_baseline leg: rank 0, N = 1): the bench workload — the same seeded scene, all V views in ONE call through the C ABI,
    i.e. the launch shapes the timings above measured — against the CPU oracle for view 0 and the last view: tile
    offsets and depth-sorted lists bit for bit, rendered latent / mask within 1e-4 abs outside the oracle's fragile
    (decision-boundary) pixels."""
    import numpy as np
    from tests import util
    from latentsplat_amd.synthetic import make_scene
    sc = make_scene(G, image_size=size, views=V, color_sh_degree=None, feature_channels=4, feature_sh_degree=0, seed=seed)
    bi = util.boundary_inputs(sc, size, size)
    run = util.HipRun(bi, dev, shared_means=True)      # (equal near planes: the scaled scene is the same for every view)
    ts, pl, T = run.tile_start(), run.point_list(), run.T
    exact, worst, over, frag_px, pairs = True, 0.0, 0, 0, 0
    checked = sorted({0, V - 1})
    for v in checked:
        o = util.oracle_forward(bi, v)
        pairs += int(o["P"])
        exact = exact and bool(np.array_equal(run.radii[v].cpu().numpy(), o["radii"]))
        exact = exact and bool(np.array_equal(np.diff(ts[v * T:(v + 1) * T + 1]), o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]))
        exact = exact and bool(np.array_equal(pl[ts[v * T]:ts[(v + 1) * T]], o["point_list"]))
        fragile = np.zeros(size * size, bool)
        if len(o["fragile"]):
            fragile[o["fragile"][:, 0].astype(np.int64)] = True
        frag_px += int(fragile.sum())
        for got, want in ((run.feat_out[v].cpu().numpy(), o["feature"]), (run.mask_out[v].cpu().numpy()[None], o["mask"].reshape(1, size, size))):
            err = np.abs(got - want).reshape(got.shape[0], -1).max(0)
            worst = max(worst, float(err[~fragile].max()))
            over += int((err[~fragile] > 1e-4).sum())
    # the timed path bins only the pairs that can reach a pixel (ABI v9 LSR_FWD_REACHED_ONLY, the autograd op's default): the same
    # call with the bit set must give the images, final_T / n_contrib and half-tile list lengths of the published-list run above
    from latentsplat_amd import _lib
    red = util.HipRun(bi, dev, shared_means=True, forward_flags=_lib.FWD_REACHED_ONLY)
    same = bool(torch.equal(red.feat_out, run.feat_out) and torch.equal(red.mask_out, run.mask_out) and torch.equal(red.depth_out, run.depth_out)
                and np.array_equal(red.n_contrib(), run.n_contrib()) and np.array_equal(red.half_count(), run.half_count()) and red.P < run.P)
    return dict(lists_bit_exact=exact, max_abs_err=worst, pixels_over_tol=over, fragile_pixels_excluded=frag_px,
                reached_only_bitwise_equal=same, pairs_published=int(run.P), pairs_binned=int(red.P),
                views_checked=checked, pairs_checked=pairs, tol=1e-4, ok=bool(exact and over == 0 and same),
                what=f"{V}-view call of the bench scene through the C ABI vs oracle/raster_oracle.c (outside the timed regions)")


def cpu_baseline_next_rows(budget_s=4.0):
    """cpu_baseline leg for the §8(f) rows: the torch-CPU oracles (= the reference's own op chains,
    oracle/adapter_oracle.py and oracle/latent_oracle.py) on the host cores, same shapes as
    adapter_step / latent_step, forward + backward."""
    from oracle import adapter_oracle as ao
    from oracle import latent_oracle as lo
    threads = min(32, os.cpu_count())      # many small elementwise ops: more threads only thrash
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(99)
    cams, rays, S = 2, 65536, 3
    E = torch.eye(4).repeat(cams, 1, 1)
    K = torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]]).repeat(cams, 1, 1)
    coords = torch.rand(cams, rays, 2, generator=g).requires_grad_()
    depths = (0.5 + 20 * torch.rand(cams, rays, S, generator=g)).requires_grad_()
    rs = torch.randn(cams, rays, 3, generator=g).requires_grad_()
    rq = torch.randn(cams, rays, 4, generator=g).requires_grad_()

    def adapter():
        m, c, _, _ = ao.adapter_geometry(E, K, coords, depths, rs, rq, (256, 256), 0.5, 15.0)
        (m.sum() + c.sum()).backward()

    b, v, C, Sz = 4, 4, 4, 256
    feats = torch.randn(b, v, C, Sz, Sz, generator=g).requires_grad_()
    mask, color = torch.rand(b, v, Sz, Sz, generator=g), torch.rand(b, v, 3, Sz, Sz, generator=g)
    noise = torch.randn(b, v, C, Sz, Sz, generator=g)

    def latent():
        o = lo.latent_epilogue(feats, mask, noise, color, 8)
        (o["z"].sum() + o["skip"].sum()).backward()

    res = {}
    for name, fn in (("adapter", adapter), ("latent", latent)):
        fn()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s and n < 50:
            fn()
            n += 1
        res[name] = dict(ms_per_step=1e3 * (time.perf_counter() - t0) / n, cores=threads, kind="port",
                         sample=f"{n} forward+backward passes of the torch-CPU oracle at the same shape")
    return res


def timed_region(step, steps, warmup, dist=None, device_sync=lambda: None, reduce_device="cpu"):
    """W untimed warm-up steps, then EXACTLY `steps` steps bracketed by barrier + device sync on
    both sides; returns the MAX elapsed seconds over ranks (every rank gets the same number)."""
    def barrier():
        if dist is not None:
            dist.barrier()
        device_sync()

    for _ in range(warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    device_sync()
    el = time.perf_counter() - t0
    barrier()
    if dist is not None:
        t = torch.tensor([el], device=reduce_device, dtype=torch.float64)
        every = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(every, t)
        PER_RANK_SECONDS[:] = [float(x.item()) for x in every]     # last timed region, every rank's own time
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    else:
        PER_RANK_SECONDS[:] = [el]
    return el


PER_RANK_SECONDS: list = []


def whole_job_views_per_s(views_per_step, steps, world, elapsed_max):
    """Weak scaling: every rank renders its own `views_per_step` views per step (disjoint scenes,
    no data-path collective), so the job rate is the total view count over the slowest rank's time."""
    return views_per_step * steps * world / elapsed_max


def rank_seed(base, rank):
    return base + rank


DUMP_BUDGET_BYTES = 60 * 10**6     # the .npy payloads of one --dump-outputs, headers aside (< 64 MB in all)


def dump_outputs(out_dir, named, budget=DUMP_BUDGET_BYTES, seed=0):
    """Write every tensor of `named` that is not None as out_dir/<name>.npy in float32 (radii: int32, exact in float32).
    Should the whole exceed `budget`, each array keeps its proportional share of it as a fixed sample of its flattened
    elements (seeded, sorted indices: the same shapes give the same sample in every run)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: v.detach().float().cpu().numpy() for k, v in named.items() if v is not None}
    total = sum(4 * a.size for a in arrays.values())
    for i, (name, a) in enumerate(arrays.items()):
        if total > budget and a.size:
            keep = max(1, a.size * budget // total)
            if keep < a.size:
                idx = np.sort(np.random.default_rng(seed + i).choice(a.size, keep, replace=False))
                a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
    return sorted(arrays)


def decoder_step_timing(dev, steps=40, scenes=1, encoder_shaped=False):
    """BASELINE configs[3] shape through the decoder surface: DecoderSplattingCUDA.forward
    (+ backward of an MSE-like loss on colour and latent mean) for batch_size 1 x 4 target views,
    G = 393 216 Gaussians (2 context views x 256^2 x 3), colour SH degree 4 + 4-channel latent SH
    degree 2 — the call the reference's training_step makes (model_wrapper.py:361-371).
    encoder_shaped: the Gaussians the reference's encoder really emits (synthetic.make_encoder_scene: pixel-aligned, three per
    ray of two context views, in ray order: encoder_epipolar.py:184-236, gaussian_adapter.py:75-114) instead of make_scene's
    random cloud."""
    from latentsplat_amd import decoder as dec
    from latentsplat_amd.synthetic import make_encoder_scene, make_scene
    if encoder_shaped:
        scs = [make_encoder_scene(seed=4321 + i).to(dev) for i in range(scenes)]
    else:
        scs = [make_scene(393_216, image_size=256, views=4, color_sh_degree=4, feature_channels=4,
                          feature_sh_degree=2, seed=4321 + i).to(dev) for i in range(scenes)]
    st = lambda name: torch.stack([getattr(sc, name) for sc in scs])
    leaf = lambda name: st(name).contiguous().requires_grad_(True)
    gauss = dec.Gaussians(leaf("means"), leaf("covariances"), leaf("opacities"), leaf("color_sh"), leaf("feature_sh"))
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), [0.0, 0.0, 0.0]).to(dev)
    args = (gauss, st("extrinsics"), st("intrinsics"), st("near"), st("far"), (256, 256))
    gc = torch.randn((scenes, 4, 3, 256, 256), device=dev)
    gf = torch.randn((scenes, 4, 4, 256, 256), device=dev)
    leaves = (gauss.means, gauss.covariances, gauss.opacities, gauss.color_harmonics, gauss.feature_harmonics)

    def fwd():
        with torch.no_grad():
            d.forward(*args)

    def fwdbwd():
        out = d.forward(*args)
        torch.autograd.backward([out.color, out.feature_posterior.mean], [gc, gf])
        for t in leaves:
            t.grad = None

    res = {}
    from latentsplat_amd import rasterizer as rz
    for name, fn in (("forward", fwd), ("forward_backward", fwdbwd)):
        before = dict(rz.SPECULATION_STATS)
        # two timed regions, BOTH reported (`ms_per_step_regions`); `ms_per_step` is the first, as the headline's single region
        # is (round 5 reported the better of the two after one run caught a single ~30 ms stall inside a 40-step region)
        els = [timed_region(fn, steps, 10, None, lambda: torch.cuda.synchronize(dev)) for _ in range(2)]
        el = els[0]
        # which host protocol the calls of this leg (warm-up included) took: speculative launches, exact (two-half) forwards,
        # speculative launches that had to be re-run — a leg that re-runs shows up here, not just as a slow number
        res[name] = dict(ms_per_step=1e3 * el / steps, ms_per_step_regions=[1e3 * e / steps for e in els], views_per_s=4 * scenes * steps / el,
                         host_protocol={k: rz.SPECULATION_STATS[k] - before[k] for k in before})   # (both regions and their warm-ups)
    res["config"] = (f"configs[{3 if scenes == 1 else 4}] per-GPU shape: {scenes} scene(s) x 4 views, 393216 Gaussians each, "
                     "colour SH deg 4 + 4-ch latent SH deg 2, 256x256; "
                     + ("encoder-shaped scene (pixel-aligned, 3 per ray of 2 context views, ray order)" if encoder_shaped else "random cloud"))
    # per-kernel times of the same step (hipEvents inside the library), and the SH kernels against the HBM roofline:
    # the path's only kernels that exist because of the reference's payload (degree-4 colour + latent harmonics).
    # Algorithmic bytes per launch (all scenes): coefficients (75 + 36 floats per Gaussian) read once per scene,
    # per (view, Gaussian) the visibility word, the position and the clamp byte; backward: the coefficients again, their
    # gradients written once per scene, the mean gradient.  The 32-byte payload half of the records (written by the
    # forward, its gradient read by the backward) is only touched for visible (view, Gaussian) pairs and is NOT
    # counted: the fractions are lower bounds.
    from latentsplat_amd import _lib
    _lib.profile_read()
    _lib.profile_enable(True)
    for _ in range(5):
        fwdbwd()
    torch.cuda.synchronize(dev)
    _lib.profile_enable(False)
    prof = _lib.profile_read()
    G, V, coeff = 393_216, 4, (25 * 3 + 9 * 4) * 4
    # (round 4: the forward SH pass runs inside the projection kernel for this shape — `preprocess` below is that fused
    # kernel: coefficients + geometry in, one 64-byte record per visible (view, Gaussian) [~0.7 of them], the 12-byte bin
    # record, the radius and the clamp byte out)
    sh_bytes = {"sh_forward": scenes * (G * coeff + V * G * (4 + 12 + 1)),
                "preprocess": scenes * (G * (coeff + 12 + 36 + 4) + V * G * (12 + 4 + 1) + int(0.7 * V * G) * 64),
                "sh_backward": scenes * (2 * G * coeff + V * G * (4 + 12 + 1) + G * 12)}
    res["kernel_ms"] = {k: round(ms / n, 4) for k, (ms, n) in prof.items() if n}
    res["sh_roofline"] = {k: dict(ms=round(prof[k][0] / prof[k][1], 4), algorithmic_bytes=nb,
                                  frac=round(nb / (prof[k][0] / prof[k][1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
                          for k, nb in sh_bytes.items() if prof.get(k, (0, 0))[1]}
    return res


def path_step_timing(dev, steps=40):
    """The three stages chained as the training step runs them (model_wrapper.py:361-385) at configs[3]'s shape:
    Gaussian adapter tail (2 context cameras x 256^2 rays x 3 samples = 393 216 Gaussians, packed covariances)
    -> DecoderSplattingCUDA.forward (1 x 4 views, colour SH 4 + latent SH 2) -> posterior sample + 1/8 rescale +
    skip concatenation, gradients from the latent / skip / colour heads back to the raw adapter inputs
    (tests/test_path_gpu.py checks the same chain against the chained CPU oracles)."""
    from latentsplat_amd import decoder as dec
    from latentsplat_amd.decoder.latent_epilogue import decoder_output_epilogue
    from latentsplat_amd.gaussian_adapter import adapter_geometry
    from latentsplat_amd.synthetic import make_scene
    cams, rays, S, size = 2, 65536, 3, 256
    G = cams * rays * S
    g = torch.Generator().manual_seed(77)
    ys, xs = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    coords = ((torch.stack([xs, ys], -1).reshape(rays, 2).float() + 0.5) / size)[None].repeat(cams, 1, 1).to(dev).requires_grad_()
    E = torch.eye(4).repeat(cams, 1, 1)
    E[1, 0, 3] = 0.3
    K = torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]]).repeat(cams, 1, 1)
    depths = (1.5 + 8.0 * torch.rand(cams, rays, S, generator=g)).to(dev).requires_grad_()
    raw = torch.randn(cams, rays, 7, generator=g).to(dev).requires_grad_()
    sc = make_scene(G, image_size=size, views=4, color_sh_degree=4, feature_channels=4, feature_sh_degree=2, seed=77).to(dev)
    E, K = E.to(dev), K.to(dev)
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg(name="splatting_cuda"), [0.0, 0.0, 0.0]).to(dev)
    noise = torch.randn(1, 4, 4, size, size, device=dev)
    gz = torch.randn(1, 4, 4, size // 8, size // 8, device=dev)
    gs = torch.randn(1, 4, 7, size, size, device=dev)
    gc = torch.randn(1, 4, 3, size, size, device=dev)

    def chain():
        means, cov, _, _ = adapter_geometry(E, K, coords, depths, raw, (size, size), 0.5, 15.0)
        gauss = dec.Gaussians(means.reshape(1, G, 3), cov.reshape(1, G, 3, 3), sc.opacities[None], sc.color_sh[None], sc.feature_sh[None])
        out = d.forward(gauss, sc.extrinsics[None], sc.intrinsics[None], sc.near[None], sc.far[None], (size, size))
        return out, decoder_output_epilogue(out, 8, noise=noise)

    def fwd():
        with torch.no_grad():
            chain()

    def fwdbwd():
        out, ep = chain()
        torch.autograd.backward([ep.z, ep.skip_z, out.color], [gz, gs, gc])
        coords.grad = depths.grad = raw.grad = None

    res = {}
    for name, fn in (("forward_ms", fwd), ("forward_backward_ms", fwdbwd)):
        el = timed_region(fn, steps, 10, None, lambda: torch.cuda.synchronize(dev))
        res[name] = 1e3 * el / steps
    res["config"] = "configs[3] shape: adapter tail (393216 Gaussians) -> decoder (1 x 4 views, SH 4 + latent SH 2, 256x256) -> latent epilogue (factor 8)"
    return res


def adapter_step_timing(dev, steps=20):
    """the Gaussian adapter tail at the configs[3] shape (2 context cameras x 256^2
    rays x 3 depth samples = 393 216 Gaussians), raw parameters read as a strided view of the
    encoder's 156-float Linear output.  HBM roofline of the two kernels from their algorithmic
    bytes (inputs read once, outputs written once) and the hipEvent times inside the library."""
    from latentsplat_amd import _lib
    from latentsplat_amd.gaussian_adapter import adapter_geometry
    cams, rays, S, width = 2, 65536, 3, 156
    g = torch.Generator(device="cpu").manual_seed(99)
    E = torch.eye(4).repeat(cams, 1, 1)
    E[:, :3, 3] = torch.randn(cams, 3, generator=g)
    K = torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]]).repeat(cams, 1, 1)
    coords = torch.rand(cams, rays, 2, generator=g).to(dev).requires_grad_()
    depths = (0.5 + 20 * torch.rand(cams, rays, S, generator=g)).to(dev).requires_grad_()
    full = torch.randn(cams, rays, width, generator=g).to(dev).requires_grad_()
    E, K = E.to(dev), K.to(dev)
    gm = torch.randn(cams, rays, S, 3, device=dev)
    gc = torch.randn(cams, rays, S, 6, device=dev)

    def fwd():
        with torch.no_grad():
            adapter_geometry(E, K, coords, depths, full[..., 2:], (256, 256), 0.5, 15.0, packed_covariance=True)

    def fwdbwd():
        m, c, _, _ = adapter_geometry(E, K, coords, depths, full[..., 2:], (256, 256), 0.5, 15.0, packed_covariance=True)
        torch.autograd.backward([m, c], [gm, gc])
        coords.grad = depths.grad = full.grad = None

    res = {}
    for name, fn in (("forward", fwd), ("forward_backward", fwdbwd)):
        el = timed_region(fn, steps, 3, None, lambda: torch.cuda.synchronize(dev))
        res[name] = dict(ms_per_step=1e3 * el / steps)
    _lib.profile_read()
    _lib.profile_enable(True)
    for _ in range(5):
        fwdbwd()
    torch.cuda.synchronize(dev)
    _lib.profile_enable(False)
    prof = _lib.profile_read()
    rows = cams * rays
    # 64-byte lines actually touched for the 7 strided raw floats: 28 B straddle <= 2 lines
    bytes_fwd = rows * (4 * (7 + 2 + S) + 4 * (S * (3 + 6 + 3) + 4))
    bytes_bwd = rows * (4 * (7 + 2 + S) + 4 * S * (3 + 6) + 4 * (2 + S + 7))
    for key, nbytes in (("adapter_forward", bytes_fwd), ("adapter_backward", bytes_bwd)):
        ms, n = prof.get(key, (0.0, 0))
        if n:
            res[key] = dict(kernel_ms=ms / n, algorithmic_bytes=nbytes, achieved_GBs=nbytes / (ms / n * 1e-3) / 1e9,
                            frac=nbytes / (ms / n * 1e-3) / 1e9 / HBM_PEAK_GBS)
    res["config"] = "configs[3] shape: 2 context cameras x 65536 rays x 3 samples = 393216 Gaussians, packed cov6, raw row stride 156 floats"
    return res


def latent_step_timing(dev, steps=20):
    """posterior sample + antialiased 1/8 rescale + skip concatenation for one
    per-GPU batch of BASELINE configs[4] (16 views x 4 latent channels x 256^2, RGB skip)."""
    from latentsplat_amd import _lib
    from latentsplat_amd.decoder.latent_epilogue import sample_rescale_skip
    b, v, C, S, f = 4, 4, 4, 256, 8
    feats = torch.randn(b, v, C, S, S, device=dev).requires_grad_()
    mask = torch.rand(b, v, S, S, device=dev)
    color = torch.rand(b, v, 3, S, S, device=dev)
    noise = torch.randn(b, v, C, S, S, device=dev)
    gz = torch.randn(b, v, C, S // f, S // f, device=dev)
    gs = torch.randn(b, v, 3 + C, S, S, device=dev)

    def fwd():
        with torch.no_grad():
            sample_rescale_skip(feats, mask, color, f, noise=noise)

    def fwdbwd():
        ep = sample_rescale_skip(feats, mask, color, f, noise=noise)
        torch.autograd.backward([ep.z, ep.skip_z], [gz, gs])
        feats.grad = None

    res = {}
    for name, fn in (("forward", fwd), ("forward_backward", fwdbwd)):
        el = timed_region(fn, steps, 3, None, lambda: torch.cuda.synchronize(dev))
        res[name] = dict(ms_per_step=1e3 * el / steps)
    _lib.profile_read()
    _lib.profile_enable(True)
    for _ in range(5):
        fwdbwd()
    torch.cuda.synchronize(dev)
    _lib.profile_enable(False)
    prof = _lib.profile_read()
    V, px = b * v, S * S
    bytes_fwd = 4 * V * (px * (C + 1 + C + 3) + px * (3 + C) + px + C * px // (f * f))     # in: feat, mask, noise, colour; out: skip, logvar, z
    bytes_bwd = 4 * V * (px * C + C * px // (f * f) + px * C)                               # in: g_skip latent part, g_z; out: d_features
    for key, nbytes in (("latent_forward", bytes_fwd), ("latent_backward", bytes_bwd)):
        ms, n = prof.get(key, (0.0, 0))
        if n:
            res[key] = dict(kernel_ms=ms / n, algorithmic_bytes=nbytes, achieved_GBs=nbytes / (ms / n * 1e-3) / 1e9,
                            frac=nbytes / (ms / n * 1e-3) / 1e9 / HBM_PEAK_GBS)
    res["config"] = "configs[4] per-GPU batch: 16 views x 4 latent channels x 256x256, factor 8, RGB skip"
    return res


def latency_timing(dev, G, S, seed, iters=30):
    """Latency of small view batches at the configs[1] scene (the reference renders ONE view per
    rasterizer call, cuda_splatting.py:124-162, and times the decoder per view with a host
    wall-clock and no device synchronisation inside, src/misc/benchmarker.py:11-37 /
    model_wrapper.py:542-550).  For V = 1 and V = 4, ms per call with a device synchronisation after
    EVERY call (latency) and over a stream of calls (throughput), for
      sync    : lsr_forward_prepare + lsr_forward_render (one host wait for the pair count),
      nosync  : lsr_forward_nosync with a pair capacity of 1.5x the measured count,
      graph   : the nosync launch sequence captured once in a hipGraph (torch.cuda.graph) and replayed;
    plus the zero-touch drop-in: a Python loop constructing GaussianRasterizationSettings /
    GaussianRasterizer per view exactly like the reference does, seconds per view Benchmarker-style."""
    import diff_gaussian_rasterization as dgr
    from latentsplat_amd.rasterizer import last_forward_status, rasterize_views
    res = {}
    sync = lambda: torch.cuda.synchronize(dev)
    for V in (1, 4):
        inp = build_inputs(G, V, S, dev, seed)
        call = lambda **kw: rasterize_views(inp["views"], S, S, 0, inp["means"], inp["cov"], inp["opac"], features=inp["features"], **kw)
        with torch.no_grad():
            call(); st = last_forward_status()
            kw = dict(pair_capacity=int(1.5 * st["num_pairs"]), max_tile_hint=int(st["max_tile_pairs"]))
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    call(**kw)
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gout = call(**kw)
            modes = dict(sync=lambda: call(), nosync=lambda: call(**kw), graph=graph.replay)
            r = {}
            for name, fn in modes.items():
                for _ in range(3):
                    fn()
                sync()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn(); sync()
                lat = (time.perf_counter() - t0) / iters
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                sync()
                thr = (time.perf_counter() - t0) / iters
                r[name] = dict(ms_per_call_synced=1e3 * lat, ms_per_call_streamed=1e3 * thr,
                               ms_per_view_streamed=1e3 * thr / V)
            r["overflow_after_graph"] = bool(last_forward_status()["overflow"])
            res[f"views_{V}"] = r
            del graph, gout
    # ---- the reference's own call pattern, untouched: one GaussianRasterizer per view ----
    from latentsplat_amd.decoder import cuda_splatting as cs
    from latentsplat_amd.decoder.geometry import get_fov
    from latentsplat_amd.synthetic import make_scene
    V = 4
    sc = make_scene(G, image_size=S, views=V, color_sh_degree=None, feature_channels=4, seed=seed).to(dev)
    means = sc.means[None].expand(V, -1, -1)
    covs = sc.covariances[None].expand(V, -1, -1, -1)
    ext, nr, fr, means, covs = cs._scale_scene(sc.extrinsics, sc.near, sc.far, means, covs)
    fov_x, fov_y = get_fov(sc.intrinsics).unbind(-1)
    cams = cs._cameras(ext, nr, fr, fov_x, fov_y)
    cov6 = cs._pack_covariances(covs).contiguous()
    feats = (0.5 + 0.28209479177387814 * sc.feature_sh[..., 0]).contiguous()
    opac = sc.opacities[:, None].contiguous()
    bg = torch.zeros(3, device=dev)

    def per_view_loop():
        outs = []
        for i in range(V):
            settings = dgr.GaussianRasterizationSettings(
                image_height=S, image_width=S, tanfovx=cams.tan_fov_x[i].item(), tanfovy=cams.tan_fov_y[i].item(), bg=bg,
                scale_modifier=1.0, viewmatrix=cams.view_matrix[i], projmatrix=cams.full_projection[i], sh_degree=0,
                campos=cams.campos[i], prefiltered=False, debug=False)
            rasterizer = dgr.GaussianRasterizer(settings)
            image, feature_map, mask, depth_map, _ = rasterizer(
                means3D=means[i], means2D=torch.zeros_like(means[i]), shs=None, colors_precomp=None, features=feats,
                opacities=opac, cov3D_precomp=cov6[i])
            outs.append(feature_map)
        return torch.stack(outs)

    with torch.no_grad():
        for _ in range(3):
            per_view_loop()
        sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            per_view_loop()
        host = (time.perf_counter() - t0) / (iters * V)       # Benchmarker semantics: host clock, no device sync
        sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            per_view_loop()
        sync()
        full = (time.perf_counter() - t0) / (iters * V)
    res["dropin_per_view_loop"] = dict(
        seconds_per_view_benchmarker=host, seconds_per_view_device_complete=full, views=V,
        note="GaussianRasterizationSettings + GaussianRasterizer constructed per view, two .item() reads per view, "
             "exactly the call pattern of cuda_splatting.py:124-162; 'benchmarker' = host wall-clock without a final "
             "device synchronisation (src/misc/benchmarker.py:16-23)")
    res["config"] = f"configs[1] scene: {G} Gaussians, 4-ch features, {S}x{S}; {iters} calls per figure"
    return res


def pipelined_timing(dev, inp, V, S, steps, warmup):
    """Throughput of the SAME steps when the caller removes the host from the loop: the no-sync forward
    (pair capacity 1.5x the measured count) issued (a) back to back on one stream, (b) round-robin on
    two HIP streams, so that the memory / latency-bound front half of batch i+1 (preprocess, scan,
    scatter, sort) runs beside the VALU-bound compositing of batch i and fills its load-imbalance tail.
    Independent batches only (inference / evaluation loops); a training step serialises on its loss.
    Reported next to the headline, which stays the default synchronous call on one stream."""
    from latentsplat_amd.rasterizer import last_forward_status, rasterize_views
    sync = lambda: torch.cuda.synchronize(dev)
    res = {}
    with torch.no_grad():
        call = lambda **kw: rasterize_views(inp["views"], S, S, 0, inp["means"], inp["cov"], inp["opac"], features=inp["features"], **kw)
        call(); st = last_forward_status()
        kw = dict(pair_capacity=int(1.5 * st["num_pairs"]), max_tile_hint=int(st["max_tile_pairs"]))
        streams = [torch.cuda.Stream(dev) for _ in range(2)]
        for name, n_streams in (("one_stream_nosync", 1), ("two_streams_nosync", 2), ("two_streams_default", 2)):
            if name == "two_streams_default":      # the default (speculative) forward: the host waits for each call's pair count
                kw = {}                            # and issues the next call on the other stream meanwhile
            def run(k):
                # (only the last result of each stream stays referenced: keeping all k alive made the caching allocator
                # grow by ~44 MB of outputs per step inside the timed loop — hipMalloc, an implicit device synchronisation)
                keep = [None] * n_streams
                for i in range(k):
                    with torch.cuda.stream(streams[i % n_streams]):
                        keep[i % n_streams] = call(**kw)
                return keep
            for st_ in streams:
                st_.wait_stream(torch.cuda.current_stream(dev))
            run(warmup); sync()
            t0 = time.perf_counter()
            outs = run(steps)
            sync()
            el = time.perf_counter() - t0
            res[name] = dict(ms_per_step=1e3 * el / steps, views_per_s=V * steps / el)
            del outs
        res["overflow"] = bool(last_forward_status()["overflow"])
    return res


def cpu_baseline_torch(budget_s=8.0):
    """Second CPU baseline (SURVEY.md §8(d) "Config #1 always"): the differentiable PyTorch-CPU oracle behind the
    GaussianRasterizer-shaped API (oracle/torch_oracle.py) on BASELINE configs[0] itself — 10 000 Gaussians,
    one 64x64 view, RGB SH degree 0 — forward + backward, all host cores.  It evaluates pixels x Gaussians
    densely, so it does not scale to the 300 k scene; the C/OpenMP port above is the baseline of the headline."""
    from oracle import torch_oracle as to
    from tests import util
    from latentsplat_amd.synthetic import make_scene
    threads = os.cpu_count()
    torch.set_num_threads(threads)
    sc = make_scene(10_000, image_size=64, views=1, color_sh_degree=0, feature_channels=None, seed=5)
    bi = util.boundary_inputs(sc, 64, 64)
    c = bi["cams"]
    args = lambda: (64, 64, float(c.tan_fov_x[0]), float(c.tan_fov_y[0]), bi["bg"][0], c.view_matrix[0], c.full_projection[0],
                    c.campos[0], 0, bi["means"][0].clone().requires_grad_(True), bi["cov6"][0].clone().requires_grad_(True),
                    bi["opac"].clone().requires_grad_(True))

    def fwdbwd():
        a = args()
        out = to.rasterize(*a, shs=bi["shs"].clone().requires_grad_(True))
        out[0].sum().backward()

    fwdbwd()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s and n < 20:
        fwdbwd()
        n += 1
    el = time.perf_counter() - t0
    return dict(value=n / el, unit="views/s (forward+backward)", cores=threads, kind="port",
                sample=f"{n} forward+backward passes of oracle/torch_oracle.py on BASELINE configs[0]: 10000 Gaussians, 64x64, RGB SH "
                       "degree 0 (dense pixels x Gaussians autograd restatement; does not scale to the 300k scene)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--clock-warmup", type=float, default=0.5,
                    help="seconds of untimed steps before the W warm-up steps: the shader clock of an idle MI355X dips to "
                         "~1.85 GHz during the first ~10 ms of load before it settles at 2.4 GHz (tools/clock_experiment.py)")
    ap.add_argument("--views", type=int, default=16, help="views per step (batch of the hot path)")
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every other leg (per-kernel times, rooflines, fwd+bwd, decoder / adapter / latent / "
                         "path steps, pipelined and latency legs, CPU baselines, parity gate); off: the headline alone")
    ap.add_argument("--full-json", metavar="PATH", default=os.path.join(ROOT, "bench_out", "bench_full.json"),
                    help="--full: where the whole result dictionary is written")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines and the parity gate")
    ap.add_argument("--no-bwd", action="store_true", help="--full: skip every forward+backward leg")
    ap.add_argument("--no-latency", action="store_true", help="--full: skip the V=1 / V=4 latency section (profiling runs: keeps one launch shape per kernel)")
    args = ap.parse_args()

    # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, the same
    # command the driver would issue), so that a plain invocation can never silently measure one GPU and call it N
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s) (WORLD_SIZE); refusing to report "
                         f"a number for a GPU count that did not run")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    if not os.environ.get("LSR_BENCH_SHARE_GPU") == "1" and torch.cuda.device_count() < (world if world > 1 else 1):
        raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} visible GPU(s)")
    # LSR_BENCH_SHARE_GPU=1: smoke test of the multi-process path on a ONE-GPU box (every rank on cuda:0,
    # rendezvous and the scalar reductions over gloo).  Never set by the driver; numbers of such a run mean nothing.
    share_gpu = os.environ.get("LSR_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from latentsplat_amd import _lib
    from latentsplat_amd.rasterizer import rasterize_views
    _lib.load()
    G, V, S = args.gaussians, args.views, args.size
    inp = build_inputs(G, V, S, dev, seed=rank_seed(1234, rank))

    def fwd(need_grad=False):
        m, c, o, f = inp["means"], inp["cov"], inp["opac"], inp["features"]
        if need_grad:
            m, c, o, f = (t.detach().requires_grad_(True) for t in (m, c, o, f))
        out = rasterize_views(inp["views"], S, S, 0, m, c, o, features=f)
        return out, (m, c, o, f)

    def timed(fn, steps, warmup):
        return timed_region(fn, steps, warmup, dist, lambda: torch.cuda.synchronize(dev), "cpu" if share_gpu else dev)

    # ---- headline: forward only (configs[1]).  With --full, in the timed region only the dominant kernel (the
    # roofline's) is bracketed by hipEvents; bracketing all five stages costs ~3 % of a step, so the
    # other per-kernel times come from a second, untimed pass over the same steps.  A plain run brackets nothing. ----
    # Clock warm-up (round 4): rounds 1-3 timed 3 + 20 steps (10 ms) on a device that had been idle, i.e. INSIDE the power
    # management's ramp — the compositing kernel measured 0.235 ms there and 0.200 ms in every later loop of the same run
    # (profiles/r04_clock_experiment.md).  The steps below are the same steps, untimed.
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < args.clock_warmup:
        fwd(False)
    torch.cuda.synchronize(dev)
    if args.full:
        _lib.profile_enable(True, only=("render_forward",))   # the roofline kernel: hipEvents over the timed region itself
        _lib.profile_read()
    last = {}

    def headline_step():
        last["out"] = fwd(False)[0]       # what a caller of the path receives (--dump-outputs writes the last step's)
    el_fwd = timed(headline_step, args.steps, args.warmup)
    per_rank_fwd = [1e3 * t / args.steps for t in PER_RANK_SECONDS]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(zip(("color", "feature", "mask", "depth", "radii"), last["out"])))
    last.clear()
    head = {
        "metric": "rendered target views/sec at 256x256, ~300k Gaussians (forward); fwd+bwd ms/view in `fwdbwd`",
        "value": whole_job_views_per_s(V, args.steps, world, el_fwd), "unit": "views/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * el_fwd / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"BASELINE configs[1]: {G} latent Gaussians (4-ch features + opacity), "
                               f"{S}x{S}, forward render; {V} views of one scene per step per GPU",
                   "views_per_step": V, "gaussians": G, "image": [S, S],
                   "parallelism": f"replicas x{world} (one scene per rank, no data-path collective)"},
    }
    if not args.full:         # a plain run: the headline figure alone
        if rank == 0:
            print(json.dumps(dict(head, per_rank_ms_per_step=[round(x, 4) for x in per_rank_fwd])))
        if dist is not None:
            dist.destroy_process_group()
        return
    prof_render = _lib.profile_read()["render_forward"]
    _lib.profile_enable(True)
    timed(lambda: fwd(False), max(5, min(50, args.steps // 2)), 1)
    prof = _lib.profile_read()
    prof["render_forward"] = prof_render
    _lib.profile_enable(False)
    views_total = V * args.steps * world
    # spread over single steps (outside the timed region: one device synchronisation per step)
    _lib.profile_enable(False)
    single = []
    for _ in range(min(args.steps, 50)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fwd(False)
        torch.cuda.synchronize(dev)
        single.append(1e3 * (time.perf_counter() - t0))
    single.sort()
    step_spread = dict(min=single[0], median=single[len(single) // 2], max=single[-1],
                       note="each step synchronised on its own (adds the launch-to-idle latency the back-to-back timed region hides)")

    # ---- fwd+bwd (configs[2]) ----
    fb = None
    if not args.no_bwd:
        gen = torch.Generator(device="cpu").manual_seed(99)
        gf = torch.randn((V, 4, S, S), generator=gen).to(dev)

        def step_fb():
            (color, feat, mask, depth, radii), leaves = fwd(True)
            feat.backward(gf)
        el_fb = timed(step_fb, args.steps, args.warmup)
        _lib.profile_enable(True)
        _lib.profile_read()
        timed(step_fb, max(5, min(50, args.steps // 2)), 1)
        prof_fb = _lib.profile_read()
        _lib.profile_enable(False)
        fb = dict(views_per_s=views_total / el_fb, ms_per_view=1e3 * el_fb / (V * args.steps),
                  ms_per_step=1e3 * el_fb / args.steps,
                  kernel_ms_per_launch={k: (ms / n if n else None) for k, (ms, n) in prof_fb.items()})

    # ---- workload statistics for the byte model (outside the timed region) ----
    # (P of the byte model is the PUBLISHED algorithm's pair count — SURVEY §8(d): the sum of the tile rectangles' areas — whatever
    # the product path bins: since round 6 it drops the quarter of those pairs that cannot reach a pixel before they are
    # counted (ABI v9 LSR_FWD_REACHED_ONLY); `pairs_binned` is what it really keyed and sorted)
    from latentsplat_amd import rasterizer as _rz
    from latentsplat_amd.rasterizer import LAST_STATS
    (color, feat, mask, depth, radii), _ = fwd(False)
    torch.cuda.synchronize(dev)
    P_binned = int(LAST_STATS["num_pairs"])
    reached = _rz._REACHED_ONLY
    _rz.set_reached_only(False)
    try:
        (color, feat, mask, depth, radii), _ = fwd(False)
        torch.cuda.synchronize(dev)
    finally:
        _rz.set_reached_only(reached)
    g_vis = int((radii > 0).sum().item())
    P = int(LAST_STATS["num_pairs"])  # sum of tile-rectangle areas over the step's V views
    C = 4
    b_in = 12 + 24 + 4 + 4 * C
    b_rec = 8 + 16 + 4 * C
    b_out = 4 * (C + 2)
    render_ms, render_n = prof["render_forward"]
    render_ms_per_launch = render_ms / max(render_n, 1)
    roofline = None
    roofline_valu = None
    roofline_bwd = None
    stage_roofline = None
    path = None
    path_fb = None
    if P is not None:
        # algorithmic bytes of ONE render launch (V views): sorted index + gathered record per pair,
        # every output word once (SURVEY.md §8(d) terms P*b_rec + H*W*b_out, plus the 4-byte index)
        render_bytes = P * (4 + b_rec) + V * S * S * b_out
        achieved = render_bytes / (render_ms_per_launch * 1e-3) / 1e9
        traffic, tinfo = None, None
        tpath = os.path.join(ROOT, "profiles", "traffic_render_forward.json")
        tstale = None
        if os.path.exists(tpath):
            try:
                tinfo = json.load(open(tpath))
                traffic = tinfo.get("hbm_bytes_per_launch")
            except Exception:
                traffic, tinfo = None, None
            # the counters were taken on a specific build of the kernel: the file carries the hash of render_forward.hip it was
            # measured with (tools/pmc_summary.py); a kernel edited since then reports no traffic rather than a stale one
            if tinfo is not None:
                have = kernel_source_hash()
                if tinfo.get("kernel_source_sha16") != have:
                    tstale = f"measured on render_forward.hip {tinfo.get('kernel_source_sha16')}, this build is {have}: re-run tools/collect_profile.sh"
                    traffic = None
        roofline = dict(bound="hbm", kernel="k_render_fwd", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=achieved / HBM_PEAK_GBS, traffic=traffic,
                        traffic_source=None if tinfo is None else (tstale or tinfo.get("source_commit")),
                        algorithmic_bytes_per_launch=render_bytes, launch_ms=render_ms_per_launch)
        # The kernel is bound by f32 VALU issue, not by HBM: report that ceiling next to the required
        # HBM figure.  Instruction counts come from the committed PMC pass (same workload), the
        # launch time is this run's; one wave64 VALU instruction occupies a SIMD for 4 cycles
        # (transcendentals 5/3 of that), 1024 SIMDs at 2.4 GHz.
        if tinfo and tinfo.get("valu_insts_per_launch"):
            n_valu, n_trans = tinfo["valu_insts_per_launch"], tinfo.get("valu_trans_insts_per_launch") or 0.0
            issue_cycles = 4.0 * (n_valu - n_trans) + 4.0 * (5.0 / 3.0) * n_trans   # transcendentals ~5/3 of a plain VALU (MI355X_MICROARCH.md)
            peak_cycles = 1024 * 2.4e9 * render_ms_per_launch * 1e-3
            roofline_valu = dict(bound="valu_issue", kernel="k_render_fwd", valu_insts_per_launch=n_valu,
                                 achieved=n_valu / (render_ms_per_launch * 1e-3) / 1e9, unit="G wave-instr/s",
                                 peak=1024 * 2.4e9 / 4 / 1e9, frac=issue_cycles / peak_cycles,
                                 source="profiles/traffic_render_forward.json (rocprofv3 --pmc SQ_INSTS_VALU, SQ_INSTS_VALU_TRANS_F32)")
        # the backward compositing kernel the same way (configs[2]): sorted index + gathered record +
        # one 64-byte gradient record per pair, per pixel: final_T, n_contrib, C upstream gradients and
        # C rendered values in
        if fb is not None and fb["kernel_ms_per_launch"].get("render_backward"):
            bwd_ms = fb["kernel_ms_per_launch"]["render_backward"]
            bwd_bytes = P * (4 + b_rec + 64) + V * S * S * (8 + 4 * C + 4 * C)
            roofline_bwd = dict(bound="hbm", kernel="k_render_bwd", achieved=bwd_bytes / (bwd_ms * 1e-3) / 1e9, peak=HBM_PEAK_GBS,
                                unit="GB/s", frac=bwd_bytes / (bwd_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, traffic=None,
                                algorithmic_bytes_per_launch=bwd_bytes, launch_ms=bwd_ms)
        # every stage against the HBM roofline with its own algorithmic bytes
        # (round 5: single-pass binning — the projection kernel also writes the 8-byte sort keys; `scatter` only appears
        # when the call took the two-phase path)
        single_pass = not prof.get("scatter", (0.0, 0))[1]
        stage_bytes = dict(
            # the shared scene is read once per block of 4 views; written: one 64-byte record per visible
            # (view, Gaussian), a 12-byte bin record and the 4-byte radius for every one (the tile scan runs in the
            # kernel's last workgroup since round 4; `tile_scan` only appears for calls with more than 4096 tiles)
            preprocess=-(-V // 4) * G * (12 + 36 + 4 + 4 * C) + g_vis * 64 + V * G * (12 + 4) + (P * 8 if single_pass else 0),
            tile_scan=V * (S // 16) * (S // 16) * 12,
            scatter=V * G * 12 + P * 8,
            # keys in, canonical list + the two half-tile render lists (0.94 entries per pair) out
            sort_tiles=P * (8 + 4 + 4),
            render_forward=render_bytes)
        stage_roofline = {}
        for k, nbytes in stage_bytes.items():
            ms, n = prof.get(k, (0.0, 0))
            if n:
                stage_roofline[k] = dict(ms=ms / n, algorithmic_bytes=nbytes, frac=nbytes / (ms / n * 1e-3) / 1e9 / HBM_PEAK_GBS)
        # whole forward path per view against the same roofline (SURVEY §8(d) B_fwd)
        B_fwd_step = V * G * b_in + g_vis * b_rec + P * 16 + P * b_rec + V * S * S * b_out
        step_s = el_fwd / args.steps
        # `frac` charges the scene's input bytes once per VIEW (SURVEY §8(d)'s per-view formula, to the letter); the V views
        # of a step share ONE scene, so `frac_shared_scene` charges them once per step — the honest figure for this launch
        B_fwd_shared = G * b_in + g_vis * b_rec + P * 16 + P * b_rec + V * S * S * b_out
        path = dict(algorithmic_bytes_per_view=B_fwd_step / V, achieved=B_fwd_step / step_s / 1e9,
                    frac=B_fwd_step / step_s / 1e9 / HBM_PEAK_GBS, pairs_per_view=P / V, pairs_binned_per_view=P_binned / V,
                    visible_fraction=g_vis / (V * G), frac_shared_scene=B_fwd_shared / step_s / 1e9 / HBM_PEAK_GBS,
                    algorithmic_bytes_per_view_shared_scene=B_fwd_shared / V)
        if fb is not None:
            # forward + backward (configs[2]) the same way: B_bwd of SURVEY §8(d) with the measured P, G_vis
            g_rec = 8 + 12 + 4 + 4 * C
            g_out = 12 + 24 + 4 + 4 * C
            B_bwd_step = V * S * S * (b_out + 8) + P * (4 + b_rec) + P * 2 * g_rec + g_vis * (12 + 24 + g_rec) + V * G * g_out
            B_bwd_shared = B_bwd_step - (V - 1) * G * g_out
            fb_s = fb["ms_per_step"] * 1e-3
            path_fb = dict(algorithmic_bytes_per_view=(B_fwd_step + B_bwd_step) / V, achieved=(B_fwd_step + B_bwd_step) / fb_s / 1e9,
                           frac=(B_fwd_step + B_bwd_step) / fb_s / 1e9 / HBM_PEAK_GBS,
                           frac_shared_scene=(B_fwd_shared + B_bwd_shared) / fb_s / 1e9 / HBM_PEAK_GBS)

    cpu = None
    gate = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(G, S, 1234)
        cpu["torch_oracle"] = cpu_baseline_torch()
        gate = parity_gate(G, V, S, 1234, dev)
    # (the decoder / adapter / latent / chained-path legs run BEFORE the pipelined and latency legs: measured behind them in
    # two runs without the CPU baselines — a minute of uninterrupted GPU load, two extra streams, a captured hipGraph and its
    # private memory pool in the process — the configs[4] forward+backward step read 2.8 ms; in a fresh process, in runs with
    # the CPU baselines in between and in tools/drift_probe.py over 240 steps the same function reads 2.39-2.43)
    dec_step = adapter_step = latent_step = path_step = None
    if rank == 0 and world == 1 and not args.no_bwd:
        torch.cuda.empty_cache()
        dec_step = decoder_step_timing(dev)
        dec_step["batch4"] = decoder_step_timing(dev, scenes=4)      # configs[4]: batch_size 4 per GPU
        # the same two steps on the Gaussian distribution the reference's encoder emits
        dec_step["encoder_shaped"] = decoder_step_timing(dev, encoder_shaped=True)
        dec_step["encoder_shaped"]["batch4"] = decoder_step_timing(dev, scenes=4, encoder_shaped=True)
        adapter_step = adapter_step_timing(dev)
        latent_step = latent_step_timing(dev)
        path_step = path_step_timing(dev)
        if not args.no_cpu_baseline:
            nxt = cpu_baseline_next_rows()
            adapter_step["cpu_baseline"], latent_step["cpu_baseline"] = nxt["adapter"], nxt["latent"]
        torch.cuda.empty_cache()
    latency = pipelined = None
    if rank == 0 and world == 1 and not args.no_bwd and not args.no_latency:
        pipelined = pipelined_timing(dev, inp, V, S, args.steps, min(args.warmup, 10))   # (50 steps after 5 read 8 % low: clocks and allocator still settling)
        latency = latency_timing(dev, G, S, 1234)

    if rank == 0:
        full = {
            **head,
            "ms_per_view_fwd": 1e3 * el_fwd / (V * args.steps), "clock_warmup_s": args.clock_warmup,
            "kernel_ms_per_launch": {k: (ms / n if n else None) for k, (ms, n) in prof.items()},
            "per_rank_ms_per_step": per_rank_fwd, "ms_per_step_spread": step_spread,
            "stage_roofline": stage_roofline, "roofline_bwd": roofline_bwd, "latency": latency, "pipelined": pipelined,
            "fwdbwd": fb, "decoder_step": dec_step, "adapter_step": adapter_step, "latent_step": latent_step, "path_step": path_step, "roofline": roofline, "roofline_valu": roofline_valu, "roofline_path": path, "roofline_path_fwdbwd": path_fb, "cpu_baseline": cpu,
            "parity_gate": gate,
        }
        # The whole dictionary goes to a side file; stdout carries ONE compact line (graded keys first, < 4 KB) so
        # that a driver record that truncates long lines still holds value / roofline / cpu_baseline / fwdbwd.
        side = None
        try:
            side = os.path.abspath(args.full_json)
            os.makedirs(os.path.dirname(side), exist_ok=True)
            with open(side, "w") as f:
                json.dump(full, f, indent=1)
        except OSError:
            side = None
        r4 = lambda x: None if x is None else (round(x, 4) if isinstance(x, float) else x)
        pick = lambda d, keys: None if d is None else {k: r4(d.get(k)) for k in keys if k in d}
        line = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                     "scaling", "vs_baseline", "dtype", "data", "config")}
        line["roofline"] = pick(roofline, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "algorithmic_bytes_per_launch", "launch_ms"))
        line["cpu_baseline"] = None if cpu is None else dict(
            pick(cpu, ("value", "unit", "cores", "kind", "sample", "fwdbwd_value")),
            torch_oracle=pick(cpu.get("torch_oracle"), ("value", "unit", "cores", "kind")))
        line["fwdbwd"] = pick(fb, ("views_per_s", "ms_per_view", "ms_per_step"))
        line["roofline_bwd"] = pick(roofline_bwd, ("kernel", "achieved", "frac", "algorithmic_bytes_per_launch", "launch_ms"))
        # (not through r4: the error is ~1e-6 and would print as 0.0)
        line["parity_gate"] = None if gate is None else {k: gate[k] for k in ("ok", "lists_bit_exact", "reached_only_bitwise_equal", "max_abs_err", "pixels_over_tol", "fragile_pixels_excluded", "views_checked", "tol")}
        line["roofline_path"] = pick(path, ("algorithmic_bytes_per_view", "achieved", "frac", "frac_shared_scene", "pairs_per_view", "pairs_binned_per_view"))
        line["roofline_path_fwdbwd"] = pick(path_fb, ("algorithmic_bytes_per_view", "achieved", "frac", "frac_shared_scene"))
        line["roofline_valu"] = pick(roofline_valu, ("valu_insts_per_launch", "frac"))
        line["kernel_ms"] = {k: r4(v) for k, v in full["kernel_ms_per_launch"].items() if v}
        if fb is not None:
            line["kernel_ms_fwdbwd"] = {k: r4(v) for k, v in fb["kernel_ms_per_launch"].items() if v}
        line["per_rank_ms_per_step"] = [r4(x) for x in per_rank_fwd]
        if dec_step is not None:
            both = lambda d: [[r4(x) for x in d["forward"]["ms_per_step_regions"]], [r4(x) for x in d["forward_backward"]["ms_per_step_regions"]]]
            enc = dec_step["encoder_shaped"]
            line["decoder_step"] = {"cfg3_1x4": both(dec_step), "cfg4_4x4": both(dec_step["batch4"]),
                                    "cfg3_encoder_shaped": both(enc), "cfg4_encoder_shaped": both(enc["batch4"]),
                                    "unit": "ms per step [[forward: region 1, region 2], [forward+backward: region 1, region 2]]; "
                                            "encoder_shaped: pixel-aligned Gaussians in ray order instead of a random cloud"}
            shr = lambda d: {k: [v["ms"], v["frac"]] for k, v in (d.get("sh_roofline") or {}).items()}
            line["decoder_step"]["sh_roofline"] = {"cfg3": shr(dec_step), "cfg4": shr(dec_step["batch4"]),
                                                   "unit": "[ms per launch, lower-bound fraction of the 8 TB/s HBM peak]"}
            # per-kernel times of the forward+backward step at the reference's real shapes (hipEvents inside the library;
            # `preprocess` is the fused projection + SH payload kernel there)
            line["decoder_step"]["cfg3_kernel_ms"] = dec_step.get("kernel_ms")
            line["decoder_step"]["cfg4_kernel_ms"] = dec_step["batch4"].get("kernel_ms")
            line["decoder_step"]["cfg4_encoder_shaped_kernel_ms"] = enc["batch4"].get("kernel_ms")
        if path_step is not None:
            line["path_step"] = pick(path_step, ("forward_ms", "forward_backward_ms"))
        if pipelined is not None:   # the same steps from two HIP streams (independent batches: inference loops); NOT the headline
            line["pipelined_views_per_s"] = {k: r4(v["views_per_s"]) for k, v in pipelined.items() if isinstance(v, dict)}
        line["full"] = None if side is None else os.path.relpath(side, ROOT)
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
