"""Antialiased rasterization (``LSR_FWD_ANTIALIAS``) on the MI355X.

Reference: tests/antialias_ref.py — rho per (view, Gaussian) in float64 torch (autograd), and the same composition in float32
(the stock baseline).  Bars:
  * record opacity o' = o rho: error against float64 <= 4 x the stock composition's own worst error on the same case;
  * everything behind the projection: BIT IDENTITY with the classic mode fed the record's opacities per view;
  * gradients: per tensor max(CLEAN_TOL x max |reference gradient|, 4 x the stock composition's own error), the reference being
    the classic op on per-view o' = o rho_ref with rho_ref the float64 autograd composition cast to float32 (CLEAN_TOL:
    tests/test_parity_gpu.py, the project's bar for gradient rows without a fragile evaluation nearby); dL/dopacities, which
    differs from the reference's by the float rounding of rho alone, without CLEAN_TOL: 4 x the stock error or 8 float32 ulps;
  * one isolated Gaussian: summed mask within 5 % of 2 pi o sqrt(det0).
  * the speculative and the pair_capacity forward (SEG = true projection instances), eager: bit identity with the exact call.
Gradients against the float64 oracle on every backward instance and layout: tests/test_antialias_grads_gpu.py.
The measured ratios are printed (-s) and quoted in DESIGN.md §2.21.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from latentsplat_amd._lib import Dims
from latentsplat_amd.decoder import cuda_splatting as cs
from latentsplat_amd.synthetic import Scene
from tests import antialias_ref as ref
from tests import util
from tests.test_parity_gpu import CLEAN_TOL

pytestmark = pytest.mark.gpu

H = W = 64
AA, REACHED, RECORD = _lib.FWD_ANTIALIAS, _lib.FWD_REACHED_ONLY, _lib.FWD_FOR_BACKWARD


# ---- cases: every projection-kernel path ---------------------------------------------------------------------------------
def _case(name: str, dev) -> dict:
    """Device tensors of one call: views (V, 44), means, cov, opac (.., G, 1), and the payload: `color` + `color_mode` (+ K,
    sh_degree), `features` (+ feat_sh_degree, -1 = direct channels), `vpg` (views per group), `fma`, size."""
    c = dict(vpg=0, fma=False, H=H, W=W, color=None, color_mode=_lib.COLOR_NONE, K=0, sh_degree=0, features=None, fdeg=-1)
    t = lambda x: x.to(dev).contiguous()

    def scene(G, views, size=64, cdeg=None, fch=4, fdeg=0, seed=5, **kw):
        sc = util.make_scene(G, image_size=size, views=views, color_sh_degree=cdeg, feature_channels=fch,
                             feature_sh_degree=fdeg, seed=seed, **kw)
        return sc, util.boundary_inputs(sc, size, size, bg=(0.1, 0.2, 0.3))

    if name in ("shared4", "fma"):          # 4 shared views: k_preprocess<NONE, LDS, VB = 4>; direct features
        sc, bi = scene(2000, 4)
        c.update(views=util.view_table(bi, dev), means=t(bi["means"][0]), cov=t(bi["cov6"][0]), opac=t(bi["opac"]),
                 features=t(sc.feature_sh[..., 0]), fma=name == "fma")
    elif name == "one_view":                # VB = 1, precomputed colour + direct features
        sc, bi = scene(3000, 1, cdeg=0, seed=6)
        c.update(views=util.view_table(bi, dev), means=t(bi["means"][0]), cov=t(bi["cov6"][0]), opac=t(bi["opac"]),
                 color=t(0.5 + 0.28 * sc.color_sh[..., 0]), color_mode=_lib.COLOR_PRECOMP, features=t(sc.feature_sh[..., 0]))
    elif name in ("per_view", "groups"):    # per-view inputs (VB = 1) / two scenes of two views (VB = 2), precomputed colour
        sc, bi = scene(1500, 4, cdeg=0, seed=7)
        S = 4 if name == "per_view" else 2
        gen = torch.Generator().manual_seed(3)
        jit = lambda x, s: x[None] * (1.0 + s * torch.rand((S,) + tuple(x.shape), generator=gen))
        c.update(views=util.view_table(bi, dev), means=t(jit(bi["means"][0], 0.01)), cov=t(jit(bi["cov6"][0], 0.3)),
                 opac=t(jit(bi["opac"], 0.5).clamp(max=0.99)), color=t(jit(0.5 + 0.28 * sc.color_sh[..., 0], 0.1)),
                 color_mode=_lib.COLOR_PRECOMP, features=t(jit(sc.feature_sh[..., 0], 0.1)), vpg=0 if name == "per_view" else 2)
    elif name == "sh":                      # k_preprocess_sh: colour SH degree 2, latent feature SH degree 1
        sc, bi = scene(2000, 4, cdeg=2, fch=4, fdeg=1, seed=8)
        c.update(views=util.view_table(bi, dev), means=t(bi["means"][0]), cov=t(bi["cov6"][0]), opac=t(bi["opac"]),
                 color=t(bi["shs"]), color_mode=_lib.COLOR_SH, K=9, sh_degree=2, features=t(sc.feature_sh), fdeg=1)
    elif name == "cov9":                    # full 3 x 3 covariances
        sc, bi = scene(1500, 2, seed=9)
        scale2 = (1.0 / sc.near[0]) ** 2
        c.update(views=util.view_table(bi, dev), means=t(bi["means"][0]), cov=t(sc.covariances * scale2), opac=t(bi["opac"]),
                 features=t(sc.feature_sh[..., 0]))
    elif name == "scaled":                  # a scale-invariant table (view[40] = 1 / near != 1) over the UNSCALED scene
        sc, _ = scene(1500, 4, seed=10)
        sc.near = torch.tensor([0.5, 0.6, 0.7, 0.8])
        views = cs._view_table(t(sc.extrinsics), t(sc.intrinsics), t(sc.near), t(sc.far), t(torch.tensor([0.1, 0.2, 0.3])), True)
        assert float((views[:, 40] - 1.0).abs().min()) > 0.2
        c.update(views=views, means=t(sc.means), cov=t(cs._pack_covariances(sc.covariances)), opac=t(sc.opacities[:, None]),
                 features=t(sc.feature_sh[..., 0]))
    elif name == "large":                   # 4 x 4096 tiles: the instance without the LDS histogram
        sc, bi = scene(500, 4, size=1024, seed=11)
        c.update(views=util.view_table(bi, dev), means=t(bi["means"][0]), cov=t(bi["cov6"][0]), opac=t(bi["opac"]),
                 features=t(sc.feature_sh[..., 0]), H=1024, W=1024)
    else:
        raise KeyError(name)
    return c


CASES = ("shared4", "one_view", "per_view", "groups", "sh", "cov9", "scaled", "fma", "large")


def _dims(c: dict, flags: int, opac=None, vpg=None, expand=False) -> tuple:
    """(Dims, tensors) of case ``c`` with ``forward_flags``; ``opac``: per-view (V, G, 1) opacities instead of the case's;
    ``expand``: a grouped case's inputs repeated per view (so that per-view opacities can be handed in)."""
    vpg = c["vpg"] if vpg is None else vpg
    V = c["views"].shape[0]
    means, cov, op, color, feats = c["means"], c["cov"], c["opac"] if opac is None else opac, c["color"], c["features"]
    if expand:
        rep = lambda x: None if x is None else x.repeat_interleave(c["vpg"], dim=0).contiguous()
        means, cov, color, feats = rep(means), rep(cov), rep(color), rep(feats)
    G = means.shape[-2]
    full = cov.shape[-2:] == (3, 3)
    fsh = c["fdeg"] >= 0
    stride = lambda x, base: 0 if (x is None or x.dim() == base) else x[0].numel()
    Cf = 0 if feats is None else (feats.shape[-2] if fsh else feats.shape[-1])
    d = Dims(V, G, c["H"], c["W"], Cf, c["color_mode"], c["sh_degree"], c["K"], stride(means, 2), stride(cov, 3 if full else 2),
             stride(op, 2), stride(color, 3 if c["color_mode"] == _lib.COLOR_SH else 2), stride(feats, 3 if fsh else 2),
             9 if full else 6, _lib.FEAT_SH if fsh else _lib.FEAT_DIRECT, max(c["fdeg"], 0), feats.shape[-1] if fsh else 0,
             0, vpg if vpg > 1 else 0, 0, flags, 0)
    return d, (c["views"], means, cov, op, color, feats)


def _run(c, flags, **kw) -> ref.Run:
    d, tensors = _dims(c, flags, **kw)
    return ref.Run(*tensors, d)


class _contraction:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        lib = _lib.load()
        self.old = lib.lsr_get_projection_contraction()
        _lib.call("lsr_set_projection_contraction", 1 if self.on else 0)

    def __exit__(self, *a):
        _lib.call("lsr_set_projection_contraction", self.old)


def _rho_pair(c):
    """(V, G) rho in float64 and in stock float32, on the host."""
    a = (c["views"].cpu(), c["means"].cpu(), c["cov"].cpu(), c["H"], c["W"])
    with torch.no_grad():
        return ref.rho(*a, dtype=torch.float64, views_per_group=c["vpg"]), ref.rho(*a, dtype=torch.float32, views_per_group=c["vpg"])


def _per_view(c, x):
    """(.., G, 1) opacities of the case -> (V, G) on the host."""
    V = c["views"].shape[0]
    x = x.cpu()[..., 0]
    if x.dim() == 1:
        return x[None].expand(V, -1)
    return x.repeat_interleave(c["vpg"], dim=0) if c["vpg"] > 1 else x


@pytest.mark.parametrize("name", CASES)
def test_record_opacity_and_bit_identity(hip_device, name):
    """1. Slot 5 of the screen records of the visible slots against o rho in float64 (bar: 4 x the stock float32 composition's
    own error).  2. Those opacities fed back per view to the CLASSIC mode: every output and list of the two forwards is the
    same bit for bit, with and without LSR_FWD_REACHED_ONLY and LSR_FWD_FOR_BACKWARD — the projection instance is all that
    differs between the two calls."""
    c = _case(name, hip_device)
    V = c["views"].shape[0]
    with _contraction(c["fma"]):
        rho64, rho32 = _rho_pair(c)
        o = _per_view(c, c["opac"])
        want, stock = o.double() * rho64, o * rho32
        first = None
        for flags in (0, REACHED, RECORD, REACHED | RECORD):
            aa = _run(c, AA | flags)
            vis = (aa.radii > 0).cpu().numpy()
            rec = aa.record_opacity()
            assert vis.sum() > 0.3 * vis.size and np.isfinite(rec[vis]).all()
            if first is None:
                first = rec
                ref.held("record o'", rec[vis], want.numpy()[vis], stock.numpy()[vis], 0.0, show=name)
                assert (rho64.numpy()[vis] < 0.98).mean() > 0.5, "the case does not exercise the factor"
            else:   # the projection does not depend on the other bits
                assert np.array_equal(rec[vis].view(np.uint32), first[vis].view(np.uint32))
            fed = torch.from_numpy(np.where(vis, rec, o.numpy()).astype(np.float32)).to(hip_device)[..., None].contiguous()
            classic = _run(c, flags, opac=fed, vpg=0, expand=c["vpg"] > 1)
            ref.assert_same_render(aa, classic, f"{name} flags {flags}")
            # and the mode does something: the classic render of the case's own opacities is another picture
            if flags == 0:
                plain = _run(c, 0)
                assert torch.equal(plain.radii, aa.radii) and not torch.equal(plain.mask_out, aa.mask_out)
                # nothing in the binning reads the footprint without LSR_FWD_REACHED_ONLY: all nine cases
                assert aa.P == plain.P and np.array_equal(aa.tile_start(), plain.tile_start()) \
                    and np.array_equal(aa.point_list(), plain.point_list()), "the canonical lists are the classic mode's"
            elif flags == REACHED:
                assert aa.P <= _run(c, REACHED).P       # smaller footprints reach fewer tiles
    assert V == aa.d.num_views


def test_captured_nosync_forward(hip_device):
    """A pair_capacity forward with the mode on, captured in a torch.cuda.graph and replayed, equals the eager synchronous one."""
    from latentsplat_amd.rasterizer import last_forward_status, rasterize_views
    dev = hip_device
    c = _case("shared4", dev)
    call = lambda **kw: rasterize_views(c["views"], H, W, 0, c["means"], c["cov"], c["opac"], features=c["features"],
                                        antialiasing=True, **kw)
    with torch.no_grad():
        eager = call()
        P = last_forward_status()["num_pairs"]
        kw = dict(pair_capacity=2 * P + 64, max_tile_hint=2048)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            call(**kw)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call(**kw)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert not last_forward_status()["overflow"]
        for a, b in zip(out[1:], eager[1:]):
            assert torch.equal(a, b)
        classic = rasterize_views(c["views"], H, W, 0, c["means"], c["cov"], c["opac"], features=c["features"])
        assert not torch.equal(classic[2], eager[2])


def _call_of(c):
    """rasterize_views of case ``c`` with the mode on; keywords pass through"""
    from latentsplat_amd.rasterizer import rasterize_views
    pay = dict(shs=c["color"], feature_sh=c["features"]) if c["color_mode"] == _lib.COLOR_SH else \
        dict(colors_precomp=c["color"], features=c["features"])
    return lambda **kw: rasterize_views(c["views"], c["H"], c["W"], c["sh_degree"], c["means"], c["cov"], c["opac"],
                                        antialiasing=True, **pay, **kw)


def _assert_same_outputs(a, b, what):
    for x, y, k in zip(a, b, ("colour", "features", "mask", "depth", "radii")):
        assert (x is None and y is None) or torch.equal(x, y), f"{what}: {k}"


@pytest.mark.parametrize("name", ["sh", "one_view"])
def test_speculative_forward_equals_the_exact_one(hip_device, name):
    """The SEG = true projection instances with the mode on, outside a captured graph: the first call of a shape takes the
    exact path (prepare + render), the second the speculative one (SPECULATION_STATS); all outputs and radii bit for bit."""
    from latentsplat_amd import rasterizer as R
    c = _case(name, hip_device)
    assert (c["color_mode"] == _lib.COLOR_SH) == (name == "sh")
    call = _call_of(c)
    with R._ESTIMATES_LOCK:
        R._ESTIMATES.clear()        # whatever ran before in this process: this shape has not been seen
    with torch.no_grad():
        s0 = dict(R.SPECULATION_STATS)
        exact = call()
        s1 = dict(R.SPECULATION_STATS)
        second = call()
        s2 = dict(R.SPECULATION_STATS)
    assert (s1["exact"], s1["speculative"], s1["reruns"]) == (s0["exact"] + 1, s0["speculative"], s0["reruns"])
    assert (s2["exact"], s2["speculative"], s2["reruns"]) == (s1["exact"], s1["speculative"] + 1, s1["reruns"])
    _assert_same_outputs(second, exact, name)
    assert int((exact[4] > 0).sum()) > 0.3 * exact[4].numel()


@pytest.mark.parametrize("name", ["sh", "one_view"])
def test_pair_capacity_forward_equals_the_exact_one(hip_device, name):
    """lsr_forward_nosync with the mode on, eager: every output and the radii of the exact call bit for bit, no overflow."""
    from latentsplat_amd import rasterizer as R
    c = _case(name, hip_device)
    call = _call_of(c)
    with R._ESTIMATES_LOCK:
        R._ESTIMATES.clear()
    with torch.no_grad():
        s0 = dict(R.SPECULATION_STATS)
        exact = call()
        assert R.SPECULATION_STATS["exact"] == s0["exact"] + 1
        st = R.last_forward_status()
        nosync = call(pair_capacity=2 * st["num_pairs"] + 64, max_tile_hint=max(4096, 2 * st["max_tile_pairs"]))
        torch.cuda.synchronize(hip_device)
        after = R.last_forward_status()
    assert not after["overflow"] and after["num_pairs"] == st["num_pairs"]
    _assert_same_outputs(nosync, exact, name)


# ---- gradients ---------------------------------------------------------------------------------------------------------
def _grad_leg(dev, sc: Scene, show: str, edit=None):
    """Forward + backward of the antialiased op (shared scene, views requiring grad) and of the reference: the classic op
    on per-view o' = o rho_ref, rho_ref the float64 (reference) / float32 (stock) autograd composition.  Returns
    ({name: (got, want, stock)}, radii)."""
    from latentsplat_amd.rasterizer import rasterize_views
    bi = util.boundary_inputs(sc, H, W, bg=(0.1, 0.2, 0.3))
    V = bi["V"]
    base = dict(views=util.view_table(bi, dev), means=bi["means"][0].to(dev), cov=bi["cov6"][0].to(dev), opac=bi["opac"].to(dev),
                feats=sc.feature_sh[..., 0].to(dev))
    if sc.color_sh is not None:
        base["colors"] = (0.5 + 0.28 * sc.color_sh[..., 0]).to(dev)
    if edit is not None:
        edit(base)
    leaves = lambda: {k: v.clone().contiguous().requires_grad_(True) for k, v in base.items()}
    gen = torch.Generator().manual_seed(1)
    w = [torch.randn(s, generator=gen).to(dev) for s in ((V, 3, H, W), (V, 4, H, W), (V, H, W), (V, H, W))]

    def loss(out):
        total = (out[1] * w[1]).sum() + (out[2] * w[2]).sum() + 0.1 * (out[3] * w[3]).sum()
        return total + (out[0] * w[0]).sum() if out[0] is not None else total

    a = leaves()
    out = rasterize_views(a["views"], H, W, 0, a["means"], a["cov"], a["opac"], colors_precomp=a.get("colors"),
                          features=a["feats"], antialiasing=True)
    loss(out).backward()
    radii = out[4]
    res = {}
    for dtype in (torch.float64, torch.float32, "constant"):
        r = leaves()
        if dtype == "constant":   # rho held constant: what a backward WITHOUT rho's term would return (the check's own check)
            rho = ref.rho(r["views"].cpu(), r["means"].cpu(), r["cov"].cpu(), H, W).detach().float().to(dev)
        else:
            rho = ref.rho(r["views"].cpu(), r["means"].cpu(), r["cov"].cpu(), H, W, dtype=dtype).float().to(dev)
        o_pv = r["opac"][None] * rho[..., None]
        cl = rasterize_views(r["views"], H, W, 0, r["means"], r["cov"], o_pv, colors_precomp=r.get("colors"), features=r["feats"])
        assert torch.equal(cl[4], radii)
        loss(cl).backward()
        res[dtype] = {k: v.grad.detach().cpu().numpy() for k, v in r.items()}
    got = {k: v.grad.detach().cpu().numpy() for k, v in a.items()}
    return {k: (got[k], res[torch.float64][k], res[torch.float32][k], res["constant"][k]) for k in got}, radii


def _hold_gradients(g: dict, show: str, rho_term=()):
    """``rho_term``: the tensors for which the leg must be able to tell a backward without rho's term from one with it — the
    reference with rho held constant is at least 10 bars away from the reference."""
    for k, (got, want, stock, const) in g.items():
        assert np.isfinite(got).all(), (show, k)
        assert np.abs(want).max() > 0, (show, k)
        floor = CLEAN_TOL * float(np.abs(want).max())
        if k == "opac":
            # dL/do = rho dL/do' on both sides: the two differ by the float rounding of rho alone, and that is exactly what
            # separates the stock composition from the reference.  No CLEAN_TOL here: 4 x the stock error, or 8 float32 ulps
            # of the tensor's scale where the stock composition happens to round like the reference (each side is itself
            # reproducible only to the order of its float atomic sums: one rounding per view, up to 4 views, two sides)
            floor = 8.0 * 2.0 ** -23 * float(np.abs(want).max())
        ref.held(f"dL/d{k}", got, want, stock, floor, show=show)
        if k in rho_term:
            bar = max(ref.MARGIN * float(np.abs(stock - want).max()), floor)
            away = float(np.abs(const - want).max())
            print(f"{show:28s} dL/d{k}: without rho's term {away:.3e} = {away / bar:.0f} bars away")
            assert away > 10 * bar, (show, k, away, bar)


def test_gradients(hip_device):
    """Means, covariances, opacities, colours, features and the view table (lsr_backward_views: the CAM instances), 4 views."""
    sc = util.make_scene(2000, image_size=64, views=4, color_sh_degree=0, feature_channels=4, seed=21)
    g, _ = _grad_leg(hip_device, sc, "ordinary")
    assert set(g) == {"views", "means", "cov", "opac", "colors", "feats"}
    _hold_gradients(g, "ordinary", rho_term=("views", "means", "cov"))


def test_gradients_of_sub_pixel_splats(hip_device):
    """sigma_px = (0.05, 0.6): rho is far from 1 and its term dominates the covariance gradient."""
    sc = util.make_scene(3000, image_size=64, views=4, color_sh_degree=0, feature_channels=4, seed=22, sigma_px=(0.05, 0.6),
                         opacity_scale=0.9)
    g, radii = _grad_leg(hip_device, sc, "sub-pixel")
    _hold_gradients(g, "sub-pixel", rho_term=("views", "means", "cov"))
    bi = util.boundary_inputs(sc, H, W)
    with torch.no_grad():
        rho = ref.rho(util.view_table(bi, "cpu"), bi["means"][0], bi["cov6"][0], H, W)
    vis = (radii > 0).cpu()
    assert float(rho[vis].median()) < 0.5


def test_gradients_with_clamped_jacobians(hip_device):
    """util.make_edge_scene("outside"): means beyond 1.3 tan(fov) whose footprints reach into the image — the clamped
    t.x / t.z is a constant of rho too."""
    sc, lab = util.make_edge_scene("outside", H, W, views=2, seed=3, feature_channels=4)
    assert (lab["clamped"].any(-1) & ~lab["culled"]).any()
    g, radii = _grad_leg(hip_device, sc, "clamped")
    _hold_gradients(g, "clamped")
    clamped_visible = torch.from_numpy(lab["clamped"].any(-1)) & (radii > 0).cpu()
    assert clamped_visible.any()


def test_degenerate_covariances(hip_device):
    """Zero covariances, rank-1 covariances and needles (det0 / det below the floor) among ordinary Gaussians, opacity 0.95 so
    that o' = 0.005 o still passes the 1/255 cut at the centre.  Forward: finite, o' = 0.005 o there (sqrtf of the float
    0.000025 and one product: 2^-22 relative).  Backward: every gradient finite; those rows get no rho term — their rows of
    dL/dmeans and dL/dcov are the classic reference's, in which rho_ref is a constant for them."""
    dev = hip_device
    sc = util.make_scene(2000, image_size=64, views=4, color_sh_degree=0, feature_channels=4, seed=23)
    n = 40
    gen = torch.Generator().manual_seed(4)
    u = torch.randn(3 * n, 3, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True)
    s = (3.0 * sc.means[:3 * n, 2] / (0.8 * 64)) ** 2                      # 3 px at the Gaussian's depth
    rank1 = s[:, None, None] * u[:, :, None] * u[:, None, :]
    cov = sc.covariances.clone()
    cov[:n] = 0.0
    cov[n:2 * n] = rank1[n:2 * n]
    cov[2 * n:3 * n] = rank1[2 * n:] + 1e-8 * s[2 * n:, None, None] * torch.eye(3)   # axes 3 px and 3e-4 px
    sc.covariances = cov
    sc.opacities = sc.opacities.clone()
    sc.opacities[:3 * n] = 0.95
    rows = np.arange(3 * n)
    # forward: the record's opacity
    bi = util.boundary_inputs(sc, H, W)
    c = dict(vpg=0, fma=False, H=H, W=W, color=None, color_mode=_lib.COLOR_NONE, K=0, sh_degree=0, fdeg=-1,
             views=util.view_table(bi, dev), means=bi["means"][0].to(dev), cov=bi["cov6"][0].to(dev).contiguous(),
             opac=bi["opac"].to(dev), features=sc.feature_sh[..., 0].to(dev).contiguous())
    run = _run(c, AA)
    rec, vis = run.record_opacity(), (run.radii > 0).cpu().numpy()
    for out in (run.feat_out, run.mask_out, run.depth_out):
        assert torch.isfinite(out).all()
    assert vis[:, rows].sum() > 2 * n and np.isfinite(rec[vis]).all()
    want = 0.005 * 0.95
    assert np.abs(rec[:, rows][vis[:, rows]] / want - 1.0).max() <= 2.0 ** -22
    with torch.no_grad():
        rho = ref.rho(c["views"].cpu(), c["means"].cpu(), c["cov"].cpu(), H, W)
    assert (rho[:, rows] == rho[:, rows].min()).all() and (rho[:, 3 * n:][torch.from_numpy(vis[:, 3 * n:])] > 0.0051).all()
    # backward
    g, _ = _grad_leg(dev, sc, "degenerate")
    _hold_gradients(g, "degenerate")
    assert (g["opac"][1][rows] != 0).sum() >= 10, "the degenerate rows reach no pixel: the check would be empty"
    for k in ("means", "cov"):
        got, want, stock = (x[rows] for x in g[k][:3])
        ref.held(f"rows dL/d{k}", got, want, stock, CLEAN_TOL * float(np.abs(want).max()), show="degenerate")


# ---- what the mode is for ------------------------------------------------------------------------------------------------
SIX_DRAWS = np.array([[1.5, 1.5, 0.3, 32.3, 31.6], [0.2, 0.2, 0.0, 30.1, 33.7], [1.5, 0.2, 0.7, 27.5, 36.2],
                      [0.6, 0.4, 2.1, 35.9, 29.4], [1.0, 0.3, 1.2, 31.5, 31.5], [0.25, 0.9, 2.8, 38.2, 25.8]])


def test_one_isolated_gaussian_emits_the_light_of_its_true_extent(hip_device):
    """One Gaussian, o = 0.9, axes of 0.2-1.5 px, over a 64 x 64 view (identity camera, depth 4): with the mode on the summed
    mask is within 5 % of 2 pi o sqrt(det0); the classic mode misses by the factor 1 / rho (1.13 ... 8.5 at these six draws).
    (tests/test_antialias_cpu.py replays the compositing rule over 2 000 such draws.)"""
    from latentsplat_amd.rasterizer import rasterize_views
    dev = hip_device
    z, tan = 4.0, 0.625
    f = W / (2.0 * tan)
    intr = torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]])[None]
    for d in SIX_DRAWS:
        a0, b, c0 = ref.isolated_cov2d(d)
        k = (z / f) ** 2
        cov = torch.tensor([[[a0 * k, b * k, 0.0], [b * k, c0 * k, 0.0], [0.0, 0.0, 0.0]]], dtype=torch.float32)
        mean = torch.tensor([[((2 * d[3] + 1) / W - 1) * tan * z, ((2 * d[4] + 1) / H - 1) * tan * z, z]], dtype=torch.float32)
        sc = Scene(mean, cov, torch.tensor([0.9]), None, torch.ones(1, 1, 1), torch.eye(4)[None], intr, torch.ones(1),
                   torch.full((1,), 100.0))
        bi = util.boundary_inputs(sc, H, W)
        args = (util.view_table(bi, dev), H, W, 0, bi["means"][0].to(dev), bi["cov6"][0].to(dev), bi["opac"].to(dev))
        with torch.no_grad():
            on = rasterize_views(*args, features=torch.ones(1, 1, device=dev), antialiasing=True)
            off = rasterize_views(*args, features=torch.ones(1, 1, device=dev))
        want = ref.isolated_want(d, 0.9)
        s_on, s_off = float(on[2].double().sum()), float(off[2].double().sum())
        inv_rho = np.sqrt(((a0 + 0.3) * (c0 + 0.3) - b * b) / (a0 * c0 - b * b))
        print(f"axes {d[0]:.2f} x {d[1]:.2f} px: antialiased / expected {s_on / want:.4f}, classic / expected {s_off / want:.4f}, "
              f"1 / rho {inv_rho:.3f}; replay {ref.isolated_mask_sum(d, 0.9, True) / want:.4f}")
        assert int(on[4][0, 0]) > 0
        assert abs(s_on / want - 1.0) <= 0.05
        assert s_off / want >= 1.1


# ---- surfaces ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_surfaces(hip_device):
    """GaussianRasterizer, render_cuda and GaussianScene.render with antialiasing=True are the corresponding rasterize_views
    call bit for bit; antialiasing=False everywhere is the call that omits the keyword."""
    import diff_gaussian_rasterization as dgr
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.rasterizer import _pack_view, rasterize_views
    dev = hip_device
    sc = util.make_scene(1500, image_size=64, views=2, color_sh_degree=2, feature_channels=4, feature_sh_degree=1, seed=31)
    bi = util.boundary_inputs(sc, H, W, bg=(0.1, 0.2, 0.3))
    cam = bi["cams"]
    with torch.no_grad():
        # the drop-in, one view per call
        means, cov6, opac, shs = (bi[k].to(dev) for k in ("means", "cov6", "opac", "shs"))
        feats = bi["features"].to(dev)
        imgs = {}
        for aa in (None, False, True):
            fields = dict(image_height=H, image_width=W, tanfovx=float(cam.tan_fov_x[0]), tanfovy=float(cam.tan_fov_y[0]),
                          bg=bi["bg"][0].to(dev), scale_modifier=1.0, viewmatrix=cam.view_matrix[0].to(dev),
                          projmatrix=cam.full_projection[0].to(dev), sh_degree=2, campos=cam.campos[0].to(dev), prefiltered=False,
                          debug=False)
            if aa is not None:
                fields["antialiasing"] = aa
            rs = dgr.GaussianRasterizationSettings(**fields)
            imgs[aa] = dgr.GaussianRasterizer(rs)(means[0], None, opac, shs=shs, features=feats[0], cov3D_precomp=cov6[0])
        table = _pack_view(rs, dev)
        want = rasterize_views(table, H, W, 2, means[0], cov6[0], opac, shs=shs, features=feats[0], antialiasing=True)
        got = imgs[True]
        assert torch.equal(got[0], want[0][0]) and torch.equal(got[1], want[1][0]) and torch.equal(got[2], want[2]) \
            and torch.equal(got[3], want[3]) and torch.equal(got[4], want[4][0])
        assert _same(imgs[False], imgs[None]) and not torch.equal(imgs[True][2], imgs[None][2])
        # the decoder's entry points
        V = 2
        args = (sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev), (H, W),
                torch.tensor([[0.1, 0.2, 0.3]]).expand(V, 3).to(dev), sc.means[None].expand(V, -1, -1).contiguous().to(dev),
                sc.covariances[None].expand(V, -1, -1, -1).contiguous().to(dev), sc.opacities[None].expand(V, -1).contiguous().to(dev),
                sc.color_sh[None].expand(V, -1, -1, -1).contiguous().to(dev), sc.feature_sh[None].expand(V, -1, -1, -1).contiguous().to(dev))
        on, off, omitted = cs.render_cuda(*args, antialiasing=True), cs.render_cuda(*args, antialiasing=False), cs.render_cuda(*args)
        views = cs._view_table(args[0], args[1], args[2], args[3], args[5], True)
        want = rasterize_views(views, H, W, 2, args[6], args[7], args[8][..., None], shs=args[9], shs_channel_major=True,
                               feature_sh=args[10], antialiasing=True)
        assert _same((on.color, on.feature, on.mask, on.depth), want[:4])
        assert _same((off.color, off.feature, off.mask, off.depth), (omitted.color, omitted.feature, omitted.mask, omitted.depth))
        assert not torch.equal(on.mask, off.mask)
        one = [x[:1] for x in args[6:]]           # the scene once, shared by its views
        scenes = cs.render_scenes(args[0][None], args[1][None], args[2][None], args[3][None], (H, W), args[5][0], *one,
                                  antialiasing=True)
        want = rasterize_views(views, H, W, 2, one[0][0], one[1][0], one[2][0][..., None], shs=one[3][0], shs_channel_major=True,
                               feature_sh=one[4][0], antialiasing=True)
        assert _same((scenes.color, scenes.feature, scenes.mask, scenes.depth), want[:4])
        s_args = (args[0][None], args[1][None], args[2][None], args[3][None], (H, W), args[5][0], *one)
        s_off, s_omitted = cs.render_scenes(*s_args, antialiasing=False), cs.render_scenes(*s_args)
        assert _same((s_off.color, s_off.feature, s_off.mask, s_off.depth),
                     (s_omitted.color, s_omitted.feature, s_omitted.mask, s_omitted.depth))
        assert not torch.equal(scenes.mask, s_off.mask)
        # the trainable scene, composed with the 3D filter
        scene = GaussianScene.from_point_cloud(sc.means.to(dev), torch.rand(1500, 3, generator=torch.Generator().manual_seed(2)).to(dev),
                                               sh_degree=2)
        tab = util.view_table(bi, dev)
        filt = scene.compute_filter_3d(tab, W)
        got = scene.render(tab, H, W, antialiasing=True, filter_3d=filt)
        shs_a, opac_a, cov_a, _, _ = scene._activate(1.0, False, filt)
        want = rasterize_views(tab, H, W, scene.active_sh_degree, scene._xyz, cov_a, opac_a, shs=shs_a, antialiasing=True)
        assert _same(got, want)
        assert _same(scene.render(tab, H, W, antialiasing=False, filter_3d=filt), scene.render(tab, H, W, filter_3d=filt))
        assert not torch.equal(got[2], scene.render(tab, H, W, filter_3d=filt)[2])
