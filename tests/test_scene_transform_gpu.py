"""Similarity transforms of a GaussianScene on the MI355X: lsr_transform_records / lsr_scene_transform against the float64
restatement of tests/transform_ref.py within the rounding bounds derived there (u = 2^-24), the indexed path with its
bit-for-bit pass-through, in place against out of place, optional outputs behind guard words, the round trip, the
backward against float64 autograd, a render of the moved scene under moved cameras against the original image, the posed
render of GaussianScene, merge, and the tool.

The unit quaternion of a rotation is defined up to its sign; the restatement takes the sign of the library's record
(tests/transform_ref.quaternion, `like`), everything else comes from the 4x4 matrix alone."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import scene_params_ref as sref
from tests import sh_rotation_ref as shref
from tests import transform_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

NAMES = ref.NAMES
# the launch caps its grid at 4 rounds of 256 x 16 workgroups of 128 Gaussians (K = 4: the LDS rows allow the 16): one n just
# past it, where workgroups take a second chunk
PAST_THE_GRID = 4 * 256 * 16 * 128 + 5
UNIFORM = [(n, K) for n in (1, 63, 64, 65, 257, 1031) for K in (1, 4, 9, 16, 25)] + [(PAST_THE_GRID, 4)]
H = W = 64
G, VIEWS = 2000, 2


def _to(scene: dict, dev):
    return [scene[k].to(dev) for k in NAMES]


def _constants(M32: np.ndarray, K: int, dev):
    """The restatement's constants of each float32 matrix (T, 4, 4), the quaternion's sign taken from the library's records;
    the records are held to the constants here: the linear part and t bit for bit, log s, q_R and the band blocks to one
    rounding."""
    from latentsplat_amd.transform import transform_records
    M32 = np.asarray(M32, np.float32).reshape(-1, 4, 4)
    deg = ref.degree_of(K)
    rec = transform_records(torch.from_numpy(M32).to(dev), deg).cpu().numpy()
    assert rec.shape == (M32.shape[0], _lib.transform_record_floats(deg))
    consts = []
    for m, r in zip(M32, rec):
        c = ref.Constants(m, deg, like_q=r[13:17])
        assert np.array_equal(r[:9].reshape(3, 3), m[:3, :3]) and np.array_equal(r[9:12], m[:3, 3]) and not r[17:20].any()
        assert abs(r[12] - c.log_s) <= ref.U * abs(c.log_s) + 1e-12
        assert np.abs(r[13:17] - c.q).max() <= ref.U
        Tk = np.zeros_like(c.T.numpy())
        off = 20
        for l in range(1, deg + 1):
            n = 2 * l + 1
            Tk[l * l - 1:(l + 1) ** 2 - 1, l * l - 1:(l + 1) ** 2 - 1] = r[off:off + n * n].reshape(n, n)
            off += n * n
        assert off == r.size
        assert (np.abs(Tk - c.T.numpy()) <= ref.U * np.abs(c.T.numpy()) + 1e-12).all()
        consts.append(c)
    return consts


def _hold(got, want, bound, what, rows=None):
    """|got - want| <= bound element by element; prints the worst error / bound of each tensor."""
    worst = {}
    for k, g, w, b in zip(NAMES, got, want, bound):
        g = g.detach().cpu().to(torch.float64)
        if rows is not None:
            g, w, b = g[rows], w[rows], b[rows]
        err = (g - w).abs()
        assert torch.isfinite(g).all(), (what, k)
        ratio = err / b.clamp_min(1e-300)
        worst[k] = float(ratio.max()) if ratio.numel() else 0.0
        assert bool((err <= b).all()), f"{what}: {k} misses its bound, worst error / bound {worst[k]:.3f}"
    print(f"[transform] {what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("n,K", UNIFORM)
def test_parameters_match_the_restatement(hip_device, n, K):
    from latentsplat_amd.transform import transform_scene
    rng = np.random.default_rng(1000 * K + n)
    M = ref.random_similarity(rng)
    scene = ref.random_scene(n, K, seed=7 * n + K)
    c = _constants(M, K, hip_device)[0]
    got = transform_scene(*_to(scene, hip_device), torch.from_numpy(M).to(hip_device))
    x = ref.f64(scene)
    assert [tuple(g.shape) for g in got] == [tuple(t.shape) for t in x]
    _hold(got, ref.forward(c, *x), ref.bounds(c, *x), f"n={n} K={K}")
    # the norm of the raw quaternion is kept up to rounding
    assert torch.allclose(got[3].cpu().double().norm(dim=1), x[3].norm(dim=1), rtol=8 * ref.U, atol=0)


def test_special_rotations_and_scales(hip_device):
    from latentsplat_amd.transform import transform_scene
    n, K = 257, 25
    scene = ref.random_scene(n, K, seed=99)
    dev_scene, x = _to(scene, hip_device), ref.f64(scene)
    quarter = [shref.axis_rotation(a, s * np.pi / 2) for a in range(3) for s in (1, -1)]
    rotations = list(shref.special_rotations()) + quarter
    for i, R in enumerate(rotations):
        for s in (0.25, 1.0, 3.7):
            M = ref.matrix(R, [10.0 * (i % 3), -3.0, 0.5 * i], s)
            c = _constants(M, K, hip_device)[0]
            got = transform_scene(*dev_scene, torch.from_numpy(M).to(hip_device))
            _hold(got, ref.forward(c, *x), ref.bounds(c, *x), f"special rotation {i} scale {s}")
    # the identity leaves every coefficient as it is
    got = transform_scene(*dev_scene, torch.eye(4, device=hip_device))
    assert torch.equal(got[1].cpu(), scene["features_rest"]) and torch.equal(got[0].cpu(), scene["xyz"])


def _indexed_case(n, K, T, seed, dev):
    rng = np.random.default_rng(seed)
    M = np.stack([ref.random_similarity(rng) for _ in range(T)])
    scene = ref.random_scene(n, K, seed=seed + 1)
    idx = torch.from_numpy(rng.integers(-1, T + 1, size=n).astype(np.int32))
    idx[:4] = torch.tensor([-1, T, 0, T - 1], dtype=torch.int32)[:min(4, n)]
    return M, scene, idx


# T = 65 fits the LDS staging beside the rows at K = 16 and not at K = 25; T = 700 does not fit at any K.  With staged records
# the grid is capped at ONE round of the resident workgroups: one n just past that, where a workgroup takes a second chunk
# with the records it staged for the first
PAST_THE_STAGED_GRID = 256 * 16 * 128 + 5


@pytest.mark.parametrize("T,K,n", [(1, 16, 1031), (3, 4, 1031), (3, 1, 1031), (65, 16, 1031), (65, 25, 1031), (700, 16, 1031),
                                   (700, 9, 1031), (3, 4, PAST_THE_STAGED_GRID)])
def test_indexed_path(hip_device, T, K, n):
    from latentsplat_amd.transform import transform_scene, transform_scene_
    M, scene, idx = _indexed_case(n, K, T, 100 * T + K, hip_device)
    outside = (idx < 0) | (idx >= T)
    assert int(outside.sum()) >= 2 and int((idx == -1).sum()) >= 1 and int((idx == T).sum()) >= 1
    # out-of-range rows hold NaN and infinities: they must come out with the bits they went in with
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")])
    for k in NAMES:
        t = scene[k]
        rows = torch.nonzero(outside)[:, 0]
        flat = t[rows].reshape(len(rows), -1)
        flat[::2] = poison[torch.arange(flat.shape[1]) % 3]
        t[rows] = flat.reshape(t[rows].shape)
    consts = _constants(M, K, hip_device)
    Mt, it = torch.from_numpy(M).to(hip_device), idx.to(hip_device)
    dev_scene = _to(scene, hip_device)
    got = transform_scene(*dev_scene, Mt, it)
    inside = torch.nonzero(~outside)[:, 0]
    x = ref.f64(scene)
    xin = tuple(t[inside] for t in x)
    want = ref.apply_indexed(ref.forward, consts, idx[inside], xin)
    bound = ref.apply_indexed(ref.bounds, consts, idx[inside], xin)
    _hold([g[inside.to(hip_device)] for g in got], want, bound, f"indexed T={T} K={K}")
    rows = torch.nonzero(outside)[:, 0]
    for k, g, t in zip(NAMES, got, dev_scene):
        assert torch.equal(_bits(g)[rows], _bits(t)[rows]), f"{k}: out-of-range rows changed"
    # int64 indices are taken too; in place gives the same bits, the out-of-range rows included
    again = transform_scene(*dev_scene, Mt, it.long())
    inplace = [t.clone() for t in dev_scene]
    transform_scene_(*inplace, Mt, it)
    for k, a, b, g in zip(NAMES, again, inplace, got):
        assert torch.equal(_bits(a), _bits(g)) and torch.equal(_bits(b), _bits(g)), k


@pytest.mark.parametrize("K", [1, 4, 16, 25])
def test_in_place_equals_out_of_place_and_calls_repeat(hip_device, K):
    from latentsplat_amd.transform import transform_scene, transform_scene_
    n = 5000
    M = torch.from_numpy(ref.random_similarity(np.random.default_rng(K))).to(hip_device)
    dev_scene = _to(ref.random_scene(n, K, seed=K), hip_device)
    a, b = transform_scene(*dev_scene, M), transform_scene(*dev_scene, M)
    inplace = [t.clone() for t in dev_scene]
    transform_scene_(*inplace, M)
    for k, x, y, z in zip(NAMES, a, b, inplace):
        assert torch.equal(_bits(x), _bits(y)), f"{k}: two calls differ"
        assert torch.equal(_bits(x), _bits(z)), f"{k}: in place differs from out of place"


def test_optional_outputs_and_guard_words(hip_device):
    """Any subset of the four outputs: the wanted ones have the bits of the full call, the others are not touched, and the
    guard words behind every buffer are intact."""
    from latentsplat_amd.transform import apply_records, transform_records, transform_scene
    n, K, GUARD, MARK = 300, 9, 64, -7.25
    M = torch.from_numpy(ref.random_similarity(np.random.default_rng(4))).to(hip_device)
    dev_scene = dict(zip(NAMES, _to(ref.random_scene(n, K, seed=4), hip_device)))
    full = dict(zip(NAMES, transform_scene(*dev_scene.values(), M)))
    records = transform_records(M, 2)
    for r in range(5):
        for wanted in itertools.combinations(NAMES, r):
            flat = {k: torch.full((t.numel() + GUARD,), MARK, device=hip_device) for k, t in dev_scene.items()}
            outs = {k: flat[k][:dev_scene[k].numel()].view(dev_scene[k].shape) for k in wanted}
            apply_records(records, None, dev_scene, outs, n, K)
            for k in NAMES:
                body, guard = flat[k][:dev_scene[k].numel()], flat[k][dev_scene[k].numel():]
                assert bool((guard == MARK).all()), (wanted, k, "guard words written")
                if k in wanted:
                    assert torch.equal(_bits(body.view(dev_scene[k].shape)), _bits(full[k])), (wanted, k)
                else:
                    assert bool((body == MARK).all()), (wanted, k, "an unwanted output was written")
    # the inputs are only read
    for k, t in zip(NAMES, _to(ref.random_scene(n, K, seed=4), hip_device)):
        assert torch.equal(_bits(t), _bits(dev_scene[k])), k


def _round_trip_bound(c1, c2, x):
    """The sum of the two passes' bounds for x -> c1 -> c2: the first pass's bound carried through the second map's absolute
    values, plus the second pass's own bound at the first pass's float64 result.  Also returns that float64 composition."""
    y = ref.forward(c1, *x)
    z = ref.forward(c2, *y)
    b1, b2 = ref.bounds(c1, *x), ref.bounds(c2, *y)
    zero = [torch.zeros_like(t) for t in b1]
    through = [a - b for a, b in zip(ref.forward(_Abs(c2), *b1), ref.forward(_Abs(c2), *zero))]
    return z, [p + q for p, q in zip(through, b2)]


def _back_to_input(z, x):
    """The input as a round trip returns it: the quaternion up to the sign of q_R2 (x) q_R1, which is +1 or -1."""
    sign = 1.0 if float((z[3] * x[3]).sum()) > 0 else -1.0
    return (x[0], x[1], x[2], sign * x[3])


def test_round_trip(hip_device):
    """M, then invert_similarity(M) rounded to float32, returns every tensor to the INPUT within the sum of the two passes'
    bounds (the first pass's carried through the second map, plus the second's own); the quaternion up to the sign of
    q_R2 (x) q_R1.  The float64 composition of the two maps is held to the same sum."""
    from latentsplat_amd.transform import invert_similarity, transform_scene
    n, K = 1031, 25
    rng = np.random.default_rng(77)
    for trial in range(3):
        M1 = ref.random_similarity(rng, t_max=100.0)
        M2 = invert_similarity(torch.from_numpy(M1).double()).float().numpy()
        scene = ref.random_scene(n, K, seed=trial)
        c1, c2 = _constants(M1, K, hip_device)[0], _constants(M2, K, hip_device)[0]
        mid = transform_scene(*_to(scene, hip_device), torch.from_numpy(M1).to(hip_device))
        got = transform_scene(*mid, torch.from_numpy(M2).to(hip_device))
        x = ref.f64(scene)
        z, bound = _round_trip_bound(c1, c2, x)
        _hold(got, _back_to_input(z, x), bound, f"round trip {trial} against the input")
        _hold(got, z, bound, f"round trip {trial} against the float64 composition")


class _Abs:
    """The constants of a map with every entry replaced by its absolute value: what carries a bound through the map."""

    def __init__(self, c):
        self.A, self.t, self.log_s, self.L, self.T = c.A.abs(), torch.zeros_like(c.t), 0.0, c.L.abs(), c.T.abs()


@pytest.mark.parametrize("n,K,T", [(n, K, T) for n in (65, 1031) for K in (1, 16, 25) for T in (0, 3)])
def test_backward_matches_float64_autograd(hip_device, n, K, T):
    """T == 0: a uniform transform; otherwise T transforms with idx in [-1, T]."""
    from latentsplat_amd.transform import transform_scene
    seed = 10000 * n + 10 * K + T
    M, scene, idx = _indexed_case(n, K, max(T, 1), seed, hip_device)
    if T == 0:
        idx = None
    consts = _constants(M, K, hip_device)
    ups = ref.random_scene(n, K, seed=seed + 5)
    leaves = [t.clone().requires_grad_(True) for t in _to(scene, hip_device)]
    outs = transform_scene(*leaves, torch.from_numpy(M).to(hip_device), None if idx is None else idx.to(hip_device))
    torch.autograd.backward(outs, _to(ups, hip_device))
    x = [t.clone().requires_grad_(True) for t in ref.f64(scene)]
    g = ref.f64(ups)
    index = torch.zeros(n, dtype=torch.int32) if idx is None else idx
    torch.autograd.backward(ref.apply_indexed(ref.forward, consts, index, x), list(g))
    bound = ref.apply_indexed(ref.adjoint_bounds, consts, index, g)
    inside = torch.nonzero((index >= 0) & (index < len(consts)))[:, 0]
    _hold([t.grad for t in leaves], [t.grad for t in x], bound, f"backward n={n} K={K} T={T}", rows=inside)
    outside = torch.nonzero((index < 0) | (index >= len(consts)))[:, 0]
    for k, leaf, up in zip(NAMES, leaves, _to(ups, hip_device)):
        assert torch.equal(_bits(leaf.grad)[outside], _bits(up)[outside]), f"{k}: the gradient of an out-of-range row changed"
    # a tensor that does not require grad gets none; the others keep their bits
    frozen = [t.detach().clone().requires_grad_(i != 1) for i, t in enumerate(leaves)]
    torch.autograd.backward(transform_scene(*frozen, torch.from_numpy(M).to(hip_device), None if idx is None else idx.to(hip_device)),
                            _to(ups, hip_device))
    assert frozen[1].grad is None
    for i in (0, 2, 3):
        assert torch.equal(_bits(frozen[i].grad), _bits(leaves[i].grad))


# ---- the module: a moved scene under moved cameras, posed parts, merge, the tool ----

REST_SCALE = 2.0


def _degree3_scene(path, dev):
    """The scene of scene_params_ref.write_scene_file (2000 Gaussians in front of 2 cameras, degree 1, f_rest scaled by
    REST_SCALE) with seeded bands 2 and 3 added: every band the transform rotates is in the render."""
    from latentsplat_amd import GaussianScene
    sc, _, _ = sref.write_scene_file(path, G, W, VIEWS, rest_scale=REST_SCALE)
    low = GaussianScene.from_ply(path, dev)
    gen = torch.Generator().manual_seed(33)
    high = 0.15 * REST_SCALE * torch.randn(G, 12, 3, generator=gen)
    rest = torch.cat([low._features_rest.detach().cpu(), high], dim=1).to(dev)
    return sc, GaussianScene(low._xyz.detach(), low._features_dc.detach(), rest, low._opacity.detach(), low._scaling.detach(),
                             low._rotation.detach())


def _views(ext, sc, near, far, dev):
    from latentsplat_amd.rasterizer import build_view_table
    return build_view_table(ext.to(dev), sc.intrinsics.to(dev), near.to(dev), far.to(dev), torch.tensor([0.1, 0.2, 0.3], device=dev))


def _scene_from(params, like, dev):
    from latentsplat_amd import GaussianScene
    xyz, rest, scaling, rotation = (t.float().to(dev) for t in params)
    return GaussianScene(xyz, like._features_dc.detach(), rest, like._opacity.detach(), scaling, rotation)


def test_render_of_the_moved_scene_under_moved_cameras(hip_device, tmp_path):
    from latentsplat_amd.transform import similarity_matrix, transform_cameras
    dev = hip_device
    sc, scene = _degree3_scene(tmp_path / "scene.ply", dev)
    assert scene.max_sh_degree == 3
    M64 = similarity_matrix([0.8, 0.3, -0.4, 0.35], [1.5, -2.0, 0.75], 2.5)
    M32 = M64.float()
    ext2, near2, far2 = transform_cameras(sc.extrinsics, sc.near, sc.far, M32)
    with torch.no_grad():
        original = scene.render(_views(sc.extrinsics, sc, sc.near, sc.far, dev), H, W)[0].cpu().numpy()
        views2 = _views(ext2, sc, near2, far2, dev)
        c = _constants(M32.numpy(), 16, dev)[0]
        x = tuple(getattr(scene, "_" + k).detach().cpu().double() for k in NAMES)
        moved64 = ref.forward(c, *x)
        image64 = _scene_from(moved64, scene, dev).render(views2, H, W)[0].cpu().numpy()
        unrotated = _scene_from((moved64[0], x[1], moved64[2], moved64[3]), scene, dev).render(views2, H, W)[0].cpu().numpy()
        kernel_scene = _scene_from(x, scene, dev)
        assert kernel_scene.transform_(M32) is kernel_scene
        _hold([getattr(kernel_scene, "_" + k) for k in NAMES], moved64, ref.bounds(c, *x), "transform_ of the scene")
        image = kernel_scene.render(views2, H, W)[0].cpu().numpy()
    # the kernel's image against the image of the float64-moved parameters: the same cameras, inputs a few ulp apart.  The
    # project's image bar, 1e-4; a pixel next to one of the compositing discontinuities (alpha == 1/255, T == 1e-4) may take
    # the other branch and move by one alpha step, bounded at 2e-2, on at most 2 % of the pixels (util.assert_close_except_fragile)
    err = np.abs(image - image64).reshape(-1, H, W).max(0).reshape(-1)       # per pixel, over views and channels
    miss = err > 1e-4
    print(f"[transform] kernel-moved against float64-moved render: max {err.max():.2e}, {int(miss.sum())} of {err.size} pixels past 1e-4")
    assert miss.sum() <= max(8, int(0.02 * err.size)) and err.max() <= 2e-2
    mae, mae64, mae_unrotated = (float(np.abs(i - original).mean()) for i in (image, image64, unrotated))
    print(f"[transform] mean |moved render - original|: kernel {mae:.3e}, float64 parameters {mae64:.3e}, f_rest left unrotated {mae_unrotated:.3e}")
    assert original.std() > 0.05                                   # there is an image
    assert mae_unrotated >= 10 * mae64, "the scene's view dependence is too weak to test anything: raise REST_SCALE"
    assert mae <= 2 * mae64


def _posed_child():
    """Body of the LSR_DETERMINISTIC=1 child process of test_posed_render."""
    import tempfile
    from latentsplat_amd.rasterizer import rasterize_views
    from latentsplat_amd.scene_model import activate_scene
    from latentsplat_amd.transform import transform_scene
    dev = torch.device("cuda:0")
    ok, failure = True, ""
    try:
        with tempfile.TemporaryDirectory() as tmp:
            sc, scene = _degree3_scene(os.path.join(tmp, "scene.ply"), dev)
        rng = np.random.default_rng(8)
        M3 = torch.from_numpy(np.stack([ref.random_similarity(rng, t_max=0.3, s_range=(0.8, 1.25)) for _ in range(3)])).to(dev)
        idx = torch.from_numpy(rng.integers(-1, 4, size=G).astype(np.int32)).to(dev)
        views = _views(sc.extrinsics, sc, sc.near, sc.far, dev)
        cot = torch.randn((VIEWS, 3, H, W), generator=torch.Generator().manual_seed(3)).to(dev)
        posed = scene.render(views, H, W, transforms=M3, transform_idx=idx)[0]
        (posed * cot).sum().backward()
        got = {k: p.grad.clone() for k, p in scene.named_parameters()}
        # the same bits as a copy moved with transform_
        copy = _scene_from([getattr(scene, "_" + k).detach() for k in NAMES], scene, dev).transform_(M3, idx)
        with torch.no_grad():
            assert torch.equal(copy.render(views, H, W)[0], posed.detach()), "posed render differs from the render of the moved copy"
            # without the host check of the matrices (what a training loop passes): the same bits
            assert torch.equal(scene.render(views, H, W, transforms=M3, transform_idx=idx, check_transforms=False)[0], posed.detach())
        act = scene.activated(transforms=M3, transform_idx=idx)
        assert torch.equal(act.means.detach(), copy._xyz.detach()) and torch.equal(act.shs[:, 1:].detach(), copy._features_rest.detach())
        # the explicit chain, the same upstream gradient
        leaf = {k: p.detach().clone().requires_grad_(True) for k, p in scene.named_parameters()}
        xyz, rest, scaling, rotation = transform_scene(leaf["_xyz"], leaf["_features_rest"], leaf["_scaling"], leaf["_rotation"], M3, idx)
        shs, opac, cov = activate_scene(leaf["_features_dc"], rest, leaf["_opacity"], scaling, rotation)
        color = rasterize_views(views, H, W, scene.active_sh_degree, xyz, cov, opac, shs=shs)[0]
        assert torch.equal(color.detach(), posed.detach()), "the explicit chain renders other bits"
        (color * cot).sum().backward()
        for k in got:
            assert got[k].abs().max() > 0, k
            assert torch.equal(got[k].view(torch.int32), leaf[k].grad.view(torch.int32)), f"gradient of {k} differs from the explicit chain's"
        try:
            scene.render(views, H, W, transforms=M3, transform_idx=idx, filter_3d=torch.ones(G, device=dev))
            raise AssertionError("transforms together with filter_3d were accepted")
        except _lib.LsrError as e:
            assert "filter_3d" in str(e)
    except AssertionError as e:
        ok, failure = False, (str(e).splitlines() or ["assert"])[0]
    print("EQUAL", ok, failure)


def test_posed_render(hip_device):
    """LSR_DETERMINISTIC=1 (read once per process: a child): the rasterizer's gradient sums are order independent, so the
    gradients of the posed render at the canonical parameters must equal the explicit chain's bit for bit."""
    code = "import sys; sys.path.insert(0, %r)\nfrom tests import test_scene_transform_gpu as m\nm._posed_child()\n" % util.ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LSR_DETERMINISTIC="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("EQUAL True"), line


def test_merge(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    dev = hip_device
    n1, n2 = 700, 1300
    s1, s2 = ref.random_scene(n1, 4, seed=1), ref.random_scene(n2, 16, seed=2)
    gen = torch.Generator().manual_seed(5)
    mk = lambda s, n: GaussianScene(s["xyz"], torch.randn(n, 1, 3, generator=gen), s["features_rest"], 3 * torch.randn(n, 1, generator=gen),
                                    s["scaling"], s["rotation"]).to(dev)
    a, b = mk(s1, n1), mk(s2, n2)
    a.active_sh_degree = 0
    rng = np.random.default_rng(6)
    M = torch.from_numpy(np.stack([ref.random_similarity(rng, t_max=10.0) for _ in range(2)])).to(dev)
    merged = GaussianScene.merge([a, b], M)
    assert merged.num_gaussians == n1 + n2 and merged.max_sh_degree == 3 and merged.active_sh_degree == 3
    alone_a = mk(s1, n1)
    alone_a._features_dc.data.copy_(a._features_dc.data); alone_a._opacity.data.copy_(a._opacity.data)
    alone_a.transform_(M[0])
    alone_b = mk(s2, n2)
    alone_b.transform_(M[1])
    for k in ("_xyz", "_scaling", "_rotation"):
        assert torch.equal(_bits(getattr(merged, k))[:n1], _bits(getattr(alone_a, k))), k
        assert torch.equal(_bits(getattr(merged, k))[n1:], _bits(getattr(alone_b, k))), k
    assert torch.equal(_bits(merged._features_rest)[:n1, :3], _bits(alone_a._features_rest))
    assert not merged._features_rest[:n1, 3:].detach().any()                       # bands 2-3 of the degree-1 scene: exactly zero
    assert torch.equal(_bits(merged._features_rest)[n1:], _bits(alone_b._features_rest))
    assert torch.equal(merged._features_dc[:n1].detach(), a._features_dc.detach()) and torch.equal(merged._opacity[n1:].detach(), b._opacity.detach())
    # without transforms: the rows as they are
    plain = GaussianScene.merge([a, b])
    assert torch.equal(plain._xyz[:n1].detach(), a._xyz.detach()) and torch.equal(plain._features_rest[n1:].detach(), b._features_rest.detach())
    with pytest.raises(_lib.LsrError, match="one per scene"):
        GaussianScene.merge([a, b], M[:1])
    merged.save_ply(tmp_path / "merged.ply")
    back = GaussianScene.from_ply(tmp_path / "merged.ply", dev, check_opacity=False)
    assert torch.equal(_bits(back.rows()), _bits(merged.rows()))


def test_transform_tool(hip_device, tmp_path):
    from latentsplat_amd import GaussianScene
    from latentsplat_amd.transform import similarity_matrix
    path = tmp_path / "in.ply"
    sref.write_scene_file(path, G, W, VIEWS)
    tool = os.path.join(util.ROOT, "tools", "transform_ply.py")
    run = lambda *args: subprocess.run([sys.executable, tool, *map(str, args)], capture_output=True, text=True, timeout=240)
    args = ("--axis-angle", 1, 2, -0.5, 40, "--scale", 1.75, "--translate", 3, -1, 2)
    r = run(path, tmp_path / "out.ply", *args)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(line) == {"matrix", "gaussians"} and line["gaussians"] == G and len(line["matrix"]) == 16
    axis = np.array([1, 2, -0.5]) / np.linalg.norm([1, 2, -0.5])
    half = np.radians(40) / 2
    want = similarity_matrix(np.concatenate([[np.cos(half)], np.sin(half) * axis]), [3, -1, 2], 1.75)
    assert np.abs(np.array(line["matrix"]).reshape(4, 4) - want.numpy()).max() < 1e-12
    src, out = GaussianScene.from_ply(path, hip_device), GaussianScene.from_ply(tmp_path / "out.ply", hip_device)
    c = _constants(want.float().numpy(), 4, hip_device)[0]
    x = tuple(getattr(src, "_" + k).detach().cpu().double() for k in NAMES)
    _hold([getattr(out, "_" + k) for k in NAMES], ref.forward(c, *x), ref.bounds(c, *x), "tool")
    assert torch.equal(out._features_dc.detach(), src._features_dc.detach()) and torch.equal(out._opacity.detach(), src._opacity.detach())
    # --inverse brings it back: within the two passes' bounds, the first carried through the second map
    r = run(tmp_path / "out.ply", tmp_path / "back.ply", *args, "--inverse")
    assert r.returncode == 0, r.stderr[-2000:]
    inv = np.array(json.loads(r.stdout.strip().splitlines()[-1])["matrix"]).reshape(4, 4)
    assert np.abs(inv @ want.numpy() - np.eye(4)).max() < 1e-12
    c2 = _constants(inv.astype(np.float32), 4, hip_device)[0]
    back = GaussianScene.from_ply(tmp_path / "back.ply", hip_device)
    y = tuple(getattr(out, "_" + k).detach().cpu().double() for k in NAMES)
    got_back = [getattr(back, "_" + k) for k in NAMES]
    _hold(got_back, ref.forward(c2, *y), ref.bounds(c2, *y), "tool --inverse, second pass")
    z, bound = _round_trip_bound(c, c2, x)
    _hold(got_back, _back_to_input(z, x), bound, "tool --inverse against the source file")
    # --merge appends the other files as they are; --center and --unit-extent normalise
    r = run(path, tmp_path / "both.ply", "--scale", 2, "--merge", path, "--merge", tmp_path / "out.ply")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["gaussians"] == 3 * G
    both = GaussianScene.from_ply(tmp_path / "both.ply", hip_device)
    assert both.num_gaussians == 3 * G and torch.equal(both._xyz[G:2 * G].detach(), src._xyz.detach())
    assert torch.equal(both._xyz[2 * G:].detach(), out._xyz.detach())
    r = run(path, tmp_path / "unit.ply", "--center", "--unit-extent")
    assert r.returncode == 0, r.stderr[-2000:]
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    try:
        from render_ply import scene_extent
    finally:
        sys.path.pop(0)
    centre, extent = scene_extent(GaussianScene.from_ply(tmp_path / "unit.ply", hip_device)._xyz.detach())
    assert abs(float(extent) - 1) < 1e-4 and float(centre.abs().max()) < 1e-4
