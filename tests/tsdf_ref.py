"""Mesh extraction (include/lsr_mesh.h) restated in numpy: one statement of operator A (fusion of rendered depth into a
truncated signed distance volume) and of operator B (marching tetrahedra on the Kuhn subdivision), evaluated in float64
(the reference) and in float32 (the "stock" composition a user would write: the error yardstick), the case builders and
the mesh checks.  Cameras come from tests/normals_ref.py, and so does the error rule (:func:`tests.normals_ref.held`):
per quantity, the kernel's largest error against float64 is at most 4 x the stock composition's own.

Nearest-pixel rounding and the skips of the update rule are discrete, so :func:`integrate` (in float64) marks a lattice
point FRAGILE for a call when, for any view that is still alive for it at that step:
  * fx + 0.5 or fy + 0.5 lies within 1e-3 of an integer (image borders included);
  * |z| or clip.w lies within 1e-4 of 0;
  * |sdf + trunc| < 1e-4 trunc;  |d_world - depth_max| < 1e-4 depth_max;  |a - alpha_min| < 1e-4.
Fragile points are left out of the comparison; :func:`check_case` asserts that they are at most 5 % of the volume (about
0.4 % per view from the two pixel margins).  On every other point the weights must be EQUAL and the values are `held`.

Operator B gets the same float32 grid as the kernel, so classification is exact: faces must be EQUAL as integer arrays."""
import functools
import itertools

import numpy as np

from tests import normals_ref as nref

FRAGILE_MAX = 0.05
PERMS = list(itertools.permutations(range(3)))          # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


# ---- operator A ----

def lattice(dims):
    """(i, j, k) index arrays of shape (nz, ny, nx)."""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i, j, k


def empty_volume(dims, color=True):
    nx, ny, nz = dims
    return dict(tsdf=np.ones((nz, ny, nx), np.float32), weight=np.zeros((nz, ny, nx), np.float32),
                color=np.zeros((3, nz, ny, nx), np.float32) if color else None)


def project(view, origin, voxel_size, dims, dt):
    """(clip.x, clip.y, clip.w, z) of every lattice point under one view record, in ``dt``, literally as the header states
    it: x = origin + voxel_size (i, j, k); p = s x; the two matrices transposed as stored."""
    view = view.astype(dt)
    s = view[40]
    VM, PM = view[:16].reshape(4, 4).T, view[16:32].reshape(4, 4).T
    idx = lattice(dims)
    p = [s * (dt(origin[c]) + dt(voxel_size) * idx[c].astype(dt)) for c in range(3)]
    row = lambda M, r: M[r, 0] * p[0] + M[r, 1] * p[1] + M[r, 2] * p[2] + M[r, 3]
    return row(PM, 0), row(PM, 1), row(PM, 3), row(VM, 2)


def nearest_pixel(cx, cy, cw, H, W, dt):
    """(fx, fy) of step 4; ix = floor(fx + 0.5)."""
    with np.errstate(all="ignore"):
        fx = ((cx / cw + dt(1)) * dt(W) - dt(1)) / dt(2)
        fy = ((cy / cw + dt(1)) * dt(H) - dt(1)) / dt(2)
    return fx, fy


def integrate(volume, case, dt, lo=0, hi=None):
    """Views lo..hi of ``case`` fused into a copy of ``volume`` in ``dt``; the state between two views is float32, as the
    header has it.  Returns ``dict(tsdf, weight, color, fragile)`` (float32 arrays; ``fragile`` is meaningful in float64)."""
    dims, origin, vs, trunc = case["dims"], case["origin"], case["voxel_size"], case["trunc"]
    V, H, W = case["depth"].shape
    hi = V if hi is None else hi
    alpha_min, depth_max, max_weight = case["alpha_min"], case["depth_max"], case["max_weight"]
    tsdf, weight = volume["tsdf"].copy(), volume["weight"].copy()
    color = None if volume["color"] is None else volume["color"].copy()
    fragile = np.zeros(tsdf.shape, bool)
    near_int = lambda f: np.abs(f + 0.5 - np.round(f + 0.5)) < 1e-3
    for v in range(lo, hi):
        s = case["views"][v].astype(dt)[40]
        cx, cy, cw, z = project(case["views"][v], origin, vs, dims, dt)
        fragile |= (np.abs(z) < 1e-4) | (np.abs(cw) < 1e-4)
        live = (z > 0) & (cw > 0)
        fx, fy = nearest_pixel(cx, cy, cw, H, W, dt)
        with np.errstate(all="ignore"):
            fragile |= live & (near_int(fx) | near_int(fy))
            px, py = np.floor(fx + dt(0.5)), np.floor(fy + dt(0.5))
            live &= (px >= 0) & (px < W) & (py >= 0) & (py < H)
        ix, iy = np.where(live, px, 0).astype(np.int64), np.where(live, py, 0).astype(np.int64)
        a = case["alpha"][v][iy, ix].astype(dt)
        fragile |= live & (np.abs(a - alpha_min) < 1e-4)
        live &= a > dt(alpha_min)
        with np.errstate(all="ignore"):
            D = case["depth"][v][iy, ix].astype(dt) / a
        live &= np.isfinite(D) & (D > 0)
        with np.errstate(all="ignore"):
            d_world = D / s
            if depth_max:
                fragile |= live & (np.abs(d_world - depth_max) < 1e-4 * depth_max)
                live &= ~(d_world > dt(depth_max))
            sdf = (D - z) / s
            fragile |= live & (np.abs(sdf + trunc) < 1e-4 * trunc)
            live &= ~(sdf < -dt(trunc))
            d = np.minimum(dt(1), sdf / dt(trunc))
            w = weight.astype(dt)
            w1 = w + dt(1)
            tsdf = np.where(live, (tsdf.astype(dt) * w + d) / w1, tsdf).astype(np.float32)
            if color is not None:
                for c in range(3):
                    pix = case["image_color"][v, c][iy, ix].astype(dt)
                    color[c] = np.where(live, (color[c].astype(dt) * w + pix) / w1, color[c]).astype(np.float32)
            w1 = np.minimum(w1, dt(max_weight)) if max_weight else w1
            weight = np.where(live, w1, weight).astype(np.float32)
    return dict(tsdf=tsdf, weight=weight, color=color, fragile=fragile)


def fusion_case(dims, V, seed, color=True, voxel_size=0.02, trunc=None, H=20, W=24, scale40=(0.5, 1.0, 2.5), depth_max=None,
                max_weight=None, cameras=5, extrinsics=None, distance=4.0, centre=(0.0, 0.0, 0.0)) -> dict:
    """A volume centred on ``centre`` under ``V`` views (cyclic over ``cameras`` distinct cameras on a circle of radius 4
    with off-centre principal points, unequal fovs and slot 40 cycling over ``scale40``; or the given camera-to-world
    ``extrinsics``): a smooth surface ``D = plane + ripples`` at about ``distance`` under a smooth alpha in [0.6, 1) with holes of
    alpha 0.1, the depth stored as ``D s alpha`` as the rasterizer renders it."""
    rng = np.random.default_rng(seed)
    n_cam = min(cameras, V) if extrinsics is None else len(extrinsics)
    scales = np.array([scale40[c % len(scale40)] for c in range(n_cam)], np.float64)
    if extrinsics is None:
        cams = nref.make_views(n_cam, seed, offcentre=True, scale=scales)
    else:
        cams = nref.view_records(np.asarray(extrinsics), rng.uniform(0.3, 0.6, n_cam), rng.uniform(0.25, 0.5, n_cam),
                                 rng.uniform(-0.3, 0.3, n_cam), rng.uniform(-0.3, 0.3, n_cam), scales)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth, alpha, image = np.empty((n_cam, H, W), np.float32), np.empty((n_cam, H, W), np.float32), np.empty((n_cam, 3, H, W), np.float32)
    for c in range(n_cam):
        gx, gy, ph = rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0, 6.28, 2)
        D = distance + gx * (xs - W / 2) + gy * (ys - H / 2) + 0.05 * np.sin(0.37 * xs + ph[0]) * np.cos(0.29 * ys + ph[1])
        al = 0.8 + 0.19 * np.sin(0.21 * xs + 0.13 * ys + ph[0])
        for (y, x, h, w) in ((H // 2, W // 2, 1, 1), (1, 1, 1, 2), (H - 2, W - 3, 1, 1), (H // 3, 0, 2, 1), (5, 7, 3, 4)):
            al[y:y + h, x:x + w] = 0.1
        alpha[c] = al
        depth[c] = D * scales[c] * alpha[c].astype(np.float64)
        image[c] = rng.uniform(0, 1, (3, H, W))
    pick = np.arange(V) % n_cam
    trunc = 4.0 * voxel_size if trunc is None else trunc
    origin = tuple(float(np.float32(centre[c] - 0.5 * voxel_size * (dims[c] - 1))) for c in range(3))
    return dict(dims=tuple(dims), origin=origin, voxel_size=float(np.float32(voxel_size)), trunc=float(np.float32(trunc)),
                views=np.ascontiguousarray(cams[pick]), depth=np.ascontiguousarray(depth[pick]), alpha=np.ascontiguousarray(alpha[pick]),
                image_color=np.ascontiguousarray(image[pick]) if color else None, alpha_min=0.5,
                depth_max=depth_max, max_weight=max_weight, has_color=color)


FUSION_NX, FUSION_V = (2, 63, 64, 65, 130), (1, 3, 5)
# seeds picked on the CPU (tests/test_mesh_cpu.py holds them to it): 100 nx + V, moved on where that seed's single camera
# sees too little of the volume (fewer than a tenth of the points inside the truncation band)
_SEED_SHIFT = {(64, 1): 1, (65, 1): 1, (130, 1): 2}


# depth_max / max_weight cases over fusion_refs((130, 5, 3), 5, fusion_seed(130, 5)): the surface lies at about 4, so a
# depth_max there cuts through it; values at which no whole pixel sits within 1e-4 of the limit
LIMIT_CASES = (dict(depth_max=4.03), dict(max_weight=2.0), dict(depth_max=3.97, max_weight=1.0))


def fusion_seed(nx: int, V: int) -> int:
    return 100 * nx + V + _SEED_SHIFT.get((nx, V), 0)


@functools.lru_cache(maxsize=None)
def fusion_refs(dims, V, seed, color=True, kind="circle", **kw):
    """``(case, float64 result, float32 result)`` from an empty volume: computed once, shared, never modified.  ``kind``:
    "circle" (cameras around the volume), "inside" (INSIDE_KW: cameras inside a larger volume), "away" (AWAY_KW: cameras
    that see none of it)."""
    case = fusion_case(dims, V, seed, color, **dict({"circle": {}, "inside": INSIDE_KW, "away": AWAY_KW}[kind], **kw))
    start = empty_volume(dims, color)
    return case, integrate(start, case, np.float64), integrate(start, case, np.float32)


def look(position, forward, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """A camera-to-world matrix (x right, y down, z forward) at ``position`` looking along ``forward``."""
    f = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, np.cross(f, r), f, position
    return m


INSIDE_KW = dict(voxel_size=0.1, distance=1.5, extrinsics=(look((0.33, 0.04, 0.02), (1, 0.1, 0.05)), look((-0.41, -0.03, 0.01), (-1, 0.05, -0.1)),
                                                          look((1.07, 0.02, -0.04), (0.6, 0.2, 0.7))))
AWAY_KW = dict(extrinsics=(look((4.0, 0.0, 0.0), (1, 0, 0)), look((4.0, 0.3, 0.2), (0.1, 0, 1)), look((0.0, 0.0, -4.0), (1, 0, 0.3))))


def pixel_of(view: np.ndarray, point, H: int, W: int):
    """(fx, fy) of a world point under one record, in float64: steps 1..4 of the header."""
    view = view.astype(np.float64)
    p = np.append(view[40] * np.asarray(point, np.float64), 1.0)
    clip = view[16:32].reshape(4, 4).T @ p
    return ((clip[0] / clip[3] + 1) * W - 1) / 2, ((clip[1] / clip[3] + 1) * H - 1) / 2


def check_case(want: dict) -> float:
    """The fragile share of a float64 result: at most FRAGILE_MAX."""
    share = float(want["fragile"].mean())
    assert share <= FRAGILE_MAX, share
    return share


def compare_fusion(got: dict, want: dict, stock: dict, show: str = "") -> None:
    """The rule of the module docstring: weights EQUAL and values `held` on every point that is not fragile."""
    share = check_case(want)
    keep = ~want["fragile"]
    print(f"{show} fragile {share:.4f}  touched {float((want['weight'] > 0).mean()):.3f}")
    assert np.array_equal(np.asarray(got["weight"])[keep], want["weight"][keep]), show
    nref.held("tsdf", np.asarray(got["tsdf"])[keep], want["tsdf"][keep].astype(np.float64), stock["tsdf"][keep].astype(np.float64), show)
    if want["color"] is not None:
        k3 = np.broadcast_to(keep, want["color"].shape)
        nref.held("color", np.asarray(got["color"])[k3], want["color"][k3].astype(np.float64), stock["color"][k3].astype(np.float64), show)


# ---- operator B ----

def marching_tets(tsdf, weight, color, origin, voxel_size, min_weight=1.0, dt=np.float64):
    """``(vertices (Nv, 3), faces (Nf, 3) int32, colors (Nv, 3) or None)`` of float32 grids ``tsdf``, ``weight`` (nz, ny, nx) and
    ``color`` (3, nz, ny, nx), positions and colours evaluated in ``dt``.  The winding is decided GEOMETRICALLY here, on the
    midpoints of the crossed edges (never degenerate, and the orientation of a case does not depend on where along its
    edges the vertices sit): the kernels decide it from the case and the parity of the permutation."""
    nz, ny, nx = tsdf.shape
    n = (nx, ny, nz)
    valid, inside = weight >= np.float32(min_weight), tsdf < 0
    pad = lambda a, fill: np.pad(a, ((0, 1), (0, 1), (0, 1)), constant_values=fill)
    valid_p, inside_p, f_p = pad(valid, False), pad(inside, False), pad(tsdf, 0)
    shifted = lambda a, d: a[d[2]:d[2] + nz, d[1]:d[1] + ny, d[0]:d[0] + nx]
    deltas = [((e + 1) & 1, (e + 1) >> 1 & 1, (e + 1) >> 2) for e in range(7)]
    # vertices: by owner (x-fastest), then edge
    has = np.stack([valid & shifted(valid_p, d) & (inside != shifted(inside_p, d)) for d in deltas], -1)      # (nz, ny, nx, 7)
    vid = (np.cumsum(has.reshape(-1)) - 1).reshape(has.shape)
    vid = np.where(has, vid, -1)
    k, j, i, e = np.nonzero(has)
    d = np.array(deltas)[e]                                                                                  # (Nv, 3)
    fa, fb = tsdf[k, j, i].astype(dt), f_p[k + d[:, 2], j + d[:, 1], i + d[:, 0]].astype(dt)
    t = fa / (fa - fb)
    at = np.stack([i, j, k], -1).astype(dt)
    vertices = np.array(origin, np.float32).astype(dt) + dt(np.float32(voxel_size)) * (at + t[:, None] * d.astype(dt))
    colors = None
    if color is not None:
        ca = color[:, k, j, i].T.astype(dt)
        cb = np.stack([np.pad(color[c], ((0, 1), (0, 1), (0, 1)))[k + d[:, 2], j + d[:, 1], i + d[:, 0]] for c in range(3)], -1).astype(dt)
        colors = (dt(1) - t)[:, None] * ca + t[:, None] * cb
    # faces: by cube (x-fastest), tetrahedron, triangle
    corner = lambda q: np.array((q & 1, q >> 1 & 1, q >> 2))
    faces = []
    cube_in = np.stack([shifted(inside_p, corner(q)) for q in range(8)], -1)[:nz - 1, :ny - 1, :nx - 1]
    mixed = cube_in.any(-1) & ~cube_in.all(-1)
    for ck, cj, ci in zip(*np.nonzero(mixed)):
        base = np.array((ci, cj, ck))
        for perm in PERMS:
            c = [np.zeros(3, int)]
            for axis in perm:
                c.append(c[-1] + np.eye(3, dtype=int)[axis])
            pts = [base + x for x in c]
            if not all(valid[p[2], p[1], p[0]] for p in pts):
                continue
            ins = [m for m in range(4) if inside[pts[m][2], pts[m][1], pts[m][0]]]
            outs = [m for m in range(4) if m not in ins]
            if not ins or not outs:
                continue

            def vertex(m0, m1):
                lo, hi_ = min(m0, m1), max(m0, m1)
                dl = c[hi_] - c[lo]
                p = pts[lo]
                v = vid[p[2], p[1], p[0], dl[0] + 2 * dl[1] + 4 * dl[2] - 1]
                assert v >= 0
                return int(v), (pts[lo] + pts[hi_]) / 2.0

            if len(ins) == 1 or len(outs) == 1:
                lone, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                loop = [vertex(lone, m) for m in rest]
            else:
                A, B, C, D = ins[0], ins[1], outs[0], outs[1]
                loop = [vertex(A, C), vertex(A, D), vertex(B, D), vertex(B, C)]
            toward = np.mean([pts[m] for m in outs], 0) - np.mean([pts[m] for m in ins], 0)
            normal = np.cross(loop[1][1] - loop[0][1], loop[2][1] - loop[0][1])
            assert abs(normal @ toward) > 1e-9
            if normal @ toward < 0:
                loop = loop[::-1]
            ids = [v for v, _ in loop]
            r = ids.index(min(ids))
            ids = ids[r:] + ids[:r]
            faces.append(ids[:3])
            if len(ids) == 4:
                faces.append([ids[0], ids[2], ids[3]])
    return vertices, np.array(faces, np.int32).reshape(-1, 3), colors


def sphere_grid(n=24, radius=0.31, seed=0):
    """An analytic sphere inside the unit cube on an n^3 lattice: float32 ``tsdf`` (distance / trunc, clamped), ``weight`` 1,
    a smooth ``color``, ``origin``, ``voxel_size``; the centre is off the lattice, so that no sample is exactly 0."""
    vs = 1.0 / (n - 1)
    trunc = 4 * vs
    k, j, i = np.meshgrid(*(np.arange(n) * vs,) * 3, indexing="ij")
    centre = np.array([0.5, 0.5, 0.5]) + np.random.default_rng(seed).uniform(-0.3, 0.3, 3) * vs
    dist = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius
    tsdf = np.clip(dist / trunc, -1, 1).astype(np.float32)
    assert (tsdf != 0).all()
    color = np.stack([i, j, k]).astype(np.float32)
    return dict(tsdf=tsdf, weight=np.ones_like(tsdf), color=color, origin=(0.0, 0.0, 0.0), voxel_size=vs, radius=radius, dims=(n, n, n))


def random_grid(dims, seed, invalid=0.3, zeros=False):
    """A random float32 grid: ``tsdf`` uniform in [-1, 1] (with ``zeros``, a third of the samples exactly 0, the lattice's
    eight corners among them), ``weight`` 0 on a share ``invalid`` of the points and 1..3 elsewhere, random ``color``."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    if zeros:
        tsdf[rng.uniform(size=tsdf.shape) < 1 / 3] = 0.0
        tsdf[::nz - 1, ::ny - 1, ::nx - 1] = 0.0
    weight = np.where(rng.uniform(size=tsdf.shape) < invalid, 0.0, rng.integers(1, 4, tsdf.shape)).astype(np.float32)
    return dict(tsdf=tsdf, weight=weight, color=rng.uniform(0, 1, (3, nz, ny, nx)).astype(np.float32),
                origin=(-0.3, 0.2, 1.1), voxel_size=0.07, dims=tuple(dims))


def grid_mesh(grid: dict, min_weight=1.0, dt=np.float64):
    return marching_tets(grid["tsdf"], grid["weight"], grid["color"], grid["origin"], grid["voxel_size"], min_weight, dt)


def mesh_stats(vertices: np.ndarray, faces: np.ndarray) -> dict:
    """What a closed, consistently oriented manifold shows: ``directed_once`` (no directed edge appears twice), ``paired``
    (the reverse of every directed edge appears), ``euler`` = V - E + F over the vertices the faces use, ``area``, and
    ``outward`` (the signed volume: positive when the faces are wound counter-clockwise seen from outside)."""
    f = np.asarray(faces, np.int64)
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = edges[:, 0] * (int(f.max()) + 1 if f.size else 1) + edges[:, 1]
    rev = edges[:, 1] * (int(f.max()) + 1 if f.size else 1) + edges[:, 0]
    p = np.asarray(vertices, np.float64)[f]
    cross = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return dict(directed_once=len(np.unique(key)) == len(key), paired=bool(np.isin(rev, key).all()),
                euler=len(np.unique(f)) - len(key) // 2 + len(f), area=float(0.5 * np.linalg.norm(cross, axis=1).sum()),
                outward=float((p[:, 0] * cross).sum() / 6.0))
