"""What the CPU oracle makes of non-finite and degenerate Gaussians (tests/poison_cases.py): the statement the HIP
kernels are held to in tests/test_poison_gpu.py, and a sanitizer run of the oracle's C on those scenes."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import poison_cases as pc
from tests import util

GX = (pc.SIZE + 15) // 16
T = GX * GX


@functools.lru_cache(maxsize=None)
def _case(cls):
    return pc.make(cls)


@functools.lru_cache(maxsize=None)
def _fwd(cls, which="bi"):
    c = _case(cls)
    return [util.oracle_forward(getattr(c, which), v) for v in range(pc.VIEWS)]


def _images(o):
    return [o[k] for k in ("color", "feature", "mask", "depth")]


def test_edited_rows_and_controls():
    for cls in ("A", "B", "C", "D", "AB"):
        c = _case(cls)
        assert {0, 63, 64, 65, pc.G - 1} <= set(c.rows.tolist()) and len(c.rows) <= pc.G // 10 and len(set(c.kinds)) == min(len(c.kinds), dict(A=10, B=10, C=6, D=4, AB=20)[cls])
        clean = np.setdiff1d(np.arange(pc.G), c.rows)
        for k in ("means", "cov6", "features"):
            assert np.array_equal(c.bi[k][:, clean].numpy().view(np.uint32), c.ctrl[k][:, clean].numpy().view(np.uint32)), (cls, k)
        for k in ("opac", "shs", "feature_sh"):
            assert np.array_equal(c.bi[k][clean].numpy().view(np.uint32), c.ctrl[k][clean].numpy().view(np.uint32)), (cls, k)
        # the control: finite everywhere, its edited rows behind every camera
        assert all(bool(np.isfinite(c.ctrl[k].numpy()).all()) for k in ("means", "cov6", "opac", "shs", "features", "feature_sh"))
        lab = util.clamp_replica(c.ctrl)
        assert (lab["t"][:, c.rows, 2] < 0).all() and lab["culled"][:, c.rows].all()
        for o in _fwd(cls, "ctrl"):
            assert (o["radii"][c.rows] == 0).all() and all(np.isfinite(img).all() for img in _images(o))
    assert pc.VIEWS * pc.G > 2048 and pc.G % 64 == 3
    assert len(pc.edited_rows(pc.G_CHUNKS, 10)) == 10 and pc.G_CHUNKS > 64 * 64


def test_class_a_is_culled_in_every_view():
    c = _case("A")
    assert len(c.rows) == 10
    for r in c.rows:     # every such row also carries a poisoned payload
        assert np.isnan(c.bi["opac"][r].numpy()).all() and np.isnan(c.bi["shs"][r].numpy()).all() and np.isnan(c.bi["features"][:, r].numpy()).all()
    for v, (o, oc) in enumerate(zip(_fwd("A"), _fwd("A", "ctrl"))):
        assert (o["radii"][c.rows] == 0).all() and (o["tiles_touched"][c.rows] == 0).all(), (v, dict(zip(c.kinds, o["radii"][c.rows])))
        assert all(np.isfinite(img).all() for img in _images(o))
        # ... and the culled rows leave no trace: the edited scene renders the control's bits
        assert o["P"] == oc["P"] and np.array_equal(o["point_list"], oc["point_list"]) and np.array_equal(o["radii"], oc["radii"])
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(_images(o), _images(oc)))


def test_classes_b_and_c_render_finite_images():
    b, c = _case("B"), _case("C")
    fb = _fwd("B")
    for o in fb + _fwd("C"):
        assert all(np.isfinite(img).all() for img in _images(o))
    kind = dict(zip(b.kinds, b.rows))
    radii = np.stack([o["radii"] for o in fb])                         # (V, G)
    rects = np.stack([o["rect"] for o in fb])
    for k in ("cov zero", "cov rank 1", "cov rank 2", "cov 1e-30 I", "cov 1e12 I"):
        assert (radii[:, kind[k]] > 0).all(), (k, radii[:, kind[k]])
    assert (radii[:, kind["cov zero"]] == 3).all()                     # the low-pass alone: a 0.3 px^2 blob
    assert (rects[:, kind["cov 1e12 I"]] == np.array([0, 0, GX, GX])).all() and (radii[:, kind["cov 1e12 I"]] > 1_000_000).all()
    assert (radii[:, kind["cov 1e18 I"]] == 0).all()                   # its determinant overflows: culled like 1e30 I
    centre = kind["mean at the camera centre of view 1"]
    assert radii[1, centre] == 0 and radii[0, centre] > 0 and radii[2, centre] > 0
    assert radii[0, kind["mean on the near-cull plane of view 0"]] == 0 and radii[0, kind["mean one ulp behind the near-cull plane"]] == 0
    assert radii[0, kind["mean one ulp in front of the near-cull plane"]] > 0
    for o in _fwd("C"):
        assert (o["radii"][c.rows] > 0).all()                          # the opacity culls nothing in the projection


def test_class_d_poisons_only_the_tiles_of_its_rectangles():
    c = _case("D")
    hit = False
    for v, (o, oc) in enumerate(zip(_fwd("D"), _fwd("D", "ctrl"))):
        assert (o["radii"][c.rows] > 0).all(), (v, o["radii"][c.rows])
        tiles = pc.rect_tiles(o, c.rows, GX)
        assert 1 <= len(tiles) <= 4, (v, sorted(tiles))
        for t in range(T):
            ty, tx = divmod(t, GX)
            sl = (Ellipsis, slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
            for a, b in zip(_images(o), _images(oc)):
                if t in tiles:
                    hit = hit or bool(np.isnan(a[sl]).any())
                else:   # not a NaN, and not a bit of difference to the control
                    assert np.array_equal(a[sl].view(np.uint32), b[sl].view(np.uint32)), (v, t)
    assert hit, "the oracle turns the pixels of the touched tiles into NaN"


@pytest.mark.parametrize("cls", ["A", "B", "C", "D"])
def test_radii_and_rectangles_stay_in_range(cls):
    for o in _fwd(cls):
        assert (o["radii"] >= 0).all()
        r = o["rect"]
        assert (r >= 0).all() and (r[:, [0, 2]] <= GX).all() and (r[:, [1, 3]] <= GX).all()
        assert (r[:, 0] <= r[:, 2]).all() and (r[:, 1] <= r[:, 3]).all()
        assert np.array_equal(o["tiles_touched"].astype(np.int64), (r[:, 2] - r[:, 0]).astype(np.int64) * (r[:, 3] - r[:, 1]))


def test_saturating_conversion_of_a_radius_beyond_int32():
    """A covariance whose 3-sigma radius is 2^31 px or more: the conversion saturates (rectangle = the whole grid, radius =
    INT_MAX, the Gaussian stays visible) instead of wrapping to INT_MIN (an empty rectangle / a "culled" negative radius)."""
    bi = pc._clone(_case("B").ctrl)
    r = 5
    bi["means"][:, r] = bi["means"].new_tensor(pc.place(0.5, 0.5, 5.0))
    bi["cov6"][:, r] = bi["cov6"].new_tensor(pc._eye(1e17))         # sigma_px^2 ~ 1e17 * (38.4 / 5)^2 = 6e18, det ~ 3.5e37 < FLT_MAX
    o = util.oracle_forward(bi, 0)
    assert o["radii"][r] == np.iinfo(np.int32).max and (o["rect"][r] == np.array([0, 0, GX, GX])).all()
    assert all(np.isfinite(img).all() for img in _images(o))


def test_oracle_runs_clean_under_the_undefined_behaviour_sanitizer(tmp_path):
    """raster_oracle.c + oracle/poison_driver.c (its own main, its own process) built with UBSan, float-cast-overflow included, on
    the class A + B scene: exit 0, i.e. no float -> int conversion of a NaN or of an out-of-range value is left."""
    c = _case("AB")
    assert len(c.rows) == 20
    here = os.path.join(util.ROOT, "oracle")
    exe, scene = str(tmp_path / "poison_driver"), str(tmp_path / "scene.bin")
    pc.write_flat_scene(scene, c.bi)
    cc = os.environ.get("CC", "gcc")
    build = subprocess.run([cc, "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas",
                            "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(here, "poison_driver.c"), os.path.join(here, "raster_oracle.c"), "-lm"],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, scene], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == pc.VIEWS
    for v, (line, o) in enumerate(zip(lines, [util.oracle_forward(c.bi, v) for v in range(pc.VIEWS)])):
        assert line == f"view {v}: pairs {o['P']} visible {int((o['radii'] > 0).sum())} non-finite pixels 0", line
