"""The COLMAP model reader (include/lsr_colmap.h, through ctypes; no GPU) and the host math of latentsplat_amd.capture:
both formats round-trip to the bits that were written, every proper prefix of every binary file and every malformed model
is refused with a negative code, and poses, split, extent and the photograph decoders are what the published loader's are."""
import ctypes as C
import os

import numpy as np
import pytest

from latentsplat_amd import _lib, capture
from tests import colmap_ref as cr

MODEL = cr.sample_model()
FIELDS = ("camera_ids", "camera_models", "camera_sizes", "camera_params", "image_ids", "qvec", "tvec", "image_camera_ids",
          "point_ids", "xyz", "rgb", "errors")


def _count(path):
    counts = _lib.ColmapCounts()
    return _lib.load().lsr_colmap_count(os.fsencode(str(path)), C.byref(counts)), counts


def test_both_formats_round_trip_to_the_written_bits(tmp_path):
    b = capture.read_colmap_model(cr.write_files(tmp_path / "bin", cr.binary_files(MODEL)))
    t = capture.read_colmap_model(cr.write_files(tmp_path / "txt", cr.text_files(MODEL)))
    assert (b.format, t.format) == ("binary", "text")
    for f in FIELDS:
        assert getattr(b, f).dtype == getattr(t, f).dtype and getattr(b, f).tobytes() == getattr(t, f).tobytes(), f
    assert b.names == t.names == [im["name"] for im in MODEL["images"]]
    # ... and to what was written: ids, sizes, and the doubles bit for bit
    assert b.camera_ids.tolist() == [c["id"] for c in MODEL["cameras"]] and b.camera_models.tolist() == [1, 2, 4]
    assert b.camera_sizes.tolist() == [[c["width"], c["height"]] for c in MODEL["cameras"]]
    for k, c in enumerate(MODEL["cameras"]):
        want = np.array(c["params"] + [0.0] * (8 - len(c["params"])), np.float64)
        assert b.camera_params[k].tobytes() == want.tobytes()
    assert b.image_ids.tolist() == [im["id"] for im in MODEL["images"]]
    assert b.image_camera_ids.tolist() == [im["camera"] for im in MODEL["images"]]
    assert b.qvec.tobytes() == np.array([im["q"] for im in MODEL["images"]], np.float64).tobytes()
    assert b.tvec.tobytes() == np.array([im["t"] for im in MODEL["images"]], np.float64).tobytes()
    assert b.point_ids.tolist() == [p["id"] for p in MODEL["points"]] and b.point_ids.dtype == np.uint64
    assert b.xyz.tobytes() == np.array([p["xyz"] for p in MODEL["points"]], np.float64).tobytes()
    assert b.rgb.tolist() == [p["rgb"] for p in MODEL["points"]]
    assert b.errors.tobytes() == np.array([p["error"] for p in MODEL["points"]], np.float64).tobytes()
    rc, counts = _count(tmp_path / "bin")
    assert rc == 0 and (counts.cameras, counts.images, counts.points, counts.format) == (3, 5, 7, _lib.COLMAP_BINARY)
    assert counts.name_bytes == sum(len(im["name"]) + 1 for im in MODEL["images"])
    assert _lib.load().lsr_colmap_last_error() == b""


def test_binary_is_preferred_and_all_five_models_are_read(tmp_path):
    model = dict(MODEL, cameras=[dict(id=k + 1, model=k, width=10 + k, height=20 + k, params=[float(v) for v in np.arange(cr.MODEL_PARAMS[k]) + 1.5])
                                 for k in range(5)],
                 images=[dict(im, camera=1 + k % 5) for k, im in enumerate(MODEL["images"])])
    other = dict(model, points=model["points"][:2])
    d = cr.write_files(tmp_path / "m", {**cr.binary_files(model), **cr.text_files(other)})
    got = capture.read_colmap_model(d)
    assert got.format == "binary" and len(got.point_ids) == 7 and got.camera_models.tolist() == [0, 1, 2, 3, 4]
    assert got.camera_params[3].tolist() == [1.5, 2.5, 3.5, 4.5, 5.5, 0, 0, 0]
    for name in cr.BIN_FILES:
        os.remove(os.path.join(d, name))
    assert capture.read_colmap_model(d).format == "text" and len(capture.read_colmap_model(d).point_ids) == 2


def test_every_proper_prefix_of_every_binary_file_is_refused(tmp_path):
    seen = 0
    for label, files in cr.proper_prefixes(MODEL):
        rc, _ = _count(cr.write_files(tmp_path / "m", files))
        assert rc < 0, label
        assert _lib.load().lsr_colmap_last_error().startswith(label.rsplit(".", 1)[0].encode()), label
        seen += 1
    assert seen == sum(len(v) for v in cr.binary_files(MODEL).values()) and seen > 300


MALFORMED = dict(cr.malformed_models(MODEL))


@pytest.mark.parametrize("label,code,words", [
    ("count_2_60_cameras", -1, "do not fit"), ("count_2_60_images", -1, "do not fit"), ("count_2_60_points", -1, "do not fit"),
    ("unknown_model", -5, "OPENCV_FISHEYE"), ("model_id_99", -5, "unknown model id 99"),
    ("dangling_camera", -1, "names camera 12345"), ("duplicate_image_id", -1, "image id is given twice"),
    ("nan_in_t", -1, "non-finite"), ("inf_in_q", -1, "non-finite"), ("zero_quaternion", -1, "zero quaternion"),
    ("unterminated_name", -1, "no terminator"), ("name_too_long", -1, "longer than 1023"),
    ("trailing_bytes_cameras", -1, "trailing"), ("trailing_bytes_images", -1, "trailing"), ("trailing_bytes_points", -1, "trailing"),
    ("width_zero", -1, "outside [1, 65536]"), ("height_65537", -1, "outside [1, 65536]"),
    ("duplicate_camera_id", -1, "camera id is given twice"), ("duplicate_point_id", -1, "point id is given twice"),
    ("inf_in_xyz", -1, "non-finite"), ("observations_2_62", -1, "observations"),
])
def test_malformed_models_are_refused(tmp_path, label, code, words):
    d = cr.write_files(tmp_path / label, MALFORMED[label])
    rc, _ = _count(d)
    assert rc == code
    assert words in _lib.load().lsr_colmap_last_error().decode()
    with pytest.raises(_lib.LsrError, match="lsr_colmap_count"):
        capture.read_colmap_model(d)


def test_every_malformed_model_has_a_case():
    assert len(MALFORMED) == 21


def test_missing_files_text_errors_and_capacities(tmp_path):
    lib = _lib.load()
    assert _count(tmp_path / "nowhere")[0] == -1 and b"cameras" in lib.lsr_colmap_last_error()
    good = cr.binary_files(MODEL)
    for name in cr.BIN_FILES[1:]:
        d = cr.write_files(tmp_path / ("without_" + name), {k: v for k, v in good.items() if k != name})
        assert _count(d)[0] == -1 and lib.lsr_colmap_last_error().startswith(name.encode())
    text = cr.text_files(MODEL)
    for label, name, old, new in [("model", "cameras.txt", b"OPENCV", b"FOV"), ("params", "cameras.txt", b" PINHOLE 640", b" SIMPLE_PINHOLE 640"),
                                  ("id", "images.txt", b"\n11 ", b"\n-11 "), ("rgb", "points3D.txt", b"\n100 ", b"\n100 0.5 ")]:
        assert old in text[name], label
        d = cr.write_files(tmp_path / ("text_" + label), {**text, name: text[name].replace(old, new, 1)})
        assert _count(d)[0] == (-5 if label == "model" else -1), label
    # phase two refuses a capacity smaller than the model and says so; NULL arrays are refused
    d = cr.write_files(tmp_path / "good", good).encode()
    ids, cams = np.zeros(5, np.uint32), np.zeros(5, np.uint32)
    q, t, names, offsets = np.zeros((5, 4)), np.zeros((5, 3)), np.zeros(256, np.uint8), np.zeros(6, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.lsr_colmap_read_images(d, p(ids), p(q), p(t), p(cams), p(names), p(offsets), 4, 256) == -1
    assert lib.lsr_colmap_read_images(d, p(ids), p(q), p(t), p(cams), p(names), p(offsets), 5, 20) == -1
    assert b"capacity" in lib.lsr_colmap_last_error()
    assert lib.lsr_colmap_read_images(d, p(ids), p(q), p(t), p(cams), p(names), p(offsets), 5, 256) == 0
    assert lib.lsr_colmap_read_images(d, None, p(q), p(t), p(cams), p(names), p(offsets), 5, 256) == -2
    assert lib.lsr_colmap_count(None, None) == -2


# ---- the host math of Capture ----

def test_pose_inversion_against_float64_numpy():
    rng = np.random.default_rng(3)
    q = rng.standard_normal((50, 4)) * rng.uniform(0.1, 10, (50, 1))          # not normalised, as a file may hold them
    t = rng.standard_normal((50, 3)) * 5
    got = capture.camera_to_world(q, t)
    assert got.dtype == np.float64
    for k in range(50):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = cr.qvec_to_rotmat(q[k]), t[k]
        assert np.abs(got[k] - np.linalg.inv(w2c)).max() < 1e-12
        assert np.abs(cr.qvec_to_rotmat(cr.rotmat_to_qvec(w2c[:3, :3])) - w2c[:3, :3]).max() < 1e-12     # (the helper's own inverse)
    # x right, y down, z forward: the identity pose looks down +z from -t
    eye = capture.camera_to_world([[2.0, 0, 0, 0]], [[1.0, 2.0, 3.0]])[0]
    assert np.array_equal(eye[:3, :3], np.eye(3)) and eye[:3, 3].tolist() == [-1.0, -2.0, -3.0]


def test_split_rule():
    assert capture.split_indices(20, 8) == ([k for k in range(20) if k % 8], [0, 8, 16])
    assert capture.split_indices(5, 0) == ([0, 1, 2, 3, 4], [])
    assert capture.split_indices(3, 1) == ([], [0, 1, 2])
    assert capture.split_indices(0, 8) == ([], [])
    with pytest.raises(_lib.LsrError):
        capture.split_indices(4, -1)


def test_cameras_extent_and_target_size():
    centres = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]])
    centre, extent = capture.cameras_extent(centres)
    assert centre.tolist() == [2.0, 2.0, 0.0] and extent == pytest.approx(1.1 * np.sqrt(8.0), rel=1e-15)
    rng = np.random.default_rng(0)
    c = rng.standard_normal((9, 3))
    centre, extent = capture.cameras_extent(c)
    assert np.allclose(centre, c.mean(0), atol=1e-15) and extent == pytest.approx(1.1 * np.linalg.norm(c - c.mean(0), axis=1).max(), rel=1e-15)
    assert capture.target_size(4946, 3286, 4) == (1236, 822)       # 1236.5 and 821.5: halves to even
    assert capture.target_size(37, 29, 2) == (18, 14) and capture.target_size(37, 29, 1) == (37, 29)
    assert capture.target_size(64, 48, 2.5) == (26, 19) and capture.target_size(3, 3, 16) == (1, 1)
    with pytest.raises(_lib.LsrError):
        capture.target_size(10, 10, 0)


def test_photograph_decoders(tmp_path):
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    head = b"P6\n# made by a test\n7 5\n255\n"
    assert np.array_equal(capture.decode_ppm(head + a.tobytes()), a)
    assert np.array_equal(capture.decode_ppm(b"P6 7 5 255\t" + a.tobytes()), a)
    for bad in (b"P5\n7 5\n255\n" + a.tobytes(), head + a.tobytes()[:-1], head + a.tobytes() + b"\0", b"P6\n7 5\n65535\n" + a.tobytes(),
                b"P6\n7 5\n", b"P6\n7 x\n255\n" + a.tobytes(), b""):
        with pytest.raises(_lib.LsrError, match="shot.ppm"):
            capture.decode_ppm(bad, "shot.ppm")
    (tmp_path / "a.ppm").write_bytes(head + a.tobytes())
    assert np.array_equal(capture.load_photograph(tmp_path / "a.ppm"), a)
    rgba = rng.integers(0, 256, (4, 6, 4), dtype=np.uint8)
    np.save(tmp_path / "b.npy", rgba)
    got = capture.load_photograph(tmp_path / "b.npy")
    assert np.array_equal(got, rgba) and got.flags["C_CONTIGUOUS"]
    np.save(tmp_path / "c.npy", rgba.astype(np.float32))
    with pytest.raises(_lib.LsrError, match="c.npy"):
        capture.load_photograph(tmp_path / "c.npy")
    np.save(tmp_path / "d.npy", rgba[..., 0])
    with pytest.raises(_lib.LsrError, match="d.npy"):
        capture.load_photograph(tmp_path / "d.npy")
    (tmp_path / "e.xyz").write_bytes(b"not an image")
    with pytest.raises(Exception, match="e.xyz"):
        capture.load_photograph(tmp_path / "e.xyz")


def test_source_camera_from_colmap_and_cpu_tensors_are_refused():
    import torch
    from latentsplat_amd.images import SourceCamera, prepare_images
    cam = SourceCamera.from_colmap(4, [1.0, 2, 3, 4, 5, 6, 7, 8])
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.dist) == (1.0, 2.0, 3.0, 4.0, (5.0, 6.0, 7.0, 8.0))
    cam = SourceCamera.from_colmap(2, [9.0, 3, 4, 0.5, 0, 0, 0, 0])
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.dist) == (9.0, 9.0, 3.0, 4.0, (0.5,))
    assert SourceCamera.from_colmap(0, [9.0, 3, 4]).dist == ()
    with pytest.raises(_lib.LsrError):
        SourceCamera.from_colmap(5, [1.0] * 8)
    with pytest.raises(_lib.LsrError):
        SourceCamera.from_colmap(1, [1.0] * 3)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        prepare_images(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), cam, 4, 4, 9.0, 9.0)


def test_image_prepare_refusals_come_before_any_gpu_work():
    """The host checks of lsr_image_prepare, with no device in the process: S = 17 and the other refusals return their codes
    with NULL buffers and batch 0 or 1, before a pointer is looked at or a kernel launched."""
    lib = _lib.load()
    dims = lambda **kw: _lib.ImageDims(**{**dict(batch=1, src_height=32, src_width=32, channels=3, height=8, width=8, fx=10.0, fy=10.0), **kw})
    cam = lambda **kw: _lib.ImageCamera(**{**dict(model=1, reserved=0, fx=40.0, fy=40.0, cx=16.0, cy=16.0), **kw})
    call = lambda d, c: lib.lsr_image_prepare(C.byref(d), C.byref(c), None, None, None, None, None)
    assert lib.lsr_image_subsamples(C.byref(dims()), C.byref(cam())) == 4
    assert lib.lsr_image_subsamples(C.byref(dims(fx=100.0, fy=100.0)), C.byref(cam())) == 1
    assert lib.lsr_image_subsamples(C.byref(dims(fx=16.0)), C.byref(cam())) == 4        # 2.5 -> 3, but fy gives 4
    assert lib.lsr_image_subsamples(C.byref(dims(fx=16.0, fy=16.0)), C.byref(cam())) == 3
    assert lib.lsr_image_subsamples(C.byref(dims()), C.byref(cam(fx=160.0))) == 16
    assert lib.lsr_image_subsamples(C.byref(dims()), C.byref(cam(fx=160.5))) == -5      # S = 17
    assert call(dims(), cam(fx=170.0)) == -5 and call(dims(batch=0), cam(fx=170.0)) == -5
    assert call(dims(), cam()) == -2                                                     # everything in order but the pointers
    assert call(dims(batch=0), cam()) == 0
    dist = lambda *v: (C.c_float * 4)(*v)
    for bad_d, bad_c in [(dims(channels=2), cam()), (dims(height=0), cam()), (dims(src_width=65537), cam()), (dims(batch=-1), cam()),
                         (dims(fx=0.0), cam()), (dims(), cam(model=5)), (dims(), cam(model=-1)), (dims(), cam(reserved=1)),
                         (dims(), cam(fy=float("nan"))), (dims(), cam(cx=float("inf"))), (dims(), cam(model=1, dist=dist(0.1, 0, 0, 0))),
                         (dims(), cam(model=2, dist=dist(0.1, 0.1, 0, 0))), (dims(), cam(model=3, dist=dist(0.1, 0.1, 0, 0.1)))]:
        assert call(bad_d, bad_c) == -1
    assert call(dims(src_height=65536, src_width=65536), cam()) == -5                    # 32-bit indices inside an image
    assert call(dims(batch=65536), cam()) == -5
    assert lib.lsr_image_prepare(None, None, None, None, None, None, None) == -2
