"""Helpers of the COLMAP / image-preparation tests: a ``struct`` writer of the three model files in both formats, a float64
numpy restatement of ``lsr_image_prepare`` (include/lsr_image.h), and a synthetic-capture maker.

``python -m tests.colmap_ref DIR`` writes the set of model directories the sanitizer check of the reader runs over
(``make -C latentsplat_amd/csrc colmap-check MODELS=DIR``): the sample model in both formats, every proper prefix of each of
its binary files, and the malformed models of ``malformed_models``."""
from __future__ import annotations

import os
import struct
import sys

import numpy as np

MODEL_NAMES = {0: "SIMPLE_PINHOLE", 1: "PINHOLE", 2: "SIMPLE_RADIAL", 3: "RADIAL", 4: "OPENCV", 5: "OPENCV_FISHEYE"}
MODEL_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8}
BIN_FILES = ("cameras.bin", "images.bin", "points3D.bin")


# ---- the model writer ----

def sample_model(seed: int = 0) -> dict:
    """3 cameras (PINHOLE, SIMPLE_RADIAL, OPENCV), 5 images, 7 points with tracks; seeded doubles with all their bits."""
    rng = np.random.default_rng(seed)
    f = lambda n: [float(v) for v in rng.standard_normal(n)]
    cameras = [dict(id=1, model=1, width=640, height=480, params=[500.25 + rng.random(), 499.75, 320.5 + rng.random(), 239.125]),
               dict(id=7, model=2, width=37, height=29, params=[30.0 + rng.random(), 18.5, 14.5, 0.01 * rng.standard_normal()]),
               dict(id=3, model=4, width=1024, height=768, params=[800.0, 801.5, 500.0 + rng.random(), 390.0] + [0.1 * v for v in f(4)])]
    images = []
    for k, (iid, cam) in enumerate([(10, 1), (11, 7), (2, 3), (40, 1), (5, 3)]):
        obs = [(float(rng.random() * 100), float(rng.random() * 100), int(rng.integers(0, 7)) if rng.random() < 0.7 else 2 ** 64 - 1)
               for _ in range([3, 0, 5, 1, 0][k])]
        images.append(dict(id=iid, q=f(4), t=f(3), camera=cam, name=f"frame_{4 - k:03d}.npy" if k != 2 else "sub/dir/photo_2.png",
                           points2D=obs))
    points = []
    for k in range(7):
        track = [(int(images[int(rng.integers(0, 5))]["id"]), int(rng.integers(0, 50))) for _ in range(int(rng.integers(0, 5)))]
        points.append(dict(id=[1, 2, 3, 100, 2 ** 40 + 5, 6, 7][k], xyz=f(3), rgb=[int(v) for v in rng.integers(0, 256, 3)],
                           error=float(rng.random()), track=track))
    return dict(cameras=cameras, images=images, points=points)


def binary_files(model: dict) -> dict:
    """``{file name: bytes}`` of the three binary files."""
    cams = struct.pack("<Q", len(model["cameras"]))
    for c in model["cameras"]:
        cams += struct.pack("<IiQQ", c["id"], c["model"], c["width"], c["height"]) + struct.pack(f"<{len(c['params'])}d", *c["params"])
    imgs = struct.pack("<Q", len(model["images"]))
    for im in model["images"]:
        imgs += struct.pack("<I4d3dI", im["id"], *im["q"], *im["t"], im["camera"]) + im["name"].encode() + b"\0"
        imgs += struct.pack("<Q", len(im["points2D"]))
        for x, y, pid in im["points2D"]:
            imgs += struct.pack("<ddQ", x, y, pid)
    pts = struct.pack("<Q", len(model["points"]))
    for p in model["points"]:
        pts += struct.pack("<Q3d3BdQ", p["id"], *p["xyz"], *p["rgb"], p["error"], len(p["track"]))
        for iid, idx in p["track"]:
            pts += struct.pack("<II", iid, idx)
    return {"cameras.bin": cams, "images.bin": imgs, "points3D.bin": pts}


def text_files(model: dict) -> dict:
    """``{file name: bytes}`` of the three text files: ``repr`` doubles (they parse back to the same bits), ``#`` headers,
    an empty second line for an image without observations, -1 for an observation without a point."""
    cams = "# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n"
    for c in model["cameras"]:
        cams += " ".join([str(c["id"]), MODEL_NAMES[c["model"]], str(c["width"]), str(c["height"])] + [repr(v) for v in c["params"]]) + "\n"
    imgs = "# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n\n"
    for im in model["images"]:
        imgs += " ".join([str(im["id"])] + [repr(v) for v in im["q"] + im["t"]] + [str(im["camera"]), im["name"]]) + "\n"
        imgs += " ".join(f"{x!r} {y!r} {-1 if pid == 2 ** 64 - 1 else pid}" for x, y, pid in im["points2D"]) + "\n"
    pts = "# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n"
    for p in model["points"]:
        pts += " ".join([str(p["id"])] + [repr(v) for v in p["xyz"]] + [str(v) for v in p["rgb"]] + [repr(p["error"])]
                        + [f"{a} {b}" for a, b in p["track"]]) + "\n"
    return {"cameras.txt": cams.encode(), "images.txt": imgs.encode(), "points3D.txt": pts.encode()}


def write_files(directory, files: dict) -> str:
    os.makedirs(directory, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(directory, name), "wb") as f:
            f.write(data)
    return str(directory)


def malformed_models(model: dict):
    """``(label, files)`` of binary models the reader must refuse, one reason each."""
    good = binary_files(model)
    with_ = lambda **kw: {**good, **{k.replace("_bin", ".bin"): v for k, v in kw.items()}}
    edit = lambda **kw: binary_files({**model, **kw})

    def image_edit(k, **kw):
        images = [dict(im) for im in model["images"]]
        images[k].update(kw)
        return edit(images=images)

    huge = struct.pack("<Q", 2 ** 60)
    yield "count_2_60_cameras", with_(cameras_bin=huge + good["cameras.bin"][8:])
    yield "count_2_60_images", with_(images_bin=huge + good["images.bin"][8:])
    yield "count_2_60_points", with_(points3D_bin=huge + good["points3D.bin"][8:])
    cams = [dict(c) for c in model["cameras"]]
    cams[2].update(model=5)
    yield "unknown_model", edit(cameras=cams)
    cams = [dict(c) for c in model["cameras"]]
    cams[1].update(model=99)
    yield "model_id_99", edit(cameras=cams)
    yield "dangling_camera", image_edit(3, camera=12345)
    yield "duplicate_image_id", image_edit(4, id=model["images"][0]["id"])
    yield "nan_in_t", image_edit(1, t=[0.5, float("nan"), 1.0])
    yield "inf_in_q", image_edit(1, q=[float("inf"), 0.0, 0.0, 1.0])
    yield "zero_quaternion", image_edit(2, q=[0.0, 0.0, 0.0, 0.0])
    # the last image's name runs to the end of the file
    last = dict(model["images"][-1], points2D=[])
    body = binary_files({**model, "images": model["images"][:-1] + [last]})["images.bin"]
    yield "unterminated_name", with_(images_bin=body[:-9] + b"xxxxxxxxx")
    yield "name_too_long", image_edit(0, name="n" * 1024)
    yield "trailing_bytes_cameras", with_(cameras_bin=good["cameras.bin"] + b"\0")
    yield "trailing_bytes_images", with_(images_bin=good["images.bin"] + b"\0\0\0\0")
    yield "trailing_bytes_points", with_(points3D_bin=good["points3D.bin"] + b"\7")
    cams = [dict(c) for c in model["cameras"]]
    cams[0].update(width=0)
    yield "width_zero", edit(cameras=cams)
    cams = [dict(c) for c in model["cameras"]]
    cams[0].update(height=65537)
    yield "height_65537", edit(cameras=cams)
    cams = [dict(c) for c in model["cameras"]]
    cams[2].update(id=cams[0]["id"])
    yield "duplicate_camera_id", edit(cameras=cams)
    pts = [dict(p) for p in model["points"]]
    pts[3].update(id=pts[0]["id"])
    yield "duplicate_point_id", edit(points=pts)
    pts = [dict(p) for p in model["points"]]
    pts[2].update(xyz=[0.0, float("-inf"), 0.0])
    yield "inf_in_xyz", edit(points=pts)
    # an observation count far beyond the file: the skip is checked before seeking
    at = good["images.bin"].index(model["images"][0]["name"].encode() + b"\0") + len(model["images"][0]["name"]) + 1
    yield "observations_2_62", with_(images_bin=good["images.bin"][:at] + struct.pack("<Q", 2 ** 62) + good["images.bin"][at + 8:])


def proper_prefixes(model: dict):
    """``(label, files)``: for each binary file every proper prefix, the other two files intact."""
    good = binary_files(model)
    for name in BIN_FILES:
        for n in range(len(good[name])):
            yield f"{name}.{n:04d}", {**good, name: good[name][:n]}


# ---- rotations ----

def rotmat_to_qvec(R: np.ndarray) -> np.ndarray:
    """w x y z of a rotation matrix (float64), w >= 0."""
    R = np.asarray(R, np.float64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        s = 2 * np.sqrt(t + 1)
        q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, 0.0]
        q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q if q[0] >= 0 else -q


def qvec_to_rotmat(q: np.ndarray) -> np.ndarray:
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---- lsr_image_prepare in float64 ----

def camera_numbers(model: int, params) -> dict:
    """fx fy cx cy k1 k2 p1 p2 of a COLMAP model's parameters, as float32 values (what the kernel is handed) held in float64."""
    p = [float(np.float32(v)) for v in params]
    if model == 0:
        fx, fy, cx, cy, d = p[0], p[0], p[1], p[2], []
    elif model == 1:
        fx, fy, cx, cy, d = p[0], p[1], p[2], p[3], []
    elif model in (2, 3):
        fx, fy, cx, cy, d = p[0], p[0], p[1], p[2], p[3:]
    else:
        fx, fy, cx, cy, d = p[0], p[1], p[2], p[3], p[4:8]
    d = list(d) + [0.0] * (4 - len(d))
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, k1=d[0], k2=d[1], p1=d[2], p2=d[3])


def subsamples(cam: dict, fx_out: float, fy_out: float) -> int:
    sx = np.float32(cam["fx"]) / np.float32(fx_out)
    sy = np.float32(cam["fy"]) / np.float32(fy_out)
    return int(np.ceil(max(sx, sy, np.float32(1.0))))


def source_positions(cam: dict, Hs: int, Ws: int, H: int, W: int, fx_out: float, fy_out: float):
    """``(u, v)`` float64 arrays ``(H S, W S)`` of the sub-samples' source positions and ``S``; row ``i S + b``, column
    ``j S + a``."""
    fxo, fyo = float(np.float32(fx_out)), float(np.float32(fy_out))
    S = subsamples(cam, fx_out, fy_out)
    up = (np.arange(W)[:, None] + (np.arange(S)[None, :] + 0.5) / S).reshape(-1)[None, :]
    vp = (np.arange(H)[:, None] + (np.arange(S)[None, :] + 0.5) / S).reshape(-1)[:, None]
    dx, dy = up - W / 2.0, vp - H / 2.0
    if cam["k1"] == 0 and cam["k2"] == 0 and cam["p1"] == 0 and cam["p2"] == 0:
        u = dx * (cam["fx"] / fxo) + cam["cx"] + 0 * dy
        v = dy * (cam["fy"] / fyo) + cam["cy"] + 0 * dx
    else:
        x, y = dx / fxo + 0 * dy, dy / fyo + 0 * dx
        r2 = x * x + y * y
        radial = 1 + cam["k1"] * r2 + cam["k2"] * r2 * r2
        xd = x * radial + 2 * cam["p1"] * x * y + cam["p2"] * (r2 + 2 * x * x)
        yd = y * radial + 2 * cam["p2"] * x * y + cam["p1"] * (r2 + 2 * y * y)
        u, v = cam["fx"] * xd + cam["cx"], cam["fy"] * yd + cam["cy"]
    return u, v, S


def _sums(images_u8: np.ndarray, cam: dict, H: int, W: int, fx_out: float, fy_out: float, background, margin: float):
    B, Hs, Ws, C = images_u8.shape
    u, v, S = source_positions(cam, Hs, Ws, H, W, fx_out, fy_out)
    inside = (u >= 0) & (u <= Ws) & (v >= 0) & (v <= Hs)
    near = (np.minimum(np.abs(u), np.abs(u - Ws)) < margin) | (np.minimum(np.abs(v), np.abs(v - Hs)) < margin)
    xs, ys = u - 0.5, v - 0.5
    xf, yf = np.floor(xs), np.floor(ys)
    wx, wy = (xs - xf)[None, :, :, None], (ys - yf)[None, :, :, None]
    clampx = lambda a: np.clip(np.nan_to_num(a), 0, Ws - 1).astype(np.int64)
    clampy = lambda a: np.clip(np.nan_to_num(a), 0, Hs - 1).astype(np.int64)
    x0, x1, y0, y1 = clampx(xf), clampx(xf + 1), clampy(yf), clampy(yf + 1)
    src = images_u8.astype(np.float64)
    top = src[:, y0, x0] + wx * (src[:, y0, x1] - src[:, y0, x0])
    bot = src[:, y1, x0] + wx * (src[:, y1, x1] - src[:, y1, x0])
    val = top + wy * (bot - top)                                            # (B, H S, W S, C)
    if C == 4:
        bg = np.zeros(3) if background is None else np.asarray(background, np.float32).astype(np.float64)
        alpha = val[..., 3:4] / 255.0
        val = val[..., :3] * alpha + 255.0 * bg * (1.0 - alpha)
    val = np.where(inside[None, :, :, None], val, 0.0)
    block = lambda a: a.reshape(a.shape[0], H, S, W, S, *a.shape[3:]).sum(axis=(2, 4))
    total = block(val)                                                      # (B, H, W, 3)
    count = block(inside[None].astype(np.float64))[0]                       # (H, W)
    fragile = block(near[None].astype(np.float64))[0] > 0
    return total, count, fragile, S


def prepare_ref(images_u8: np.ndarray, cam: dict, H: int, W: int, fx_out: float, fy_out: float, background=None, margin: float = 1e-3):
    """``(image (B, 3, H, W), coverage (B, H, W), fragile (H, W))`` in float64: include/lsr_image.h restated.  ``fragile``
    marks the output pixels that own a sub-sample within ``margin`` source pixels of the source border on either axis,
    whose coverage float32 may decide the other way."""
    total, count, fragile, S = _sums(images_u8, cam, H, W, fx_out, fy_out, background, margin)
    image = np.where(count[None, :, :, None] > 0, total / np.maximum(255.0 * count, 1.0)[None, :, :, None], 0.0)
    return image.transpose(0, 3, 1, 2), np.broadcast_to(count / (S * S), (images_u8.shape[0], H, W)).copy(), fragile


def block_sums(images_u8: np.ndarray, cam: dict, H: int, W: int, fx_out: float, fy_out: float):
    """``(total (B, H, W, 3), count (H, W))`` of :func:`prepare_ref` before the division, for the exact path: the sums the
    library must reproduce bit for bit as ``float32(total) / float32(255 count)``."""
    return _sums(images_u8, cam, H, W, fx_out, fy_out, None, 1e-3)[:2]


def stock_prepare(images_u8, cam: dict, H: int, W: int, fx_out: float, fy_out: float, background=None):
    """The stock float32 composition on the images' own device: the sub-sample positions from elementwise torch operations,
    ``F.grid_sample(bilinear, align_corners=False, padding_mode="border")`` on the sub-sample grid, the coverage mask, and
    ``avg_pool2d``.  ``images_u8 (B, Hs, Ws, C)`` is a torch tensor; returns ``(image (B, 3, H, W), coverage (B, H, W))``."""
    import torch
    import torch.nn.functional as F
    dev = images_u8.device
    B, Hs, Ws, C = images_u8.shape
    S = subsamples(cam, fx_out, fy_out)
    f32 = lambda x: torch.tensor(float(x), dtype=torch.float32, device=dev)
    a = (torch.arange(S, dtype=torch.float32, device=dev) + 0.5) / S
    up = (torch.arange(W, dtype=torch.float32, device=dev)[:, None] + a[None, :]).reshape(1, -1)
    vp = (torch.arange(H, dtype=torch.float32, device=dev)[:, None] + a[None, :]).reshape(-1, 1)
    dx, dy = up - W / 2.0, vp - H / 2.0
    if cam["k1"] == 0 and cam["k2"] == 0 and cam["p1"] == 0 and cam["p2"] == 0:
        u = (dx * (f32(cam["fx"]) / f32(fx_out)) + f32(cam["cx"])).expand(H * S, W * S)
        v = (dy * (f32(cam["fy"]) / f32(fy_out)) + f32(cam["cy"])).expand(H * S, W * S)
    else:
        x, y = (dx / f32(fx_out)).expand(H * S, W * S), (dy / f32(fy_out)).expand(H * S, W * S)
        r2 = x * x + y * y
        radial = 1 + f32(cam["k1"]) * r2 + f32(cam["k2"]) * r2 * r2
        xd = x * radial + 2 * f32(cam["p1"]) * x * y + f32(cam["p2"]) * (r2 + 2 * x * x)
        yd = y * radial + 2 * f32(cam["p2"]) * x * y + f32(cam["p1"]) * (r2 + 2 * y * y)
        u, v = f32(cam["fx"]) * xd + f32(cam["cx"]), f32(cam["fy"]) * yd + f32(cam["cy"])
    grid = torch.stack([u / Ws * 2 - 1, v / Hs * 2 - 1], dim=-1)[None].expand(B, H * S, W * S, 2)
    val = F.grid_sample(images_u8.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="border", align_corners=False)
    if C == 4:
        bg = torch.zeros(3, device=dev) if background is None else background.to(dev).float()
        alpha = val[:, 3:4] / 255.0
        val = val[:, :3] * alpha + 255.0 * bg.view(1, 3, 1, 1) * (1.0 - alpha)
    inside = ((u >= 0) & (u <= Ws) & (v >= 0) & (v <= Hs)).float()[None, None]
    total = F.avg_pool2d(val * inside, S) * float(S * S)
    count = F.avg_pool2d(inside, S) * float(S * S)
    image = torch.where(count > 0, total / (255.0 * count.clamp_min(1.0)), torch.zeros_like(total))
    return image, (count / float(S * S))[:, 0].expand(B, H, W).contiguous()


# ---- a synthetic capture on disk ----

def write_capture(root, c2w: np.ndarray, cameras: list, camera_of: list, photographs: list, names: list, points_xyz: np.ndarray,
                  points_rgb: np.ndarray, fmt: str = "bin", sparse: str = "sparse/0", images: str = "images") -> dict:
    """A capture directory: ``cameras`` as in :func:`sample_model`, image ``k`` with the camera-to-world pose ``c2w[k]``
    (float64), the camera id ``camera_of[k]``, the uint8 HWC array ``photographs[k]`` stored under ``names[k]`` (``.npy``
    or ``.ppm``), and the points.  Returns the model dict."""
    ims = []
    for k, name in enumerate(names):
        w2c = np.linalg.inv(np.asarray(c2w[k], np.float64))
        ims.append(dict(id=k + 1, q=[float(v) for v in rotmat_to_qvec(w2c[:3, :3])], t=[float(v) for v in w2c[:3, 3]],
                        camera=camera_of[k], name=name, points2D=[]))
        path = os.path.join(str(root), images, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        a = np.ascontiguousarray(photographs[k])
        if name.endswith(".npy"):
            np.save(path, a)
        else:
            with open(path, "wb") as f:
                f.write(b"P6\n# a comment\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a[..., :3].tobytes())
    pts = [dict(id=k + 1, xyz=[float(v) for v in points_xyz[k]], rgb=[int(v) for v in points_rgb[k]], error=0.5, track=[])
           for k in range(len(points_xyz))]
    model = dict(cameras=cameras, images=ims, points=pts)
    write_files(os.path.join(str(root), sparse), binary_files(model) if fmt == "bin" else text_files(model))
    return model


def write_check_set(directory) -> int:
    model = sample_model()
    write_files(os.path.join(directory, "good_bin"), binary_files(model))
    write_files(os.path.join(directory, "good_txt"), text_files(model))
    n = 2
    for label, files in list(malformed_models(model)) + list(proper_prefixes(model)):
        write_files(os.path.join(directory, label), files)
        n += 1
    return n


if __name__ == "__main__":
    print(f"{write_check_set(sys.argv[1])} model directories written to {sys.argv[1]}")
