"""A photographed capture as a trainer needs it: the COLMAP sparse model (cameras, poses, points) through the library's
strict host reader (csrc/colmap_reader.cpp; C ABI include/lsr_colmap.h), the photographs resampled onto the rasterizer's
centred, distortion-free camera in HIP (:mod:`latentsplat_amd.images`), a train / test split, and the camera tables, targets
and coverage maps that :class:`latentsplat_amd.scene_model.GaussianScene` and :func:`latentsplat_amd.losses.photometric_loss`
take.

:func:`read_colmap_model` and the host math (:func:`camera_to_world`, :func:`cameras_extent`, :func:`split_indices`,
:func:`target_size`, :func:`decode_ppm`, :func:`load_photograph`) need no GPU; :meth:`Capture.load` does (there is no CPU
fallback for the image preparation).

Conventions.  COLMAP's ``(q, t)`` is world-to-camera with x right, y down, z forward: the camera axes of this package, so
``extrinsics`` is just the inverse.  The rasterizer's camera has its principal point at the centre: ``intrinsics`` are
``fx' / W, fy' / H, 0.5, 0.5`` for the TARGET camera, and the photographs are moved onto it, not the camera onto them.
Tables built as ``tools/fit_ply.py`` builds them (``build_view_table`` with its default scale invariance) place the
rasterizer's near cull at ``0.2 x near``."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .images import SourceCamera, prepare_images


@dataclass
class ColmapModel:
    """A sparse model as the files hold it, in file order (numpy, host)."""
    format: str                    # "binary" or "text"
    camera_ids: np.ndarray         # (C,) uint32
    camera_models: np.ndarray      # (C,) int32: COLMAP's model ids, 0..4
    camera_sizes: np.ndarray       # (C, 2) int64: width, height
    camera_params: np.ndarray      # (C, 8) float64: the model's own order, zeros beyond
    image_ids: np.ndarray          # (I,) uint32
    qvec: np.ndarray               # (I, 4) float64: w x y z, world-to-camera, as stored
    tvec: np.ndarray               # (I, 3) float64
    image_camera_ids: np.ndarray   # (I,) uint32
    names: List[str]               # (I,)
    point_ids: np.ndarray          # (P,) uint64
    xyz: np.ndarray                # (P, 3) float64
    rgb: np.ndarray                # (P, 3) uint8
    errors: np.ndarray             # (P,) float64
    # the 2D observations that carry a point, read on request (read_colmap_model(observations=True)), else None
    obs_offsets: Optional[np.ndarray] = None     # (I + 1,) int64: image k (file order) owns [obs_offsets[k], obs_offsets[k + 1])
    obs_xy: Optional[np.ndarray] = None          # (M, 2) float64: COLMAP's measured position, in source pixels
    obs_point_ids: Optional[np.ndarray] = None   # (M,) uint64: ids of points3D


def _colmap_call(name: str, path, *args) -> None:
    lib = _lib.load()
    rc = getattr(lib, name)(os.fsencode(str(path)), *args)
    if rc != 0:
        raise _lib.LsrError(f"{name}({path}) failed: {lib.lsr_colmap_last_error().decode(errors='replace')} "
                            f"({lib.lsr_error_string(rc).decode()}, code {rc})")


def _p(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def read_colmap_model(path, observations: bool = False) -> ColmapModel:
    """The sparse model in the directory ``path``: ``cameras / images / points3D`` as ``.bin`` (taken when ``cameras.bin``
    is there) or ``.txt``.  Two phases, count and fill, both in the library; the tracks are skipped, and so are the 2D
    observations unless ``observations`` is set: then the model also carries, per image, the observations that have a 3D
    point (``obs_offsets``, ``obs_xy``, ``obs_point_ids``), and one that names a point the model does not have is refused
    with the image's name and the id.  Models ``SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV``; anything
    malformed is refused with the file, the record and the reason.  Host only."""
    counts = _lib.ColmapCounts()
    _colmap_call("lsr_colmap_count", path, C.byref(counts))
    nc, ni, npts = counts.cameras, counts.images, counts.points
    cam_ids, models = np.zeros(nc, np.uint32), np.zeros(nc, np.int32)
    sizes, params = np.zeros((nc, 2), np.int64), np.zeros((nc, _lib.COLMAP_MAX_PARAMS), np.float64)
    _colmap_call("lsr_colmap_read_cameras", path, _p(cam_ids), _p(models), _p(sizes), _p(params), nc)
    img_ids, img_cams = np.zeros(ni, np.uint32), np.zeros(ni, np.uint32)
    q, t = np.zeros((ni, 4), np.float64), np.zeros((ni, 3), np.float64)
    names, offsets = np.zeros(max(counts.name_bytes, 1), np.uint8), np.zeros(ni + 1, np.int64)
    _colmap_call("lsr_colmap_read_images", path, _p(img_ids), _p(q), _p(t), _p(img_cams), _p(names), _p(offsets), ni, counts.name_bytes)
    raw = names.tobytes()
    name_list = [os.fsdecode(raw[offsets[k]:offsets[k + 1] - 1]) for k in range(ni)]
    pt_ids, xyz = np.zeros(npts, np.uint64), np.zeros((npts, 3), np.float64)
    rgb, errors = np.zeros((npts, 3), np.uint8), np.zeros(npts, np.float64)
    _colmap_call("lsr_colmap_read_points", path, _p(pt_ids), _p(xyz), _p(rgb), _p(errors), npts)
    model = ColmapModel("binary" if counts.format == _lib.COLMAP_BINARY else "text", cam_ids, models, sizes, params, img_ids, q, t,
                        img_cams, name_list, pt_ids, xyz, rgb, errors)
    if observations:
        total = C.c_int64(0)
        _colmap_call("lsr_colmap_count_observations", path, C.byref(total))
        m = total.value
        obs_offsets, obs_xy, obs_ids = np.zeros(ni + 1, np.int64), np.zeros((m, 2), np.float64), np.zeros(m, np.uint64)
        _colmap_call("lsr_colmap_read_observations", path, _p(obs_offsets), _p(obs_xy), _p(obs_ids), ni, m)
        known = np.isin(obs_ids, pt_ids)
        if not known.all():
            at = int(np.flatnonzero(~known)[0])
            image = int(np.searchsorted(obs_offsets, at, side="right")) - 1
            raise _lib.LsrError(f"read_colmap_model({path}): image {name_list[image]!r} observes point {int(obs_ids[at])}, which the "
                                f"model does not have")
        model.obs_offsets, model.obs_xy, model.obs_point_ids = obs_offsets, obs_xy, obs_ids
    return model


# ---- host math ----

def camera_to_world(qvec: np.ndarray, tvec: np.ndarray) -> np.ndarray:
    """``(n, 4, 4)`` float64 camera-to-world matrices from COLMAP's world-to-camera ``qvec (n, 4)`` (w x y z, any non-zero
    norm) and ``tvec (n, 3)``: ``[R^T | -R^T t]`` with ``R`` the rotation of the normalised quaternion."""
    q = np.asarray(qvec, np.float64).reshape(-1, 4)
    t = np.asarray(tvec, np.float64).reshape(-1, 3)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    out = np.zeros((q.shape[0], 4, 4), np.float64)
    out[:, :3, :3] = R.transpose(0, 2, 1)
    out[:, :3, 3] = -np.einsum("nji,nj->ni", R, t)
    out[:, 3, 3] = 1.0
    return out


def cameras_extent(centres: np.ndarray) -> Tuple[np.ndarray, float]:
    """``(centre (3,), extent)``: the mean of the camera centres and 1.1 x the largest distance of a centre from it (the
    published trainer's scene normalisation; its learning rates and density thresholds are multiples of the extent)."""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    centre = c.mean(axis=0)
    return centre, 1.1 * float(np.linalg.norm(c - centre, axis=1).max())


def split_indices(count: int, hold: int = 8) -> Tuple[List[int], List[int]]:
    """``(train, test)`` index lists into the images sorted by name: every ``hold``-th image (0, hold, 2 hold, ...) is test
    (the published rule); ``hold = 0``: all train."""
    if hold < 0:
        raise _lib.LsrError("hold must not be negative")
    test = [k for k in range(count) if hold and k % hold == 0]
    return [k for k in range(count) if not (hold and k % hold == 0)], test


def target_size(src_width: int, src_height: int, resolution: float) -> Tuple[int, int]:
    """``(W, H) = (round(Ws / r), round(Hs / r))`` with Python's ``round`` (halves to even, as the published loader), at
    least 1."""
    if not resolution > 0:
        raise _lib.LsrError("resolution must be positive")
    return max(1, round(src_width / resolution)), max(1, round(src_height / resolution))


def decode_ppm(data: bytes, name: str = "<bytes>") -> np.ndarray:
    """A binary PPM (``P6``, maxval 255) as ``(H, W, 3)`` uint8, with numpy alone.  ``#`` comments in the header are
    skipped; anything else is refused with ``name``."""
    pos, fields = 0, []
    while len(fields) < 4:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if pos < len(data) and data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] != b"\n":
                pos += 1
            continue
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace():
            pos += 1
        if start == pos:
            raise _lib.LsrError(f"{name}: the PPM header ends early")
        fields.append(data[start:pos])
    if fields[0] != b"P6" or not all(f.isdigit() for f in fields[1:]):
        raise _lib.LsrError(f"{name}: not a binary PPM (P6)")
    w, h, maxval = (int(f) for f in fields[1:])
    if maxval != 255 or not (1 <= w <= _lib.IMAGE_MAX_EXTENT and 1 <= h <= _lib.IMAGE_MAX_EXTENT):
        raise _lib.LsrError(f"{name}: a PPM of maxval 255 and extents in 1..{_lib.IMAGE_MAX_EXTENT} is needed, got {w} x {h}, maxval {maxval}")
    pos += 1                                     # the single whitespace byte after maxval
    if len(data) - pos != 3 * w * h:
        raise _lib.LsrError(f"{name}: {len(data) - pos} bytes of pixels, {w} x {h} x 3 needs {3 * w * h}")
    return np.frombuffer(data, np.uint8, 3 * w * h, pos).reshape(h, w, 3)


def load_photograph(path) -> np.ndarray:
    """``(H, W, 3 or 4)`` uint8 from ``.npy`` (a uint8 HWC array) or a binary ``.ppm``, with numpy alone; any other format
    through PIL where it imports, and otherwise an error that names the file."""
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path, allow_pickle=False)
    elif ext == ".ppm":
        with open(path, "rb") as f:
            a = decode_ppm(f.read(), path)
    else:
        try:
            from PIL import Image
        except ImportError as e:
            raise _lib.LsrError(f"{path}: only .npy (uint8 HWC) and binary .ppm are decoded without PIL, and PIL does not "
                                f"import ({e}); convert the photograph or install Pillow") from e
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGBA" if "A" in im.getbands() else "RGB"))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise _lib.LsrError(f"{path}: a photograph must be uint8 of shape (H, W, 3 or 4), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


# ---- the capture ----

class Capture:
    """A loaded capture: :meth:`load`.  The images are ordered by name; every index below is into that order.

    Attributes: ``names``; ``extrinsics (N, 4, 4)`` camera-to-world and ``intrinsics (N, 3, 3)`` normalised, of the TARGET
    cameras, float32 on the device; ``near, far (N,)``; ``sizes``: ``(H, W)`` per image; ``centre (3,)`` and
    ``cameras_extent`` (float); ``model``: the :class:`ColmapModel`; ``source_cameras``: per image the
    :class:`latentsplat_amd.images.SourceCamera`; ``resolution``; ``device``."""

    def __init__(self):
        raise _lib.LsrError("use Capture.load(root)")

    @classmethod
    def load(cls, root, sparse: str = "sparse/0", images: str = "images", resolution: float = 1, device="cuda:0", *,
             near: Optional[float] = None, far: Optional[float] = None, background: Optional[Sequence[float]] = None,
             batch: int = 8, observations: bool = False) -> "Capture":
        """``root / sparse`` holds the model, ``root / images`` the photographs under the model's image names.  With
        ``resolution = r`` the targets are ``round(Ws / r) x round(Hs / r)`` with focal lengths ``fx / r, fy / r``.
        ``near`` / ``far`` default to ``0.01`` / ``100`` times ``cameras_extent``.  ``background (3,)``: what RGBA
        photographs are composited over (default black).  The photographs go to the device as uint8, ``batch`` at a time
        per camera, and only the float32 targets and coverage maps stay.  ``observations``: read the model's 2D
        observations too, which :meth:`sparse_depth` and :meth:`load_depth_priors` need."""
        self = object.__new__(cls)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.LsrError("Capture.load needs a ROCm device (no CPU fallback for the image preparation)")
        if batch < 1:
            raise _lib.LsrError("batch must be positive")
        model = read_colmap_model(os.path.join(str(root), sparse), observations=observations)
        if len(model.names) == 0:
            raise _lib.LsrError(f"{root}: the model has no images")
        order = sorted(range(len(model.names)), key=lambda k: model.names[k])
        self.model, self.device, self.resolution = model, dev, resolution
        self.names = [model.names[k] for k in order]
        self._rows = order                                        # image k of this capture is row _rows[k] of the model
        c2w = camera_to_world(model.qvec[order], model.tvec[order])
        centre, extent = cameras_extent(c2w[:, :3, 3])
        if not extent > 0.0:
            raise _lib.LsrError(f"{root}: the cameras span no extent (one image, or every camera at one point)")
        self.centre, self.cameras_extent = torch.from_numpy(centre.astype(np.float32)).to(dev), extent
        N = len(order)
        self.extrinsics = torch.from_numpy(c2w.astype(np.float32)).to(dev)
        self._near = 0.01 * extent if near is None else float(near)
        self.near = torch.full((N,), self._near, dtype=torch.float32, device=dev)
        self.far = torch.full((N,), 100.0 * extent if far is None else float(far), dtype=torch.float32, device=dev)
        row_of = {int(cid): k for k, cid in enumerate(model.camera_ids)}
        cam_row = [row_of[int(model.image_camera_ids[k])] for k in order]
        cams = [SourceCamera.from_colmap(int(model.camera_models[r]), model.camera_params[r]) for r in range(len(model.camera_ids))]
        self.source_cameras = [cams[r] for r in cam_row]
        intr = np.zeros((N, 3, 3), np.float32)
        self.sizes: List[Tuple[int, int]] = []
        self._source_sizes = [tuple(int(v) for v in model.camera_sizes[r]) for r in cam_row]      # (Ws, Hs) per image
        self._focal = [(cams[r].fx / resolution, cams[r].fy / resolution) for r in cam_row]       # of the target cameras, in pixels
        # depth supervision (latentsplat_amd.depth_sup): built on request, per output size like the targets
        self._sparse: Dict[Tuple[int, int], Tensor] = {}
        self._sparse_built: set = set()
        self._priors: Dict[Tuple[int, int], Tensor] = {}
        self._prior_affine: Optional[Tensor] = None
        for k, r in enumerate(cam_row):
            Ws, Hs = (int(v) for v in model.camera_sizes[r])
            W, H = target_size(Ws, Hs, resolution)
            intr[k] = [[cams[r].fx / resolution / W, 0, 0.5], [0, cams[r].fy / resolution / H, 0.5], [0, 0, 1]]
            self.sizes.append((H, W))
        self.intrinsics = torch.from_numpy(intr).to(dev)
        bg = None if background is None else torch.tensor([float(b) for b in background], dtype=torch.float32, device=dev)
        # targets and coverage per output size; _slot[k] = (size, row inside the group)
        self._targets: Dict[Tuple[int, int], Tensor] = {}
        self._coverage: Dict[Tuple[int, int], Tensor] = {}
        self._slot: List[Optional[Tuple[Tuple[int, int], int]]] = [None] * N
        members: Dict[Tuple[int, int], List[int]] = {}
        for k, size in enumerate(self.sizes):
            self._slot[k] = (size, len(members.setdefault(size, [])))
            members[size].append(k)
        for size, idx in members.items():
            self._targets[size] = torch.empty((len(idx), 3) + size, dtype=torch.float32, device=dev)
            self._coverage[size] = torch.empty((len(idx),) + size, dtype=torch.float32, device=dev)
        folder = os.path.join(str(root), images)
        for r in sorted(set(cam_row)):
            mine = [k for k in range(N) if cam_row[k] == r]
            Ws, Hs = (int(v) for v in model.camera_sizes[r])
            H, W = self.sizes[mine[0]]
            for at in range(0, len(mine), batch):
                chunk = mine[at:at + batch]
                photos = []
                for k in chunk:
                    a = load_photograph(os.path.join(folder, self.names[k]))
                    if a.shape[:2] != (Hs, Ws):
                        raise _lib.LsrError(f"{self.names[k]} is {a.shape[1]} x {a.shape[0]}, its camera {int(model.camera_ids[r])} says {Ws} x {Hs}")
                    photos.append(a)
                if len({a.shape[2] for a in photos}) != 1:        # RGB and RGBA in one chunk: one at a time
                    groups = [[k] for k in range(len(chunk))]
                else:
                    groups = [list(range(len(chunk)))]
                for g in groups:
                    u8 = torch.from_numpy(np.stack([photos[k] for k in g])).to(dev)
                    image, cover = prepare_images(u8, cams[r], H, W, cams[r].fx / resolution, cams[r].fy / resolution, bg)
                    rows = torch.tensor([self._slot[chunk[k]][1] for k in g], device=dev)
                    self._targets[(H, W)][rows] = image
                    self._coverage[(H, W)][rows] = cover
        pts = model.xyz.astype(np.float32)
        self._points = (torch.from_numpy(pts).to(dev), torch.from_numpy(model.rgb.astype(np.float32) / np.float32(255.0)).to(dev))
        return self

    def __len__(self) -> int:
        return len(self.names)

    def split(self, hold: int = 8) -> Tuple[List[int], List[int]]:
        """:func:`split_indices` over this capture's images (sorted by name)."""
        return split_indices(len(self.names), hold)

    def size_groups(self, idx: Optional[Sequence[int]] = None) -> Dict[Tuple[int, int], List[int]]:
        """``{(H, W): [indices]}`` of ``idx`` (default: all images): what can be rendered and compared in one batch."""
        out: Dict[Tuple[int, int], List[int]] = {}
        for k in (range(len(self.names)) if idx is None else idx):
            out.setdefault(self.sizes[k], []).append(int(k))
        return out

    def _index(self, idx) -> Tensor:
        idx = [int(k) for k in idx]
        if any(not 0 <= k < len(self.names) for k in idx):
            raise _lib.LsrError(f"image indices must lie in 0..{len(self.names) - 1}")
        return torch.tensor(idx, dtype=torch.long, device=self.device)

    def views(self, idx: Sequence[int], background: Tensor) -> Tensor:
        """The ``(V, 44)`` camera table of the images ``idx`` (:func:`latentsplat_amd.rasterizer.build_view_table`);
        ``background`` is ``(3,)`` or ``(V, 3)`` on the device."""
        from .rasterizer import build_view_table
        sel = self._index(idx)
        return build_view_table(self.extrinsics[sel], self.intrinsics[sel], self.near[sel], self.far[sel], background)

    def _gather(self, store: Dict[Tuple[int, int], Tensor], idx) -> Tensor:
        idx = [int(k) for k in idx]
        self._index(idx)
        sizes = {self.sizes[k] for k in idx}
        if len(sizes) != 1:
            raise _lib.LsrError(f"the images {idx} have {len(sizes)} output sizes; ask per size group (Capture.size_groups)")
        rows = torch.tensor([self._slot[k][1] for k in idx], dtype=torch.long, device=self.device)
        return store[sizes.pop()][rows]

    def targets(self, idx: Sequence[int]) -> Tensor:
        """``(V, 3, H, W)`` float32 targets of the images ``idx``, which must share one output size."""
        return self._gather(self._targets, idx)

    def coverage(self, idx: Sequence[int]) -> Tensor:
        """``(V, H, W)`` coverage of the images ``idx`` (1: the photograph covers the pixel, 0: it has nothing to say)."""
        return self._gather(self._coverage, idx)

    def _sparse_map(self, k: int) -> np.ndarray:
        from .depth_sup import sparse_inverse_depth
        (H, W), (fx, fy) = self.sizes[k], self._focal[k]
        return sparse_inverse_depth(self.model, self._rows[k], H, W, fx, fy, self._near)

    def sparse_depth(self, idx: Sequence[int]) -> Tensor:
        """``(V, H, W)`` float32: per image ``idx`` (one output size) the inverse depths of the sparse points it observes
        (:func:`latentsplat_amd.depth_sup.sparse_inverse_depth` through the target camera, ``near`` as the cut), 0 where
        there is none and where the coverage is 0.  Built on first use per image and kept.  Needs
        ``Capture.load(..., observations=True)``."""
        if self.model.obs_offsets is None:
            raise _lib.LsrError("sparse_depth needs the model's observations: this capture was loaded without them "
                                "(Capture.load(..., observations=True))")
        idx = [int(k) for k in idx]
        self._index(idx)
        for k in idx:
            if k not in self._sparse_built:
                size, row = self._slot[k]
                if size not in self._sparse:
                    self._sparse[size] = torch.zeros_like(self._coverage[size])
                m = torch.from_numpy(self._sparse_map(k)).to(self.device)
                self._sparse[size][row] = m * (self._coverage[size][row] > 0)
                self._sparse_built.add(k)
        return self._gather(self._sparse, idx)

    def load_depth_priors(self, folder) -> int:
        """Read one monocular inverse-depth prior per image from ``folder``: a 16-bit file
        (:func:`latentsplat_amd.depth_sup.load_depth_prior`) under the image's name, whole or without its extension, with
        one of ``.npy .pgm .png .tif .tiff`` appended.  Each is resampled onto the image's target camera
        (:func:`latentsplat_amd.depth_sup.prepare_depth_priors`; a prior of another size than the photograph is taken to
        cover the same field of view) and aligned to the sparse points (``align_depth_prior``, then ``reliable_alignments``
        over all images).  A missing file means that image has no prior: a zero map and the row ``(0, 0)``.  Returns the
        number of priors read.  Needs ``Capture.load(..., observations=True)``."""
        from .depth_sup import PRIOR_EXTENSIONS, align_depth_prior, load_depth_prior, prepare_depth_priors, reliable_alignments
        if self.model.obs_offsets is None:
            raise _lib.LsrError("load_depth_priors aligns the priors to the sparse points and needs the model's observations: "
                                "this capture was loaded without them (Capture.load(..., observations=True))")
        self._priors = {size: torch.zeros_like(c) for size, c in self._coverage.items()}
        affine = np.zeros((len(self.names), 2), np.float64)
        found = 0
        for k, name in enumerate(self.names):
            stems = [name, os.path.splitext(name)[0]]
            path = next((p for p in (os.path.join(str(folder), s + e) for s in stems for e in PRIOR_EXTENSIONS) if os.path.isfile(p)), None)
            if path is None:
                continue
            a = load_depth_prior(path)
            (Ws, Hs), (H, W), (fx, fy), cam = self._source_sizes[k], self.sizes[k], self._focal[k], self.source_cameras[k]
            sx, sy = a.shape[1] / Ws, a.shape[0] / Hs
            scaled = SourceCamera(cam.model, cam.fx * sx, cam.fy * sy, cam.cx * sx, cam.cy * sy, cam.dist)
            prior = prepare_depth_priors(a[None], scaled, H, W, fx, fy, self.device)[0]
            size, row = self._slot[k]
            self._priors[size][row] = prior
            affine[k] = align_depth_prior(self.sparse_depth([k])[0], prior)
            found += 1
        self._prior_affine = torch.from_numpy(reliable_alignments(affine).astype(np.float32)).to(self.device)
        return found

    def depth_priors(self, idx: Sequence[int]) -> Tuple[Tensor, Tensor]:
        """``(prior (V, H, W), affine (V, 2))`` of the images ``idx`` (one output size): the prepared priors and their
        ``(scale, offset)`` rows, ``(0, 0)`` for an image without a usable prior: what
        :func:`latentsplat_amd.depth_sup.inverse_depth_loss` takes as ``target`` and ``affine`` under ``align="given"``."""
        if self._prior_affine is None:
            raise _lib.LsrError("no depth priors have been loaded: Capture.load_depth_priors(folder)")
        return self._gather(self._priors, idx), self._prior_affine[self._index(idx)]

    @property
    def points(self) -> Tuple[Tensor, Tensor]:
        """``(xyz (P, 3) float32, rgb (P, 3) in [0, 1])`` of the sparse cloud, on the device."""
        return self._points

    def initial_scene(self, sh_degree: int = 3):
        """:meth:`latentsplat_amd.scene_model.GaussianScene.from_point_cloud` of the sparse cloud."""
        from .scene_model import GaussianScene
        xyz, rgb = self._points
        return GaussianScene.from_point_cloud(xyz, rgb, sh_degree=sh_degree)
