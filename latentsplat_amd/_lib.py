"""ctypes binding of ``liblsr_hip.so`` (C ABI: include/lsr_rasterizer.h, include/lsr_adapter.h, include/lsr_latent.h, include/lsr_ply.h,
include/lsr_sh_rotate.h, include/lsr_depth_head.h, include/lsr_scene.h, include/lsr_loss.h, include/lsr_density.h, include/lsr_optim.h, include/lsr_knn.h, include/lsr_mcmc.h, include/lsr_filter3d.h, include/lsr_bilagrid.h, include/lsr_transform.h, include/lsr_vq.h, include/lsr_pose.h, include/lsr_normals.h, include/lsr_mesh.h, include/lsr_nn.h, include/lsr_colmap.h, include/lsr_image.h, include/lsr_depth_loss.h, include/lsr_distortion.h).

The library is built in-tree by ``latentsplat_amd/csrc/Makefile`` (``__graft_entry__.build()``).
There is no CPU fallback: if the shared object is missing or not loadable this module raises, and
every product entry point above it fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# LSR_LIB selects an alternative build of the same library (kernel A/B experiments only)
_SO = os.environ.get("LSR_LIB") or os.path.join(_CSRC, "liblsr_hip.so")

VIEW_FLOATS = 44
COLOR_NONE, COLOR_SH, COLOR_PRECOMP = 0, 1, 2
FEAT_DIRECT, FEAT_SH = 0, 1
SH_AXES_3DGS, SH_AXES_REFERENCE = 0, 1   # lsr_dims.color_sh_convention
DEPTH_NATIVE, DEPTH_DEPTH, DEPTH_DISPARITY, DEPTH_RELATIVE_DISPARITY, DEPTH_LOG = 0, 1, 2, 3, 4   # LSR_DEPTH_*: view slot 41
FWD_FOR_BACKWARD = 1                      # lsr_dims.forward_flags
FWD_CLEARS_GRAD = 2
FWD_REACHED_ONLY = 4
FWD_FRONT_DONE = 8      # (ABI v10) lsr_forward_front has launched the front half of this forward
FWD_ANTIALIAS = 32      # opacity compensation for the 0.3 low-pass (bit 4 is reserved)
MAX_SH_GROUP_FLOATS = 120   # C*Kf the fused latent-SH path supports (LDS budget of sh.hip)
MAX_FEAT_CHANNELS = 32
ABSGRAD_MAX_CHANNELS = 4   # payload channels (colour counts 3) lsr_backward_absgrad supports: kAbsGradMaxChannels of csrc/lsr_internal.h


class LsrError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [("num_views", C.c_int32), ("num_gaussians", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("feat_channels", C.c_int32), ("color_mode", C.c_int32),
                ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32), ("vs_means", C.c_int64),
                ("vs_cov", C.c_int64), ("vs_opac", C.c_int64), ("vs_color", C.c_int64),
                ("vs_feat", C.c_int64), ("cov_elems", C.c_int32), ("feat_mode", C.c_int32),
                ("feat_sh_degree", C.c_int32), ("feat_sh_coeffs", C.c_int32),
                ("color_sh_channel_major", C.c_int32), ("views_per_group", C.c_int32),
                ("color_sh_convention", C.c_int32), ("forward_flags", C.c_int32), ("seg_cap_hint", C.c_int32)]


class Inputs(C.Structure):
    _fields_ = [("views", C.c_void_p), ("means3D", C.c_void_p), ("cov3D", C.c_void_p),
                ("opacities", C.c_void_p), ("color", C.c_void_p), ("features", C.c_void_p)]


class Outputs(C.Structure):
    _fields_ = [("color", C.c_void_p), ("feature", C.c_void_p), ("mask", C.c_void_p),
                ("depth", C.c_void_p), ("radii", C.c_void_p), ("grad_ws", C.c_void_p)]


class OutGrads(C.Structure):
    _fields_ = [("color", C.c_void_p), ("feature", C.c_void_p), ("mask", C.c_void_p),
                ("depth", C.c_void_p)]


class InGrads(C.Structure):
    _fields_ = [("means3D", C.c_void_p), ("cov3D", C.c_void_p), ("opacities", C.c_void_p),
                ("color", C.c_void_p), ("features", C.c_void_p), ("means2D", C.c_void_p)]


class Layout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in
                ("geom_rec", "geom_rec_floats", "geom_bin", "geom_tile_count", "geom_tile_start",
                 "geom_header", "bin_keys", "bin_point_list", "img_final_T", "img_n_contrib", "geom_bin_stride",
                 "bin_half_list", "geom_half_count", "geom_item_flags")]


class AdapterDims(C.Structure):      # lsr_adapter_dims (include/lsr_adapter.h, include/lsr_latent.h, include/lsr_ply.h)
    _fields_ = [("num_cameras", C.c_int32), ("rays", C.c_int32), ("samples", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("cov_elems", C.c_int32),
                ("scale_min", C.c_float), ("scale_max", C.c_float), ("eps", C.c_float),
                ("raw_stride", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


class AdapterInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("extrinsics", "intrinsics", "coordinates", "depths", "raw")]


class AdapterOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("means", "covariances", "scales", "rotations")]


class AdapterOutGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("means", "covariances", "scales", "rotations")]


class AdapterInGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("coordinates", "depths", "raw")]


class LatentDims(C.Structure):       # lsr_latent_dims (include/lsr_latent.h, include/lsr_ply.h)
    _fields_ = [("num_views", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("logvar_mode", C.c_int32), ("color_channels", C.c_int32),
                ("logvar_min", C.c_float), ("logvar_max", C.c_float),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


class LatentInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("features", "mask", "noise", "color")]


class LatentOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("skip", "z", "logvar")]


class LatentOutGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("skip", "z")]


class PlyInputs(C.Structure):        # lsr_ply_inputs (include/lsr_ply.h)
    _fields_ = [(n, C.c_void_p) for n in ("extrinsics", "means", "scales", "rotations", "harmonics",
                                          "opacities", "center", "scale_factor")]


PLY_VERTEX_FLOATS = 17
PLY_MAX_SH_COEFFS, PLY_MAX_REST, PLY_MAX_STRIDE = 25, 72, 8192   # LSR_PLY_MAX_*
PLY_OPACITY_RAW = 1                                               # lsr_ply_unpack flags


class PlyLayout(C.Structure):        # lsr_ply_layout (include/lsr_ply.h): where each named property sits inside a row
    _fields_ = [("n", C.c_int64), ("data_offset", C.c_int64), ("stride", C.c_int32), ("sh_coeffs", C.c_int32),
                ("xyz", C.c_int32 * 3), ("f_dc", C.c_int32 * 3), ("opacity", C.c_int32), ("scale", C.c_int32 * 3),
                ("rot", C.c_int32 * 4), ("f_rest", C.c_int32 * PLY_MAX_REST)]


class PlyOutputs(C.Structure):       # lsr_ply_outputs
    _fields_ = [(n, C.c_void_p) for n in ("means", "shs", "opacities", "scales", "rotations", "cov3D")]


class PlySceneInputs(C.Structure):   # lsr_ply_scene_inputs
    _fields_ = [(n, C.c_void_p) for n in ("means", "opacities", "shs", "cov", "scales", "rotations")] + \
               [(n, C.c_int32) for n in ("sh_coeffs", "sh_channel_major", "cov_elems", "reserved0")]


class PlySceneOpts(C.Structure):     # lsr_ply_scene_opts
    _fields_ = [(n, C.c_int32) for n in ("sh_convention", "sh_coeffs_out", "reserved0", "reserved1")]


def ply_scene_row_floats(sh_coeffs: int) -> int:
    """LSR_PLY_SCENE_ROW_FLOATS."""
    return 14 + 3 * sh_coeffs


class ShRotateDims(C.Structure):     # lsr_sh_rotate_dims (include/lsr_sh_rotate.h)
    _fields_ = [("num_cameras", C.c_int32), ("rays", C.c_int32), ("samples", C.c_int32),
                ("color_coeffs", C.c_int32), ("feat_channels", C.c_int32), ("feat_coeffs", C.c_int32),
                ("table_stride", C.c_int32), ("reserved0", C.c_int32), ("row_stride", C.c_int64)]


SH_ROTATE_MAX_DEGREE = 4


class DepthHeadDims(C.Structure):    # lsr_depth_head_dims (include/lsr_depth_head.h)
    _fields_ = [("num_cameras", C.c_int32), ("rays", C.c_int32), ("buckets", C.c_int32),
                ("surfaces", C.c_int32), ("samples", C.c_int32), ("flags", C.c_int32),
                ("opacity_exponent", C.c_float), ("opacity_scale", C.c_float),
                ("row_stride", C.c_int64), ("grad_row_stride", C.c_int64)]


DEPTH_HEAD_DETERMINISTIC, DEPTH_HEAD_TRANSMITTANCE = 1, 2   # lsr_depth_head_dims.flags
DEPTH_HEAD_MAX_BUCKETS, DEPTH_HEAD_MAX_SAMPLES, DEPTH_HEAD_MAX_ROW_FLOATS = 64, 8, 4096


class SceneParams(C.Structure):      # lsr_scene_params (include/lsr_scene.h)
    _fields_ = [(n, C.c_void_p) for n in ("features_dc", "features_rest", "opacity", "scaling", "rotation")]


class SceneDims(C.Structure):        # lsr_scene_dims
    _fields_ = [("n", C.c_int64), ("sh_coeffs", C.c_int32), ("scale_modifier", C.c_float),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


class SceneOutputs(C.Structure):     # lsr_scene_outputs
    _fields_ = [(n, C.c_void_p) for n in ("shs", "opacities", "cov3D", "scales", "rotations")]


class SceneOutGrads(C.Structure):    # lsr_scene_out_grads
    _fields_ = [(n, C.c_void_p) for n in ("shs", "opacities", "cov3D")]


class SceneInGrads(C.Structure):     # lsr_scene_in_grads
    _fields_ = [(n, C.c_void_p) for n in ("features_dc", "features_rest", "opacity", "scaling", "rotation")]


class PhotometricDims(C.Structure):  # lsr_photometric_dims (include/lsr_loss.h)
    _fields_ = [("num_images", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("lambda_dssim", C.c_float), ("cov_norm", C.c_float), ("crop", C.c_int32), ("reserved0", C.c_int32)]


class BilagridDims(C.Structure):     # lsr_bilagrid_dims (include/lsr_bilagrid.h)
    _fields_ = [(n, C.c_int32) for n in ("num_views", "height", "width", "num_grids", "grid_l", "grid_y", "grid_x", "reserved0")]


BILAGRID_MAX_XY, BILAGRID_MAX_L = 64, 16                            # LSR_BILAGRID_MAX_*


class DensifyParams(C.Structure):   # lsr_densify_params (include/lsr_density.h)
    _fields_ = [("grad_threshold", C.c_float), ("dense_extent", C.c_float), ("min_opacity", C.c_float),
                ("max_screen_size", C.c_float), ("world_limit", C.c_float), ("n_split", C.c_int32),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


class DensifyTable(C.Structure):    # lsr_densify_table
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_int32), ("rule", C.c_int32)]


DENSIFY_COPY, DENSIFY_ZERO_NEW, DENSIFY_XYZ, DENSIFY_SCALING = 0, 1, 2, 3   # lsr_densify_table.rule
DENSIFY_KEPT, DENSIFY_CLONE, DENSIFY_CHILD0 = 0, 1, 2                      # map kinds
DENSIFY_MAX_SPLIT, DENSIFY_MAX_TABLES, DENSIFY_MAX_WIDTH, DENSIFY_KIND_SHIFT, DENSIFY_MAX_ROWS = 8, 24, 4096, 28, 1 << 28


class AdamTable(C.Structure):       # lsr_adam_table (include/lsr_optim.h)
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("rows", C.c_int64), ("width", C.c_int32), ("reserved", C.c_int32), ("beta1", C.c_float), ("beta2", C.c_float),
                ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float), ("step_size", C.c_float), ("inv_sqrt_bc2", C.c_float), ("reserved_f", C.c_float)]


ADAM_MAX_TABLES, ADAM_MAX_WIDTH, ADAM_MAX_ROWS = 24, 4096, 1 << 40   # LSR_ADAM_MAX_*
KNN_MAX_POINTS = 1 << 28                                            # LSR_KNN_MAX_POINTS (include/lsr_knn.h)


class McmcTable(C.Structure):       # lsr_mcmc_table (include/lsr_mcmc.h)
    _fields_ = [("table", C.c_void_p), ("width", C.c_int32), ("role", C.c_int32)]


MCMC_COPY, MCMC_OPACITY, MCMC_SCALING, MCMC_MOMENT = 0, 1, 2, 3     # lsr_mcmc_table.role
MCMC_MAX_ROWS, MCMC_MAX_TABLES, MCMC_MAX_WIDTH, MCMC_MAX_RATIO, MCMC_WEIGHT_BITS = 1 << 28, 24, 4096, 50, 30   # LSR_MCMC_*
FILTER3D_PUBLISHED, FILTER3D_PER_VIEW = 0, 1                        # lsr_filter3d_compute mode (include/lsr_filter3d.h)
FILTER3D_MAX_ROWS, FILTER3D_MAX_VIEWS = 1 << 28, 65536              # LSR_FILTER3D_MAX_*


class TransformDims(C.Structure):    # lsr_transform_dims (include/lsr_transform.h)
    _fields_ = [("n", C.c_int64), ("sh_coeffs", C.c_int32), ("num_transforms", C.c_int32),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


class TransformIn(C.Structure):      # lsr_transform_in
    _fields_ = [(n, C.c_void_p) for n in ("xyz", "features_rest", "scaling", "rotation")]


class TransformOut(C.Structure):     # lsr_transform_out
    _fields_ = [(n, C.c_void_p) for n in ("xyz", "features_rest", "scaling", "rotation")]


TRANSFORM_MAX_DEGREE, TRANSFORM_HEADER_FLOATS = 4, 20               # LSR_TRANSFORM_*


class PoseGradIn(C.Structure):       # lsr_pose_grad_in (include/lsr_pose.h)
    _fields_ = [(n, C.c_void_p) for n in ("xyz", "rotation", "features_rest", "g_xyz", "g_features_rest", "g_scaling",
                                          "g_rotation")]


POSE_MAX_TRANSFORMS = 256                                           # LSR_POSE_MAX_TRANSFORMS


class VqDims(C.Structure):           # lsr_vq_dims (include/lsr_vq.h)
    _fields_ = [("n", C.c_int64), ("k", C.c_int32), ("d", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


VQ_MAX_DIM, VQ_MAX_CODES, VQ_MAX_ROWS = 96, 65536, 1 << 28          # LSR_VQ_MAX_*
VQ_ROWS, VQ_CODES, VQ_KSTEP = 128, 64, 4                            # LSR_VQ_ROWS / _CODES / _KSTEP: the tiling of lsr_vq_assign


class NormalDims(C.Structure):       # lsr_normal_dims (include/lsr_normals.h)
    _fields_ = [("num_images", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("alpha_min", C.c_float),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


NORMALS_MAX_ROWS, NORMALS_MAX_VIEWS = 1 << 28, 65536                # LSR_NORMALS_MAX_*


class TsdfDims(C.Structure):         # lsr_tsdf_dims (include/lsr_mesh.h)
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel_size", C.c_float),
                ("trunc", C.c_float), ("has_color", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32),
                ("reserved2", C.c_int32)]


TSDF_MIN_EXTENT, TSDF_MAX_EXTENT, TSDF_MAX_VOXELS, TSDF_MAX_VIEWS = 2, 2048, 1 << 30, 1024   # LSR_TSDF_*
MESH_MAX_ELEMENTS, MESH_COMPONENT_ROUNDS = 1 << 30, 64              # LSR_MESH_MAX_ELEMENTS; the cap of mesh.mesh_components


class ColmapCounts(C.Structure):     # lsr_colmap_counts (include/lsr_colmap.h)
    _fields_ = [("cameras", C.c_int64), ("images", C.c_int64), ("points", C.c_int64), ("name_bytes", C.c_int64),
                ("format", C.c_int32), ("reserved", C.c_int32)]


COLMAP_BINARY, COLMAP_TEXT = 0, 1                                   # lsr_colmap_counts.format
COLMAP_MAX_PARAMS, COLMAP_MAX_EXTENT, COLMAP_MAX_NAME = 8, 65536, 1023   # LSR_COLMAP_MAX_*
# COLMAP's model ids the reader takes: name, parameter count (f cx cy | fx fy cx cy | f cx cy k | f cx cy k1 k2 | fx fy cx cy k1 k2 p1 p2)
COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8)}


class ImageCamera(C.Structure):      # lsr_image_camera (include/lsr_image.h)
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("dist", C.c_float * 4)]


class ImageDims(C.Structure):        # lsr_image_dims
    _fields_ = [("batch", C.c_int32), ("src_height", C.c_int32), ("src_width", C.c_int32), ("channels", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("fx", C.c_float), ("fy", C.c_float)]


IMAGE_MAX_SUBSAMPLES, IMAGE_MAX_EXTENT = 16, 65536                  # LSR_IMAGE_MAX_*


class DepthLossDims(C.Structure):    # lsr_depth_loss_dims (include/lsr_depth_loss.h)
    _fields_ = [("num_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("align", C.c_int32),
                ("normalize", C.c_int32), ("alpha_min", C.c_float), ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


DEPTH_ALIGN_GIVEN, DEPTH_ALIGN_FIT = 0, 1                           # LSR_DEPTH_ALIGN_*
DEPTH_NORM_PIXELS, DEPTH_NORM_WEIGHTS = 0, 1                        # LSR_DEPTH_NORM_*
DEPTH_LOSS_CHUNK = 2048                                             # LSR_DEPTH_LOSS_CHUNK: pixels of a view per workgroup


class DistortionDims(C.Structure):   # lsr_distortion_dims (include/lsr_distortion.h)
    _fields_ = [("num_images", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved0", C.c_int32),
                ("reserved1", C.c_int32), ("reserved2", C.c_int32)]


DIST_LINEAR, DIST_NDC, DIST_DISPARITY = 0, 1, 2                     # LSR_DIST_*
DIST_MAX_ROWS, DIST_MAX_VIEWS = 1 << 28, 65536                      # LSR_DIST_MAX_*
DIST_THREADS, DIST_MAX_BLOCKS, DIST_CHUNK = 256, 2048, 2048         # LSR_DIST_THREADS / _MAX_BLOCKS / _CHUNK


def transform_record_floats(degree: int) -> int:
    """LSR_TRANSFORM_RECORD_FLOATS: the 20-float header and the band blocks 1..degree (20, 29, 54, 103, 184)."""
    return TRANSFORM_HEADER_FLOATS + sh_rotate_table_floats(degree) - 1


def sh_rotate_table_floats(degree: int) -> int:
    """LSR_SH_ROTATE_TABLE_FLOATS: sum of (2l+1)^2 over l <= degree."""
    return (degree + 1) * (2 * degree + 1) * (2 * degree + 3) // 3


_P, _I32, _I64, _SZ, _F, _INT, _STR = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float, C.c_int, C.c_char_p
_ptr_to = C.POINTER
_FWD = [_ptr_to(Dims), _ptr_to(Inputs), _P, _P, _P, _I64, _I32, _ptr_to(Outputs)]
_BWD = [_ptr_to(Dims), _ptr_to(Inputs), _P, _P, _P, _I64, _P, _ptr_to(Outputs), _ptr_to(OutGrads), _P, _ptr_to(InGrads), _P]
_SCENE = [_ptr_to(SceneDims), _ptr_to(SceneParams)]

# every export of the library: name -> (restype, argtypes); argtypes None = left unset (no arguments, or ctypes' conversions)
PROTOTYPES = {
    "lsr_abi_version": (_INT, None),
    "lsr_error_string": (_STR, [_INT]),
    "lsr_last_hip_error": (_INT, None),
    "lsr_geom_workspace_bytes": (_SZ, [_ptr_to(Dims)]),
    "lsr_image_workspace_bytes": (_SZ, [_ptr_to(Dims)]),
    "lsr_binning_workspace_bytes": (_SZ, [_ptr_to(Dims), _I64, _I32]),
    "lsr_grad_workspace_bytes": (_SZ, [_ptr_to(Dims)]),
    "lsr_get_layout": (_INT, [_ptr_to(Dims), _I64, _ptr_to(Layout)]),
    "lsr_build_views": (_INT, [_I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "lsr_build_views_depth": (_INT, [_I32, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "lsr_pack_view": (_INT, [_P, _P, _P, _P, _F, _F, _P, _P, _P, _P]),
    "lsr_forward_prepare": (_INT, [_ptr_to(Dims), _ptr_to(Inputs), _P, _P, _ptr_to(_I64), _ptr_to(_I32), _P]),
    "lsr_forward_render": (_INT, _FWD + [_P]),
    "lsr_forward_nosync": (_INT, _FWD + [_P]),
    "lsr_forward_speculative": (_INT, _FWD + [_ptr_to(_I64), _ptr_to(_I32), _ptr_to(_I32), _P]),
    "lsr_forward_front": (_INT, [_ptr_to(Dims), _ptr_to(Inputs), _P, _P, _I64, _P]),
    "lsr_forward_status": (_INT, [_ptr_to(Dims), _P, _ptr_to(_I64), _ptr_to(_I32), _ptr_to(_I32), _P]),
    "lsr_forward_abandon": (_INT, [_P]),
    "lsr_backward": (_INT, _BWD),
    "lsr_view_grad_workspace_bytes": (_SZ, [_ptr_to(Dims)]),
    "lsr_backward_views": (_INT, _BWD + [_P, _P]),
    "lsr_backward_absgrad": (_INT, _BWD + [_P, _P, _P]),
    "lsr_profile_enable": (None, [_INT]),
    "lsr_profile_num_stages": (_INT, None),
    "lsr_profile_stage_name": (_STR, [_INT]),
    "lsr_profile_read": (_INT, [_ptr_to(C.c_double), _ptr_to(_I64)]),
    "lsr_debug_set_knob": (_INT, [_STR, _INT]),
    "lsr_set_projection_contraction": (_INT, [_INT]),
    "lsr_get_projection_contraction": (_INT, None),
    "lsr_adapter_forward": (_INT, [_ptr_to(AdapterDims), _ptr_to(AdapterInputs), _ptr_to(AdapterOutputs), _P]),
    "lsr_adapter_backward": (_INT, [_ptr_to(AdapterDims), _ptr_to(AdapterInputs), _ptr_to(AdapterOutGrads),
                                    _ptr_to(AdapterInGrads), _P]),
    "lsr_latent_forward": (_INT, [_ptr_to(LatentDims), _ptr_to(LatentInputs), _ptr_to(LatentOutputs), _P]),
    "lsr_latent_backward": (_INT, [_ptr_to(LatentDims), _ptr_to(LatentInputs), _ptr_to(LatentOutGrads), _P, _P]),
    "lsr_ply_pack": (_INT, [_I64, _I32, _ptr_to(PlyInputs), _P, _P]),
    "lsr_ply_write_host": (_INT, [_STR, _P, _I64]),
    "lsr_ply_read_header": (_INT, [_STR, _ptr_to(PlyLayout)]),
    "lsr_ply_read_rows": (_INT, [_STR, _P, _I64]),
    "lsr_ply_unpack": (_INT, [_ptr_to(PlyLayout), _P, _I32, _ptr_to(PlyOutputs), _P]),
    "lsr_ply_pack_scene": (_INT, [_I64, _ptr_to(PlySceneInputs), _ptr_to(PlySceneOpts), _P, _P]),
    "lsr_ply_sh_axes_matrix": (_INT, [_P]),
    "lsr_ply_write_scene_host": (_INT, [_STR, _P, _I64, _I32]),
    "lsr_sh_rotation_matrices": (_INT, [_I32, _P, _I64, _I64, _I32, _P, _P]),
    "lsr_sh_rotate_forward": (_INT, [_ptr_to(ShRotateDims)] + [_P] * 7),
    "lsr_sh_rotate_backward": (_INT, [_ptr_to(ShRotateDims)] + [_P] * 7),
    "lsr_depth_head_forward": (_INT, [_ptr_to(DepthHeadDims)] + [_P] * 8),
    "lsr_depth_head_backward": (_INT, [_ptr_to(DepthHeadDims)] + [_P] * 8),
    "lsr_scene_activate_forward": (_INT, _SCENE + [_ptr_to(SceneOutputs), _P]),
    "lsr_scene_activate_backward": (_INT, _SCENE + [_ptr_to(SceneOutGrads), _ptr_to(SceneInGrads), _P]),
    "lsr_photometric_workspace_bytes": (_SZ, [_ptr_to(PhotometricDims)]),
    "lsr_photometric_forward": (_INT, [_ptr_to(PhotometricDims)] + [_P] * 9),
    "lsr_photometric_backward": (_INT, [_ptr_to(PhotometricDims)] + [_P] * 6),
    "lsr_density_accumulate": (_INT, [_I32, _I64, _P, _P, _P, _P, _P, _P]),
    "lsr_densify_workspace_bytes": (_SZ, [_I64]),
    "lsr_densify_plan": (_INT, [_I64, _P, _P, _P, _P, _P, _ptr_to(DensifyParams), _P, _I64, _P, _P, _P]),
    "lsr_densify_apply": (_INT, [_I64, _I64, _P, _P, _I32, _ptr_to(DensifyTable), _I32, _P, _P, _P, _I64, _P]),
    "lsr_adam_step": (_INT, [_ptr_to(AdamTable), _I32, _P, _I64, _P]),
    "lsr_knn3_workspace_bytes": (_SZ, [_I64]),
    "lsr_knn3": (_INT, [_I64, _P, _P, _P, _P, _P, _P]),
    "lsr_ply_read_points_header": (_INT, [_STR, _ptr_to(_I64), _ptr_to(_I32)]),
    "lsr_ply_read_points": (_INT, [_STR, _P, _P, _I64]),
    "lsr_mcmc_workspace_bytes": (_SZ, [_I64, _I64]),
    "lsr_mcmc_classify": (_INT, [_I64, _P, _F, _P, _P, _P, _P, _P]),
    "lsr_mcmc_sample": (_INT, [_I64, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "lsr_mcmc_apply": (_INT, [_I64, _I64, _P, _P, _P, _ptr_to(McmcTable), _I32, _F, _P, _P]),
    "lsr_mcmc_noise": (_INT, [_I64, _P, _P, _P, _P, _P, _F, _P]),
    "lsr_filter3d_workspace_bytes": (_SZ, [_I64, _I32]),
    "lsr_filter3d_compute": (_INT, [_I64, _P, _I32, _P, _I32, _F, _F, _I32, _P, _P, _P, _P]),
    "lsr_scene_activate_filtered_forward": (_INT, _SCENE + [_P, _ptr_to(SceneOutputs), _P]),
    "lsr_scene_activate_filtered_backward": (_INT, _SCENE + [_P, _ptr_to(SceneOutGrads), _ptr_to(SceneInGrads), _P]),
    "lsr_bilagrid_slice_path": (_INT, [_ptr_to(BilagridDims)]),
    "lsr_bilagrid_slice_forward": (_INT, [_ptr_to(BilagridDims)] + [_P] * 5),
    "lsr_bilagrid_slice_backward": (_INT, [_ptr_to(BilagridDims)] + [_P] * 7),
    "lsr_bilagrid_tv_workspace_bytes": (_SZ, [_ptr_to(BilagridDims)]),
    "lsr_bilagrid_tv_forward": (_INT, [_ptr_to(BilagridDims)] + [_P] * 4),
    "lsr_bilagrid_tv_backward": (_INT, [_ptr_to(BilagridDims)] + [_P] * 4),
    "lsr_transform_records": (_INT, [_I32, _P, _I32, _I32, _P, _P]),
    "lsr_scene_transform": (_INT, [_ptr_to(TransformDims), _P, _P, _ptr_to(TransformIn), _ptr_to(TransformOut), _P]),
    "lsr_vq_workspace_bytes": (_SZ, [_I64, _I32, _I32]),
    "lsr_vq_assign": (_INT, [_ptr_to(VqDims)] + [_P] * 6),
    "lsr_vq_update": (_INT, [_ptr_to(VqDims)] + [_P] * 8),
    "lsr_pose_matrices": (_INT, [_I32, _P, _P, _P, _P, _P]),
    "lsr_pose_grad_workspace_bytes": (_SZ, [_I64, _I32, _I32]),
    "lsr_scene_pose_grad": (_INT, [_ptr_to(TransformDims), _P, _P, _P, _ptr_to(PoseGradIn), _P, _SZ, _P, _P, _P, _P]),
    "lsr_scene_normals_workspace_bytes": (_SZ, [_I64, _I32]),
    "lsr_scene_normals_forward": (_INT, [_I64, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "lsr_scene_normals_backward": (_INT, [_I64, _P, _P, _P, _I32, _P, _P, _P, _P, _P]),
    "lsr_normal_consistency_workspace_bytes": (_SZ, [_ptr_to(NormalDims)]),
    "lsr_normal_consistency_forward": (_INT, [_ptr_to(NormalDims)] + [_P] * 10),
    "lsr_normal_consistency_backward": (_INT, [_ptr_to(NormalDims)] + [_P] * 9),
    "lsr_tsdf_workspace_bytes": (_SZ, [_I32]),
    "lsr_tsdf_integrate": (_INT, [_ptr_to(TsdfDims), _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _F, _F, _F, _P, _P]),
    "lsr_mesh_workspace_bytes": (_SZ, [_ptr_to(TsdfDims)]),
    "lsr_mesh_count": (_INT, [_ptr_to(TsdfDims), _P, _P, _F, _P, _P, _P]),
    "lsr_mesh_emit": (_INT, [_ptr_to(TsdfDims), _P, _P, _P, _F, _P, _P, _I64, _I64, _P, _P, _P, _P]),
    "lsr_mesh_components_init": (_INT, [_I64, _P, _P]),
    "lsr_mesh_components_round": (_INT, [_I64, _I64, _P, _P, _P, _P]),
    "lsr_nn_index_bytes": (_SZ, [_I64]),
    "lsr_nn_build_workspace_bytes": (_SZ, [_I64]),
    "lsr_nn_build": (_INT, [_I64, _P, _P, _P, _P]),
    "lsr_nn_query_workspace_bytes": (_SZ, [_I64]),
    "lsr_nn_query": (_INT, [_I64, _P, _I64, _P, _P, _P, _P, _P]),
    "lsr_colmap_count": (_INT, [_STR, _ptr_to(ColmapCounts)]),
    "lsr_colmap_read_cameras": (_INT, [_STR, _P, _P, _P, _P, _I64]),
    "lsr_colmap_read_images": (_INT, [_STR, _P, _P, _P, _P, _P, _P, _I64, _I64]),
    "lsr_colmap_read_points": (_INT, [_STR, _P, _P, _P, _P, _I64]),
    "lsr_colmap_count_observations": (_INT, [_STR, _ptr_to(_I64)]),
    "lsr_colmap_read_observations": (_INT, [_STR, _P, _P, _P, _I64, _I64]),
    "lsr_colmap_last_error": (_STR, None),
    "lsr_image_subsamples": (_INT, [_ptr_to(ImageDims), _ptr_to(ImageCamera)]),
    "lsr_image_prepare": (_INT, [_ptr_to(ImageDims), _ptr_to(ImageCamera), _P, _P, _P, _P, _P]),
    "lsr_depth_loss_workspace_bytes": (_SZ, [_ptr_to(DepthLossDims)]),
    "lsr_depth_loss_forward": (_INT, [_ptr_to(DepthLossDims)] + [_P] * 12),
    "lsr_depth_loss_backward": (_INT, [_ptr_to(DepthLossDims)] + [_P] * 11),
    "lsr_scene_depth_moments_workspace_bytes": (_SZ, [_I64, _I32]),
    "lsr_scene_depth_moments_forward": (_INT, [_I64, _P, _I32, _P, _P, _I32, _P, _P, _P]),
    "lsr_scene_depth_moments_backward": (_INT, [_I64, _P, _I32, _P, _P, _I32, _P, _P, _P, _P]),
    "lsr_distortion_loss_workspace_bytes": (_SZ, [_ptr_to(DistortionDims)]),
    "lsr_distortion_loss_forward": (_INT, [_ptr_to(DistortionDims)] + [_P] * 8),
    "lsr_distortion_loss_backward": (_INT, [_ptr_to(DistortionDims)] + [_P] * 7),
}
EXPORTS = tuple(PROTOTYPES)

_lib = None
ABI_VERSION = 10    # include/lsr_rasterizer.h LSR_ABI_VERSION


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-j8"] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return _SO


def so_path() -> str:
    return _SO


def load():
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64; it has to be the HIP runtime of the process, so make sure it
    # is loaded before our library pulls in the system copy (two runtimes = "no device" at launch)
    import torch  # noqa: F401
    if not os.path.exists(_SO):
        raise LsrError(
            f"{_SO} not found: the MI355X rasterizer extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU "
            "fallback for the product path.")
    try:
        lib = C.CDLL(_SO)
    except OSError as e:  # e.g. libamdhip64 missing on a machine without ROCm
        raise LsrError(f"cannot load {_SO}: {e}") from e
    lib.lsr_abi_version.restype = PROTOTYPES["lsr_abi_version"][0]
    # checked before any other prototype is bound: the structs above are this version's (an older or newer build would
    # be handed structs of the wrong size; there is no compatibility mode)
    abi = lib.lsr_abi_version()
    if abi != ABI_VERSION:
        raise LsrError(f"{_SO}: ABI version {abi}, this package needs {ABI_VERSION}; rebuild it "
                       "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib


def set_knob(name: str, value: int) -> None:
    """Override one LSR_* development knob of the library for the rest of the process (A/B experiments only)."""
    call("lsr_debug_set_knob", name.encode(), int(value))


def profile_enable(on, only: tuple = ()) -> None:
    """on: all stages; only=("render_forward", ...): just those stages (two event packets each)."""
    lib = load()
    if only:
        names = [lib.lsr_profile_stage_name(i).decode() for i in range(lib.lsr_profile_num_stages())]
        mask = 0
        for n in only:
            mask |= 1 << (names.index(n) + 1)
        lib.lsr_profile_enable(mask)
    else:
        lib.lsr_profile_enable(1 if on else 0)


def profile_read() -> dict:
    """{stage: (total_ms, launches)} since the previous read (blocks until the events finish)."""
    lib = load()
    n = lib.lsr_profile_num_stages()
    ms, cnt = (C.c_double * n)(), (C.c_int64 * n)()
    call("lsr_profile_read", ms, cnt)
    return {lib.lsr_profile_stage_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}


def call(name: str, *args) -> None:
    """``lib.<name>(*args)``, and :class:`LsrError` with that name unless it returns LSR_OK."""
    check(getattr(load(), name)(*args), name)


def check(rc: int, what: str):
    if rc != 0:
        lib = load()
        msg = lib.lsr_error_string(rc).decode()
        raise LsrError(f"{what} failed: {msg} (code {rc}, hipError {lib.lsr_last_hip_error()})")
