/*
 * lsr_ply.h — C ABI of the 3DGS `.ply` export (the on-disk format next
 * to the path).  Same library and conventions as lsr_rasterizer.h.
 *
 * Replaces /root/reference/src/model/ply_export.py:26-92 (`export_ply`): per-Gaussian recentring
 * and rescaling (:35-41), the viewer rotation `Rz(-45 deg) @ [[0,0,1],[-1,0,0],[0,-1,0]] @
 * extrinsics[:3,:3]^-1` applied to positions (:43-66) and to the orientation quaternions through
 * rotation matrices (:68-73, scipy `Rotation.from_quat / from_matrix / as_quat`, output order
 * w,x,y,z), DC band of the harmonics (:77), log-scales (:87), and the 17-float vertex record of
 * `construct_list_of_attributes(0)` (:13-23): x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3.
 * The reference does this with torch + scipy + a Python tuple list per Gaussian and writes through
 * `plyfile`; here one kernel packs the vertex records on the device and a host function writes the
 * binary little-endian file.  The two global statistics (median, 0.95-quantile) are the caller's
 * (two torch reductions) and are passed in as device scalars.
 */
#ifndef LSR_PLY_H
#define LSR_PLY_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_PLY_VERTEX_FLOATS 17

typedef struct lsr_ply_inputs {
    const float *extrinsics;  /* [4][4] camera-to-world of the reference view */
    const float *means;       /* [n][3] */
    const float *scales;      /* [n][3] */
    const float *rotations;   /* [n][4] xyzw */
    const float *harmonics;   /* [n][3][d_sh]; only coefficient 0 of each channel is exported */
    const float *opacities;   /* [n] */
    const float *center;      /* [3]  device: means.median(dim=0) */
    const float *scale_factor;/* [1]  device: means(centred).abs().quantile(0.95, dim=0).max() */
} lsr_ply_inputs;

/* Fill vertices[n][LSR_PLY_VERTEX_FLOATS] on the device.  Asynchronous. */
int lsr_ply_pack(int64_t n, int32_t d_sh, const lsr_ply_inputs *in, float *vertices, lsr_stream_t stream);

/* Write a binary little-endian PLY with one `vertex` element of n records from HOST memory
 * (header as plyfile emits it for float32 properties).  Returns LSR_EINVAL if the file cannot be
 * created or written. */
int lsr_ply_write_host(const char *path, const float *vertices_host, int64_t n);

/*
 * ---- import: standard 3DGS scene files (the published `point_cloud.ply` layout) ----
 *
 * A scene file is one binary little-endian `vertex` element of float properties: x y z, optional
 * nx ny nz, f_dc_0..2, f_rest_0..3(K-1)-1 (K = (degree+1)^2 SH coefficients per channel, stored
 * channel-major), opacity (a logit), scale_0..2 (logs), rot_0..3 (w,x,y,z, not normalised).  The
 * files lsr_ply_write_host writes are the K = 1 case (with the opacity stored raw).
 *
 * The host reader turns the header into a layout (where each named property sits inside a row)
 * and copies the rows, untouched, into the caller's host buffer; lsr_ply_unpack turns the row
 * table into the rasterizer's tensors on the device.
 */
#define LSR_PLY_MAX_SH_COEFFS ((LSR_MAX_SH_DEGREE + 1) * (LSR_MAX_SH_DEGREE + 1))  /* 25 */
#define LSR_PLY_MAX_REST (3 * (LSR_PLY_MAX_SH_COEFFS - 1))                          /* 72 */
#define LSR_PLY_MAX_STRIDE 8192   /* floats per row the reader and the unpack accept */

typedef struct lsr_ply_layout {
    int64_t n;            /* vertex count */
    int64_t data_offset;  /* bytes of header in front of the first row (reader only; unpack ignores it) */
    int32_t stride;       /* floats per row, unknown properties included */
    int32_t sh_coeffs;    /* K in {1,4,9,16,25} */
    /* float offsets inside a row, each in [0, stride) */
    int32_t xyz[3];
    int32_t f_dc[3];
    int32_t opacity;
    int32_t scale[3];
    int32_t rot[4];
    int32_t f_rest[LSR_PLY_MAX_REST];   /* the first 3(K-1) are used */
} lsr_ply_layout;

/* Parse the header of `path` and check the file's size against it.  Properties may come in any
 * order; float properties with other names are skipped but counted into the stride; `comment` and
 * `obj_info` lines are ignored.  Nothing but the header is read and nothing is allocated.
 * LSR_EUNSUPPORTED: a format other than `binary_little_endian 1.0`, an element other than one
 *   `vertex`, a property that is not `float` / `float32` (lists included), an f_rest count that is
 *   not 3(K-1) for K in {1,4,9,16,25}, more than LSR_PLY_MAX_STRIDE properties.
 * LSR_EINVAL: the file cannot be opened, is not a PLY, has a malformed or over-long (> 255 bytes)
 *   header line or no `end_header`, a negative or overflowing vertex count, a required property
 *   missing or given twice, or fewer than data_offset + n * stride * 4 bytes.
 * `*layout` is written only on LSR_OK. */
int lsr_ply_read_header(const char *path, lsr_ply_layout *layout);

/* Copy the n * stride floats of the file's rows into rows_host (HOST memory, e.g. pinned).  The
 * header is parsed and checked again as in lsr_ply_read_header; capacity_floats < n * stride is
 * LSR_EINVAL.  rows_host is written only when every check has passed. */
int lsr_ply_read_rows(const char *path, float *rows_host, int64_t capacity_floats);

#define LSR_PLY_OPACITY_RAW 1   /* lsr_ply_unpack flags: opacities = the stored value, not sigmoid of it */

typedef struct lsr_ply_outputs {  /* device; every pointer is optional (NULL = not wanted) */
    float *means;      /* [n][3] */
    float *shs;        /* [n][K][3]: [g][0][c] = f_dc_c, [g][1+k][c] = f_rest_{c(K-1)+k} */
    float *opacities;  /* [n][1] sigmoid(opacity), or the stored value with LSR_PLY_OPACITY_RAW */
    float *scales;     /* [n][3] exp(scale_k) */
    float *rotations;  /* [n][4] w,x,y,z normalised */
    float *cov3D;      /* [n][6] R S^2 R^T as xx,xy,xz,yy,yz,zz */
} lsr_ply_outputs;

/* rows [n][stride] on the device -> the outputs above.  Asynchronous; n == 0 launches nothing.
 * `rows` needs no more than float alignment (a table may start anywhere inside a larger buffer);
 * `rotations` is stored as one 16-byte quad per Gaussian and must be 16-byte aligned.
 * The values are taken as they are: a stored quaternion of norm 0 (or a non-finite value) gives
 * NaN rotations and cov3D for that Gaussian, as the PyTorch formula does; screen untrusted files
 * for finite outputs where that matters.
 * LSR_EINVAL for a layout whose offsets do not lie inside the row, whose stride exceeds
 * LSR_PLY_MAX_STRIDE or whose K is not one of the five, for unknown flags or a misaligned pointer. */
int lsr_ply_unpack(const lsr_ply_layout *layout, const float *rows, int32_t flags, const lsr_ply_outputs *out,
                   lsr_stream_t stream);

/*
 * ---- scene export: the rasterizer's tensors back to a standard 3DGS scene file ----
 *
 * The inverse of the import: lsr_ply_pack_scene builds the row table of the published layout on the device — every SH
 * band, the opacity as a logit, log-scales and a quaternion taken from the covariance — and lsr_ply_write_scene_host
 * writes it.  Unlike lsr_ply_pack (a viewer's copy: recentred, rescaled, rotated, DC band only) nothing about the
 * scene is changed: lsr_ply_read_* / lsr_ply_unpack give it back.
 */
#define LSR_PLY_SCENE_ROW_FLOATS(K) (14 + 3 * (K))   /* x y z nx ny nz f_dc_0..2 f_rest_0..3(K-1)-1 opacity scale_0..2 rot_0..3 */

typedef struct lsr_ply_scene_inputs {   /* device */
    const float *means;       /* [n][3] */
    const float *opacities;   /* [n] probabilities */
    const float *shs;         /* colour SH: [n][sh_coeffs][3], or [n][3][sh_coeffs] with sh_channel_major */
    const float *cov;         /* [n][cov_elems]: 6 = xx,xy,xz,yy,yz,zz; 9 = row-major 3x3 whose upper triangle is read (that
                                 IS the symmetrised input).  NULL: scales and rotations are given instead */
    const float *scales;      /* [n][3]; used (with rotations) only when cov is NULL */
    const float *rotations;   /* [n][4] w,x,y,z, any non-zero norm */
    int32_t sh_coeffs;        /* K_in in {1,4,9,16,25} */
    int32_t sh_channel_major; /* 0 or 1 */
    int32_t cov_elems;        /* 6 or 9 (ignored when cov is NULL) */
    int32_t reserved0;        /* 0 */
} lsr_ply_scene_inputs;

typedef struct lsr_ply_scene_opts {
    int32_t sh_convention;    /* basis the caller's shs are in: LSR_SH_AXES_3DGS or LSR_SH_AXES_REFERENCE */
    int32_t sh_coeffs_out;    /* K_out in {1,4,9,16,25}, <= K_in: the lower bands are kept */
    int32_t reserved0, reserved1;   /* 0 */
} lsr_ply_scene_opts;

/* rows[n][14 + 3 K_out] on the device, in the published property order (above).  Device to device, asynchronous;
 * n == 0 launches nothing.  Every row has one owner and nothing is accumulated: two calls give the same bits.
 *   x y z      means, bit for bit.  nx ny nz: 0.0f.
 *   opacity    log(p / (1 - p)) clamped to [-20, 20]: always finite for p in [0, 1] (p = 1 loads back as 1.0f, p = 0
 *              as 2e-9); NaN in gives NaN out, and so does p outside [0, 1].
 *   f_dc, f_rest   LSR_SH_AXES_3DGS: a pure re-layout, bit for bit: f_dc_c = shs[g][0][c],
 *              f_rest_{c (K_out - 1) + k} = shs[g][1 + k][c].  LSR_SH_AXES_REFERENCE: per band c' = M_l c first (the
 *              matrix of lsr_ply_sh_axes_matrix, rounded to float), so that the file renders under the 3dgs basis what
 *              the input renders under the reference's.
 *   scale, rot from cov: eigenvalues lambda_k and orthonormal eigenvectors (float32 cyclic Jacobi, fixed sweeps);
 *              lambda_k <- max(lambda_k, 1e-12 lambda_max, 1e-37), scale_k = 0.5 log lambda_k in DESCENDING order; the
 *              eigenvector matrix has its last column flipped where needed so that det = +1, and rot is its unit
 *              quaternion w,x,y,z with w >= 0.  R S^2 R^T rebuilt from the row is within 1e-5 of the largest |cov| entry.
 *              From scales / rotations: log(scale_k) in the caller's order and the caller's quaternion normalised,
 *              negated where w < 0.
 * `rows` and the inputs need float alignment only.
 * LSR_EINVAL: n < 0, K_in or K_out not one of the five, K_out > K_in, an unknown convention, sh_channel_major not 0 / 1,
 * cov_elems not 6 / 9 with cov given, a non-zero reserved field.  LSR_ENULL: a NULL struct, means, opacities, shs or
 * rows, or neither cov nor both of scales and rotations (n > 0). */
int lsr_ply_pack_scene(int64_t n, const lsr_ply_scene_inputs *in, const lsr_ply_scene_opts *opts, float *rows,
                       lsr_stream_t stream);

/* The change of basis as one 25 x 25 row-major matrix M, out[25 * i + j]: c' = M c.  Block diagonal (band l in rows and
 * columns l^2 .. (l+1)^2 - 1, exact zeros elsewhere) and orthogonal; with Y the basis of the kernels,
 * Y(d) . M = Y(d_z, d_x, d_y) for every unit d.  Host only. */
int lsr_ply_sh_axes_matrix(double *out);

/* Write rows_host[n][14 + 3 sh_coeffs] (HOST memory) as a binary little-endian scene file: the header plyfile emits for
 * those float properties, then the rows.  sh_coeffs not in {1,4,9,16,25} or n < 0: LSR_EINVAL; LSR_EINVAL as well if the
 * file cannot be created or fully written. */
int lsr_ply_write_scene_host(const char *path, const float *rows_host, int64_t n, int32_t sh_coeffs);

/*
 * ---- point clouds: the sparse SfM cloud a 3DGS fit starts from ----
 *
 * The file the published trainer's storePly writes (x y z nx ny nz red green blue) and COLMAP conversions produce: one
 * binary little-endian `vertex` element of scalar properties, of any PLY scalar type under either spelling (char / int8,
 * uchar / uint8, short / int16, ushort / uint16, int / int32, uint / uint32, float / float32, double / float64) and in
 * any order.  x y z are required, as float or double (doubles are rounded to float); red green blue are optional, must
 * be uchar and come out divided by 255; everything else (nx ny nz, alpha, ...) is skipped by its size.
 * LSR_EUNSUPPORTED: a format other than `binary_little_endian 1.0`, a list property, an element other than one `vertex`,
 *   x y z or colours of another type, only some of the three colours, more than 1024 properties.
 * LSR_EINVAL: the file cannot be opened, is not a PLY, has a malformed or over-long (> 255 bytes) header line, an unknown
 *   scalar type or no `end_header`, a negative or overflowing vertex count, x, y or z missing, one of the six names given
 *   twice, or fewer bytes than the header promises.
 * Host only; the outputs are written only when every check has passed.
 */
int lsr_ply_read_points_header(const char *path, int64_t *n, int32_t *has_colors);

/* xyz_host[n][3] and, where the file has colours and rgb_host is not NULL, rgb_host[n][3] in [0, 1] (HOST memory).  The
 * header is parsed and checked again; capacity_points < n is LSR_EINVAL, xyz_host NULL with n > 0 LSR_ENULL. */
int lsr_ply_read_points(const char *path, float *xyz_host, float *rgb_host, int64_t capacity_points);

#ifdef __cplusplus
}
#endif
#endif /* LSR_PLY_H */
