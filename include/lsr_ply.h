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

#ifdef __cplusplus
}
#endif
#endif /* LSR_PLY_H */
