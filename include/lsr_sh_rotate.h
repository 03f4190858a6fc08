/*
 * lsr_sh_rotate.h — C ABI of the SH coefficient rotation: the colour and latent-feature harmonics
 * of the Gaussian adapter, from camera space to world space.  Same library (liblsr_hip.so), same
 * conventions as lsr_adapter.h: device pointers, sizes, a hipStream_t, negative LSR_E* codes;
 * every call is asynchronous on `stream` and allocates nothing.
 *
 * What it replaces in the reference (paths relative to /root/reference):
 *   - src/model/encoder/common/gaussian_adapter.py:90-93    the broadcast of the raw coefficients
 *         over the depth samples and the multiply by the degree masks;
 *   - gaussian_adapter.py:107-108 + src/misc/sh_utils.py:100-120   rotate_sh: e3nn's
 *         matrix_to_angles / wigner_D, one batched matmul per band and a cat, per tensor,
 *         forward and again in autograd's backward.
 * e3nn is not needed: the matrices are computed from the 3x3 rotation itself.
 *
 * Contract.  Per band l (coefficients l^2 .. (l+1)^2 - 1):  out_l = D_l(R) . (mask_l * in_l),
 * where D_l(R) is the matrix e3nn's wigner_D(l, *matrix_to_angles(R)) denotes, DEFINED by
 *       Y_l(R x) = D_l(R) . Y_l(x)    for every unit vector x,
 * with Y e3nn's real SH basis: up to a positive factor per band, the polynomials of the reference's
 * eval_sh (sh_utils.py:59-96) in the same order, every constant positive and index 14 = y (zz - xx).
 * D_l is an exact polynomial of degree l in the entries of R (no Euler angles, nothing special near
 * gimbal lock); D_1 = R.  Specified for proper rotations.
 *
 * Table layout.  The band blocks of one rotation, row-major, one after another:
 * sum_{l <= L} (2l+1)^2 floats = 1, 10, 35, 84, 165 for L = 0..4.  The table of degree L is a
 * prefix of the table of any higher degree, so one table of the larger degree serves both tensors.
 */
#ifndef LSR_SH_ROTATE_H
#define LSR_SH_ROTATE_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_SH_ROTATE_MAX_DEGREE 4
#define LSR_SH_ROTATE_TABLE_FLOATS(L) (((L) + 1) * (2 * (L) + 1) * (2 * (L) + 3) / 3)

typedef struct lsr_sh_rotate_dims {
    int32_t num_cameras;    /* >= 1: one rotation (table) per camera */
    int32_t rays;           /* rows per camera, >= 0 (0: nothing is launched, LSR_OK) */
    int32_t samples;        /* S >= 1: every row is written S times (the spp broadcast) */
    int32_t color_coeffs;   /* Kc in {0 (no colour tensor), 1, 4, 9, 16, 25}; 3 channels */
    int32_t feat_channels;  /* C in 1..LSR_MAX_FEAT_CHANNELS when feat_coeffs > 0 (ignored otherwise) */
    int32_t feat_coeffs;    /* Kf in {0 (no feature tensor), 1, 4, 9, 16, 25} */
    int32_t table_stride;   /* floats between consecutive cameras' tables, >= the table of the larger degree */
    int32_t reserved0;      /* 0 */
    int64_t row_stride;     /* forward: floats between consecutive rows of `rows`, >= 3 Kc + C Kf
                             * (the encoder hands a strided view of its Linear output) */
} lsr_sh_rotate_dims;

/* tables[r][...] (LSR_SH_ROTATE_TABLE_FLOATS(degree) floats each, dense) for `num_rot` rotations.
 * Matrix r, entry (i, j) is rotations[r * mat_stride + i * row_stride + j]: (3, 9) for packed 3x3
 * matrices, (4, 16) reads the rotation corner of a [cam][4][4] camera-to-world table in place.
 * One small launch; evaluated in double.  num_rot == 0: LSR_OK, nothing launched. */
int lsr_sh_rotation_matrices(int32_t num_rot, const float *rotations, int64_t row_stride, int64_t mat_stride,
                             int32_t degree, float *tables, lsr_stream_t stream);

/* rows [cam][rays] (row_stride floats apart), content [3 Kc colour | C Kf feature] ->
 *   color_out   [cam][rays][S][3][Kc]     (Gaussians.color_harmonics)
 *   feature_out [cam][rays][S][C][Kf]     (Gaussians.feature_harmonics), both contiguous.
 * color_mask (Kc floats) / feature_mask (Kf floats) multiply the coefficients before the rotation
 * (gaussian_adapter.py:92-93); NULL = ones.  One launch. */
int lsr_sh_rotate_forward(const lsr_sh_rotate_dims *d, const float *tables, const float *rows,
                          const float *color_mask, const float *feature_mask,
                          float *color_out, float *feature_out, lsr_stream_t stream);

/* d_rows [cam][rays][3 Kc + C Kf] dense, WRITTEN (not accumulated):
 *   d_row_l = mask_l * sum_s D_l^T g_s.
 * Either upstream gradient may be NULL (= zero; its columns are written as zeros).  No atomics: a
 * row has one owner, the result is bitwise reproducible.  The rotation is data (no gradient), as
 * the cameras are in lsr_adapter_backward.  d->row_stride is not used.  One launch. */
int lsr_sh_rotate_backward(const lsr_sh_rotate_dims *d, const float *tables, const float *g_color,
                           const float *g_feature, const float *color_mask, const float *feature_mask,
                           float *d_rows, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_SH_ROTATE_H */
