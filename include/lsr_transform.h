/*
 * lsr_transform.h — C ABI of the similarity transform of a 3DGS scene: the raw parameters a trainer
 * holds (lsr_scene.h), moved by x' = s R x + t.  Same library (liblsr_hip.so) and conventions as
 * lsr_scene.h: device pointers, sizes, a stream, negative LSR_E* codes, asynchronous on the caller's
 * stream, nothing allocated.
 *
 * The map, for M = [[sR, t], [0, 1]] with R a proper rotation and s > 0:
 *   xyz            s R x + t
 *   rotation       q_R (x) q   (Hamilton product, w,x,y,z; q_R the unit quaternion of R; the norm of
 *                  the raw quaternion is kept up to rounding)
 *   scaling        scaling + log s
 *   features_rest  band l (rows l^2 - 1 .. (l+1)^2 - 2), each of the 3 channels:  T_l(R) . c_l
 *   features_dc and opacity do not change and are not part of the call.
 * T_l(R) is DEFINED by  B_l(R d) = T_l(R) . B_l(d)  for every unit d, with B the "3dgs" colour basis
 * (sh_basis of csrc/lsr_sh.h): the colour the moved scene shows along R d is the colour the scene
 * showed along d.  With D_l the matrices of lsr_sh_rotate.h and A_l the constant orthogonal matrix
 * with B_l = A_l Y_l (csrc/lsr_sh_basis_table.h):  T_l(R) = A_l D_l(R) A_l^T.
 *
 * The adjoint of the linear part is the same map with other constants (xyz: (sR)^T g; rotation:
 * conj(q_R) (x) g; scaling: g; band l: T_l(R)^T g), so one kernel serves forward and backward: the
 * mode lives in the per-transform records.
 *
 * Record layout (float32, LSR_TRANSFORM_RECORD_FLOATS(degree) each, dense):
 *   [0..8]   the linear part row-major: sR, or (sR)^T for the adjoint
 *   [9..11]  t                          (0 for the adjoint)
 *   [12]     log s                      (0 for the adjoint)
 *   [13..16] q_R as w,x,y,z             (its conjugate for the adjoint)
 *   [17..19] 0 (padding: the band blocks start on a 16-byte boundary of the record)
 *   [20.. ]  T_1 .. T_degree row-major, one after another (9, 25, 49, 81 floats); transposed for
 *            the adjoint
 */
#ifndef LSR_TRANSFORM_H
#define LSR_TRANSFORM_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_TRANSFORM_MAX_DEGREE 4
#define LSR_TRANSFORM_HEADER_FLOATS 20
/* 20, 29, 54, 103, 184 for degree 0..4 */
#define LSR_TRANSFORM_RECORD_FLOATS(L) (LSR_TRANSFORM_HEADER_FLOATS + ((L) + 1) * (2 * (L) + 1) * (2 * (L) + 3) / 3 - 1)

/* matrices [T][4][4] row-major float32 (device) -> records [T][LSR_TRANSFORM_RECORD_FLOATS(degree)].
 * One small launch, evaluated in double: with A the upper-left 3x3 block, s = cbrt(det A) and R the
 * rotation nearest to A / s (A / s is one only to the rounding of its float32 entries; q_R and T_l
 * are those of its orthogonal polar factor); the linear part of the record is A itself, bit for
 * bit.  The matrices are taken as they are: nothing checks that they are similarities, the last row
 * is not read, and a singular or non-finite matrix gives non-finite records without an error (the
 * Python wrapper's check refuses those).  adjoint: 0 or 1.
 * T == 0: LSR_OK, nothing launched.  LSR_EINVAL: T < 0, degree outside 0..4, adjoint not 0 or 1.
 * LSR_ENULL: T > 0 and a NULL pointer. */
int lsr_transform_records(int32_t T, const float *matrices, int32_t degree, int32_t adjoint, float *records,
                          lsr_stream_t stream);

typedef struct lsr_transform_dims {
    int64_t n;               /* Gaussians, >= 0 */
    int32_t sh_coeffs;       /* K in 1,4,9,16,25; the records are those of degree sqrt(K) - 1 */
    int32_t num_transforms;  /* T >= 1 */
    int32_t reserved0, reserved1;   /* 0 */
} lsr_transform_dims;

typedef struct lsr_transform_in {      /* device, float32; an input is read only where its output is wanted */
    const float *xyz;            /* [n][3] */
    const float *features_rest;  /* [n][K-1][3]; NULL when K == 1 */
    const float *scaling;        /* [n][3] logs */
    const float *rotation;       /* [n][4] w,x,y,z, any norm; 16-byte aligned */
} lsr_transform_in;

typedef struct lsr_transform_out {     /* every pointer optional (NULL = not wanted); each may alias its input */
    float *xyz;
    float *features_rest;
    float *scaling;
    float *rotation;             /* 16-byte aligned */
} lsr_transform_out;

/* One launch, no atomics: the same bits every call.  idx: int32 [n], the record of each Gaussian, or
 * NULL (every Gaussian takes record 0).  A Gaussian whose idx lies outside [0, T) passes through bit
 * for bit (whatever its values: NaN and infinities too): copied out of place, written with the bits it
 * had in place.  Every out pointer may be its input: a Gaussian's row has one owner, which reads it
 * whole before it writes any of it.  Partially overlapping buffers are not supported.
 * With idx, the records are staged in LDS when T of them fit beside the staged rows (64 KB in all)
 * and gathered from global memory otherwise; the results are the same bits.
 * n == 0: LSR_OK.  LSR_EINVAL (before any GPU work): n < 0, K not one of the five, T < 1, a non-zero
 * reserved field, features_rest (in or out) given with K == 1, out->features_rest wanted with K > 1
 * and in->features_rest missing, a rotation pointer that is not 16-byte aligned.  LSR_ENULL: a NULL
 * struct; with n > 0, NULL records, or a wanted output whose input is NULL. */
int lsr_scene_transform(const lsr_transform_dims *dims, const float *records, const int32_t *idx,
                        const lsr_transform_in *in, const lsr_transform_out *out, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_TRANSFORM_H */
