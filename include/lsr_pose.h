/*
 * lsr_pose.h — C ABI of the pose gradient of a 3DGS scene's rigid parts: the similarity transform of
 * lsr_transform.h, differentiated in the transforms themselves.  Same library (liblsr_hip.so) and
 * conventions as lsr_transform.h: device pointers, sizes, a stream, negative LSR_E* codes,
 * asynchronous on the caller's stream, nothing allocated.
 *
 * A pose is a raw quaternion p (w,x,y,z, any non-zero norm), a translation t and a log-scale l:
 * R = R(p / |p|), s = exp(l), M = [[sR, t], [0, 1]].  The forward is the map of lsr_transform.h on
 * those matrices (lsr_pose_matrices, then lsr_transform_records and lsr_scene_transform), unchanged.
 *
 * The gradient.  For the world-frame perturbation R -> exp([w]x) R each output's derivative needs only
 * that output, the upstream gradient g and constants:
 *   positions, y = sRx:      dL/dw += y x g_x,   dL/dt += g_x,   dL/dl += g_x . y
 *                            (y from the INPUT position and the record's linear part: x' - t would
 *                            cancel at large |t|)
 *   log-scales:              dL/dl += g_s0 + g_s1 + g_s2
 *   quaternions q' = (w, v), g_q = (g_w, g_v):   dL/dw += (w g_v - g_w v + v x g_v) / 2
 *   colour band l:           dL/dw_a += sum over channels of g_l^T J_a^l c'_l, with J_a^l the constant
 *                            generators of T_l (csrc/lsr_sh_generator_table.h)
 * Each Gaussian contributes 7 numbers (w, t, l) to its transform; they are summed per transform
 * without atomics, in a fixed order, in double.  Then, with G_w, G_t, G_l per transform:
 *   dL/dp = (2 / |p|) (0, G_w) (x) p / |p|   (Hamilton product; orthogonal to p),
 *   dL/dt = G_t,   dL/dl = G_l.
 */
#ifndef LSR_POSE_H
#define LSR_POSE_H

#include "lsr_transform.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the per-wave reduction tables ([T][7] doubles in LDS) bound the number of transforms of one call */
#define LSR_POSE_MAX_TRANSFORMS 256

/* quaternions [T][4] (w,x,y,z, any non-zero norm), translations [T][3], log_scales [T] or NULL (s = 1)
 * -> matrices [T][4][4] row-major float32 (last row 0 0 0 1).  One small launch, evaluated in double.
 * A zero or non-finite quaternion gives a non-finite matrix without an error.
 * T == 0: LSR_OK, nothing launched.  LSR_EINVAL: T < 0.  LSR_ENULL: T > 0 and NULL quaternions,
 * translations or matrices. */
int lsr_pose_matrices(int32_t T, const float *quaternions, const float *translations, const float *log_scales,
                      float *matrices, lsr_stream_t stream);

/* Bytes of the workspace of lsr_scene_pose_grad for n Gaussians of sh_coeffs coefficients per channel
 * and T transforms: the per-workgroup partial sums.  A pure function of its arguments, non-decreasing
 * in each; 0 for arguments lsr_scene_pose_grad refuses (n < 0, K not one of 1,4,9,16,25, T outside
 * 0..LSR_POSE_MAX_TRANSFORMS). */
size_t lsr_pose_grad_workspace_bytes(int64_t n, int32_t sh_coeffs, int32_t T);

typedef struct lsr_pose_grad_in {      /* device, float32 */
    const float *xyz;              /* [n][3]: the INPUT positions of the forward; read only with g_xyz */
    const float *rotation;         /* [n][4]: the OUTPUT quaternions q' of the forward; 16-byte aligned; read only with
                                      g_rotation */
    const float *features_rest;    /* [n][K-1][3]: the OUTPUT coefficients c' of the forward; read only with
                                      g_features_rest; NULL when K == 1 */
    /* upstream gradients of the four outputs; each optional: NULL means zeros, and its companion above is not read */
    const float *g_xyz;            /* [n][3] */
    const float *g_features_rest;  /* [n][K-1][3]; NULL when K == 1 */
    const float *g_scaling;        /* [n][3] */
    const float *g_rotation;       /* [n][4]; 16-byte aligned */
} lsr_pose_grad_in;

/* dims: as for lsr_scene_transform, but num_transforms may be 0.  records: the FORWARD records of
 * lsr_transform_records for these transforms at degree sqrt(K) - 1 (the linear part is read).  idx: int32
 * [n] or NULL (every Gaussian belongs to transform 0); a Gaussian whose idx lies outside [0, T)
 * contributes nothing.  quaternions: the raw [T][4] the matrices were made from (read only when
 * grad_quaternion is wanted).  Outputs, each optional (NULL = not wanted): grad_quaternion [T][4],
 * grad_translation [T][3], grad_log_scale [T]; every element is written, a transform that owns no
 * Gaussian gets exact zeros.  Two launches (plus none for n == 0), no atomics: the same bits every call;
 * the result does not depend on what the workspace held.
 * T == 0, or no output wanted: LSR_OK, nothing launched.  n == 0: LSR_OK, the outputs are zeroed.
 * LSR_EINVAL (before any GPU work): n < 0, K not one of the five, T < 0, a non-zero reserved field,
 * features_rest or g_features_rest given with K == 1, a rotation or g_rotation pointer that is not
 * 16-byte aligned, workspace_bytes below lsr_pose_grad_workspace_bytes(n, K, T).
 * LSR_EUNSUPPORTED: T > LSR_POSE_MAX_TRANSFORMS.
 * LSR_ENULL: a NULL dims or in; grad_quaternion wanted with NULL quaternions; with n > 0: NULL records
 * or workspace, or an upstream gradient given whose companion (xyz, rotation, features_rest) is NULL. */
int lsr_scene_pose_grad(const lsr_transform_dims *dims, const float *records, const int32_t *idx,
                        const float *quaternions, const lsr_pose_grad_in *in, void *workspace, size_t workspace_bytes,
                        float *grad_quaternion, float *grad_translation, float *grad_log_scale, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_POSE_H */
