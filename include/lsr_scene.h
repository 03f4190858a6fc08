/*
 * lsr_scene.h — C ABI of the 3DGS activation map: the raw parameters a 3DGS trainer holds (and a
 * scene file stores) to the tensors the rasterizer takes, and its backward.  Same library
 * (liblsr_hip.so) and conventions as lsr_rasterizer.h: device pointers, sizes, a stream, negative
 * LSR_E* codes, asynchronous on the caller's stream.
 *
 * The forward is what lsr_ply_unpack (lsr_ply.h) does to the rows of a scene file, taken from live
 * parameter tensors instead of a row table: colour SH concatenated into one [n][K][3] tensor,
 * sigmoid of the opacity logits, and R diag((m s)^2) R^T from the log-scales and the unnormalised
 * quaternions (m = scale_modifier).  The backward takes the upstream gradients of those three
 * tensors to the gradients of the five raw tensors, one launch each way, so that a scene can be
 * optimised in the parameterisation its file and its optimiser recipes use.
 */
#ifndef LSR_SCENE_H
#define LSR_SCENE_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsr_scene_params {      /* device, float32; what a 3DGS trainer holds */
    const float *features_dc;    /* [n][1][3] */
    const float *features_rest;  /* [n][K-1][3]; NULL iff K == 1 */
    const float *opacity;        /* [n][1] logits */
    const float *scaling;        /* [n][3] logs */
    const float *rotation;       /* [n][4] w,x,y,z, any non-zero norm; 16-byte aligned */
} lsr_scene_params;

typedef struct lsr_scene_dims {
    int64_t n;               /* Gaussians, >= 0 */
    int32_t sh_coeffs;       /* K in 1,4,9,16,25 */
    float scale_modifier;    /* m: finite, > 0 */
    int32_t reserved0, reserved1;   /* 0 */
} lsr_scene_dims;

typedef struct lsr_scene_outputs {     /* every pointer optional (NULL = not wanted) */
    float *shs;        /* [n][K][3]: [g][0][c] = dc, [g][1+k][c] = rest[g][k][c] */
    float *opacities;  /* [n][1] sigmoid */
    float *cov3D;      /* [n][6] R diag((m s)^2) R^T as xx,xy,xz,yy,yz,zz, s = exp(scaling), m = scale_modifier */
    float *scales;     /* [n][3] m * exp(scaling)   (forward only) */
    float *rotations;  /* [n][4] unit quaternion    (forward only; 16-byte aligned) */
} lsr_scene_outputs;

/* Upstream gradients of the three differentiable outputs; each optional (NULL = zero). */
typedef struct lsr_scene_out_grads {
    const float *shs;        /* [n][K][3] */
    const float *opacities;  /* [n][1] */
    const float *cov3D;      /* [n][6]; the gradient of an off-diagonal entry is that of the packed value */
} lsr_scene_out_grads;

/* Gradients of the five raw tensors; each optional (NULL = not wanted); written, never accumulated. */
typedef struct lsr_scene_in_grads {
    float *features_dc;    /* [n][1][3] */
    float *features_rest;  /* [n][K-1][3]; ignored when K == 1 */
    float *opacity;        /* [n][1] */
    float *scaling;        /* [n][3] */
    float *rotation;       /* [n][4]; 16-byte aligned */
} lsr_scene_in_grads;

/* One launch.  n == 0 launches nothing and returns LSR_OK.  Values are taken as they are: a quaternion of norm 0 (or a
 * non-finite value) gives NaN for that Gaussian, as lsr_ply_unpack documents and as the PyTorch formula does.  Every
 * output element has one owner and nothing is accumulated: two calls give the same bits.
 * LSR_EINVAL (before any GPU work): n < 0, K not one of the five, features_rest given with K == 1 or missing with K > 1,
 * a scale_modifier that is not finite and positive, a non-zero reserved field, a quad pointer (rotation, rotations) that
 * is not 16-byte aligned.  LSR_ENULL: a NULL struct, or with n > 0 a NULL features_dc, opacity, scaling or rotation. */
int lsr_scene_activate_forward(const lsr_scene_dims *dims, const lsr_scene_params *params, const lsr_scene_outputs *out,
                               lsr_stream_t stream);

/* Upstream gradients of shs / opacities / cov3D (each optional, NULL = zero) -> gradients of the five raw tensors (each
 * optional; written, never accumulated).  Reads opacity, scaling and rotation of `params` (required with n > 0; the
 * feature tensors are not read, but features_rest must agree with K as in the forward).  With G the symmetric matrix of
 * the covariance gradient (diagonal as given, each off-diagonal entry half of its packed value) and M = R diag(m s):
 * dM = 2 G M, d scaling_k = m s_k sum_i dM_ik R_ik, dR_ik = dM_ik m s_k, dR through the unit-quaternion formula to
 * dq_hat, d rotation = (dq_hat - (dq_hat . q_hat) q_hat) / |q|; d opacity = g o (1 - o); the SH gradients are the
 * forward's re-layout run backwards, bit for bit.  Same checks and codes as the forward. */
int lsr_scene_activate_backward(const lsr_scene_dims *dims, const lsr_scene_params *params,
                                const lsr_scene_out_grads *dout, const lsr_scene_in_grads *din, lsr_stream_t stream);

/* The same map with the 3D smoothing filter of Mip-Splatting inside it: filter3d [n] is what lsr_filter3d_compute
 * (lsr_filter3d.h) writes, one float per Gaussian, a constant of the map.  With s_k = exp(scaling_k), f = filter3d[g] and
 * v_k = s_k^2 + f^2 (the Gaussian convolved with an isotropic Gaussian of variance f^2):
 *   scales_k  = m sqrt(v_k)
 *   cov3D     = R diag(m^2 v_k) R^T
 *   opacities = sigmoid(opacity) c,  c = prod_k (s_k / sqrt(v_k))   — the determinant ratio, formed as three ratios each
 *               at most 1 and never as sqrt(det / det)
 *   shs and rotations as in the unfiltered map.  f == 0 gives the unfiltered values.
 * The same kernel as lsr_scene_activate_forward, instantiated with the filter: one launch, 4 bytes more per Gaussian.  A
 * non-finite or negative entry of filter3d is taken as it is (NaN in, NaN out for that Gaussian).  Same checks and codes as
 * the unfiltered forward, plus LSR_ENULL for a NULL filter3d with n > 0. */
int lsr_scene_activate_filtered_forward(const lsr_scene_dims *dims, const lsr_scene_params *params, const float *filter3d,
                                        const lsr_scene_outputs *out, lsr_stream_t stream);

/* Its backward; the filter receives no gradient.  With o = sigmoid(opacity), c as above and g_o the upstream gradient of
 * opacities:  d opacity = g_o c o (1 - o);  M = R diag(m sqrt(v_k)), dM = 2 G M as in the unfiltered backward;
 *   d scaling_k = m sqrt(v_k) (sum_i dM_ik R_ik) (s_k^2 / v_k)  +  g_o o c f^2 / v_k
 * (d v_k / d scaling_k = 2 s_k^2; d log c / d scaling_k = f^2 / v_k);  dR_ik = dM_ik m sqrt(v_k), then as before.  A NULL
 * upstream opacities gradient is zero in both places.  Same checks and codes as the filtered forward. */
int lsr_scene_activate_filtered_backward(const lsr_scene_dims *dims, const lsr_scene_params *params, const float *filter3d,
                                         const lsr_scene_out_grads *dout, const lsr_scene_in_grads *din, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_SCENE_H */
