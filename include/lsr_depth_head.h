/*
 * lsr_depth_head.h — C ABI of the fused depth head: the encoder's depth logits to sampled depths and
 * opacities, the two inputs of the Gaussian adapter (lsr_adapter.h) that the adapter itself does not
 * compute.  Same library (liblsr_hip.so), same conventions as lsr_adapter.h: device pointers, sizes, a
 * hipStream_t, negative LSR_E* codes; every call is asynchronous on `stream`, allocates nothing and
 * validates its arguments on the host before anything is launched.
 *
 * What it replaces in the reference (paths relative to the reference's root), about fifteen elementwise
 * PyTorch kernels forward plus autograd's backward over a (b, v, rays, 2 S F) tensor:
 *   - src/model/encoder/epipolar/depth_predictor_monocular.py:37-81   everything after `projection`;
 *   - src/misc/discrete_probability_distribution.py:7-33              sampling / top-k;
 *   - src/model/encoder/epipolar/conversions.py:5-14                  relative disparity -> depth;
 *   - src/model/encoder/encoder_epipolar.py:113-126,190               map_pdf_to_opacity / gaussians_per_pixel.
 *
 * Input rows.  The head's Linear output is read in place: rows = num_cameras * rays rows, row_stride
 * floats apart, of W = 2 S F floats; S = buckets, F = surfaces.  Channel (bucket * F + surface) * 2 + c:
 * c = 0 the pdf logit, c = 1 the offset logit (the reference's "... (dpt srf c) -> c ... srf dpt").
 *
 * Forward, per (row, surface), in float32:
 *   1. p = softmax(pdf logits)                     (exp(l - max) / sum)
 *   2. o = sigmoid(offset logits)                  (1 / (1 + exp(-a)))
 *   3. n = p / (FLT_EPSILON + sum p)
 *   4. stochastic: for each of the k samples, with the caller's uniform u (an INPUT: the random
 *      generator stays with the caller),
 *          index = min(#{ i : c_i <= u }, S - 1),   c = inclusive cumulative sum of n
 *      (searchsorted(c, u, right=True).clip(max = S - 1)).  The kernel sums c in float32 in scan order,
 *      so a u within a few float32 ulps of an edge may land on either side of it.
 *   5. LSR_DEPTH_HEAD_DETERMINISTIC: the k largest p, in descending order; ties go to the LOWEST
 *      index (torch.topk leaves tie order open).  Needs k <= S.
 *   6. rd = (index + o[index]) / S
 *   7. depth = 1 / ((1 - rd) (1/(near + 1e-10) - 1/(far + 1e-10)) + 1/(far + 1e-10) + 1e-10),
 *      near / far per camera
 *   8. x = n[index];  with LSR_DEPTH_HEAD_TRANSMITTANCE instead
 *      x = (p / (1 - E + 1e-10))[index],  E = exclusive cumulative sum of p
 *   9. opacity = opacity_scale * 0.5 (1 - (1 - x)^e + x^(1/e)),  e = opacity_exponent (what
 *      map_pdf_to_opacity computes as 2**x_cfg).  e == 1 is evaluated as opacity_scale * x: with scale 1
 *      exactly what DepthPredictorMonocular returns by itself.
 * Outputs depth, opacity (float) and index (int32), each [rows][F][k], contiguous.
 *
 * Backward.  dL/dlogits from dL/ddepth and dL/dopacity: the gradient torch autograd computes for the
 * composition above — through o[index]; through n[index] including the dense normalisation term and
 * the epsilon; through the transmittance quotient and its cumulative sum; through the softmax.  Nothing
 * flows through index or u; near / far are constants (no gradient is computed for them).  Repeated
 * indices of a row accumulate.  p is recomputed from the logits (nothing but the int32 indices is kept
 * from the forward).  A (row, surface) has one owner and its sums run in a fixed order: no atomics, the
 * result is bitwise reproducible.  Every element of the W-float row of d_logits is WRITTEN (not
 * accumulated); floats between W and grad_row_stride are not touched.
 */
#ifndef LSR_DEPTH_HEAD_H
#define LSR_DEPTH_HEAD_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_DEPTH_HEAD_MAX_BUCKETS 64
#define LSR_DEPTH_HEAD_MAX_SAMPLES 8
#define LSR_DEPTH_HEAD_MAX_ROW_FLOATS 4096
#define LSR_DEPTH_HEAD_DETERMINISTIC 1   /* flags: top-k instead of sampling (uniforms is not read) */
#define LSR_DEPTH_HEAD_TRANSMITTANCE 2   /* flags: step 8's transmittance quotient */

typedef struct lsr_depth_head_dims {
    int32_t num_cameras;      /* >= 1: one near / far pair per camera */
    int32_t rays;             /* rows per camera, >= 0 (0: nothing is launched, LSR_OK) */
    int32_t buckets;          /* S in 1..LSR_DEPTH_HEAD_MAX_BUCKETS, any value (not only powers of two) */
    int32_t surfaces;         /* F >= 1; 2 S F > LSR_DEPTH_HEAD_MAX_ROW_FLOATS: LSR_EUNSUPPORTED */
    int32_t samples;          /* k in 1..LSR_DEPTH_HEAD_MAX_SAMPLES (deterministic: k <= S) */
    int32_t flags;            /* LSR_DEPTH_HEAD_*; other bits must be 0 */
    float opacity_exponent;   /* e > 0, finite */
    float opacity_scale;      /* finite (1 / gaussians_per_pixel in the encoder) */
    int64_t row_stride;       /* floats between consecutive rows of `logits`, >= 2 S F */
    int64_t grad_row_stride;  /* backward: floats between consecutive rows of `d_logits`, >= 2 S F
                               * (the forward ignores it) */
} lsr_depth_head_dims;

/* logits [rows] (row_stride apart) x 2 S F, near / far [num_cameras], uniforms [rows][F][k] in [0, 1]
 * (may be NULL with LSR_DEPTH_HEAD_DETERMINISTIC) -> depth, opacity, index [rows][F][k].  One launch. */
int lsr_depth_head_forward(const lsr_depth_head_dims *d, const float *logits, const float *near,
                           const float *far, const float *uniforms, float *depth, float *opacity,
                           int32_t *index, lsr_stream_t stream);

/* index [rows][F][k] as the forward wrote it (values outside 0..S-1 are clamped); g_depth / g_opacity
 * [rows][F][k], either may be NULL (= zero) -> d_logits [rows] (grad_row_stride apart) x 2 S F, written.
 * One launch. */
int lsr_depth_head_backward(const lsr_depth_head_dims *d, const float *logits, const float *near,
                            const float *far, const int32_t *index, const float *g_depth,
                            const float *g_opacity, float *d_logits, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_DEPTH_HEAD_H */
