/*
 * lsr_distortion.h — C ABI of the depth distortion regulariser of a trainable 3DGS scene (lsr_scene.h): the term of
 * Mip-NeRF 360 in the squared form of 2DGS, which pulls the Gaussians along a ray onto one surface.  For one pixel with
 * blending weights w_i = alpha_i T_i and per-Gaussian depths m_i,
 *   D = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2 = A M2 - M1^2,   A = sum w_i,  M1 = sum w_i m_i,  M2 = sum w_i m_i^2
 * (expand 1/2 sum_{i,j}).  A is the mask the rasterizer returns; M1 and M2 are two `features` payload channels blended with
 * the weights, skips and early stop of every other channel.  Two streaming operators on either side of the unchanged
 * rasterizer, like lsr_normals.h:
 *   A  lsr_scene_depth_moments_*   (m', m'^2) per (view, Gaussian), m' = m - pivot
 *   B  lsr_distortion_loss_*       the image-space loss A M2 - M1^2 and its gradient.
 * D does not change when one constant is subtracted from every m of a pixel; A M2 - M1^2 in float32 cancels when the layers
 * along a ray are close compared with their distance.  So A subtracts a per-view pivot BEFORE squaring and B forms the
 * difference in double.
 * Same library (liblsr_hip.so) and conventions as lsr_normals.h and lsr_depth_loss.h: device float32 pointers, a stream,
 * asynchronous, negative LSR_E* codes returned before any GPU work, nothing allocated, nothing read back,
 * graph-capturable.  No atomics at all: every sum is formed in a fixed order and two calls give the same bits.
 */
#ifndef LSR_DISTORTION_H
#define LSR_DISTORTION_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_DIST_MAX_ROWS (1 << 28)        /* n stays below this */
#define LSR_DIST_MAX_VIEWS 65536           /* num_views stays at or below this */
#define LSR_DIST_THREADS 256               /* lanes of a workgroup of operator A, and of its camera compaction launch */
#define LSR_DIST_MAX_BLOCKS 2048           /* workgroups of operator A: beyond 2048 * 256 Gaussians a lane takes a second one */
#define LSR_DIST_CHUNK 2048                /* pixels of one view that one workgroup of operator B owns */

enum { LSR_DIST_LINEAR = 0, LSR_DIST_NDC = 1, LSR_DIST_DISPARITY = 2 };

/* ---- A: per-(view, Gaussian) depth moments ---- */

/* Bytes of device scratch the two calls below need (0 for n <= 0 or num_views out of range): one compacted 48-byte record
 * per camera. */
size_t lsr_scene_depth_moments_workspace_bytes(int64_t n, int32_t num_views);

/* xyz [n][3]; views [num_views][LSR_VIEW_FLOATS], the rasterizer's own records; pivot [num_views] (NULL: 0);
 * moments [num_views][n][2].  Per Gaussian g and view v:
 *   z  = the camera-space depth of the unscaled scene: the view-space z the projection kernels compute (row 2 of the
 *        world->view matrix applied to s x_g, s = view[40]) divided by s: the z of the depth modes of lsr_rasterizer.h
 *   m  = z                              LSR_DIST_LINEAR
 *        f / (f - n) (1 - n / z)        LSR_DIST_NDC, n = view[42], f = view[43] (the mapping of 2DGS)
 *        1 / z                          LSR_DIST_DISPARITY
 *   m' = m - pivot[v];   moments[v][g] = (m', m'^2).
 * A pair that is not finite (a NaN or infinite coordinate or record, an overflowing square) or has z <= 0 writes (0, 0);
 * the rasterizer culls it anyway.
 * Near and far live on the device, so this call cannot look at them: n >= f or a non-finite near / far under LSR_DIST_NDC
 * is refused on the host side, in latentsplat_amd/distortion.py (LsrError, the sentence of LSR_EINVAL).  Here such a view
 * yields pairs that are not finite and write (0, 0).
 *
 * Two launches: one workgroup compacts the cameras in double (row 2 of the view matrix, its translation divided by s,
 * the two constants of the mapping, the pivot); then a lane per Gaussian loads xyz once and loops over the compacted
 * records, which reach the wave as scalar loads.  Per pair z is formed from the record's doubles and rounded to float32
 * once; everything after it is float32, m' = (m - pivot) formed once and then squared.
 *
 * LSR_EINVAL: n < 0 or n >= 2^28, num_views < 1 or > LSR_DIST_MAX_VIEWS, an unknown space, a workspace that is not
 * 16-byte aligned, a moments (grad_moments) pointer that is not 8-byte aligned: a pair moves as one 8-byte store.
 * LSR_ENULL: with n > 0 a NULL xyz, views, moments or workspace.  n == 0 launches nothing and returns LSR_OK. */
int lsr_scene_depth_moments_forward(int64_t n, const float *xyz, int32_t num_views, const float *views, const float *pivot,
                                    int32_t space, float *moments, void *workspace, lsr_stream_t stream);

/* grad_moments [num_views][n][2] -> grad_xyz [n][3], WRITTEN, never accumulated: the sum over the views, formed in view
 * order (in double) by the lane that owns the Gaussian, of (g0 + 2 m' g1) dm/dz row, row = row 2 of the world->view
 * matrix.  Pairs whose forward wrote (0, 0) contribute 0.  The view table and the pivot are constants of this operator:
 * the call has no output for them.  Same launches, codes and limits as the forward. */
int lsr_scene_depth_moments_backward(int64_t n, const float *xyz, int32_t num_views, const float *views, const float *pivot,
                                     int32_t space, const float *grad_moments, float *grad_xyz, void *workspace,
                                     lsr_stream_t stream);

/* ---- B: the distortion loss ---- */

typedef struct lsr_distortion_dims {
    int32_t num_images;    /* V >= 1 */
    int32_t height;        /* H >= 1 */
    int32_t width;         /* W >= 1 */
    int32_t reserved0;     /* 0 */
    int32_t reserved1;     /* 0 */
    int32_t reserved2;     /* 0 */
} lsr_distortion_dims;

/* Bytes of the workspace the forward needs (one double partial sum per LSR_DIST_CHUNK pixels of every image): a pure
 * function of the dims, host only.  0 for dims the forward would refuse. */
size_t lsr_distortion_loss_workspace_bytes(const lsr_distortion_dims *dims);

/* moment_map [V][2][H][W]: the rendered sums of alpha T m' and alpha T m'^2; alpha [V][H][W]: the rendered sum of alpha T;
 * weight [V][H][W], optional (NULL: 1).  Per pixel, in double from the float32 inputs:
 *   d(p) = alpha(p) M2(p) - M1(p)^2        NOT clamped: a negative value is rounding and keeps its gradient
 *   per_view[v] = sum_p weight(p) d(p) / (H W);   loss = mean_v per_view[v].
 * Outputs, each optional (NULL = not wanted): loss [1], per_view [V], distortion [V][H][W] (d, without the weight, rounded
 * to float32 once).
 * Two launches: a workgroup owns LSR_DIST_CHUNK consecutive pixels of one view and writes their sum (wave butterfly, then
 * the four waves in order) into its own workspace slot; a finishing launch adds the slots of an image in a fixed order.
 * The numbers of a view do not depend on which other views share the call.
 * LSR_ENULL: a NULL dims, moment_map, alpha or workspace.  LSR_EINVAL: a size < 1, a non-zero reserved field, a workspace
 * that is not 16-byte aligned.  LSR_EUNSUPPORTED: 2 V H W >= 2^31. */
int lsr_distortion_loss_forward(const lsr_distortion_dims *dims, const float *moment_map, const float *alpha,
                                const float *weight, void *workspace, float *loss, float *per_view, float *distortion,
                                lsr_stream_t stream);

/* One launch: with g(p) = *grad_loss weight(p) / (V H W) (*grad_loss a DEVICE float), each output WRITTEN, never
 * accumulated, each optional (NULL = not wanted):
 *   grad_moment_map [V][2][H][W] = (-2 g M1, g alpha);   grad_alpha [V][H][W] = g M2.
 * weight receives no gradient.  Same codes as the forward (no workspace is needed; LSR_ENULL also for a NULL grad_loss). */
int lsr_distortion_loss_backward(const lsr_distortion_dims *dims, const float *moment_map, const float *alpha,
                                 const float *weight, const float *grad_loss, float *grad_moment_map, float *grad_alpha,
                                 lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_DISTORTION_H */
