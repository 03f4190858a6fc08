/*
 * lsr_normals.h — C ABI of the depth-normal consistency regulariser of a trainable 3DGS scene (lsr_scene.h): the term of
 * 2DGS, Gaussian Surfels, GOF, RaDe-GS and PGSR that ties the orientation of the Gaussians to the surface the rendered
 * depth describes.  Two streaming operators on either side of the unchanged rasterizer:
 *   A  lsr_scene_normals_*       one normal per (view, Gaussian): the shortest axis, turned toward the camera, in camera
 *                                space.  The rasterizer blends it as a 3-channel `features` payload (background 0).
 *   B  lsr_normal_consistency_*  the image-space loss between that blended normal map and the normals obtained by
 *                                differentiating the rendered depth map, and its gradient.
 * Same library (liblsr_hip.so) and conventions as lsr_filter3d.h and lsr_loss.h: device float32 pointers, a stream,
 * asynchronous, negative LSR_E* codes returned before any GPU work, nothing allocated, nothing read back.  No atomics at
 * all: every sum is formed in a fixed order and two calls give the same bits.
 */
#ifndef LSR_NORMALS_H
#define LSR_NORMALS_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_NORMALS_MAX_ROWS (1 << 28)     /* n stays below this */
#define LSR_NORMALS_MAX_VIEWS 65536        /* num_views stays at or below this */

/* ---- A: per-(view, Gaussian) normals ---- */

/* Bytes of device scratch the two calls below need (0 for n <= 0 or num_views out of range): one compacted 64-byte record
 * per camera. */
size_t lsr_scene_normals_workspace_bytes(int64_t n, int32_t num_views);

/* xyz [n][3]; scaling [n][3]; rotation [n][4] (16-byte aligned); views [num_views][LSR_VIEW_FLOATS], the rasterizer's own
 * records; normals [num_views][n][3].  Per Gaussian g and view v:
 *   k = the index of the smallest scaling[g][.], ties to the lowest index.  Only the argmin is used, so any strictly
 *       monotone image of the scales serves: raw log-scales or activated scales give the same bits.
 *   a = column k of R(q / |q|), q = rotation[g] in the scene's component order (w, x, y, z; lsr_scene.h): any non-zero
 *       quaternion, raw or unit.
 *   a is negated when <a, campos_v - s x_g> < 0 (0 does not flip), s = view[40] and campos = view[32..34]: the space
 *       lsr_filter3d_compute puts them in (the camera position is stored already scaled, the mean is not).
 *   normals[v][g] = W3 a / c, W3 the upper 3 x 3 of the world->view matrix (slots 0..15, transposed as stored) and
 *       c = sqrt(sum of the squares of its nine entries / 3): a uniform scale in that block is normalised away and the
 *       output has unit length.
 * A row that is not finite (a NaN or infinite parameter or record, a zero quaternion) writes 0.
 *
 * Two launches: one workgroup compacts the cameras in double (W3 / c, campos, s); then one lane per Gaussian forms a
 * once and loops over the compacted records, which reach the wave as scalar loads.
 *
 * LSR_EINVAL: n < 0 or n >= 2^28, num_views < 1 or > LSR_NORMALS_MAX_VIEWS, a rotation pointer that is not 16-byte
 * aligned.  LSR_ENULL: with n > 0 a NULL pointer.  n == 0 launches nothing and returns LSR_OK. */
int lsr_scene_normals_forward(int64_t n, const float *xyz, const float *scaling, const float *rotation, int32_t num_views,
                              const float *views, float *normals, void *workspace, lsr_stream_t stream);

/* grad_normals [num_views][n][3] -> grad_rotation [n][4], WRITTEN, never accumulated: the sum over the views, formed by
 * the lane that owns the Gaussian looping over the views in order, of the gradient through R and through the
 * normalisation q / |q|.  Rows whose forward wrote 0 contribute 0.
 * The argmin k and the sign are piecewise constant: xyz, scaling and the view table receive NO gradient from this operator
 * (there is none to give), and the call has no output for them.
 * Same launches, codes and limits as the forward. */
int lsr_scene_normals_backward(int64_t n, const float *xyz, const float *scaling, const float *rotation, int32_t num_views,
                               const float *views, const float *grad_normals, float *grad_rotation, void *workspace,
                               lsr_stream_t stream);

/* ---- B: depth-normal consistency ---- */

typedef struct lsr_normal_dims {
    int32_t num_images;    /* V >= 1 */
    int32_t height;        /* H >= 1 */
    int32_t width;         /* W >= 1 */
    float alpha_min;       /* finite, > 0 */
    int32_t reserved0;     /* 0 */
    int32_t reserved1;     /* 0 */
} lsr_normal_dims;

/* Bytes of the workspace the forward needs (one double partial sum per 32 x 32 tile of every image): a pure function of
 * the dims, host only.  0 for dims the forward would refuse. */
size_t lsr_normal_consistency_workspace_bytes(const lsr_normal_dims *dims);

/* normal_map [V][3][H][W]: the rendered sum of alpha T n of operator A's normals, NOT renormalised; depth [V][H][W]: the
 * rendered sum of alpha T z of depth mode LSR_DEPTH_NATIVE; alpha [V][H][W]: the rendered sum of alpha T (the mask);
 * views [V][LSR_VIEW_FLOATS].
 *   D(p)   = depth(p) / alpha(p)
 *   r_v(p) = the camera-space ray with z = 1 through the centre of pixel p = (x, y), ndc = ((2 x + 1) / W - 1,
 *            (2 y + 1) / H - 1), from the record's OWN matrices: Q = rows 0, 1, 3 of projmatrix (slots 16..31) times the
 *            inverse of the upper 3 x 3 of viewmatrix (slots 0..15), both transposed as stored, and r solves
 *            Q0 . r = ndc_x Q3 . r,  Q1 . r = ndc_y Q3 . r.  An off-centre principal point and unequal fovs are
 *            honoured.  The record must be a pinhole's (clip x, y, w linear in the camera-space point with no constant
 *            term, as every record of lsr_build_views / lsr_pack_view is): the ray is then affine in (x, y), and the
 *            kernels derive its six coefficients per view in double.
 *   P(p)   = D(p) r_v(p)
 *   p is VALID when it is at least one pixel from every border, alpha > alpha_min at p and at its four neighbours, all
 *            five D are finite, and m = (P(x+1,y) - P(x-1,y)) x (P(x,y+1) - P(x,y-1)) has FLT_MIN <= |m| <= FLT_MAX.
 *   n~(p)  = sigma m / |m|, sigma = -1 when the ray's Jacobian d(r.x, r.y)/d(x, y) has a positive determinant, else +1:
 *            fixed once per view, so that a surface facing the camera gets the direction operator A gives a Gaussian
 *            facing the camera (camera-space z < 0 for a fronto-parallel one).
 *   e(p)   = alpha(p) - <N(p), n~(p)> at valid pixels, 0 elsewhere;   per_view[v] = sum_p e(p) / (H W);
 *   loss   = mean_v per_view[v].
 * The uniform scene scale of slot 40 multiplies every P and cancels in m / |m|: it is never divided by.
 * Outputs, each optional (NULL = not wanted): loss [1], per_view [V], depth_normals [V][3][H][W] (n~, 0 where invalid),
 * valid [V][H][W] uint8.
 * Two launches: one over 32 x 32 tiles (D with a 1-pixel halo staged in LDS, each workgroup deriving its view's ray in
 * double first; the arithmetic per pixel in double; e summed per tile in double into the tile's workspace slot), one
 * that adds the slots per image in a fixed order.  Images with H < 3 or W < 3 have no valid pixel: loss 0, not an error.
 * LSR_ENULL: a NULL dims, depth, alpha, views or workspace; a NULL normal_map when loss or per_view is wanted (without
 * them the map is not read: depth_normals and valid depend on depth and alpha alone).  LSR_EINVAL (before any GPU work): a size < 1, an
 * alpha_min that is not finite and positive, a non-zero reserved field, a workspace that is not 16-byte aligned.
 * LSR_EUNSUPPORTED: 3 V H W >= 2^31. */
int lsr_normal_consistency_forward(const lsr_normal_dims *dims, const float *normal_map, const float *depth, const float *alpha,
                                   const float *views, void *workspace, float *loss, float *per_view, float *depth_normals,
                                   uint8_t *valid, lsr_stream_t stream);

/* One launch: *grad_loss (a DEVICE pointer to one float) times the gradient of the loss, each output WRITTEN, never
 * accumulated, each optional (NULL = not wanted):
 *   grad_normal_map [V][3][H][W] = -g n~(p) / (V H W) at valid pixels, 0 elsewhere;
 *   grad_depth, grad_alpha [V][H][W]: through D alone.  The leading alpha(p) of e is a CONSTANT WEIGHT in the backward, as
 *   the published regulariser detaches it (it would otherwise reward transparency); so alpha receives a gradient only as
 *   the denominator of D.  A pixel gathers the contributions of the four stencils it belongs to (D with a 2-pixel halo in
 *   LDS, n~ recomputed), in the fixed order left, right, up, down.
 * Same codes as the forward (no workspace is needed). */
int lsr_normal_consistency_backward(const lsr_normal_dims *dims, const float *normal_map, const float *depth, const float *alpha,
                                    const float *views, const float *grad_loss, float *grad_normal_map, float *grad_depth,
                                    float *grad_alpha, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_NORMALS_H */
