/*
 * lsr_depth_loss.h — C ABI of the inverse-depth loss of a trainable 3DGS scene (lsr_scene.h): an L1 between the inverse
 * depth the rasterizer rendered and a target inverse depth, the supervision of geometry both published trainers have
 * (gsplat's `depth_loss` on the sparse points a capture comes with; the 3DGS trainer's depth regularisation against a
 * monocular prior brought to the scene's scale by a per-image scale and offset).  One streaming operator beside the
 * unchanged rasterizer.  Same library (liblsr_hip.so) and conventions as lsr_normals.h and lsr_loss.h: device float32
 * pointers, a stream, asynchronous, negative LSR_E* codes returned before any GPU work, nothing allocated, nothing read
 * back, graph-capturable.  No atomics at all: every sum is formed in a fixed order, two calls give the same bits, and
 * the numbers of a view do not depend on which other views share the call, nor on how its planes are aligned.
 *
 * Per view v and pixel p, with depth [V][H][W] the rendered sum of alpha T tz of depth mode LSR_DEPTH_NATIVE (tz the
 * view-space z of the SCALED scene), alpha [V][H][W] the rendered sum of alpha T, views [V][LSR_VIEW_FLOATS] the table
 * the render used, target [V][H][W] and the optional weight [V][H][W]:
 *   s      = views[v][40]: the scene scale, the same slot and meaning as in lsr_normals.h (tz = s z)
 *   I(p)   = s alpha / depth  where alpha > alpha_min, depth > 0 and both are finite;  0 elsewhere, and there neither input
 *            receives a gradient: an unrendered pixel is "infinitely far", penalised and not excused
 *   w(p)   = weight(p) when weight is given (expected >= 0), else 1 where target > 0 and 0 elsewhere
 *   r(p)   = w(p) (I(p) - (a_v target(p) + b_v))
 *   per_view[v] = sum_p |r(p)| / N_v,   N_v = H W (LSR_DEPTH_NORM_PIXELS) or sum_p w(p) (LSR_DEPTH_NORM_WEIGHTS; 0 gives 0)
 *   loss   = mean_v per_view[v]
 * LSR_DEPTH_ALIGN_GIVEN: (a_v, b_v) = affine[v], (1, 0) when affine is NULL.  A row with a_v == 0 means "no usable target
 *   for this view": per_view[v] = 0 and no gradient.
 * LSR_DEPTH_ALIGN_FIT: (a_v, b_v) minimise sum_p w (a target + b - I)^2 over the view's pixels, solved in double from the
 *   five sums of w, w t, w I, w t^2, w t I (formed in double).  They are CONSTANTS in the backward (the published trainer's
 *   are constants too; the dependence is second order under an L1).  When fewer than two pixels have w > 0, or the target's
 *   weighted variance is at most 2^-24 of its weighted mean square (a target flat to float32 precision), or the solution
 *   is not finite, the row is (0, 0), with the consequence above.
 * All per-pixel arithmetic is in double; I is rounded to float32 only where it is stored.
 *
 * A workgroup owns LSR_DEPTH_LOSS_CHUNK consecutive pixels of one view and writes its partial sums to its own workspace
 * slot; a finishing launch adds the slots of a view in a fixed order (lsr_wave.h: lane-strided, the wave butterfly).  A lane
 * owns groups of 4 consecutive pixels counted from the start of the VIEW: where all input planes of the view are 16-byte
 * aligned (planes of H W floats are aligned only when H W % 4 == 0, or by chance) a whole group moves as one 16-byte load
 * per array, elsewhere, and in the last group of a view with H W % 4 != 0, as single floats; every output plane decides
 * likewise for itself.  The assignment of pixels to lanes is the same either way, so the order of every sum is that of the
 * pixel indices alone.  (A scalar head up to the first aligned address would shift that assignment with the address of
 * the plane, and a view would give other bits in a batch than alone.)
 * GIVEN is two launches forward; FIT adds the moments pass and its finish before them; the backward is one launch.
 */
#ifndef LSR_DEPTH_LOSS_H
#define LSR_DEPTH_LOSS_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_DEPTH_LOSS_CHUNK 2048          /* pixels of one view that one workgroup owns */

enum { LSR_DEPTH_ALIGN_GIVEN = 0, LSR_DEPTH_ALIGN_FIT = 1 };
enum { LSR_DEPTH_NORM_PIXELS = 0, LSR_DEPTH_NORM_WEIGHTS = 1 };

typedef struct lsr_depth_loss_dims {
    int32_t num_views;     /* V >= 1 */
    int32_t height;        /* H >= 1 */
    int32_t width;         /* W >= 1 */
    int32_t align;         /* LSR_DEPTH_ALIGN_* */
    int32_t normalize;     /* LSR_DEPTH_NORM_* */
    float alpha_min;       /* finite, >= 0 */
    int32_t reserved0;     /* 0 */
    int32_t reserved1;     /* 0 */
} lsr_depth_loss_dims;

/* Bytes of the workspace: the per-view table (a, b, 1 / N_v; doubles) and the workgroups' slots.  A pure function of the
 * dims, host only; 0 for dims the forward would refuse.  The forward writes the table and the backward reads it: the SAME
 * workspace, untouched in between, goes to both. */
size_t lsr_depth_loss_workspace_bytes(const lsr_depth_loss_dims *dims);

/* Outputs, each optional (NULL = not wanted), each WRITTEN: loss [1], per_view [V], inverse_depth [V][H][W] (I),
 * affine_out [V][2] (the (a, b) in use: the given ones, (1, 0), the fitted ones, (0, 0) for a refused fit).
 * weight may be NULL; affine_in may be NULL and is not read under LSR_DEPTH_ALIGN_FIT.
 * LSR_ENULL: a NULL dims, depth, alpha, views, target or workspace.  LSR_EINVAL: a size < 1, an unknown align or normalize,
 * an alpha_min that is negative or not finite, a non-zero reserved field, a workspace that is not 16-byte aligned.
 * LSR_EUNSUPPORTED: V H W >= 2^31. */
int lsr_depth_loss_forward(const lsr_depth_loss_dims *dims, const float *depth, const float *alpha, const float *views,
                           const float *target, const float *weight, const float *affine_in, void *workspace, float *loss,
                           float *per_view, float *inverse_depth, float *affine_out, lsr_stream_t stream);

/* One launch.  The upstream gradient of view v is u_v = *grad_loss / V + grad_per_view[v] (DEVICE pointers; either may be
 * NULL and then counts 0; both NULL is LSR_ENULL), so that per_view is differentiable too and a view's gradient does not
 * depend on V when it arrives through grad_per_view.  With k = u_v w(p) sign(r(p)) / N_v (sign(0) = 0; 0 for a row with
 * a_v == 0 or N_v == 0) at the pixels where I is defined:
 *   grad_depth(p) = -k I(p) / depth(p),   grad_alpha(p) = k s / depth(p);   0 elsewhere.
 * Each output is optional and WRITTEN in full, never accumulated.  target and weight receive no gradient.
 * `workspace` is the forward's, with the table it left.  Same codes as the forward. */
int lsr_depth_loss_backward(const lsr_depth_loss_dims *dims, const float *depth, const float *alpha, const float *views,
                            const float *target, const float *weight, const void *workspace, const float *grad_loss,
                            const float *grad_per_view, float *grad_depth, float *grad_alpha, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_DEPTH_LOSS_H */
