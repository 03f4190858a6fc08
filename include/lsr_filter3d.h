/*
 * lsr_filter3d.h — C ABI of the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024) for a trainable 3DGS scene
 * (lsr_scene.h): for every Gaussian the smallest size the training cameras can resolve, from the highest sampling rate
 * (focal length over depth) among the cameras that see it.  The filtered activation that uses the result is
 * lsr_scene_activate_filtered_forward / _backward (lsr_scene.h).  Same library (liblsr_hip.so) and conventions as
 * lsr_mcmc.h: device float32 pointers, a stream, asynchronous, negative LSR_E* codes returned before any GPU work,
 * n == 0 launches nothing and returns LSR_OK, nothing is read back.  No float atomics; the one atomic is an integer
 * maximum, whose result does not depend on the order: two calls give the same bits.
 *
 * The screen-space half of Mip-Splatting (the 2D box filter that replaces the rasterizer's +0.3 dilation) is not part
 * of this library.
 */
#ifndef LSR_FILTER3D_H
#define LSR_FILTER3D_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_FILTER3D_MAX_ROWS (1 << 28)     /* n stays below this */
#define LSR_FILTER3D_MAX_VIEWS 65536        /* num_views stays at or below this (4 MiB of workspace) */

enum {                              /* lsr_filter3d_compute mode */
    LSR_FILTER3D_PUBLISHED = 0,     /* smallest depth among the cameras that see the Gaussian over the LARGEST focal length of all */
    LSR_FILTER3D_PER_VIEW = 1       /* the largest focal length over depth among the cameras that see it: the exact bound */
};

/* Bytes of device scratch lsr_filter3d_compute needs (0 for n <= 0 or num_views out of range): a 64-byte header and one
 * compacted 64-byte record per camera. */
size_t lsr_filter3d_workspace_bytes(int64_t n, int32_t num_views);

/* xyz [n][3]; views [num_views][LSR_VIEW_FLOATS], the rasterizer's own records (lsr_build_views, lsr_pack_view); filter [n];
 * seen [n] uint8, optional (NULL = not wanted).  Per camera v, with s = view[40] and W the world->view matrix held
 * transposed in slots 0..15,
 *   p = W (s x, 1):  p.x = view[0] s x + view[4] s y + view[8] s z + view[12],  p.y from slots 1, 5, 9, 13,
 *                    p.z = view[2] s x + view[6] s y + view[10] s z + view[14];
 *   the Gaussian is VALID for v exactly when  p.z > 0.2  (the rasterizer's near-plane cull, in the scaled space),
 *   |p.x| <= (1 + 2 margin) view[35] p.z  and  |p.y| <= (1 + 2 margin) view[36] p.z  (no division; with margin = 0.15 the
 *   published -0.15 W <= pixel <= 1.15 W for a centred principal point, and the 1.3 of the rasterizer's frustum clamp);
 *   a NaN anywhere makes the pair invalid, and so does a camera whose s, view[35] or view[36] is not finite and positive;
 *   z_v = p.z / s,  focal_v = width / (2 view[35]).
 * LSR_FILTER3D_PUBLISHED:  filter[g] = (min over valid v of z_v) / (max over all v of focal_v) * sqrt(variance)
 * LSR_FILTER3D_PER_VIEW:   filter[g] = sqrt(variance) / (max over valid v of focal_v / z_v)
 * (the same value when all focal lengths agree; the published variance is 0.2).  A Gaussian that no camera sees takes the
 * LARGEST filter among the seen ones (the published distance[~valid] = distance[valid].max()); when none is seen every
 * filter is 0.  A Gaussian whose smallest z_v is not finite (an infinite coordinate) counts as unseen, so that it cannot
 * make the largest filter infinite.  seen[g] = 1 where some camera sees g, else 0.
 *
 * Three launches: one workgroup compacts the cameras (the products view[i] s, the two frustum limits, 1 / s or
 * 1 / (s focal_v), all per camera and evaluated in double) and clears the maximum; each lane loops over the compacted
 * records for its own Gaussians (four per lane), the records reaching the wave as scalar loads, keeps the minima in
 * registers, and the wave adds its largest filter to the global maximum with one integer atomicMax on the bit pattern of a
 * non-negative float; the last launch writes the rows of the unseen.  p.z is three FMAs; the filter is that times two
 * per-call constants.
 *
 * LSR_EINVAL: n < 0 or n >= 2^28, num_views < 1 or > LSR_FILTER3D_MAX_VIEWS, width < 1, margin not finite or negative,
 * variance not finite or not positive, an unknown mode.  LSR_ENULL: with n > 0 a NULL xyz, views, filter or workspace. */
int lsr_filter3d_compute(int64_t n, const float *xyz, int32_t num_views, const float *views, int32_t width, float margin,
                         float variance, int32_t mode, float *filter, uint8_t *seen, void *workspace, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_FILTER3D_H */
