/*
 * lsr_bilagrid.h — C ABI of the bilateral-grid appearance compensation: an operator between a render and the photometric
 * loss that absorbs what changes from photograph to photograph (exposure, white balance, vignetting).  Same library
 * (liblsr_hip.so) and conventions as lsr_loss.h: device pointers, a dims struct, a stream, negative LSR_E* codes,
 * asynchronous on the caller's stream, nothing allocated, the host never waited for.
 *
 * A bilateral grid ("Bilateral Guided Radiance Field Processing", Wang et al., SIGGRAPH 2024) is a 3-D table of 3 x 4
 * colour affines.  grids is [N][12][L][Y][X] float32, the published parameter layout (channel, luminance, y, x); channel
 * 4 r + k is entry (r, k) of the matrix.  image is [V][3][H][W]; view v is sliced by grid grid_idx[v].  For pixel (v, y, x)
 * with p = image[v][:][y][x]:
 *   u_x = (x + 0.5) / W (X - 1),  u_y = (y + 0.5) / H (Y - 1),  u_z = (0.299 p0 + 0.587 p1 + 0.114 p2) (L - 1),
 * each clamped to [0, size - 1]; A is the trilinear interpolation of the matrices of the two neighbouring nodes per axis (an
 * axis of size 1: its single node), and
 *   out[v][:][y][x] = A[:, :3] p + A[:, 3].
 * That is torch's grid_sample(grids[idx], 2 (x, y, luma) - 1, "bilinear", "border", align_corners=True) followed by the
 * affine.  A 1 x 1 x 1 grid is one affine per image.  A non-finite luminance reads node 0 (the pixel's own output is then
 * whatever the arithmetic gives; no other pixel and nothing outside the arrays is touched).
 * grid_idx[v] outside [0, N) means that view v has no grid: out is image and grad_image is grad_out, bit for bit, and no grid
 * receives anything from it.
 *
 * Gradients, with g = grad_out[v][:][y][x] and q = (p, 1):
 *   d grids[idx[v]][4 r + k][node] += w_node g_r q_k   for the 8 nodes,
 *   d p = A[:, :3]^T g + (L - 1) [0 < u_z < L - 1] (g^T (dA/dz) q) (0.299, 0.587, 0.114),
 * u_z unclamped, dA/dz the xy-interpolated difference of the upper and the lower luminance node.
 *
 * Total variation: tv = sum over the three grid axes of size >= 2 of mean((g[i + 1] - g[i])^2), the mean over all grids,
 * channels and cells of the difference; an axis of size 1 contributes 0.
 */
#ifndef LSR_BILAGRID_H
#define LSR_BILAGRID_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_BILAGRID_MAX_XY 64
#define LSR_BILAGRID_MAX_L 16

typedef struct lsr_bilagrid_dims {
    int32_t num_views;     /* V >= 1 (the tv calls do not read num_views, height, width) */
    int32_t height;        /* H >= 1 */
    int32_t width;         /* W >= 1 */
    int32_t num_grids;     /* N >= 1 */
    int32_t grid_l;        /* 1 <= L <= 16 */
    int32_t grid_y;        /* 1 <= Y <= 64 */
    int32_t grid_x;        /* 1 <= X <= 64 */
    int32_t reserved0;     /* 0 */
} lsr_bilagrid_dims;

/* The kernel path the slice calls take for these dims: a pure function of the dims, host only.  32 or 16: one workgroup per
 * 32 x 32 / 16 x 16 pixel tile of one view, the grid nodes the tile can reach (known from its pixel range alone, every
 * luminance level) staged in LDS cell-major, 12 contiguous floats per node; the largest tile whose footprint is at most
 * 640 nodes (30 KiB; the backward holds it twice).  0: no tile's footprint fits (a grid much finer than the image): the same
 * per-pixel arithmetic on 16 x 16 tiles reading the parameter directly.  Negative: the code the slice calls would return. */
int lsr_bilagrid_slice_path(const lsr_bilagrid_dims *dims);

/* One launch, no atomics: two calls give the same bits.  out [V][3][H][W] is written.
 * LSR_ENULL: a NULL dims, grids, image, grid_idx or out.  LSR_EINVAL (before any GPU work): a size < 1, a non-zero reserved
 * field.  LSR_EUNSUPPORTED: X or Y > 64, L > 16, V 3 H W >= 2^31, N 12 L Y X >= 2^31. */
int lsr_bilagrid_slice_forward(const lsr_bilagrid_dims *dims, const float *grids, const float *image, const int32_t *grid_idx,
                               float *out, lsr_stream_t stream);

/* Two launches.  grad_image [V][3][H][W] is written.  grad_grids is the whole [N][12][L][Y][X] tensor (4-byte alignment
 * is enough): zeroed inside the call by the first launch, then accumulated by the second.  A is recomputed from grids and
 * image: the forward saves nothing.  grad_grids may be NULL (frozen grids: only the image's gradient is wanted): one launch,
 * nothing zeroed or accumulated, grad_image the same bits.
 * How the grid gradient is summed: ATOMICS, not slabs.  A wave sums the contributions of its pixels that share a node, adds
 * the sums into an LDS copy of the workgroup's footprint (LDS float atomics), and the workgroup flushes the non-zero
 * entries once, with global float atomics in runs along x (path 0: one global float atomic per contribution).  grad_grids is
 * therefore reproducible to summation order only, not bit for bit; grad_image is.
 * Same codes as the forward; every pointer but grad_grids is required. */
int lsr_bilagrid_slice_backward(const lsr_bilagrid_dims *dims, const float *grids, const float *image, const int32_t *grid_idx,
                                const float *grad_out, float *grad_image, float *grad_grids, lsr_stream_t stream);

/* Bytes of the workspace lsr_bilagrid_tv_forward needs (three double partial sums per workgroup): a pure function of the
 * dims, host only.  0 for dims the call would refuse. */
size_t lsr_bilagrid_tv_workspace_bytes(const lsr_bilagrid_dims *dims);

/* tv [1] = the total variation of grids.  One launch that leaves the three axes' sums of squared differences of every
 * workgroup's share of the elements (a fixed share, summed in double in a fixed order) in the workgroup's own workspace
 * slot, and one workgroup that adds the slots in a fixed order.  No atomics: two calls give the same bits.
 * LSR_ENULL: a NULL dims, grids, workspace or tv.  LSR_EINVAL: a grid size or N < 1, a non-zero reserved field, a workspace
 * that is not 8-byte aligned.  LSR_EUNSUPPORTED: the grid limits above. */
int lsr_bilagrid_tv_forward(const lsr_bilagrid_dims *dims, const float *grids, void *workspace, float *tv, lsr_stream_t stream);

/* One launch: grad_grids [N][12][L][Y][X] = *grad_tv * d tv / d grids, written, never accumulated; a gather over each
 * element's six neighbours, so the same bits every call.  grad_tv is a DEVICE pointer to one float. */
int lsr_bilagrid_tv_backward(const lsr_bilagrid_dims *dims, const float *grids, const float *grad_tv, float *grad_grids,
                             lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_BILAGRID_H */
