/*
 * lsr_density.h — C ABI of adaptive density control for a trainable 3DGS scene (lsr_scene.h): the per-step
 * densification statistics, and the published trainer's densify_and_clone -> densify_and_split -> prune_points
 * sequence as a plan (classify, scan, emit a row map) and one element-dense gather over every per-Gaussian table
 * (parameters and optimiser moments).  Same library (liblsr_hip.so) and conventions as lsr_scene.h: device float32
 * pointers, a stream, asynchronous, negative LSR_E* codes returned before any GPU work, n == 0 launches nothing and
 * returns LSR_OK.  No float atomics; every output element has one owner: two calls give the same bits.
 */
#ifndef LSR_DENSITY_H
#define LSR_DENSITY_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_DENSIFY_MAX_SPLIT 8          /* children per split parent: 1..8 */
#define LSR_DENSIFY_MAX_TABLES 24
#define LSR_DENSIFY_MAX_WIDTH 4096       /* floats per row of a table */
#define LSR_DENSIFY_KIND_SHIFT 28        /* map[j] = parent | kind << 28 */
#define LSR_DENSIFY_MAX_ROWS (1 << 28)   /* n * max(2, N) and n_out stay below this */

enum {                       /* map kinds: what output row j is */
    LSR_DENSIFY_KEPT = 0,    /* the original */
    LSR_DENSIFY_CLONE = 1,   /* a clone of a clone-selected Gaussian */
    LSR_DENSIFY_CHILD0 = 2   /* LSR_DENSIFY_CHILD0 + c: child c of a split-selected Gaussian */
};

enum {                       /* lsr_densify_table.rule */
    LSR_DENSIFY_COPY = 0,      /* every row copies its parent's row */
    LSR_DENSIFY_ZERO_NEW = 1,  /* kept rows copy; clones and children are 0 (optimiser moments) */
    LSR_DENSIFY_XYZ = 2,       /* width 3; kept rows and clones copy; a child is its parent's mean plus a rotated, scaled normal draw */
    LSR_DENSIFY_SCALING = 3    /* width 3; children get logf(expf(s) / (0.8f N)); other rows copy */
};

/* The published add_densification_stats and max_radii2D update, once per view, in one launch: for each Gaussian g, for
 * v = 0 .. V-1 in that order, if radii[v][g] > 0: grad_accum[g] += sqrtf(gx^2 + gy^2) of grad_means2D[v][g],
 * denom[g] += 1, max_radii[g] = max(max_radii[g], (float)radii[v][g]).  grad_means2D is [V][n][3] (the third component
 * is not read), radii [V][n] int32; the three statistics [n] float32 are updated in place.  The gradient is taken as it
 * is: nothing is rescaled.  LSR_EINVAL: V < 0 or n < 0.  LSR_ENULL: a NULL pointer with V > 0 and n > 0. */
int lsr_density_accumulate(int32_t V, int64_t n, const float *grad_means2D, const int32_t *radii, float *grad_accum,
                           float *denom, float *max_radii, lsr_stream_t stream);

typedef struct lsr_densify_params {
    float grad_threshold;    /* on avg = grad_accum / denom (NaN -> 0) */
    float dense_extent;      /* percent_dense * extent: clone at or below, split above */
    float min_opacity;       /* rows with sigmoid(opacity) below it are not emitted */
    float max_screen_size;   /* 0: no size pruning */
    float world_limit;       /* 0.1 * extent; read only when max_screen_size > 0 */
    int32_t n_split;         /* N: 1 .. LSR_DENSIFY_MAX_SPLIT */
    int32_t reserved0, reserved1;   /* 0 */
} lsr_densify_params;

/* Bytes of device scratch lsr_densify_plan needs for n Gaussians (0 for n <= 0). */
size_t lsr_densify_workspace_bytes(int64_t n);

/* The plan.  With avg = grad_accum / denom (NaN -> 0), smax = max_k expf(scaling[g][k]), o = 1 / (1 + expf(-opacity[g]))
 * and big = max_screen_size > 0, a Gaussian is clone-selected when avg >= grad_threshold && smax <= dense_extent and
 * split-selected when avg >= grad_threshold && smax > dense_extent.  Emitted:
 *   the original, unless split-selected, o < min_opacity, or big && (max_radii > max_screen_size || smax > world_limit);
 *   one clone of a clone-selected Gaussian, unless o < min_opacity or big && smax > world_limit;
 *   the N children of a split-selected Gaussian, unless o < min_opacity or big && smax / (0.8f N) > world_limit
 * — what the published densify_and_clone -> densify_and_split -> prune_points sequence keeps, with new rows carrying a
 * max_radii2D of 0.  Output order: the kept originals in index order, then the clones in parent order, then the children
 * child-major (child 0 of every emitting parent in parent order, then child 1, ...).  map[j] = parent | kind << 28 for
 * j < n_out; counts = {kept, clones, split_parents (the emitting ones), n_out}; n_out = kept + clones + N split_parents.
 * A per-chunk classification, a scan of the chunk sums and a per-chunk emission: three launches, nothing read back.
 * LSR_EINVAL: n < 0, N out of range, n * max(2, N) >= 2^28, capacity < n * max(2, N), a threshold that is not finite
 * (world_limit only when it is read), a non-zero reserved field.  LSR_ENULL: params NULL, or with n > 0 any other NULL
 * pointer.  With n == 0 nothing is launched and counts is not written. */
int lsr_densify_plan(int64_t n, const float *opacity, const float *scaling, const float *grad_accum, const float *denom,
                     const float *max_radii, const lsr_densify_params *params, uint32_t *map, int64_t capacity,
                     uint32_t *counts, void *workspace, lsr_stream_t stream);

typedef struct lsr_densify_table {
    const float *src;    /* [n][width] */
    float *dst;          /* [n_out][width]; must not overlap any src */
    int32_t width;       /* 1 .. LSR_DENSIFY_MAX_WIDTH; 3 for the XYZ and SCALING rules */
    int32_t rule;        /* LSR_DENSIFY_* */
} lsr_densify_table;

/* dst[j][:] of every table from the plan's map, in ONE launch, element-dense (consecutive lanes move consecutive floats
 * of dst).  n_out is the host's copy of counts[3] and sizes every dst; kept and clones are read from `counts` on the
 * device.  XYZ: child row r = j - kept - clones is xyz + R(q / |q|) (expf(scaling) * eps[r]) with the parent's scaling
 * [n][3] logs, rotation [n][4] w,x,y,z and the caller's standard normals eps [eps_rows][3], eps_rows = N split_parents
 * (the shape and order of the published draw).  scaling is required with an XYZ or SCALING table, rotation with an XYZ
 * table, eps with an XYZ table and eps_rows > 0.  A map entry whose parent is not below n, or a child row beyond
 * eps_rows, writes 0 and reads nothing.
 * LSR_EINVAL: n < 0, n_out < 0 or >= 2^28, n == 0 with n_out > 0, N out of range, num_tables out of 0..24, a width or
 * rule out of range, eps_rows < 0.  LSR_ENULL: with n_out > 0 and num_tables > 0, a NULL map, counts, tables, src, dst
 * or required extra pointer.  n_out == 0 or num_tables == 0 launches nothing. */
int lsr_densify_apply(int64_t n, int64_t n_out, const uint32_t *map, const uint32_t *counts, int32_t n_split,
                      const lsr_densify_table *tables, int32_t num_tables, const float *scaling, const float *rotation,
                      const float *eps, int64_t eps_rows, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_DENSITY_H */
