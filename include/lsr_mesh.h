/*
 * lsr_mesh.h — C ABI of mesh extraction for a trainable 3DGS scene (lsr_scene.h): the step every surface method (2DGS,
 * Gaussian Surfels, GOF, RaDe-GS, PGSR) ends with.  Rendered depth maps are fused into a truncated signed distance volume
 * and a triangle mesh is taken from its zero level set.  Two operators beside the unchanged rasterizer:
 *   A  lsr_tsdf_integrate   one call fuses V rendered views into a dense volume;
 *   B  lsr_mesh_count/emit  marching tetrahedra on the Kuhn subdivision of the lattice: vertices, colours, faces.
 * Same library (liblsr_hip.so) and conventions as lsr_normals.h and lsr_filter3d.h: device float32 pointers, a stream,
 * asynchronous, negative LSR_E* codes returned before any GPU work, nothing allocated, nothing read back.  No atomics at
 * all: two calls give the same bits, and every call can be captured into a graph.
 */
#ifndef LSR_MESH_H
#define LSR_MESH_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_TSDF_MIN_EXTENT 2
#define LSR_TSDF_MAX_EXTENT 2048            /* nx, ny, nz each */
#define LSR_TSDF_MAX_VOXELS (1 << 30)       /* nx ny nz stays at or below this */
#define LSR_TSDF_MAX_VIEWS 1024             /* views per lsr_tsdf_integrate call */

/* The volume.  The sample of lattice point (i, j, k) sits at origin + voxel_size (i, j, k) in WORLD units: the scene's own
 * space, before slot 40 of a view record scales it.  Arrays are x-fastest:
 *   tsdf   [nz][ny][nx]      the mean of the clamped distances, in units of trunc, in [-1, 1]
 *   weight [nz][ny][nx]      the number of observations (capped at max_weight when that is set)
 *   color  [3][nz][ny][nx]   optional planes: the mean of the observed colours */
typedef struct lsr_tsdf_dims {
    int32_t nx, ny, nz;     /* each in LSR_TSDF_MIN_EXTENT..LSR_TSDF_MAX_EXTENT, nx ny nz <= LSR_TSDF_MAX_VOXELS */
    float origin[3];        /* finite */
    float voxel_size;       /* finite, > 0 */
    float trunc;            /* finite, > 0, world units */
    int32_t has_color;      /* 0 or 1 */
    int32_t reserved0;      /* 0 */
    int32_t reserved1;      /* 0 */
    int32_t reserved2;      /* 0 */
} lsr_tsdf_dims;

/* LSR_EINVAL: an extent below 2, a voxel_size or trunc that is not finite and positive, an origin that is not finite, a
 * has_color other than 0 / 1, a non-zero reserved field.  LSR_EUNSUPPORTED: an extent above 2048, more than 2^30 lattice
 * points.  Every call below applies these first. */

/* ---- A: fusion ---- */

/* Bytes of device scratch lsr_tsdf_integrate needs: one compacted 192-byte record per view.  0 for num_views outside
 * 1..LSR_TSDF_MAX_VIEWS.  Host only, a pure function of its argument. */
size_t lsr_tsdf_workspace_bytes(int32_t num_views);

/* depth [V][H][W]: the rendered sum of alpha T z of depth mode LSR_DEPTH_NATIVE; alpha [V][H][W]: the rendered sum of
 * alpha T (the mask); image_color [V][3][H][W]: required exactly when the volume has colour; views [V][LSR_VIEW_FLOATS];
 * alpha_min finite; depth_max: world units, 0 = none; max_weight: 0 = none.
 * For each lattice point x the views are taken in order v = 0..V-1:
 *    1  s = view[40]; c = viewmatrix (s x, 1), z = c.z; clip = projmatrix (s x, 1) (both transposed as stored)
 *    2  skip the view when z <= 0 or clip.w <= 0
 *    3  ndc = clip.xy / clip.w
 *    4  fx = ((ndc_x + 1) W - 1) / 2, ix = floor(fx + 0.5) (the inverse of the rasterizer's ndc = (2 x + 1) / W - 1); same in y
 *    5  skip when (ix, iy) is outside the image: the NEAREST pixel, depth is never interpolated across an edge
 *    6  a = alpha[v][iy][ix]; skip unless a > alpha_min
 *    7  D = depth[v][iy][ix] / a; skip unless D is finite and positive
 *    8  skip when depth_max > 0 and D / s > depth_max
 *    9  sdf = (D - z) / s, the projective distance along the camera axis; skip when sdf < -trunc
 *   10  d = min(1, sdf / trunc)
 *   11  w' = w + 1; tsdf <- (tsdf w + d) / w'; each colour plane likewise from the same pixel; w <- w', capped at
 *       max_weight when that is set
 * The recurrence is float32 and the state between two views is float32, in registers or in memory alike: integrating
 * views 0..4 in one call gives the bits of integrating 0..2 and then 3..4.  A lattice point that no view touched is not
 * written.
 *
 * Two launches.  One workgroup compacts the cameras in double: the affine map from the lattice index to (clip.x, clip.y,
 * clip.w, z) with origin, voxel size and slot 40 folded in, and the six half-space functions of the frustum, rounded to
 * float records in the workspace.  Then a wave owns a brick of 64 x 4 x 1 lattice points (lanes along x), holds their state
 * in registers across all V views, rejects a view for the whole brick with one wave-uniform test of the brick's extent
 * against that view's frustum (conservative: it never rejects a view that steps 2..5 would accept for any of its points),
 * and reads and writes the volume once per CALL.
 *
 * LSR_ENULL: a NULL dims, tsdf, weight, depth, alpha, views or workspace; with has_color a NULL color or image_color.
 * LSR_EINVAL: image_color without has_color; V outside 1..LSR_TSDF_MAX_VIEWS; H or W < 1; alpha_min not finite; depth_max
 * or max_weight negative or not finite; a workspace that is not 16-byte aligned.  LSR_EUNSUPPORTED: V H W >= 2^31. */
int lsr_tsdf_integrate(const lsr_tsdf_dims *dims, float *tsdf, float *weight, float *color, int32_t num_views, int32_t height,
                       int32_t width, const float *depth, const float *alpha, const float *image_color, const float *views,
                       float alpha_min, float depth_max, float max_weight, void *workspace, lsr_stream_t stream);

/* ---- B: marching tetrahedra on the Kuhn subdivision ----
 *
 * Each cube of 8 lattice points, corner (dx, dy, dz) numbered dx + 2 dy + 4 dz, is cut into 6 tetrahedra, one per
 * permutation pi of the axes in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx: v0 = (0,0,0), v1 = v0 + e_pi(0),
 * v2 = v1 + e_pi(1), v3 = (1,1,1).  The subdivision is translation-invariant and face-compatible, so the surface is
 * watertight with no case table.
 * EDGES.  Every edge runs from a lattice point a to a + delta, delta in {0,1}^3 \ 0; it is owned by a with edge index
 * e = delta_x + 2 delta_y + 4 delta_z - 1.  An edge that would leave the grid does not exist.
 * A lattice point is VALID when weight >= min_weight and INSIDE when tsdf < 0 (an exact 0 is outside).
 * VERTICES.  One on every edge whose ends are both valid and exactly one of them inside, at
 * origin + voxel_size (a + t delta), t = f_a / (f_a - f_b), with colour (1 - t) c_a + t c_b.  Vertices are numbered by
 * owner lattice index (x-fastest), then by e.  A vertex that no face uses may remain (at the grid border, next to
 * unobserved space): documented, not filtered.
 * TRIANGLES.  A tetrahedron whose four corners are valid emits one triangle when 1 or 3 corners are inside and, when 2
 * are, a quad split along the diagonal from its lowest-numbered vertex: (q0, q1, q2) then (q0, q2, q3).  Each triangle is
 * wound so that (p1 - p0) x (p2 - p0) points from the inside corners to the outside ones (toward positive distance, toward
 * the cameras), decided from the case and the parity of pi alone, so degenerate triangles get it too (they are kept); its
 * first index is its lowest vertex number.  Triangles are ordered by cube (x-fastest), then tetrahedron, then triangle.
 */

/* Bytes of device scratch the two calls below share: per lattice point a uint32 vertex base, a uint32 face base (of the
 * cube the point is the low corner of) and a uint8 edge mask (a vertex id is the base plus the popcount of the lower mask
 * bits), and two int64 sums per chunk of 256 points.  0 for dims the calls would refuse.  Host only. */
size_t lsr_mesh_workspace_bytes(const lsr_tsdf_dims *dims);

/* Classifies every lattice point and cube, scans (lsr_wave.h: fixed order) and writes counts[0] = vertices,
 * counts[1] = faces (int64, device), exact also beyond 2^31.  Four launches.  color and has_color are not used.
 * LSR_ENULL: a NULL pointer.  LSR_EINVAL: a min_weight that is NaN, a workspace or counts that is not 16-byte / 8-byte
 * aligned. */
int lsr_mesh_count(const lsr_tsdf_dims *dims, const float *tsdf, const float *weight, float min_weight, void *workspace,
                   int64_t *counts, lsr_stream_t stream);

/* After lsr_mesh_count with the same dims, arrays, min_weight, workspace and counts: vertices [Nv][3], vertex_colors
 * [Nv][3] or NULL (needs color and has_color), faces [Nf][3] int32.  A vertex or face whose number is at or beyond its
 * capacity is not written: a capacity below the count writes nothing at or beyond the capacity, the call still returns
 * LSR_OK, and the caller compares counts.  When either count is 2^31 or more nothing is written at all.  One launch.
 * LSR_ENULL: a NULL dims, tsdf, weight, workspace or counts; a NULL vertices with capacity_vertices > 0, a NULL faces with
 * capacity_faces > 0; vertex_colors with a NULL color.  LSR_EINVAL: a negative capacity, vertex_colors without has_color,
 * a misaligned workspace.  LSR_EUNSUPPORTED: a capacity of 2^31 or more. */
int lsr_mesh_emit(const lsr_tsdf_dims *dims, const float *tsdf, const float *weight, const float *color, float min_weight,
                  void *workspace, const int64_t *counts, int64_t capacity_vertices, int64_t capacity_faces, float *vertices,
                  float *vertex_colors, int32_t *faces, lsr_stream_t stream);

/* ---- C: connected components over shared vertex indices (the cleanup after extraction: keep the largest clusters) ----
 *
 * labels[v] ends as the lowest vertex index of v's connected component; two vertices are connected when a face names
 * both BY INDEX (lsr_mesh_emit numbers a vertex once per lattice edge, so its meshes qualify).  A vertex in no face
 * labels itself.  The caller drives rounds:
 *   lsr_mesh_components_init    labels[v] = v;
 *   lsr_mesh_components_round   clears *changed (device int32), then HOOK: per face, each corner's label chain is
 *                               followed to its root and the larger roots' labels take the smallest root by integer
 *                               atomicMin, and *changed becomes 1 when a face saw two roots; then COMPRESS:
 *                               labels[v] = root(v).  Three stream operations.
 * and repeats the round until *changed stays 0; it reads the flag itself and caps the rounds (O(log nv) are needed unless
 * the numbering is adversarial).  labels[x] <= x always and every write lowers a label, so every walk inside a round ends
 * in at most x steps; the fixed point is each component's minimum whatever order the threads ran in (integer atomicMin
 * only): two runs give the same labels.  A face with a corner outside [0, nv) is skipped by the kernel; callers are
 * expected to refuse such a mesh.
 * LSR_EINVAL: a negative count, a count above LSR_MESH_MAX_ELEMENTS.  LSR_ENULL: labels NULL with nv > 0 (init); changed
 * NULL, faces or labels NULL with nv > 0 and nf > 0 (round).  nv == 0 or nf == 0: a round only clears the flag. */
#define LSR_MESH_MAX_ELEMENTS (1 << 30)
int lsr_mesh_components_init(int64_t num_vertices, int32_t *labels, lsr_stream_t stream);
int lsr_mesh_components_round(int64_t num_vertices, int64_t num_faces, const int32_t *faces, int32_t *labels, int32_t *changed,
                              lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_MESH_H */
