/*
 * lsr_knn.h — C ABI of the exact three-nearest-neighbour search behind the point-cloud initialisation of a trainable
 * 3DGS scene (lsr_scene.h): for every point of a cloud, the squared distances to its three nearest neighbours, their
 * indices and the mean of the three (what the published trainer's create_from_pcd takes each Gaussian's initial
 * log-scale from).  Same library (liblsr_hip.so) and conventions as lsr_density.h: device float32 pointers, a stream,
 * asynchronous, negative LSR_E* codes returned before any GPU work, n == 0 launches nothing and returns LSR_OK.  No float
 * atomics; every output element has one owner and the result does not depend on the scan order: two calls give the same
 * bits.
 *
 * The search is exact.  The points are sorted along a Morton curve (21 bits per axis), cut into chunks of 128 with an
 * axis-aligned box each (and a box per 64 chunks above them); a wavefront answers 64 consecutive queries and skips only
 * chunks whose box lies farther from the wave's query box than its largest third-best distance, or from every one of
 * its queries than that query's own third-best.  On a cloud with spatial structure that scans a handful of chunks per
 * wave; the worst case stays O(n^2): a cloud whose points all fall into one Morton cell (all points coincident is
 * one), or whose every chunk box overlaps every other, is scanned chunk against chunk.
 */
#ifndef LSR_KNN_H
#define LSR_KNN_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_KNN_MAX_POINTS (1 << 28)

/* Bytes of device scratch lsr_knn3 needs for n points (0 for n <= 0).  A pure function of n: it can be asked without a
 * device. */
size_t lsr_knn3_workspace_bytes(int64_t n);

/* For every point i of points[n][3], over every j != i BY INDEX (coincident points are neighbours at distance 0):
 *   dist2[i][k]   the three smallest |p_i - p_j|^2, ascending;
 *   index[i][k]   the j that gave dist2[i][k]; where distances tie, the lower j comes first (this fixes the indices
 *                 whatever order the search visits the points in);
 *   mean_dist2[i] (dist2[i][0] + dist2[i][1] + dist2[i][2]) / 3.
 * Each output is optional (NULL = not wanted); the ones asked for hold the same bits whichever others are.
 * A squared distance is computed from the caller's coordinates as differences, dx dx + dy dy + dz dz in float32, each
 * operation rounded once (nothing is contracted, recentred or expanded into |a|^2 + |b|^2 - 2 a.b): it is within
 * 8 * 2^-24 relative of the exact value, exact zeros are exact, and so are integer lattices.
 * Coordinates are expected to be finite.  For non-finite input the outputs are unspecified (an index may then be
 * INT32_MAX and a distance +inf); every cell index and loop bound is clamped all the same: no access leaves a buffer and
 * every loop ends.
 * LSR_EINVAL: n < 0, n in 1..3 (there are no three neighbours), n > LSR_KNN_MAX_POINTS.  LSR_ENULL, with n > 0: points
 * NULL, all three outputs NULL, workspace NULL.  LSR_EUNSUPPORTED: the device's sort asks for more scratch than
 * lsr_knn3_workspace_bytes reserves for it (checked on the host, before any launch). */
int lsr_knn3(int64_t n, const float *points, float *mean_dist2, float *dist2, int32_t *index, void *workspace,
             lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_KNN_H */
