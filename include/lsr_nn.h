/*
 * lsr_nn.h — C ABI of the exact nearest-neighbour query of one point cloud against ANOTHER: a persistent index over a
 * reference cloud, and for every foreign query point the squared distance to its nearest reference point and that
 * point's index.  It is the hot path of the mesh metrics (accuracy, completeness, Chamfer, precision / recall / F-score:
 * latentsplat_amd/mesh_eval.py).  lsr_knn3 (lsr_knn.h) does not answer it: it searches a cloud against itself, excludes
 * the query's own index and owns its index for one call.
 * Same library (liblsr_hip.so) and conventions as lsr_knn.h: device float32 pointers, a stream, asynchronous, negative
 * LSR_E* codes returned before any GPU work, nothing read back.  No float atomics; every output element has one owner and
 * the result does not depend on the visiting order: two calls give the same bits.  Sizes are pure functions of the counts
 * and can be asked without a device.
 *
 * The index is lsr_knn3's: the reference sorted along a Morton curve (21 bits per axis of one isotropic grid), 16-byte
 * records (x, y, z, original index), an axis-aligned box per chunk of 128 sorted points and per 64 chunks, and the
 * sorted keys.  A query call sorts the queries along the Morton curve OF THE REFERENCE'S GRID (cells clamped at its
 * faces, so a query far outside still gets a key); a wavefront answers 64 consecutive sorted queries, seeds its bound
 * from the chunk that a binary search of its middle query's key finds in the reference's keys, and walks outward from it
 * as lsr_knn3 does, skipping only chunks whose box lies strictly farther from the wave's query box than the largest best
 * distance any lane holds, or from every query than that query's own best.  The seed only sets the first bound: the
 * result does not depend on it.  The worst case stays O(n m): a reference whose boxes all overlap is scanned whole.
 */
#ifndef LSR_NN_H
#define LSR_NN_H

#include "lsr_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the persistent index over n reference points, and of the scratch lsr_nn_build needs beside it (0 for
 * n <= 0; n above LSR_KNN_MAX_POINTS sizes as LSR_KNN_MAX_POINTS). */
size_t lsr_nn_index_bytes(int64_t n);
size_t lsr_nn_build_workspace_bytes(int64_t n);

/* Builds the index over points[n][3], 1 <= n <= LSR_KNN_MAX_POINTS, into index_mem (256-byte aligned, as a device
 * allocation is).  The index is everything a query needs: `points` and `workspace` may be freed once the stream has run
 * the call.  It is read-only afterwards: any number of queries, on any streams ordered after the build.
 * LSR_EINVAL: n < 1, n > LSR_KNN_MAX_POINTS.  LSR_ENULL: points, index_mem or workspace NULL.  LSR_EUNSUPPORTED: the
 * device's sort asks for more scratch than lsr_nn_build_workspace_bytes reserves for it (checked on the host, before
 * any launch). */
int lsr_nn_build(int64_t n, const float *points, void *index_mem, void *workspace, lsr_stream_t stream);

/* Bytes of device scratch one lsr_nn_query of m queries needs (0 for m <= 0). */
size_t lsr_nn_query_workspace_bytes(int64_t m);

/* For every query i of queries[m][3], over ALL j of the n reference points the index was built from:
 *   dist2[i]   min_j |q_i - r_j|^2;
 *   index[i]   the LOWEST j that attains it (this fixes the index whatever order the search visits the points in).
 * Either output may be NULL (not both); the other holds the same bits.  m == 0 launches nothing and returns LSR_OK.
 * A squared distance is lsr_knn3's: differences of the caller's coordinates, dx dx + dy dy + dz dz left to right in
 * float32, each operation rounded once: within 8 * 2^-24 relative of the exact value, exact zeros are exact.
 * Coordinates are expected to be finite.  For non-finite input the outputs are unspecified (an index may then be
 * INT32_MAX and a distance +inf); every cell index and loop bound is clamped all the same: no access leaves a buffer and
 * every loop ends.
 * LSR_EINVAL: n < 1, n > LSR_KNN_MAX_POINTS, m < 0, m > LSR_KNN_MAX_POINTS.  LSR_ENULL, with m > 0: index_mem or
 * queries NULL, both outputs NULL, workspace NULL.  LSR_EUNSUPPORTED: as lsr_nn_build, for the sort of the queries. */
int lsr_nn_query(int64_t n, const void *index_mem, int64_t m, const float *queries, float *dist2, int32_t *index,
                 void *workspace, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_NN_H */
