// nn.hip — exact nearest neighbour of foreign query points in a persistent index over a reference cloud
// (include/lsr_nn.h): the hot path of the mesh metrics (accuracy / completeness / Chamfer, precision / recall / F-score).
//
// The index is knn.hip's, kept: grid, sorted keys, sorted 16-byte records (x, y, z, original index), chunk boxes, group
// boxes.  It is built by the kernels of knn.hip through the host entry points of lsr_morton.h; this unit adds one kernel.
//
// A query call, all on the caller's stream, nothing read back:
//   morton_sort     the queries' 63-bit Morton codes IN THE REFERENCE'S GRID (k_knn_keys clamps a cell at the grid's
//                   faces: a query far outside the reference still gets a key) and the stable sort of (code, index);
//   k_nn_search     one wavefront per kQueries consecutive sorted queries, one query per lane, its best (distance, index)
//                   in registers; results are written at the queries' original positions.
//
// The search.  A wave's queries are neighbours in space, so the wave walks the reference once for all of them.
//   seed   a binary search of the key of the wave's middle query in the reference's sorted keys gives a position, and
//          the chunk it lies in is scanned first, unconditionally.  This only sets the first bound: a useless seed (all
//          queries outside the reference's box share a few clamped keys) costs scans, never correctness;
//   walk   exactly k_knn_search's: the seed's group of kGroup chunks first, outward from the seed, then the other groups,
//          outward in blocks of 64, with the same two wave-uniform tests before a chunk is staged:
//            box against box    the chunk's (group's) box lies strictly farther from the box of the wave's queries than
//                               the largest best distance any lane holds (lane-parallel over 64 boxes, one ballot);
//            query against box  each lane compares the distance from ITS query to the chunk's box with ITS OWN best; the
//                               chunk is staged only if some lane can still gain;
//   scan   a chunk that passes is staged in LDS and scanned by every lane with broadcast reads.
// One wavefront per workgroup, as in knn.hip: the bound is a wave reduction, the decisions are ballots.
//
// Why it is exact in float32: this unit is compiled with -ffp-contract=off, so a squared distance is the same three
// rounded differences, three rounded squares and two rounded sums wherever it is computed; a box gap is one rounded
// difference of two coordinates that bracket the pair's, and rounding is monotonic, so a box distance never exceeds the
// computed distance of any pair it covers.  The comparisons are strict: a chunk that holds an equally distant point is
// still visited, and the kept pair is the minimum in (distance, index) order, which does not depend on the visiting order.
//
// Every loop is bounded by a count (chunks, groups, 64 bits of a ballot, 32 steps of the binary search) and every index
// is clamped, whatever the coordinates are.  The worst case stays O(n m): when the boxes all overlap every wave scans
// every chunk.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "lsr_morton.h"
#include "lsr_nn.h"

namespace lsr {

// every lane against the `count` records staged in LDS: all lanes read the same record (a broadcast read)
__device__ __forceinline__ void scan_staged1(float &bd, int &bi, const float4 &q, const float4 *s_pts, int count) {
#pragma unroll 4
    for (int j = 0; j < count; ++j) {
        const float4 p = s_pts[j];
        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
        const float d = dx * dx + dy * dy + dz * dz;
        const int idx = __float_as_int(p.w);
        if (d < bd || (d == bd && idx < bi)) { bd = d; bi = idx; }
    }
}

// One wavefront per workgroup: kQueries == LSR_WAVE.  (__syncthreads here orders the one wave's LDS traffic.)
__global__ __launch_bounds__(kQueries) void k_nn_search(int64_t n, int64_t chunks, int64_t groups, const uint64_t *__restrict__ ref_keys,
                                                       const float4 *__restrict__ sorted, const float4 *__restrict__ chunk_boxes,
                                                       const float4 *__restrict__ group_boxes, int64_t m,
                                                       const float *__restrict__ queries, const uint64_t *__restrict__ query_keys,
                                                       const uint32_t *__restrict__ query_order, float *__restrict__ dist2,
                                                       int32_t *__restrict__ index) {
    __shared__ float4 s_pts[kChunk];
    const int lane = threadIdx.x;
    const int64_t first_query = (int64_t)blockIdx.x * kQueries;
    const uint32_t me = first_query + lane < m ? query_order[first_query + lane] : 0xffffffffu;
    const bool valid = (int64_t)me < m;                    // (always, for a lane below m: the sort permutes 0 .. m-1)
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (valid) { q.x = queries[3 * (int64_t)me]; q.y = queries[3 * (int64_t)me + 1]; q.z = queries[3 * (int64_t)me + 2]; }
    float bd = INFINITY;
    int bi = INT32_MAX;

    // the box of the wave's queries
    const float4 qmin = make_float4(wave_all(valid ? q.x : INFINITY, Min()), wave_all(valid ? q.y : INFINITY, Min()), wave_all(valid ? q.z : INFINITY, Min()), 0.0f);
    const float4 qmax = make_float4(wave_all(valid ? q.x : -INFINITY, Max()), wave_all(valid ? q.y : -INFINITY, Max()), wave_all(valid ? q.z : -INFINITY, Max()), 0.0f);

    // the seed: where the wave's middle query would stand in the reference's sorted keys (wave-uniform)
    const uint64_t key = query_keys[std::min<int64_t>(first_query + kQueries / 2, m - 1)];
    int64_t lo = 0, hi = n;
    for (int step = 0; step < 32 && lo < hi; ++step) {     // n <= 2^28: at most 29 halvings
        const int64_t mid = lo + (hi - lo) / 2;
        if (ref_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int64_t c = std::min<int64_t>(std::max<int64_t>(lo, 0), n - 1) / kChunk;

    // stage chunk ch, scan it, and return the wave's bound: the largest best distance of its queries
    const auto scan_chunk = [&](int64_t ch) {
        __syncthreads();                                   // the previous scan has left s_pts
        const int count = (int)std::min<int64_t>(kChunk, n - ch * kChunk);
        for (int i = lane; i < count; i += kQueries) s_pts[i] = sorted[ch * kChunk + i];
        __syncthreads();
        scan_staged1(bd, bi, q, s_pts, count);
        return wave_all(valid ? bd : 0.0f, Max());
    };

    float r2 = scan_chunk(c);

    // the chunks of group g other than c, nearest to c first
    const auto visit_group = [&](int64_t g) {
        const int64_t first = g * kGroup, ch = first + lane;
        const bool in = ch < chunks && ch != c;
        const float4 cmin = in ? chunk_boxes[2 * ch] : qmin, cmax = in ? chunk_boxes[2 * ch + 1] : qmax;
        const float cd2 = box_dist2(qmin, qmax, cmin, cmax);
        uint64_t mask = __ballot(in && !(cd2 > r2));
        const int pos = (int)std::min<int64_t>(std::max<int64_t>(c - first, 0), kGroup - 1);
        while (mask) {                                     // (every trip clears one of 64 bits)
            const int bit = nearest_bit(mask, pos);
            mask &= ~(1ull << bit);
            if (__shfl(cd2, bit) > r2) continue;           // (the bound has tightened since the ballot)
            // before anything is staged: can any query of the wave still gain from this chunk?
            const float4 bmin = make_float4(__shfl(cmin.x, bit), __shfl(cmin.y, bit), __shfl(cmin.z, bit), 0.0f);
            const float4 bmax = make_float4(__shfl(cmax.x, bit), __shfl(cmax.y, bit), __shfl(cmax.z, bit), 0.0f);
            if (!__any(valid && !(box_dist2(q, q, bmin, bmax) > bd))) continue;
            r2 = scan_chunk(first + bit);
        }
    };

    const int64_t g0 = c / kGroup;
    visit_group(g0);
    const int64_t blocks = (groups + 63) / 64, block0 = g0 / 64;
    for (int64_t t = 0; t < blocks; ++t)
        for (int side = 0; side < 2; ++side) {
            const int64_t blk = side ? block0 + t : block0 - t;
            if ((t == 0 && side) || blk < 0 || blk >= blocks) continue;
            const int64_t first = blk * 64, g = first + lane;
            const bool in = g < groups && g != g0;
            const float gd2 = in ? box_dist2(qmin, qmax, group_boxes[2 * g], group_boxes[2 * g + 1]) : 0.0f;
            uint64_t mask = __ballot(in && !(gd2 > r2));
            const int pos = (int)std::min<int64_t>(std::max<int64_t>(g0 - first, 0), 63);
            while (mask) {
                const int bit = nearest_bit(mask, pos);
                mask &= ~(1ull << bit);
                if (__shfl(gd2, bit) > r2) continue;
                visit_group(first + bit);
            }
        }

    if (valid) {
        if (dist2) dist2[me] = bd;
        if (index) index[me] = bi;
    }
}

// ---- the index and the two workspaces: pure functions of the counts ----
struct NnIndex {
    size_t grid, keys, sorted, chunk_boxes, group_boxes, total;
};

static NnIndex nn_index(int64_t n) {
    NnIndex w;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t here = at; at += align_up(bytes); return here; };
    w.grid = take(4 * sizeof(float));
    w.keys = take((size_t)n * sizeof(uint64_t));
    w.sorted = take((size_t)n * sizeof(float4));
    w.chunk_boxes = take((size_t)morton_chunks(n) * 2 * sizeof(float4));
    w.group_boxes = take((size_t)morton_groups(n) * 2 * sizeof(float4));
    w.total = at;
    return w;
}

struct NnScratch {      // of a build over n points (partial used) or of a query of n points (partial unused)
    size_t partial, keys_in, keys_out, order, sort_temp, sort_temp_bytes, total;
};

static NnScratch nn_scratch(int64_t n, bool build) {
    NnScratch w;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t here = at; at += align_up(bytes); return here; };
    w.partial = take(build ? (size_t)kBBoxBlocks * 6 * sizeof(float) : 0);
    w.keys_in = take((size_t)n * sizeof(uint64_t));
    w.keys_out = take(build ? 0 : (size_t)n * sizeof(uint64_t));      // a build sorts its keys straight into the index
    w.order = take((size_t)n * sizeof(uint32_t));
    w.sort_temp_bytes = morton_sort_temp_bytes(n);
    w.sort_temp = take(w.sort_temp_bytes);
    w.total = at;
    return w;
}

}  // namespace lsr

using namespace lsr;

static_assert(kQueries == LSR_WAVE && kGroup == LSR_WAVE, "one query per lane; one ballot per group of chunk boxes");

extern "C" {

size_t lsr_nn_index_bytes(int64_t n) {
    if (n <= 0) return 0;
    return nn_index(std::min<int64_t>(n, LSR_KNN_MAX_POINTS)).total;
}

size_t lsr_nn_build_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return nn_scratch(std::min<int64_t>(n, LSR_KNN_MAX_POINTS), true).total;
}

size_t lsr_nn_query_workspace_bytes(int64_t m) {
    if (m <= 0) return 0;
    return nn_scratch(std::min<int64_t>(m, LSR_KNN_MAX_POINTS), false).total;
}

int lsr_nn_build(int64_t n, const float *points, void *index_mem, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 1 || n > LSR_KNN_MAX_POINTS) return LSR_EINVAL;
    if (!points || !index_mem || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const NnIndex ix = nn_index(n);
    const NnScratch w = nn_scratch(n, true);
    char *mem = (char *)index_mem, *base = (char *)workspace;
    float *grid = (float *)(mem + ix.grid);
    uint32_t *order = (uint32_t *)(base + w.order);
    int rc = morton_sort_fits(n, w.sort_temp_bytes, s);
    if (rc != LSR_OK) return rc;
    morton_grid(n, points, (float *)(base + w.partial), grid, s);
    rc = morton_sort(n, points, grid, (uint64_t *)(base + w.keys_in), (uint64_t *)(mem + ix.keys), order, base + w.sort_temp,
                     w.sort_temp_bytes, s);
    if (rc != LSR_OK) return rc;
    morton_gather(n, points, order, (float4 *)(mem + ix.sorted), (float4 *)(mem + ix.chunk_boxes), (float4 *)(mem + ix.group_boxes), s);
    return launch_status();
}

int lsr_nn_query(int64_t n, const void *index_mem, int64_t m, const float *queries, float *dist2, int32_t *index,
                 void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 1 || n > LSR_KNN_MAX_POINTS || m < 0 || m > LSR_KNN_MAX_POINTS) return LSR_EINVAL;
    if (m == 0) return LSR_OK;
    if (!index_mem || !queries || (!dist2 && !index) || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const NnIndex ix = nn_index(n);
    const NnScratch w = nn_scratch(m, false);
    const char *mem = (const char *)index_mem;
    char *base = (char *)workspace;
    uint64_t *keys_out = (uint64_t *)(base + w.keys_out);
    uint32_t *order = (uint32_t *)(base + w.order);
    int rc = morton_sort_fits(m, w.sort_temp_bytes, s);
    if (rc != LSR_OK) return rc;
    rc = morton_sort(m, queries, (const float *)(mem + ix.grid), (uint64_t *)(base + w.keys_in), keys_out, order,
                     base + w.sort_temp, w.sort_temp_bytes, s);
    if (rc != LSR_OK) return rc;
    hipLaunchKernelGGL(k_nn_search, dim3((unsigned)((m + kQueries - 1) / kQueries)), dim3(kQueries), 0, s, n, morton_chunks(n),
                       morton_groups(n), (const uint64_t *)(mem + ix.keys), (const float4 *)(mem + ix.sorted),
                       (const float4 *)(mem + ix.chunk_boxes), (const float4 *)(mem + ix.group_boxes), m, queries, keys_out, order,
                       dist2, index);
    return launch_status();
}

}  // extern "C"
