// knn.hip — exact three-nearest-neighbour search over a point cloud (include/lsr_knn.h): what the point-cloud
// initialisation of a trainable 3DGS scene takes every Gaussian's first log-scale from.
//
// The pipeline, all on the caller's stream, nothing read back:
//   k_knn_bbox / k_knn_bbox_final   the cloud's bounding box (per-block partials, then one workgroup) and the cell scale;
//   k_knn_keys                      a 63-bit Morton code per point: 21 bits per axis of one isotropic grid over the
//                                   longest extent, so that a single far outlier still leaves the rest of the scene
//                                   fine cells rather than one;
//   rocprim::radix_sort_pairs       (code, index) pairs; stable, so equal codes keep their index order.  Its temporary
//                                   storage lies inside the caller's workspace;
//   k_knn_gather                    the points in sorted order as 16-byte records (x, y, z, original index), and the
//                                   axis-aligned box of every chunk of kChunk sorted points;
//   k_knn_group_boxes               a box per kGroup chunk boxes;
//   k_knn_search                    one wavefront per kQueries consecutive sorted points, one query per lane with its
//                                   best three in registers.
//
// The search.  A wave's queries are neighbours in space (a run of the Morton order), so the wave walks the cloud once
// for all of them.  It seeds every lane from the chunk its queries lie in, then visits the other chunks: its own group of
// kGroup chunks first, outward from its own position, then the other groups, outward in blocks of 64.  Two tests stand
// between a chunk and a scan, both exact and both decided for the whole wave (nothing diverges per lane):
//   box against box   the distance between the chunk's box (a group's box) and the box of the wave's queries exceeds,
//                     strictly, the largest third-best distance any lane holds.  Tested lane-parallel: lane l tests box l
//                     of the 64 at hand and one ballot gives the candidates; the bound is refreshed after every scan;
//   query against box for a candidate, each lane compares the distance from ITS query to the chunk's box (the box
//                     crosses from the lane that holds it) with ITS OWN third-best; the chunk is staged only if some
//                     lane can still gain.  This is what keeps a wave whose queries are a sparse halo around a dense
//                     core from staging the core's thousands of chunks.
// A chunk that passes is staged in LDS and scanned by every lane with broadcast reads (all lanes read the same 16-byte
// record).  One wavefront per workgroup: the bound is a wave reduction and the decisions are ballots, with no second
// level through LDS and no barrier between waves; 2 KiB of LDS per workgroup leaves residency to the wave slots.
//
// Why the skips are exact in float32: this unit is compiled with -ffp-contract=off, so a squared distance is the same
// three rounded differences, three rounded squares and two rounded sums wherever it is computed; a box gap is one
// rounded difference of two coordinates that bracket the pair's, and rounding is monotonic, so a box distance never
// exceeds the computed distance of any pair it covers.  With strict comparisons a chunk that holds an equally distant
// point is still visited, and the order (distance, then index) of the kept three does not depend on the visiting order.
//
// The worst case stays O(n^2): when every point falls into one cell (all points coincident, say), or when the boxes all
// overlap, every wave scans every chunk.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "lsr_morton.h"
#include "lsr_knn.h"

namespace lsr {

// (the constants, block_minmax3, spread_bits, box_dist2 and nearest_bit are in lsr_morton.h, shared with nn.hip)

__global__ __launch_bounds__(kKnnThreads) void k_knn_bbox(int64_t n, const float *__restrict__ points, float *__restrict__ partial) {
    __shared__ float s[6 * kKnnThreads / LSR_WAVE];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kKnnThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = points[3 * i + k];
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    block_minmax3<kKnnThreads>(lo, hi, s);
    if (threadIdx.x == 0) {
        float *out = partial + 6 * blockIdx.x;
        out[0] = lo[0]; out[1] = lo[1]; out[2] = lo[2]; out[3] = hi[0]; out[4] = hi[1]; out[5] = hi[2];
    }
}

// one workgroup: grid[0..2] the box's minimum, grid[3] cells per unit length (0 for a box of no or no finite extent)
__global__ __launch_bounds__(kKnnThreads) void k_knn_bbox_final(int blocks, const float *__restrict__ partial, float *__restrict__ grid) {
    __shared__ float s[6 * kKnnThreads / LSR_WAVE];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < blocks; i += kKnnThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], partial[6 * i + k]);
            hi[k] = fmaxf(hi[k], partial[6 * i + 3 + k]);
        }
    block_minmax3<kKnnThreads>(lo, hi, s);
    if (threadIdx.x == 0) {
        const float extent = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
        grid[0] = lo[0]; grid[1] = lo[1]; grid[2] = lo[2];
        grid[3] = extent > 0.0f && extent < INFINITY ? kCellMax / extent : 0.0f;      // (no division by a zero extent)
    }
}

__global__ __launch_bounds__(kKnnThreads) void k_knn_keys(int64_t n, const float *__restrict__ points, const float *__restrict__ grid,
                                                         uint64_t *__restrict__ keys) {
    const float inv = grid[3];
    for (int64_t i = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kKnnThreads) {
        uint64_t key = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // clamped whatever the coordinate is: fmaxf drops a NaN, fminf an infinity
            const float cell = fminf(fmaxf((points[3 * i + k] - grid[k]) * inv, 0.0f), kCellMax);
            key |= spread_bits((uint64_t)(uint32_t)cell) << k;
        }
        keys[i] = key;
    }
}

// a box is two float4: the minimum and the maximum (w unused)
__global__ __launch_bounds__(kChunk) void k_knn_gather(int64_t n, const float *__restrict__ points, const uint32_t *__restrict__ order,
                                                      float4 *__restrict__ sorted, float4 *__restrict__ chunk_boxes) {
    __shared__ float s[6 * kChunk / LSR_WAVE];
    const int64_t i = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const uint32_t j = order[i];
        if ((int64_t)j < n) {      // (always: the sort permutes 0 .. n-1)
            const float x = points[3 * (int64_t)j], y = points[3 * (int64_t)j + 1], z = points[3 * (int64_t)j + 2];
            sorted[i] = make_float4(x, y, z, __int_as_float((int)j));
            lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
        } else {
            sorted[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
        }
    }
    block_minmax3<kChunk>(lo, hi, s);
    if (threadIdx.x == 0) {
        chunk_boxes[2 * (int64_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        chunk_boxes[2 * (int64_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// one wave per group: lane l takes chunk box l of the group
__global__ __launch_bounds__(kGroup) void k_knn_group_boxes(int64_t chunks, const float4 *__restrict__ chunk_boxes,
                                                           float4 *__restrict__ group_boxes) {
    const int64_t ch = (int64_t)blockIdx.x * kGroup + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (ch < chunks) {
        const float4 a = chunk_boxes[2 * ch], b = chunk_boxes[2 * ch + 1];
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = wave_all(lo[k], Min()); hi[k] = wave_all(hi[k], Max()); }
    if (threadIdx.x == 0) {
        group_boxes[2 * (int64_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        group_boxes[2 * (int64_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// the best three of a query, ordered by (distance, index)
struct Best3 {
    float d0, d1, d2;
    int i0, i1, i2;
};

__device__ __forceinline__ void consider(Best3 &b, float d, int j) {
    if (d < b.d2 || (d == b.d2 && j < b.i2)) {
        if (d < b.d1 || (d == b.d1 && j < b.i1)) {
            b.d2 = b.d1; b.i2 = b.i1;
            if (d < b.d0 || (d == b.d0 && j < b.i0)) { b.d1 = b.d0; b.i1 = b.i0; b.d0 = d; b.i0 = j; }
            else { b.d1 = d; b.i1 = j; }
        } else {
            b.d2 = d; b.i2 = j;
        }
    }
}

// every lane against the `count` records staged in LDS: all lanes read the same record (a broadcast read)
template <bool kSkipSelf>
__device__ __forceinline__ void scan_staged(Best3 &b, const float4 &q, int me, const float4 *s_pts, int count) {
#pragma unroll 4
    for (int j = 0; j < count; ++j) {
        const float4 p = s_pts[j];
        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
        const float d = dx * dx + dy * dy + dz * dz;
        const int idx = __float_as_int(p.w);
        if (d <= b.d2 && (!kSkipSelf || idx != me)) consider(b, d, idx);
    }
}

// One wavefront per workgroup: kQueries == LSR_WAVE, so the workgroup's bound and its decisions are the wave's own — a
// wave reduction and a ballot, no second level through LDS.  (__syncthreads here orders the one wave's LDS traffic.)
__global__ __launch_bounds__(kQueries) void k_knn_search(int64_t n, int64_t chunks, int64_t groups, const float4 *__restrict__ sorted,
                                                        const float4 *__restrict__ chunk_boxes, const float4 *__restrict__ group_boxes,
                                                        float *__restrict__ mean_dist2, float *__restrict__ dist2,
                                                        int32_t *__restrict__ index) {
    __shared__ float4 s_pts[kChunk];
    const int lane = threadIdx.x;
    const int64_t first_query = (int64_t)blockIdx.x * kQueries;
    const int64_t c = first_query / kChunk;                // the chunk the wave's queries lie in
    const bool valid = first_query + lane < n;
    const float4 q = valid ? sorted[first_query + lane] : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
    const int me = __float_as_int(q.w);
    Best3 b = {INFINITY, INFINITY, INFINITY, INT32_MAX, INT32_MAX, INT32_MAX};

    // the box of the wave's queries
    const float4 qmin = make_float4(wave_all(valid ? q.x : INFINITY, Min()), wave_all(valid ? q.y : INFINITY, Min()), wave_all(valid ? q.z : INFINITY, Min()), 0.0f);
    const float4 qmax = make_float4(wave_all(valid ? q.x : -INFINITY, Max()), wave_all(valid ? q.y : -INFINITY, Max()), wave_all(valid ? q.z : -INFINITY, Max()), 0.0f);

    // stage chunk ch, scan it, and return the wave's bound: the largest third-best distance of its queries
    const auto scan_chunk = [&](int64_t ch, bool own) {
        __syncthreads();                                   // the previous scan has left s_pts
        const int count = (int)std::min<int64_t>(kChunk, n - ch * kChunk);
        for (int i = lane; i < count; i += kQueries) s_pts[i] = sorted[ch * kChunk + i];
        __syncthreads();
        if (own) scan_staged<true>(b, q, me, s_pts, count);
        else scan_staged<false>(b, q, me, s_pts, count);
        return wave_all(valid ? b.d2 : 0.0f, Max());
    };

    float r2 = scan_chunk(c, true);

    // the chunks of group g other than c, nearest to c first
    const auto visit_group = [&](int64_t g) {
        const int64_t first = g * kGroup, ch = first + lane;
        const bool in = ch < chunks && ch != c;
        const float4 cmin = in ? chunk_boxes[2 * ch] : qmin, cmax = in ? chunk_boxes[2 * ch + 1] : qmax;
        const float cd2 = box_dist2(qmin, qmax, cmin, cmax);
        uint64_t mask = __ballot(in && !(cd2 > r2));
        const int pos = (int)std::min<int64_t>(std::max<int64_t>(c - first, 0), kGroup - 1);
        while (mask) {
            const int bit = nearest_bit(mask, pos);
            mask &= ~(1ull << bit);
            if (__shfl(cd2, bit) > r2) continue;           // (the bound has tightened since the ballot)
            // before anything is staged: can any query of the wave still gain from this chunk?  Its box crosses from
            // the lane that holds it; each lane tests its own query against its own third-best
            const float4 bmin = make_float4(__shfl(cmin.x, bit), __shfl(cmin.y, bit), __shfl(cmin.z, bit), 0.0f);
            const float4 bmax = make_float4(__shfl(cmax.x, bit), __shfl(cmax.y, bit), __shfl(cmax.z, bit), 0.0f);
            if (!__any(valid && !(box_dist2(q, q, bmin, bmax) > b.d2))) continue;
            r2 = scan_chunk(first + bit, false);
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

    if (valid && (int64_t)(uint32_t)me < n) {
        if (dist2) { dist2[3 * (int64_t)me] = b.d0; dist2[3 * (int64_t)me + 1] = b.d1; dist2[3 * (int64_t)me + 2] = b.d2; }
        if (index) { index[3 * (int64_t)me] = b.i0; index[3 * (int64_t)me + 1] = b.i1; index[3 * (int64_t)me + 2] = b.i2; }
        if (mean_dist2) mean_dist2[me] = ((b.d0 + b.d1) + b.d2) / 3.0f;
    }
}

// ---- the workspace: a pure function of n ----
struct KnnWorkspace {
    size_t partial, grid, keys_in, keys_out, order, sorted, chunk_boxes, group_boxes, sort_temp, sort_temp_bytes, total;
};

static KnnWorkspace knn_workspace(int64_t n) {
    KnnWorkspace w;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t here = at; at += align_up(bytes); return here; };
    w.partial = take((size_t)kBBoxBlocks * 6 * sizeof(float));
    w.grid = take(4 * sizeof(float));
    w.keys_in = take((size_t)n * sizeof(uint64_t));
    w.keys_out = take((size_t)n * sizeof(uint64_t));
    w.order = take((size_t)n * sizeof(uint32_t));
    w.sorted = take((size_t)n * sizeof(float4));
    w.chunk_boxes = take((size_t)morton_chunks(n) * 2 * sizeof(float4));
    w.group_boxes = take((size_t)morton_groups(n) * 2 * sizeof(float4));
    w.sort_temp_bytes = morton_sort_temp_bytes(n);      // a reservation: lsr_knn3 checks the sort's own figure against it
    w.sort_temp = take(w.sort_temp_bytes);
    w.total = at;
    return w;
}

// ---- the build of the index (lsr_morton.h): what lsr_knn3 and nn.hip share ----

int morton_sort_fits(int64_t n, size_t reserved, hipStream_t stream) {
    const rocprim::counting_iterator<uint32_t> iota(0u);
    size_t temp_bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, temp_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, iota,
                                                   (uint32_t *)nullptr, (unsigned int)n, 0u, 3u * kCellBits, stream);
    if (e != hipSuccess) { note_hip_error((int)e); return LSR_ELAUNCH; }
    return temp_bytes > reserved ? LSR_EUNSUPPORTED : LSR_OK;
}

static unsigned morton_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + kKnnThreads - 1) / kKnnThreads, kBBoxBlocks); }

void morton_grid(int64_t n, const float *points, float *partial, float *grid, hipStream_t stream) {
    const unsigned blocks = morton_blocks(n);
    hipLaunchKernelGGL(k_knn_bbox, dim3(blocks), dim3(kKnnThreads), 0, stream, n, points, partial);
    hipLaunchKernelGGL(k_knn_bbox_final, dim3(1), dim3(kKnnThreads), 0, stream, (int)blocks, partial, grid);
}

int morton_sort(int64_t n, const float *points, const float *grid, uint64_t *keys_in, uint64_t *keys_out, uint32_t *order,
                void *sort_temp, size_t sort_temp_bytes, hipStream_t stream) {
    const rocprim::counting_iterator<uint32_t> iota(0u);
    hipLaunchKernelGGL(k_knn_keys, dim3(morton_blocks(n)), dim3(kKnnThreads), 0, stream, n, points, grid, keys_in);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(sort_temp, sort_temp_bytes, keys_in, keys_out, iota, order, (unsigned int)n, 0u,
                                      3u * kCellBits, stream);
    if (e != hipSuccess) { note_hip_error((int)e); return LSR_ELAUNCH; }
    return LSR_OK;
}

void morton_gather(int64_t n, const float *points, const uint32_t *order, float4 *sorted, float4 *chunk_boxes,
                   float4 *group_boxes, hipStream_t stream) {
    const int64_t chunks = morton_chunks(n), groups = morton_groups(n);
    hipLaunchKernelGGL(k_knn_gather, dim3((unsigned)chunks), dim3(kChunk), 0, stream, n, points, order, sorted, chunk_boxes);
    hipLaunchKernelGGL(k_knn_group_boxes, dim3((unsigned)groups), dim3(kGroup), 0, stream, chunks, chunk_boxes, group_boxes);
}

}  // namespace lsr

using namespace lsr;

static_assert(kChunk % kQueries == 0 && kQueries == LSR_WAVE && kGroup == LSR_WAVE,
              "a wave's queries lie in one chunk; one query per lane; one ballot per group of chunk boxes");
static_assert(LSR_KNN_MAX_POINTS <= (1 << 30), "32-bit indices and sort sizes");

extern "C" {

size_t lsr_knn3_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return knn_workspace(std::min<int64_t>(n, LSR_KNN_MAX_POINTS)).total;
}

int lsr_knn3(int64_t n, const float *points, float *mean_dist2, float *dist2, int32_t *index, void *workspace,
             lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || (n >= 1 && n <= 3) || n > LSR_KNN_MAX_POINTS) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!points || (!mean_dist2 && !dist2 && !index) || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const KnnWorkspace w = knn_workspace(n);
    char *base = (char *)workspace;
    float *partial = (float *)(base + w.partial), *grid = (float *)(base + w.grid);
    uint64_t *keys_in = (uint64_t *)(base + w.keys_in), *keys_out = (uint64_t *)(base + w.keys_out);
    uint32_t *order = (uint32_t *)(base + w.order);
    float4 *sorted = (float4 *)(base + w.sorted), *chunk_boxes = (float4 *)(base + w.chunk_boxes);
    float4 *group_boxes = (float4 *)(base + w.group_boxes);
    int rc = morton_sort_fits(n, w.sort_temp_bytes, s);
    if (rc != LSR_OK) return rc;
    morton_grid(n, points, partial, grid, s);
    rc = morton_sort(n, points, grid, keys_in, keys_out, order, base + w.sort_temp, w.sort_temp_bytes, s);
    if (rc != LSR_OK) return rc;
    morton_gather(n, points, order, sorted, chunk_boxes, group_boxes, s);
    hipLaunchKernelGGL(k_knn_search, dim3((unsigned)((n + kQueries - 1) / kQueries)), dim3(kQueries), 0, s, n, morton_chunks(n),
                       morton_groups(n), sorted, chunk_boxes, group_boxes, mean_dist2, dist2, index);
    return launch_status();
}

}  // extern "C"
