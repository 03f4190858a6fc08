// lsr_morton.h — what the two nearest-neighbour units share (knn.hip: a cloud against itself, three neighbours; nn.hip: a
// persistent index over a reference cloud, one neighbour of foreign queries): the constants of the Morton-sorted index,
// the device helpers of its walk, and the host entry points of its build.
//
// The index of a cloud of n points:
//   grid         4 floats: the bounding box's minimum and the cells per unit length of one isotropic 21-bit grid;
//   keys         the 63-bit Morton codes in sorted order;
//   sorted       the points in sorted order as 16-byte records (x, y, z, original index);
//   chunk_boxes  the axis-aligned box (two float4) of every chunk of kChunk sorted points;
//   group_boxes  a box per kGroup chunk boxes.
// The kernels that build it (bounding box, keys, gather, group boxes) are defined once, in knn.hip; the morton_* functions
// below launch them and are what another unit calls.  Everything here is compiled with -ffp-contract=off in both units:
// a box distance and a squared distance round the same way wherever they are computed (the exactness argument of knn.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#include "lsr_wave.h"

namespace lsr {

constexpr int kChunk = 128;            // sorted points per chunk: one box of the first level, one LDS stage
constexpr int kQueries = 64;           // queries per workgroup of the search: one wavefront, one query per lane
constexpr int kGroup = 64;             // chunks per second-level box = lanes of one ballot
constexpr int kKnnThreads = 256;       // lanes per workgroup of the box and key kernels
constexpr int kBBoxBlocks = 1024;
constexpr int kCellBits = 21;
constexpr float kCellMax = (float)((1 << kCellBits) - 1);

// min / max of three coordinates over a workgroup of kThreads; the result in every thread (s: 6 floats per wave)
template <int kThreads>
__device__ __forceinline__ void block_minmax3(float lo[3], float hi[3], float *s) {
    const int lane = threadIdx.x & (LSR_WAVE - 1), wave = threadIdx.x / LSR_WAVE;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = wave_all(lo[k], Min());
        hi[k] = wave_all(hi[k], Max());
        if (lane == 0) { s[6 * wave + k] = lo[k]; s[6 * wave + 3 + k] = hi[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int w = 0; w < kThreads / LSR_WAVE; ++w) {
            lo[k] = fminf(lo[k], s[6 * w + k]);
            hi[k] = fmaxf(hi[k], s[6 * w + 3 + k]);
        }
}

__device__ __forceinline__ uint64_t spread_bits(uint64_t x) {      // bit i of 21 to bit 3 i
    x = (x | x << 32) & 0x001f00000000ffffull;
    x = (x | x << 16) & 0x001f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// squared distance between two boxes (0 where they overlap); a point is the box with amin == amax
__device__ __forceinline__ float box_dist2(const float4 &amin, const float4 &amax, const float4 &bmin, const float4 &bmax) {
    const float gx = fmaxf(0.0f, fmaxf(bmin.x - amax.x, amin.x - bmax.x));
    const float gy = fmaxf(0.0f, fmaxf(bmin.y - amax.y, amin.y - bmax.y));
    const float gz = fmaxf(0.0f, fmaxf(bmin.z - amax.z, amin.z - bmax.z));
    return gx * gx + gy * gy + gz * gz;
}

// the set bit of `mask` nearest to position `pos` (0..63); mask != 0
__device__ __forceinline__ int nearest_bit(uint64_t mask, int pos) {
    const uint64_t up = mask >> pos, down = pos ? mask & ((1ull << pos) - 1ull) : 0ull;
    const int u = up ? pos + __builtin_ctzll(up) : 1 << 20, d = down ? 63 - __builtin_clzll(down) : -(1 << 20);
    return u - pos <= pos - d ? u : d;
}

inline int64_t morton_chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }
inline int64_t morton_groups(int64_t n) { return (morton_chunks(n) + kGroup - 1) / kGroup; }

// The sort's temporary storage for n (key, index) pairs: its own copies of the keys and the values, histograms and
// per-block states.  What it asks for depends on the device's tuning, which cannot be asked without a device: this is a
// reservation, and morton_sort_fits checks the sort's own figure against it before anything is launched.
inline size_t morton_sort_temp_bytes(int64_t n) {
    return align_up((size_t)n * sizeof(uint64_t)) + align_up((size_t)n * sizeof(uint32_t)) + (size_t)n * 16 + (1u << 20);
}

// ---- host entry points, defined in knn.hip; all asynchronous on `stream`, nothing read back ----

// LSR_OK when the device's sort of n pairs fits `reserved` bytes of temporary storage, LSR_EUNSUPPORTED when it does not,
// LSR_ELAUNCH when the sort cannot say.  Host only: nothing is launched.
int morton_sort_fits(int64_t n, size_t reserved, hipStream_t stream);
// partial: kBBoxBlocks * 6 floats of scratch; grid: 4 floats out
void morton_grid(int64_t n, const float *points, float *partial, float *grid, hipStream_t stream);
// keys of `points` in the cells of `grid` (clamped at its faces) into keys_in, then the stable sort: keys_out the sorted
// keys, order the sorted original indices.  LSR_OK or LSR_ELAUNCH.
int morton_sort(int64_t n, const float *points, const float *grid, uint64_t *keys_in, uint64_t *keys_out, uint32_t *order,
                void *sort_temp, size_t sort_temp_bytes, hipStream_t stream);
// the sorted records and the two levels of boxes
void morton_gather(int64_t n, const float *points, const uint32_t *order, float4 *sorted, float4 *chunk_boxes,
                   float4 *group_boxes, hipStream_t stream);

}  // namespace lsr
