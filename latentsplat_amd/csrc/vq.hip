// vq.hip — the two halves of a weighted Lloyd iteration (include/lsr_vq.h): what the codebook compression of a 3DGS scene
// spends its time in.  Nothing is read back, nothing is allocated, no float atomics.
//
// lsr_vq_assign: the nearest of k codes for n rows of d floats, as the largest score  x . c_j - |c_j|^2 / 2.
//   k_vq_pack     the codebook, every row zero-padded to vq_stride(d) floats and the rows to a multiple of kCodes, and the
//                 bias -|c_j|^2 / 2 of every code (-inf for the padding codes: they never win), into the workspace;
//   k_vq_assign   a workgroup of four waves owns kRows = 128 rows, staged once in LDS (dword loads: a row of odd d is not
//                 16-byte aligned).  The packed codebook streams through two LDS buffers of kCodes = 64 codes: the next
//                 tile's global loads are issued before the current tile's products and land in the other buffer after
//                 them, one barrier per tile.  Each wave multiplies its own 32 rows against the whole tile on
//                 v_mfma_f32_32x32x2_f32 with the CODES as the A operand and the ROWS as the B operand, so that a lane's
//                 16 accumulator registers are 16 codes of ONE row (column = lane & 31): the running (best score, best
//                 index) is a chain of compares down the lane's own registers, in ascending code order, and the only
//                 exchange is between lanes l and l + 32 at the very end.  The accumulator is seeded with the bias (the C
//                 operand), so the score costs no extra operation.  The n x k scores never leave the registers.
//   k_vq_dist2    (optional) the squared distance of every row to its code, from the differences.
//   The K order: one trip of the inner loop covers kStep = 4 floats of a row with two MFMAs; lane half h supplies floats
//   4 s + 2 h and 4 s + 2 h + 1 of both operands (one ds_read_b64 each).  The sum over d is therefore a permuted, still
//   fixed, chain of fmaf.  LDS rows are vq_stride(d) = 4 ceil(d / 4) + 2 floats apart: half the stride is odd, so the 32
//   lanes of a half hit 32 distinct pairs of banks with their 8-byte reads.
//
// lsr_vq_update: the weighted mean of every code's rows, the same bits on every call.
//   k_vq_keys                  key = idx where 0 <= idx < k, else k (the rows to skip sort behind everything);
//   rocprim::radix_sort_pairs  (key, row) over the bits of k: stable, so a code's rows stay in row order;
//   k_vq_bounds                start[j] = first sorted position of code j (a binary search per code), j = 0 .. k;
//   k_vq_partial               a workgroup per kBlock = 256 sorted positions, a thread per coordinate, walks the block in
//                              order with float64 sums.  A code whose rows all lie inside the block is finished here; the
//                              (at most two) runs that touch the block's ends leave their sums in the block's two slots;
//   k_vq_finish                a workgroup per code: empty codes copy prev_codebook; a code that spans blocks adds its
//                              blocks' slots in eight contiguous chunks of blocks, each in block order, then the eight in
//                              order (k = 1 with millions of rows: thousands of slots, not a serial loop over them).
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "lsr_internal.h"
#include "lsr_vq.h"

namespace lsr {

constexpr int kRows = LSR_VQ_ROWS;       // rows per workgroup of k_vq_assign: 32 per wave
constexpr int kCodes = LSR_VQ_CODES;     // codes per LDS tile: two 32-code accumulator blocks per wave
constexpr int kStep = LSR_VQ_KSTEP;      // floats of a row per trip of the inner loop (two MFMAs of K = 2)
constexpr int kVqThreads = 256;
constexpr int kBlock = 256;              // sorted positions per workgroup of k_vq_partial
constexpr int kFinishChunks = 8;         // k_vq_finish adds a code's block sums in this many chunks
constexpr int kMaxTileLoads = (kCodes * (LSR_VQ_MAX_DIM + 2) / 4 + kVqThreads - 1) / kVqThreads;   // float4 per thread per tile

typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int vq_stride(int d) { return (d + kStep - 1) / kStep * kStep + 2; }
inline int64_t vq_padded_codes(int k) { return ((int64_t)k + kCodes - 1) / kCodes * kCodes; }

// one thread per code of the padded codebook
__global__ __launch_bounds__(kVqThreads) void k_vq_pack(int k, int k_pad, int d, const float *__restrict__ codebook,
                                                       float *__restrict__ packed, float *__restrict__ bias) {
    const int j = blockIdx.x * kVqThreads + threadIdx.x;
    if (j >= k_pad) return;
    const int S = vq_stride(d);
    float *row = packed + (int64_t)j * S;
    float sq = 0.0f;
    for (int c = 0; c < S; ++c) {
        const float v = j < k && c < d ? codebook[(int64_t)j * d + c] : 0.0f;
        row[c] = v;
        sq = fmaf(v, v, sq);
    }
    bias[j] = j < k ? -0.5f * sq : -INFINITY;
}

__global__ __launch_bounds__(kVqThreads) void k_vq_assign(int64_t n, int k_pad, int d, const float *__restrict__ x,
                                                         const float *__restrict__ packed, const float *__restrict__ bias,
                                                         int32_t *__restrict__ idx_out) {
    extern __shared__ float4 vq_lds4[];
    const int S = vq_stride(d), steps = (d + kStep - 1) / kStep;
    float *s_x = (float *)vq_lds4;                           // [kRows][S]
    float *s_c = s_x + kRows * S;                            // [2][kCodes][S]
    float *s_b = s_c + 2 * kCodes * S;                       // [2][kCodes]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    const int count = (int)std::min<int64_t>(kRows, n - r0);
    const int tile_f4 = kCodes * S / 4, tiles = k_pad / kCodes;

    // the rows: zeros first (the padding columns, the rows past n), then the values, one dword each
    for (int q = tid; q < kRows * S / 4; q += kVqThreads) ((float4 *)s_x)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    {   // tile 0 straight into buffer 0
        const float4 *src = (const float4 *)packed;
        for (int q = tid; q < tile_f4; q += kVqThreads) ((float4 *)s_c)[q] = src[q];
        if (tid < kCodes) s_b[tid] = bias[tid];
    }
    __syncthreads();
    {
        const float *src = x + r0 * d;
        const int total = count * d;
        for (int e = tid; e < total; e += kVqThreads) {
            const int row = e / d;
            s_x[row * S + (e - row * d)] = src[e];
        }
    }
    __syncthreads();

    const float *xr = s_x + (wave * 32 + col) * S + 2 * h;
    float best = -INFINITY;
    int best_j = 0;
    for (int t = 0; t < tiles; ++t) {
        const int buf = t & 1;
        // the next tile: loads now, LDS writes behind the products
        float4 pre[kMaxTileLoads];
#pragma unroll
        for (int u = 0; u < kMaxTileLoads; ++u) pre[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float pre_b = 0.0f;
        const bool more = t + 1 < tiles;
        if (more) {
            const float4 *src = (const float4 *)(packed + (int64_t)(t + 1) * kCodes * S);
#pragma unroll
            for (int u = 0; u < kMaxTileLoads; ++u) {
                const int q = tid + u * kVqThreads;
                if (q < tile_f4) pre[u] = src[q];
            }
            if (tid < kCodes) pre_b = bias[(t + 1) * kCodes + tid];
        }

        const float *c0 = s_c + buf * kCodes * S + col * S + 2 * h, *c1 = c0 + 32 * S;
        const float *sb = s_b + buf * kCodes + 4 * h;
        f32x16 acc0, acc1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {       // accumulator register 4 g + e is code 8 g + 4 h + e of its block
            const float4 b0 = *(const float4 *)(sb + 8 * g), b1 = *(const float4 *)(sb + 32 + 8 * g);
            acc0[4 * g] = b0.x; acc0[4 * g + 1] = b0.y; acc0[4 * g + 2] = b0.z; acc0[4 * g + 3] = b0.w;
            acc1[4 * g] = b1.x; acc1[4 * g + 1] = b1.y; acc1[4 * g + 2] = b1.z; acc1[4 * g + 3] = b1.w;
        }
        // the operands of trip s + 1 are read while the products of trip s run (the last trip reads its own again)
        float2 xv = *(const float2 *)xr, a0 = *(const float2 *)c0, a1 = *(const float2 *)c1;
        for (int s = 0; s < steps; ++s) {
            const int nx = kStep * std::min(s + 1, steps - 1);
            const float2 xn = *(const float2 *)(xr + nx), a0n = *(const float2 *)(c0 + nx), a1n = *(const float2 *)(c1 + nx);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, xv.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, xv.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, xv.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, xv.y, acc1, 0, 0, 0);
            xv = xn; a0 = a0n; a1 = a1n;
        }
        // ascending code order inside the lane and strict comparisons: the lowest index among equal scores; a NaN never wins
        const int base = t * kCodes + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = base + (r & 3) + 8 * (r >> 2);
            if (acc0[r] > best) { best = acc0[r]; best_j = j; }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = base + 32 + (r & 3) + 8 * (r >> 2);
            if (acc1[r] > best) { best = acc1[r]; best_j = j; }
        }

        if (more) {
            float4 *dst = (float4 *)(s_c + (buf ^ 1) * kCodes * S);
#pragma unroll
            for (int u = 0; u < kMaxTileLoads; ++u) {
                const int q = tid + u * kVqThreads;
                if (q < tile_f4) dst[q] = pre[u];
            }
            if (tid < kCodes) s_b[(buf ^ 1) * kCodes + tid] = pre_b;
        }
        __syncthreads();      // every wave has left buffer `buf`, and the other buffer is whole
    }
    // lanes l and l + 32 hold the two halves of a row's codes
    const float other = __shfl_xor(best, 32);
    const int other_j = __shfl_xor(best_j, 32);
    if (other > best || (other == best && other_j < best_j)) best_j = other_j;
    const int row = wave * 32 + col;
    if (h == 0 && row < count) idx_out[r0 + row] = best_j;
}

__global__ __launch_bounds__(kVqThreads) void k_vq_dist2(int64_t n, int k, int d, const float *__restrict__ x,
                                                        const float *__restrict__ codebook, const int32_t *__restrict__ idx,
                                                        float *__restrict__ dist2) {
    const int64_t i = (int64_t)blockIdx.x * kVqThreads + threadIdx.x;
    if (i >= n) return;
    const int j = std::min(std::max(idx[i], 0), k - 1);
    const float *a = x + i * d, *c = codebook + (int64_t)j * d;
    float acc = 0.0f;
    for (int e = 0; e < d; ++e) {
        const float t = a[e] - c[e];
        acc = fmaf(t, t, acc);
    }
    dist2[i] = acc;
}

// ---- update ----

__global__ __launch_bounds__(kVqThreads) void k_vq_keys(int64_t n, int k, const int32_t *__restrict__ idx, uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kVqThreads + threadIdx.x;
    if (i < n) keys[i] = (uint32_t)idx[i] < (uint32_t)k ? (uint32_t)idx[i] : (uint32_t)k;
}

// start[j], j = 0 .. k: the first sorted position whose key is >= j (start[k] = the number of rows that count)
__global__ __launch_bounds__(kVqThreads) void k_vq_bounds(int64_t n, int k, const uint32_t *__restrict__ sorted_keys, int32_t *__restrict__ start) {
    const int j = blockIdx.x * kVqThreads + threadIdx.x;
    if (j > k) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted_keys[mid] < (uint32_t)j) lo = mid + 1; else hi = mid;
    }
    start[j] = (int32_t)lo;
}

// partial: [blocks][2 slots][d + 1] float64 (the d sums, then the mass)
__global__ void k_vq_partial(int k, int d, const float *__restrict__ x, const float *__restrict__ weights,
                             const uint32_t *__restrict__ sorted_keys, const uint32_t *__restrict__ order,
                             const int32_t *__restrict__ start, const float *__restrict__ prev, float *__restrict__ out,
                             float *__restrict__ mass_out, double *__restrict__ partial) {
    __shared__ uint32_t s_key[kBlock], s_row[kBlock];
    __shared__ float s_w[kBlock];
    const int64_t p0 = (int64_t)blockIdx.x * kBlock;
    const int64_t valid = start[k];
    if (p0 >= valid) return;
    const int cnt = (int)std::min<int64_t>(kBlock, valid - p0);
    for (int p = threadIdx.x; p < cnt; p += blockDim.x) {
        const uint32_t row = order[p0 + p];
        s_key[p] = sorted_keys[p0 + p];
        s_row[p] = row;
        s_w[p] = weights ? weights[row] : 1.0f;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= d) return;
    double *slots = partial + (int64_t)blockIdx.x * 2 * (d + 1);
    const auto flush = [&](uint32_t code, double acc, double m, bool first) {
        if (code >= (uint32_t)k) return;     // (never: the block ends at start[k])
        const int64_t s = start[code], e = start[code + 1];
        if (s >= p0 && e <= p0 + kBlock) {   // the whole code lies in this block
            out[(int64_t)code * d + c] = m > 0.0 ? (float)(acc / m) : prev[(int64_t)code * d + c];
            if (c == 0) mass_out[code] = m > 0.0 ? (float)m : 0.0f;
        } else {                             // it touches an end of the block: the first run, or else the last
            double *slot = slots + (first ? 0 : d + 1);
            slot[c] = acc;
            if (c == 0) slot[d] = m;
        }
    };
    uint32_t cur = s_key[0];
    double acc = 0.0, m = 0.0;
    bool first = true;
    for (int p = 0; p < cnt; p += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p + u < cnt ? x[(int64_t)s_row[p + u] * d + c] : 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (p + u < cnt) {
                const uint32_t code = s_key[p + u];
                if (code != cur) {
                    flush(cur, acc, m, first);
                    cur = code; acc = 0.0; m = 0.0; first = false;
                }
                const double w = (double)s_w[p + u];
                acc += w * (double)v[u];
                m += w;
            }
    }
    flush(cur, acc, m, first);
}

__global__ __launch_bounds__(kVqThreads) void k_vq_finish(int k, int d, const int32_t *__restrict__ start, const double *__restrict__ partial,
                                                         const float *__restrict__ prev, float *__restrict__ out, float *__restrict__ mass_out) {
    __shared__ double s_sum[kFinishChunks][32];
    __shared__ double s_tot[LSR_VQ_MAX_DIM + 1];
    const int j = blockIdx.x, t = threadIdx.x;
    const int64_t s = start[j], e = start[j + 1];
    if (s == e) {                            // nothing chose this code
        if (t < d) out[(int64_t)j * d + t] = prev[(int64_t)j * d + t];
        if (t == 0) mass_out[j] = 0.0f;
        return;
    }
    const int64_t b0 = s / kBlock, b1 = (e - 1) / kBlock;
    if (b0 == b1) return;                    // k_vq_partial finished it
    const int64_t P = b1 - b0 + 1, chunk = (P + kFinishChunks - 1) / kFinishChunks;
    const bool first_is_tail = s != b0 * kBlock;     // in its first block the code is the last run, unless it starts the block
    const int q = t >> 5, dd = t & 31, row = d + 1;
    for (int c0 = 0; c0 <= d; c0 += 32) {
        const int c = c0 + dd;
        double sum = 0.0;
        if (c <= d) {
            const int64_t pe = std::min<int64_t>(P, (q + 1) * chunk);
            for (int64_t p = q * chunk; p < pe; ++p)
                sum += partial[((b0 + p) * 2 + (p == 0 && first_is_tail ? 1 : 0)) * row + c];
        }
        s_sum[q][dd] = sum;
        __syncthreads();
        if (q == 0 && c <= d) {
            double total = s_sum[0][dd];
#pragma unroll
            for (int g = 1; g < kFinishChunks; ++g) total += s_sum[g][dd];
            s_tot[c] = total;
        }
        __syncthreads();
    }
    const double m = s_tot[d];
    if (t < d) out[(int64_t)j * d + t] = m > 0.0 ? (float)(s_tot[t] / m) : prev[(int64_t)j * d + t];
    if (t == 0) mass_out[j] = m > 0.0 ? (float)m : 0.0f;
}

// ---- the workspace: a pure function of (n, k, d) ----
struct VqWorkspace {
    size_t packed, bias, keys_in, keys_out, order, start, partial, sort_temp, sort_temp_bytes, total;
};

static int64_t vq_blocks(int64_t n) { return (n + kBlock - 1) / kBlock; }

static VqWorkspace vq_workspace(int64_t n, int k, int d) {
    VqWorkspace w;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t here = at; at += align_up(bytes); return here; };
    w.packed = take((size_t)vq_padded_codes(k) * vq_stride(d) * sizeof(float));
    w.bias = take((size_t)vq_padded_codes(k) * sizeof(float));
    w.keys_in = take((size_t)n * sizeof(uint32_t));
    w.keys_out = take((size_t)n * sizeof(uint32_t));
    w.order = take((size_t)n * sizeof(uint32_t));
    w.start = take(((size_t)k + 1) * sizeof(int32_t));
    w.partial = take((size_t)vq_blocks(n) * 2 * (d + 1) * sizeof(double));
    // the sort's temporary storage: a reservation (see knn.hip); lsr_vq_update checks the sort's own figure against it
    w.sort_temp_bytes = 2 * align_up((size_t)n * sizeof(uint32_t)) + (size_t)n * 16 + (1u << 20);
    w.sort_temp = take(w.sort_temp_bytes);
    w.total = at;
    return w;
}

static bool vq_dims_ok(int64_t n, int64_t k, int64_t d) {
    return n >= 0 && n <= LSR_VQ_MAX_ROWS && k >= 1 && k <= LSR_VQ_MAX_CODES && d >= 1 && d <= LSR_VQ_MAX_DIM;
}

static size_t vq_assign_lds(int d) { return ((size_t)(kRows + 2 * kCodes) * vq_stride(d) + 2 * kCodes) * sizeof(float); }

}  // namespace lsr

using namespace lsr;

static_assert(kRows == 32 * (kVqThreads / LSR_WAVE), "32 rows (the columns of one 32x32 accumulator) per wave");
static_assert(kCodes == 64 && kStep == 4, "two 32-code accumulator blocks per tile; two K = 2 products per trip");
static_assert(kMaxTileLoads * kVqThreads * 4 >= kCodes * (LSR_VQ_MAX_DIM + 2), "a tile fits the prefetch registers");
static_assert(LSR_VQ_MAX_DIM <= 128 && kVqThreads >= LSR_VQ_MAX_DIM + 1, "a thread per coordinate");
static_assert(LSR_VQ_MAX_ROWS <= (1 << 30) && (int64_t)LSR_VQ_ROWS * LSR_VQ_MAX_DIM < (1 << 30), "32-bit sizes");

extern "C" {

size_t lsr_vq_workspace_bytes(int64_t n, int32_t k, int32_t d) {
    if (!vq_dims_ok(n, k, d) || n == 0) return 0;
    return vq_workspace(n, k, d).total;
}

int lsr_vq_assign(const lsr_vq_dims *dims, const float *x, const float *codebook, int32_t *idx_out, float *dist2_out,
                  void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims) return LSR_ENULL;
    if (!vq_dims_ok(dims->n, dims->k, dims->d) || dims->reserved0 || dims->reserved1) return LSR_EINVAL;
    const int64_t n = dims->n;
    const int k = dims->k, d = dims->d;
    if (n == 0) return LSR_OK;
    if (!x || !codebook || !idx_out || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const VqWorkspace w = vq_workspace(n, k, d);
    float *packed = (float *)((char *)workspace + w.packed), *bias = (float *)((char *)workspace + w.bias);
    const int k_pad = (int)vq_padded_codes(k);
    const size_t lds = vq_assign_lds(d);
    // function attributes are per device: set on every launch that needs it (a process may drive several GPUs)
    if (lds > 65536) {
        const hipError_t a = hipFuncSetAttribute((const void *)k_vq_assign, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
        if (a != hipSuccess) { note_hip_error((int)a); return LSR_ELAUNCH; }
    }
    hipLaunchKernelGGL(k_vq_pack, dim3((unsigned)((k_pad + kVqThreads - 1) / kVqThreads)), dim3(kVqThreads), 0, s, k, k_pad, d, codebook, packed, bias);
    hipLaunchKernelGGL(k_vq_assign, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kVqThreads), lds, s, n, k_pad, d, x, packed, bias, idx_out);
    if (dist2_out)
        hipLaunchKernelGGL(k_vq_dist2, dim3((unsigned)((n + kVqThreads - 1) / kVqThreads)), dim3(kVqThreads), 0, s, n, k, d, x, codebook, idx_out, dist2_out);
    return launch_status();
}

int lsr_vq_update(const lsr_vq_dims *dims, const float *x, const int32_t *idx, const float *weights,
                  const float *prev_codebook, float *codebook_out, float *mass_out, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims) return LSR_ENULL;
    if (!vq_dims_ok(dims->n, dims->k, dims->d) || dims->reserved0 || dims->reserved1) return LSR_EINVAL;
    const int64_t n = dims->n;
    const int k = dims->k, d = dims->d;
    if (n == 0) return LSR_OK;
    if (!x || !idx || !prev_codebook || !codebook_out || !mass_out || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const VqWorkspace w = vq_workspace(n, k, d);
    char *base = (char *)workspace;
    uint32_t *keys_in = (uint32_t *)(base + w.keys_in), *keys_out = (uint32_t *)(base + w.keys_out), *order = (uint32_t *)(base + w.order);
    int32_t *start = (int32_t *)(base + w.start);
    double *partial = (double *)(base + w.partial);
    unsigned bits = 1;
    while ((1u << bits) <= (unsigned)k) ++bits;      // the keys are 0 .. k
    const rocprim::counting_iterator<uint32_t> iota(0u);
    size_t temp_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, iota, order, (unsigned int)n, 0u, bits, s);
    if (e != hipSuccess) { note_hip_error((int)e); return LSR_ELAUNCH; }
    if (temp_bytes > w.sort_temp_bytes) return LSR_EUNSUPPORTED;
    const unsigned row_blocks = (unsigned)((n + kVqThreads - 1) / kVqThreads);
    hipLaunchKernelGGL(k_vq_keys, dim3(row_blocks), dim3(kVqThreads), 0, s, n, k, idx, keys_in);
    e = hipGetLastError();
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(base + w.sort_temp, temp_bytes, keys_in, keys_out, iota, order, (unsigned int)n, 0u, bits, s);
    if (e != hipSuccess) { note_hip_error((int)e); return LSR_ELAUNCH; }
    hipLaunchKernelGGL(k_vq_bounds, dim3((unsigned)((k + 1 + kVqThreads - 1) / kVqThreads)), dim3(kVqThreads), 0, s, n, k, keys_out, start);
    hipLaunchKernelGGL(k_vq_partial, dim3((unsigned)vq_blocks(n)), dim3(d <= 64 ? 64 : 128), 0, s, k, d, x, weights, keys_out, order, start,
                       prev_codebook, codebook_out, mass_out, partial);
    hipLaunchKernelGGL(k_vq_finish, dim3((unsigned)k), dim3(kVqThreads), 0, s, k, d, start, partial, prev_codebook, codebook_out, mass_out);
    return launch_status();
}

}  // extern "C"
