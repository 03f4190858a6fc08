// optim.hip — the fused Adam step of a trainable 3DGS scene (include/lsr_optim.h): every table of every parameter group
// in ONE launch, densely or on the rows a visibility mask names.
//
// A pure streaming kernel: per element four reads (parameter, gradient, two moments) and three writes, 28 bytes, against
// a dozen float operations.  As in k_densify_apply (density.hip) the table descriptors travel by value, each table owns
// a contiguous range of workgroups (first_block) and selecting the table is block-uniform; the work is cut by ELEMENTS,
// not rows (f_rest and its moments are 45 floats wide at degree 3 and carry most of the bytes): a workgroup owns
// kAdamElems consecutive floats of one table.  A lane owns GROUPS of four consecutive floats, group k of the workgroup
// at floats 4 k .. 4 k + 3 of its span, lane j group j + 256 u in pass u: where the table's four pointers are 16-byte
// aligned (a span starts at a multiple of 4096 floats, so alignment is the table's) a whole group moves as one 16-byte
// access per array, 1 KiB contiguous per wave instruction.  A group that is cut by the table's end or by the mask, and
// every group of a table with a misaligned pointer, moves as single floats, each guarded by its own bit: nothing is
// touched past the end, and nothing of an invisible row.  Both ways run the same arithmetic on the same element (the
// fused operations are written out, see adam_element), so the bits do not depend on the path.  No batching of loads by
// hand: at 47 VGPRs eight waves per SIMD are resident and each has 64 bytes per lane in flight per pass, far more than
// latency x bandwidth needs.
//
// Sparse mode: the workgroup's rows cross through LDS once (one mask byte per row, at most 4097 rows for a span), the
// row of an element is a multiplication by the table's reciprocal (exact for the offsets that occur inside a span, as
// in k_densify_apply), and a wave whose groups are all masked out skips the pass on a wave-uniform branch before any
// load from the four arrays is issued.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "lsr_optim.h"
#include "lsr_internal.h"

namespace lsr {

constexpr int kAdamThreads = 256;
constexpr int kAdamElems = 4096;           // floats per workgroup
constexpr int kAdamPasses = kAdamElems / (4 * kAdamThreads);

struct AdamTable {
    float *p;
    const float *g;
    float *m, *v;
    int64_t total;          // rows * width
    uint32_t width;
    uint32_t magic;         // ceil(2^32 / width) for width >= 2: x / width == umulhi(x, magic) for x < 2^13
    uint32_t first_block;   // of the launch's grid
    uint32_t vec;           // all four pointers 16-byte aligned
    float beta1, beta2, c1, c2, eps, step_size, inv_sqrt_bc2;   // c = the host's (float)(1 - beta)
};

struct AdamArgs {
    AdamTable t[LSR_ADAM_MAX_TABLES];
    const uint8_t *visible;
    int num_tables;
};

// The header's three lines with their fused operations SPELLED OUT: left to the compiler's contraction, the vector and
// the scalar copy of this function came out differently (beta * m + (c * g) has two candidates for the fused operation)
// and the same element got different last bits on the two paths.  Nothing else here can contract: a lone product feeds
// each fmaf, and a division stands between the last product and the subtraction.
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamTable &t) {
    m = fmaf(t.beta1, m, t.c1 * g);
    v = fmaf(t.beta2, v, t.c2 * g * g);
    p = p - t.step_size * m / fmaf(sqrtf(v), t.inv_sqrt_bc2, t.eps);
}

__global__ __launch_bounds__(kAdamThreads) void k_adam_step(AdamArgs a) {
    __shared__ uint8_t s_vis[kAdamElems + 8];
    const int tid = threadIdx.x;
    AdamTable tb = a.t[0];
    for (int i = 1; i < a.num_tables; ++i)
        if (blockIdx.x >= a.t[i].first_block) tb = a.t[i];
    const uint32_t w = tb.width;
    const int64_t e0 = (int64_t)(blockIdx.x - tb.first_block) * kAdamElems;
    if (e0 >= tb.total) return;                           // (never: the grid is sized from the same numbers)
    const int count = tb.total - e0 < (int64_t)kAdamElems ? (int)(tb.total - e0) : kAdamElems;
    const bool sparse = a.visible != nullptr;
    uint32_t off0 = 0;
    if (sparse) {
        const int64_t r0 = e0 / w;
        off0 = (uint32_t)(e0 - r0 * w);
        // rows r0 .. r0 + rows - 1 hold this span; the last one is the row of element e0 + count - 1 < rows * width
        const int rows = (int)((off0 + (uint32_t)count - 1u) / w) + 1;     // <= kAdamElems + 1
        for (int i = tid; i < rows; i += kAdamThreads) s_vis[i] = a.visible[r0 + i];
        __syncthreads();
    }
    float *__restrict__ P = tb.p + e0;
    const float *__restrict__ G = tb.g + e0;
    float *__restrict__ M = tb.m + e0;
    float *__restrict__ V = tb.v + e0;
#pragma unroll
    for (int u = 0; u < kAdamPasses; ++u) {
        const int j = 4 * (u * kAdamThreads + tid);       // the group's first float within the span
        uint32_t live = 0;                                // bit k: float j + k is inside the table and its row visible
        if (j < count) {
            live = count - j >= 4 ? 15u : (1u << (count - j)) - 1u;
            if (sparse) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t x = off0 + (uint32_t)(j + k);           // < width + kAdamElems <= 2^13
                    const uint32_t q = w == 1u ? x : __umulhi(x, tb.magic);
                    if ((live >> k & 1u) && s_vis[q] == 0) live &= ~(1u << k);
                }
            }
        }
        if (__ballot(live != 0u) == 0ull) continue;       // wave-uniform: nothing of this wave's pass is loaded
        if (tb.vec && live == 15u) {
            float4 p = *reinterpret_cast<const float4 *>(P + j);
            const float4 g = *reinterpret_cast<const float4 *>(G + j);
            float4 m = *reinterpret_cast<const float4 *>(M + j);
            float4 v = *reinterpret_cast<const float4 *>(V + j);
            adam_element(p.x, g.x, m.x, v.x, tb);
            adam_element(p.y, g.y, m.y, v.y, tb);
            adam_element(p.z, g.z, m.z, v.z, tb);
            adam_element(p.w, g.w, m.w, v.w, tb);
            *reinterpret_cast<float4 *>(M + j) = m;
            *reinterpret_cast<float4 *>(V + j) = v;
            *reinterpret_cast<float4 *>(P + j) = p;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (live >> k & 1u) {
                    float p = P[j + k], m = M[j + k], v = V[j + k];
                    adam_element(p, G[j + k], m, v, tb);
                    M[j + k] = m; V[j + k] = v; P[j + k] = p;
                }
            }
        }
    }
}

}  // namespace lsr

using namespace lsr;

static_assert(LSR_ADAM_MAX_WIDTH + kAdamElems <= (1 << 13), "the reciprocal division of k_adam_step");
static_assert(kAdamElems % (4 * kAdamThreads) == 0, "whole passes of four-float groups");
static_assert(sizeof(AdamArgs) <= 4096, "kernel arguments");

extern "C" {

int lsr_adam_step(const lsr_adam_table *tables, int32_t num_tables, const uint8_t *visible, int64_t visible_rows,
                  lsr_stream_t stream) {
    note_hip_error(0);
    if (num_tables < 0 || num_tables > LSR_ADAM_MAX_TABLES) return LSR_EINVAL;
    if (visible && visible_rows < 0) return LSR_EINVAL;
    if (num_tables == 0) return LSR_OK;
    if (!tables) return LSR_ENULL;
    int64_t blocks = 0;
    for (int i = 0; i < num_tables; ++i) {
        const lsr_adam_table &t = tables[i];
        if (t.rows < 0 || t.rows > LSR_ADAM_MAX_ROWS || t.width < 1 || t.width > LSR_ADAM_MAX_WIDTH) return LSR_EINVAL;
        if (t.reserved != 0 || t.reserved_f != 0.0f) return LSR_EINVAL;
        if (!std::isfinite(t.beta1) || !std::isfinite(t.beta2) || !std::isfinite(t.one_minus_beta1) || !std::isfinite(t.one_minus_beta2) ||
            !std::isfinite(t.eps) || !std::isfinite(t.step_size) || !std::isfinite(t.inv_sqrt_bc2))
            return LSR_EINVAL;
        if (t.beta1 < 0.0f || t.beta1 >= 1.0f || t.beta2 < 0.0f || t.beta2 >= 1.0f || t.eps < 0.0f) return LSR_EINVAL;
        if (t.one_minus_beta1 < 0.0f || t.one_minus_beta1 > 1.0f || t.one_minus_beta2 < 0.0f || t.one_minus_beta2 > 1.0f) return LSR_EINVAL;
        if (visible && t.rows > 0 && t.rows != visible_rows) return LSR_EINVAL;
        blocks += (t.rows * t.width + kAdamElems - 1) / kAdamElems;        // rows * width <= 2^52
        if (blocks > 0x7FFFFFFFll) return LSR_EINVAL;                      // beyond one grid
    }
    if (blocks == 0) return LSR_OK;
    AdamArgs a{};
    blocks = 0;
    int used = 0;
    for (int i = 0; i < num_tables; ++i) {
        const lsr_adam_table &t = tables[i];
        if (t.rows == 0) continue;
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return LSR_ENULL;
        AdamTable &d = a.t[used++];
        d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq;
        d.total = t.rows * t.width;
        d.width = (uint32_t)t.width;
        d.magic = t.width >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)t.width - 1) / (uint64_t)t.width) : 0u;
        d.first_block = (uint32_t)blocks;
        d.vec = (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15u) == 0 ? 1u : 0u;
        d.beta1 = t.beta1; d.beta2 = t.beta2; d.c1 = t.one_minus_beta1; d.c2 = t.one_minus_beta2; d.eps = t.eps; d.step_size = t.step_size; d.inv_sqrt_bc2 = t.inv_sqrt_bc2;
        blocks += (d.total + kAdamElems - 1) / kAdamElems;
    }
    a.visible = visible;
    a.num_tables = used;
    hipLaunchKernelGGL(k_adam_step, dim3((unsigned)blocks), dim3(kAdamThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
