// density.hip — adaptive density control for a trainable 3DGS scene (include/lsr_density.h): the densification
// statistics of a step in one launch, and the published densify_and_clone -> densify_and_split -> prune_points sequence
// as a plan (three small launches: classify, scan the chunk sums, emit a row map) and ONE gather over every per-Gaussian
// table — the six parameters and, with them, the optimiser's moments.
//
// The plan: a workgroup owns a chunk of kPlanChunk consecutive Gaussians, one per lane.  k_densify_classify writes a
// flag byte per Gaussian (bit 0 the original is emitted, bit 1 a clone, bit 2 the children) and the chunk's three sums;
// k_densify_scan, one workgroup, turns the sums into exclusive bases (each lane a run of consecutive chunks) and writes
// the counts; k_densify_emit scans the flags of its chunk again (block_exclusive_scan of lsr_wave.h) and writes the
// map entries at base + rank.  The order is fixed by the indices alone: no atomics, the same bits every call.
//
// The gather is a streaming kernel.  f_rest and its two moments are 45 floats wide at degree 3 and carry most of the
// bytes, so the work is cut by ELEMENTS, not rows: a workgroup owns kApplyElems consecutive floats of one destination
// table, lane j element j, four independent elements per lane in flight.  The destination is written densely; the kept
// part of the map is monotonic, so the source is read as ascending runs of whole rows, and the map entries of the
// workgroup's rows cross through LDS (read once, densely).  Accesses are dwords: a 45-float row starts on a 4-byte
// boundary, and one dword per lane is 256 contiguous bytes per wave instruction on either side.  The row of an element
// is a multiplication by a per-table reciprocal (exact for the offsets that occur inside a workgroup's span), so no
// integer division runs per element.
#include <math.h>

#include <algorithm>

#include "lsr_density.h"
#include "lsr_internal.h"
#include "lsr_wave.h"

namespace lsr {

constexpr int kDensityThreads = 256;
constexpr int kDensityMaxBlocks = 2048;    // 256 CUs x 8 resident workgroups
constexpr int kPlanChunk = 256;            // Gaussians per chunk = lanes per workgroup of classify / emit
constexpr int kPlanScanThreads = 256;      // the one workgroup that scans the chunk sums
constexpr int kApplyThreads = 256;
constexpr int kApplyElems = 4096;          // destination floats per workgroup of the gather
constexpr uint32_t kParentMask = (1u << LSR_DENSIFY_KIND_SHIFT) - 1u;
enum : uint32_t { kEmitKept = 1u, kEmitClone = 2u, kEmitChildren = 4u };

__global__ __launch_bounds__(kDensityThreads) void k_density_accumulate(int V, int64_t n, const float *__restrict__ grad,
                                                                       const int32_t *__restrict__ radii,
                                                                       float *__restrict__ grad_accum,
                                                                       float *__restrict__ denom,
                                                                       float *__restrict__ max_radii) {
    for (int64_t g = (int64_t)blockIdx.x * kDensityThreads + threadIdx.x; g < n; g += (int64_t)gridDim.x * kDensityThreads) {
        float acc = grad_accum[g], den = denom[g], mr = max_radii[g];
        for (int v = 0; v < V; ++v) {
            const int64_t at = (int64_t)v * n + g;
            // (loaded whether visible or not: in bounds either way, and independent of the radius load)
            const int32_t r = radii[at];
            const float gx = grad[3 * at], gy = grad[3 * at + 1];
            if (r > 0) {
                acc += sqrtf(gx * gx + gy * gy);
                den += 1.0f;
                mr = fmaxf(mr, (float)r);
            }
        }
        grad_accum[g] = acc; denom[g] = den; max_radii[g] = mr;
    }
}

// workspace of the plan: [3][chunks] chunk sums -> exclusive bases (kept, clones, emitting split parents), then the flags
struct PlanWorkspace {
    uint32_t *sums;
    uint8_t *flags;
};

static int64_t plan_chunks(int64_t n) { return (n + kPlanChunk - 1) / kPlanChunk; }

static PlanWorkspace plan_workspace(void *ws, int64_t n) {
    PlanWorkspace p;
    p.sums = (uint32_t *)ws;
    p.flags = (uint8_t *)(p.sums + 3 * plan_chunks(n));
    return p;
}

__global__ __launch_bounds__(kPlanChunk) void k_densify_classify(int64_t n, const float *__restrict__ opacity,
                                                                const float *__restrict__ scaling,
                                                                const float *__restrict__ grad_accum,
                                                                const float *__restrict__ denom,
                                                                const float *__restrict__ max_radii, lsr_densify_params p,
                                                                PlanWorkspace ws) {
    __shared__ uint32_t s_wave[kPlanChunk / LSR_WAVE];
    const int64_t chunks = gridDim.x;
    const int64_t g = (int64_t)blockIdx.x * kPlanChunk + threadIdx.x;
    uint32_t f = 0;
    if (g < n) {
        float avg = grad_accum[g] / denom[g];
        if (avg != avg) avg = 0.0f;
        const float smax = fmaxf(fmaxf(expf(scaling[3 * g]), expf(scaling[3 * g + 1])), expf(scaling[3 * g + 2]));
        const float o = 1.0f / (1.0f + expf(-opacity[g]));
        const bool big = p.max_screen_size > 0.0f;
        const bool selected = avg >= p.grad_threshold;
        const bool clone = selected && smax <= p.dense_extent, split = selected && smax > p.dense_extent;
        const bool faint = o < p.min_opacity;
        if (!split && !faint && !(big && (max_radii[g] > p.max_screen_size || smax > p.world_limit))) f |= kEmitKept;
        if (clone && !faint && !(big && smax > p.world_limit)) f |= kEmitClone;
        if (split && !faint && !(big && smax / (0.8f * (float)p.n_split) > p.world_limit)) f |= kEmitChildren;
        ws.flags[g] = (uint8_t)f;
    }
    // the chunk's three sums, each at most 256: ten bits apiece in one word
    uint32_t total;
    block_exclusive_scan<kPlanChunk>((f & 1u) | ((f >> 1 & 1u) << 10) | ((f >> 2 & 1u) << 20), s_wave, total);
    if (threadIdx.x == 0) {
        ws.sums[blockIdx.x] = total & 1023u;
        ws.sums[chunks + blockIdx.x] = total >> 10 & 1023u;
        ws.sums[2 * chunks + blockIdx.x] = total >> 20;
    }
}

// one workgroup: the three rows of chunk sums to exclusive bases, in place; the counts
__global__ __launch_bounds__(kPlanScanThreads) void k_densify_scan(int64_t chunks, int n_split, uint32_t *__restrict__ sums,
                                                                  uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_wave[kPlanScanThreads / LSR_WAVE];
    uint32_t totals[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) scan_chunk_sums<kPlanScanThreads>(sums + k * chunks, chunks, s_wave, totals[k]);
    if (threadIdx.x == 0) {
        counts[0] = totals[0]; counts[1] = totals[1]; counts[2] = totals[2];
        counts[3] = totals[0] + totals[1] + (uint32_t)n_split * totals[2];
    }
}

__global__ __launch_bounds__(kPlanChunk) void k_densify_emit(int64_t n, int n_split, PlanWorkspace ws,
                                                            const uint32_t *__restrict__ counts, uint32_t *__restrict__ map) {
    __shared__ uint32_t s_wave[kPlanChunk / LSR_WAVE];
    const int64_t chunks = gridDim.x;
    const int64_t g = (int64_t)blockIdx.x * kPlanChunk + threadIdx.x;
    const uint32_t f = g < n ? ws.flags[g] : 0u;
    uint32_t total;
    const uint32_t rank = block_exclusive_scan<kPlanChunk>((f & 1u) | ((f >> 1 & 1u) << 10) | ((f >> 2 & 1u) << 20), s_wave, total);
    const uint32_t kept = counts[0], clones = counts[1], parents = counts[2];
    // every index below is < kept + clones + N parents = n_out <= n max(2, N) <= capacity
    if (f & kEmitKept) map[ws.sums[blockIdx.x] + (rank & 1023u)] = (uint32_t)g;
    if (f & kEmitClone)
        map[kept + ws.sums[chunks + blockIdx.x] + (rank >> 10 & 1023u)] = (uint32_t)g | (uint32_t)LSR_DENSIFY_CLONE << LSR_DENSIFY_KIND_SHIFT;
    if (f & kEmitChildren) {
        const uint32_t at = kept + clones + ws.sums[2 * chunks + blockIdx.x] + (rank >> 20);
        for (int c = 0; c < n_split; ++c)
            map[at + (uint32_t)c * parents] = (uint32_t)g | (uint32_t)(LSR_DENSIFY_CHILD0 + c) << LSR_DENSIFY_KIND_SHIFT;
    }
}

struct ApplyTable {
    const float *src;
    float *dst;
    uint32_t width, rule;
    uint32_t magic;         // ceil(2^32 / width) for width >= 2: x / width == umulhi(x, magic) for x < 2^13
    uint32_t first_block;   // of the launch's grid
};

struct ApplyArgs {
    ApplyTable t[LSR_DENSIFY_MAX_TABLES];
    int num_tables, n_split;
    int64_t n, n_out, eps_rows;
    const uint32_t *map, *counts;
    const float *scaling, *rotation, *eps;
};

__device__ __forceinline__ float apply_value(const ApplyArgs &a, const ApplyTable &tb, uint32_t m, uint32_t col, int64_t row,
                                             uint32_t kept_and_clones) {
    const uint32_t parent = m & kParentMask, kind = m >> LSR_DENSIFY_KIND_SHIFT;
    if ((int64_t)parent >= a.n) return 0.0f;
    const bool fresh = kind >= (uint32_t)LSR_DENSIFY_CHILD0;
    if (tb.rule == LSR_DENSIFY_ZERO_NEW && kind != (uint32_t)LSR_DENSIFY_KEPT) return 0.0f;
    if (tb.rule == LSR_DENSIFY_SCALING && fresh) return logf(expf(a.scaling[3 * (int64_t)parent + col]) / (0.8f * (float)a.n_split));
    const float own = tb.src[(int64_t)parent * tb.width + col];
    if (tb.rule != LSR_DENSIFY_XYZ || !fresh) return own;
    const int64_t r = row - (int64_t)kept_and_clones;
    if (r < 0 || r >= a.eps_rows) return 0.0f;
    const float *q = a.rotation + 4 * (int64_t)parent, *s = a.scaling + 3 * (int64_t)parent, *e = a.eps + 3 * r;
    const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    const float d0 = expf(s[0]) * e[0], d1 = expf(s[1]) * e[1], d2 = expf(s[2]) * e[2];
    float r0, r1, r2;                                   // row `col` of R(q / |q|)
    if (col == 0) { r0 = 1.0f - 2.0f * (y * y + z * z); r1 = 2.0f * (x * y - w * z); r2 = 2.0f * (x * z + w * y); }
    else if (col == 1) { r0 = 2.0f * (x * y + w * z); r1 = 1.0f - 2.0f * (x * x + z * z); r2 = 2.0f * (y * z - w * x); }
    else { r0 = 2.0f * (x * z - w * y); r1 = 2.0f * (y * z + w * x); r2 = 1.0f - 2.0f * (x * x + y * y); }
    return (r0 * d0 + r1 * d1 + r2 * d2) + own;
}

__global__ __launch_bounds__(kApplyThreads) void k_densify_apply(ApplyArgs a) {
    __shared__ uint32_t s_map[kApplyElems + 1];
    const int tid = threadIdx.x;
    ApplyTable tb = a.t[0];
    for (int i = 1; i < a.num_tables; ++i)
        if (blockIdx.x >= a.t[i].first_block) tb = a.t[i];
    const uint32_t w = tb.width;
    const int64_t total = a.n_out * (int64_t)w;
    const int64_t e0 = (int64_t)(blockIdx.x - tb.first_block) * kApplyElems;
    if (e0 >= total) return;                              // (never: the grid is sized from the same numbers)
    const int count = total - e0 < (int64_t)kApplyElems ? (int)(total - e0) : kApplyElems;
    const int64_t r0 = e0 / w;
    const uint32_t off0 = (uint32_t)(e0 - r0 * w);
    // rows r0 .. r0 + rows - 1 hold this span; the last one is the row of element e0 + count - 1 < n_out * w
    const int rows = (int)((off0 + (uint32_t)count - 1u) / w) + 1;        // <= kApplyElems + 1
    for (int i = tid; i < rows; i += kApplyThreads) s_map[i] = a.map[r0 + i];
    __syncthreads();
    const uint32_t kept_and_clones = a.counts[0] + a.counts[1];
    float *__restrict__ dst = tb.dst + e0;
    for (int j0 = tid; j0 < count; j0 += 4 * kApplyThreads) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * kApplyThreads;
            if (j < count) {
                const uint32_t x = off0 + (uint32_t)j;    // < width + kApplyElems <= 2^13
                const uint32_t q = w == 1u ? x : __umulhi(x, tb.magic);
                v[u] = apply_value(a, tb, s_map[q], x - q * w, r0 + q, kept_and_clones);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * kApplyThreads;
            if (j < count) dst[j] = v[u];
        }
    }
}

}  // namespace lsr

using namespace lsr;

static_assert(LSR_DENSIFY_MAX_WIDTH + kApplyElems <= (1 << 13), "the reciprocal division of k_densify_apply");
static_assert(kPlanChunk <= 1023, "three ten-bit chunk sums in one word");

extern "C" {

int lsr_density_accumulate(int32_t V, int64_t n, const float *grad_means2D, const int32_t *radii, float *grad_accum,
                           float *denom, float *max_radii, lsr_stream_t stream) {
    note_hip_error(0);
    if (V < 0 || n < 0) return LSR_EINVAL;
    if (V == 0 || n == 0) return LSR_OK;
    if (!grad_means2D || !radii || !grad_accum || !denom || !max_radii) return LSR_ENULL;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kDensityThreads - 1) / kDensityThreads, kDensityMaxBlocks);
    hipLaunchKernelGGL(k_density_accumulate, dim3(blocks), dim3(kDensityThreads), 0, (hipStream_t)stream, (int)V, n,
                       grad_means2D, radii, grad_accum, denom, max_radii);
    return launch_status();
}

size_t lsr_densify_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return (size_t)(3 * plan_chunks(n)) * sizeof(uint32_t) + (size_t)n;
}

int lsr_densify_plan(int64_t n, const float *opacity, const float *scaling, const float *grad_accum, const float *denom,
                     const float *max_radii, const lsr_densify_params *params, uint32_t *map, int64_t capacity,
                     uint32_t *counts, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (!params) return LSR_ENULL;
    const lsr_densify_params &p = *params;
    if (n < 0 || p.n_split < 1 || p.n_split > LSR_DENSIFY_MAX_SPLIT || p.reserved0 || p.reserved1) return LSR_EINVAL;
    if (!std::isfinite(p.grad_threshold) || !std::isfinite(p.dense_extent) || !std::isfinite(p.min_opacity) ||
        !std::isfinite(p.max_screen_size) || (p.max_screen_size > 0.0f && !std::isfinite(p.world_limit)))
        return LSR_EINVAL;
    const int64_t most = std::max(2, (int)p.n_split);
    if (n >= (LSR_DENSIFY_MAX_ROWS + most - 1) / most || capacity < n * most) return LSR_EINVAL;   // n * most >= 2^28
    if (n == 0) return LSR_OK;
    if (!opacity || !scaling || !grad_accum || !denom || !max_radii || !map || !counts || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const PlanWorkspace ws = plan_workspace(workspace, n);
    const int64_t chunks = plan_chunks(n);                 // < 2^28 / 256
    hipLaunchKernelGGL(k_densify_classify, dim3((unsigned)chunks), dim3(kPlanChunk), 0, s, n, opacity, scaling, grad_accum,
                       denom, max_radii, p, ws);
    hipLaunchKernelGGL(k_densify_scan, dim3(1), dim3(kPlanScanThreads), 0, s, chunks, (int)p.n_split, ws.sums, counts);
    hipLaunchKernelGGL(k_densify_emit, dim3((unsigned)chunks), dim3(kPlanChunk), 0, s, n, (int)p.n_split, ws, counts, map);
    return launch_status();
}

int lsr_densify_apply(int64_t n, int64_t n_out, const uint32_t *map, const uint32_t *counts, int32_t n_split,
                      const lsr_densify_table *tables, int32_t num_tables, const float *scaling, const float *rotation,
                      const float *eps, int64_t eps_rows, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || n_out < 0 || n_out >= LSR_DENSIFY_MAX_ROWS || (n == 0 && n_out > 0)) return LSR_EINVAL;
    if (n_split < 1 || n_split > LSR_DENSIFY_MAX_SPLIT || num_tables < 0 || num_tables > LSR_DENSIFY_MAX_TABLES || eps_rows < 0)
        return LSR_EINVAL;
    if (num_tables > 0 && !tables) return n_out > 0 ? LSR_ENULL : LSR_OK;
    bool xyz = false, scal = false;
    for (int i = 0; i < num_tables; ++i) {
        const lsr_densify_table &t = tables[i];
        if (t.rule < LSR_DENSIFY_COPY || t.rule > LSR_DENSIFY_SCALING || t.width < 1 || t.width > LSR_DENSIFY_MAX_WIDTH) return LSR_EINVAL;
        if ((t.rule == LSR_DENSIFY_XYZ || t.rule == LSR_DENSIFY_SCALING) && t.width != 3) return LSR_EINVAL;
        xyz |= t.rule == LSR_DENSIFY_XYZ;
        scal |= t.rule == LSR_DENSIFY_SCALING;
    }
    if (n_out == 0 || num_tables == 0) return LSR_OK;
    if (!map || !counts) return LSR_ENULL;
    if ((xyz || scal) && !scaling) return LSR_ENULL;
    if (xyz && (!rotation || (eps_rows > 0 && !eps))) return LSR_ENULL;
    ApplyArgs a{};
    int64_t blocks = 0;
    for (int i = 0; i < num_tables; ++i) {
        const lsr_densify_table &t = tables[i];
        if (!t.src || !t.dst) return LSR_ENULL;
        a.t[i].src = t.src; a.t[i].dst = t.dst; a.t[i].width = (uint32_t)t.width; a.t[i].rule = (uint32_t)t.rule;
        a.t[i].magic = t.width >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)t.width - 1) / (uint64_t)t.width) : 0u;
        a.t[i].first_block = (uint32_t)blocks;
        blocks += (n_out * t.width + kApplyElems - 1) / kApplyElems;
        if (blocks > 0x7FFFFFFFll) return LSR_EINVAL;      // 24 tables of 2^28 rows x 4096 floats: beyond one grid
    }
    a.num_tables = num_tables; a.n_split = n_split; a.n = n; a.n_out = n_out; a.eps_rows = eps ? eps_rows : 0;
    a.map = map; a.counts = counts; a.scaling = scaling; a.rotation = rotation; a.eps = eps;
    hipLaunchKernelGGL(k_densify_apply, dim3((unsigned)blocks), dim3(kApplyThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
