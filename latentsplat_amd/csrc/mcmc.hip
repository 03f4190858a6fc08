// mcmc.hip — the MCMC densification strategy for a trainable 3DGS scene (include/lsr_mcmc.h): dead-row classification,
// sampling of rows in proportion to a weight, the published relocate_gs / add_new_gs over every per-Gaussian table, and
// the per-step covariance-shaped noise on the positions.
//
// Sampling is exact integer arithmetic.  A weight becomes a 30-bit quantum; a workgroup owns a chunk of kMcmcChunk
// consecutive rows, one per lane.  k_mcmc_sums writes the chunk's sum (uint64: 256 quanta of 2^30 pass 32 bits) and
// zeroes `count`; k_mcmc_scan, one workgroup, turns the sums into exclusive bases (each lane a run of consecutive chunks)
// and appends the total; k_mcmc_cum writes cum[g] = base + the inclusive scan inside the chunk; k_mcmc_draw, one lane per
// draw, searches the bases and then its chunk.  Integer sums are associative, so the answer is the header's whatever the
// scan's shape.  `count` is incremented with ordinary integer atomics: the result does not depend on their order.
//
// Classification is the plan of density.hip with one flag: per-chunk count (and the weights), scan of the chunk sums,
// emission of the dead indices at base + rank.  No atomics.
//
// Relocation, the ownership argument.  Two launches.
//   k_mcmc_sources, a workgroup per chunk of rows: lane g with count[g] > 0 evaluates the new (opacity, scaling) from ITS
//     OWN old values, writes them to stage[g] (scratch, 16 bytes per row, written at sources only) and then over its own
//     opacity / scaling row; the chunk's sources are compacted in LDS and all lanes zero their MOMENT rows.  Every element
//     written here belongs to a source row g, and g belongs to exactly one lane (stage, opacity, scaling) or one workgroup
//     (the moment rows, each element by one lane of it).
//   k_mcmc_dests: work cut by elements of the virtual [m][width] array of each table, as k_densify_apply.  Element
//     (j, col) writes row dest[j] (or n + j) of its table: COPY from row idx[j] of the same table — a column no launch
//     writes at a source row —, OPACITY / SCALING from stage[idx[j]], MOMENT 0 (growth only; a relocation gives MOMENT
//     tables no workgroups).  A destination is never a source and appears once, so (dest[j], col) has one owner, and a
//     destination never reads opacity / scaling of a source: the one hazard, reading what the first launch overwrites, does
//     not exist.  The values a destination receives are the bits the source received: both come from stage.
// The new values are evaluated in double (only sampled rows pay): the alternating sum D cancels badly in float32 near
// o -> 1 at large N.  The binomials come from a table built at compile time by Pascal's rule, exact in double (the largest,
// C(50, 25) = 1.26e14, is below 2^53).
//
// Noise: a streaming kernel, 68 bytes per Gaussian (xyz read and written, opacity, scaling, rotation, eps), one Gaussian
// per lane as the geometry part of k_scene_fwd: the quaternion is one 16-byte access, the 3-float rows are accessed
// directly by their lane (the three strided dword accesses of a wave together cover whole cache lines).  Sigma v is
// evaluated as R (s^2 * (R^T v)): no 3x3 temporaries.  The unit is compiled with -ffp-contract=off (Makefile): the
// increment is the same float whatever it is added to, and xyz + increment is one rounding.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "lsr_mcmc.h"
#include "lsr_internal.h"
#include "lsr_wave.h"

namespace lsr {

constexpr int kMcmcChunk = 256;            // rows per chunk = lanes per workgroup of the chunked kernels
constexpr int kMcmcScanThreads = 256;      // the one workgroup that scans the chunk sums
constexpr int kMcmcThreads = 256;          // draw and noise kernels
constexpr int kMcmcMaxBlocks = 2048;       // 256 CUs x 8 resident workgroups (noise: chunks strided over the grid)
constexpr int kMcmcApplyElems = 2048;      // destination floats per workgroup of k_mcmc_dests
constexpr double kMcmcOpacityMax = 1.0 - 1.1920929e-7;

struct Binomials {
    double c[LSR_MCMC_MAX_RATIO + 1][LSR_MCMC_MAX_RATIO + 2];
    constexpr Binomials() : c{} {
        for (int n = 0; n <= LSR_MCMC_MAX_RATIO; ++n) {
            c[n][0] = 1.0;
            for (int k = 1; k <= n; ++k) c[n][k] = c[n - 1][k - 1] + (k < n ? c[n - 1][k] : 0.0);
        }
    }
};
__constant__ const Binomials kBinomials{};

static int64_t mcmc_chunks(int64_t n) { return (n + kMcmcChunk - 1) / kMcmcChunk; }

// ---- classification ----

__device__ __forceinline__ bool mcmc_dead(float o, float dead_logit) { return o <= dead_logit; }

// with sums == nullptr: the weights alone
__global__ __launch_bounds__(kMcmcChunk) void k_mcmc_classify(int64_t n, const float *__restrict__ opacity, float dead_logit,
                                                             float *__restrict__ weights, uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_wave[kMcmcChunk / LSR_WAVE];
    const int64_t g = (int64_t)blockIdx.x * kMcmcChunk + threadIdx.x;
    uint32_t dead = 0;
    if (g < n) {
        const float o = opacity[g];
        dead = mcmc_dead(o, dead_logit) ? 1u : 0u;
        weights[g] = dead ? 0.0f : 1.0f / (1.0f + expf(-o));
    }
    if (!sums) return;                                    // block-uniform
    uint32_t total;
    block_exclusive_scan<kMcmcChunk>(dead, s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the chunk sums to exclusive bases, in place; counts = {dead, alive}
__global__ __launch_bounds__(kMcmcScanThreads) void k_mcmc_classify_scan(int64_t n, int64_t chunks, uint32_t *__restrict__ sums,
                                                                        uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_wave[kMcmcScanThreads / LSR_WAVE];
    uint32_t total;
    scan_chunk_sums<kMcmcScanThreads>(sums, chunks, s_wave, total);
    if (threadIdx.x == 0) { counts[0] = total; counts[1] = (uint32_t)n - total; }
}

__global__ __launch_bounds__(kMcmcChunk) void k_mcmc_classify_emit(int64_t n, const float *__restrict__ opacity, float dead_logit,
                                                                  const uint32_t *__restrict__ sums, int32_t *__restrict__ dead_rows) {
    __shared__ uint32_t s_wave[kMcmcChunk / LSR_WAVE];
    const int64_t g = (int64_t)blockIdx.x * kMcmcChunk + threadIdx.x;
    const uint32_t dead = g < n && mcmc_dead(opacity[g], dead_logit) ? 1u : 0u;
    uint32_t total;
    const uint32_t rank = block_exclusive_scan<kMcmcChunk>(dead, s_wave, total);
    // base + rank < the number of dead rows <= n: inside dead_rows [n]
    if (dead) dead_rows[sums[blockIdx.x] + rank] = (int32_t)g;
}

// ---- sampling ----

__device__ __forceinline__ uint32_t mcmc_quantum(float w) {
    if (!(w > 0.0f)) return 0u;                           // NaN, negatives, zero
    if (w >= 1.0f) return 1u << LSR_MCMC_WEIGHT_BITS;
    return (uint32_t)(w * (float)(1u << LSR_MCMC_WEIGHT_BITS));   // a power of two: exact, then truncated
}

// workspace of a sample call: bases [chunks + 1] (exclusive; the last word is the total), then cum [n]
struct SampleWorkspace {
    uint64_t *bases, *cum;
};

static SampleWorkspace sample_workspace(void *ws, int64_t n) {
    SampleWorkspace s;
    s.bases = (uint64_t *)ws;
    s.cum = s.bases + mcmc_chunks(n) + 1;
    return s;
}

__global__ __launch_bounds__(kMcmcChunk) void k_mcmc_sums(int64_t n, const float *__restrict__ weights, uint32_t *__restrict__ count,
                                                         uint64_t *__restrict__ sums) {
    __shared__ uint64_t s_wave[kMcmcChunk / LSR_WAVE];
    const int64_t g = (int64_t)blockIdx.x * kMcmcChunk + threadIdx.x;
    uint64_t q = 0;
    if (g < n) { q = mcmc_quantum(weights[g]); count[g] = 0u; }
    uint64_t total;
    block_exclusive_scan<kMcmcChunk>(q, s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums [chunks] to exclusive bases in place, bases[chunks] = total
__global__ __launch_bounds__(kMcmcScanThreads) void k_mcmc_scan(int64_t chunks, uint64_t *__restrict__ sums, uint64_t *__restrict__ total_out) {
    __shared__ uint64_t s_wave[kMcmcScanThreads / LSR_WAVE];
    uint64_t total;
    scan_chunk_sums<kMcmcScanThreads>(sums, chunks, s_wave, total);
    if (threadIdx.x == 0) {
        sums[chunks] = total;
        if (total_out) *total_out = total;
    }
}

__global__ __launch_bounds__(kMcmcChunk) void k_mcmc_cum(int64_t n, const float *__restrict__ weights, SampleWorkspace ws) {
    __shared__ uint64_t s_wave[kMcmcChunk / LSR_WAVE];
    const int64_t g = (int64_t)blockIdx.x * kMcmcChunk + threadIdx.x;
    const uint64_t q = g < n ? mcmc_quantum(weights[g]) : 0u;
    uint64_t total;
    const uint64_t before = block_exclusive_scan<kMcmcChunk>(q, s_wave, total);
    if (g < n) ws.cum[g] = ws.bases[blockIdx.x] + before + q;
}

__global__ __launch_bounds__(kMcmcThreads) void k_mcmc_draw(int64_t n, int64_t chunks, int64_t m, const double *__restrict__ uniforms,
                                                           SampleWorkspace ws, int32_t *__restrict__ idx, uint32_t *__restrict__ count) {
    const int64_t j = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x;
    if (j >= m) return;
    const uint64_t total = ws.bases[chunks];
    if (total == 0) { idx[j] = -1; return; }
    double u = uniforms[j];
    if (!(u > 0.0)) u = 0.0;                              // NaN, negatives
    u = fmin(u, 1.0 - 0x1p-53);
    uint64_t t = (uint64_t)(u * (double)total);           // one product, rounded once, truncated
    if (t > total - 1) t = total - 1;
    // the last chunk c with bases[c] <= t: bases[0] = 0 <= t; then bases[c + 1] > t (or c + 1 == chunks and total > t)
    int64_t lo = 0, hi = chunks;                          // invariant: bases[lo] <= t, and hi == chunks or bases[hi] > t
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ws.bases[mid] <= t) lo = mid; else hi = mid;
    }
    // the smallest g of chunk lo with cum[g] > t; the chunk's last cum is bases[lo + 1] > t
    int64_t a = lo * kMcmcChunk, b = std::min<int64_t>(a + kMcmcChunk, n) - 1;     // the answer lies in [a, b]
    while (a < b) {
        const int64_t mid = a + (b - a) / 2;
        if (ws.cum[mid] > t) b = mid; else a = mid + 1;
    }
    idx[j] = (int32_t)a;                                  // a <= n - 1
    atomicAdd(&count[a], 1u);
}

// ---- relocation ----

// The header's formulas for one source, in double: out = {logit(o'), log(scale'[0..2])}.
__device__ __forceinline__ float4 mcmc_new_values(float opacity, float s0, float s1, float s2, uint32_t c, double min_opacity) {
    const int N = (int)std::min<uint32_t>(c, LSR_MCMC_MAX_RATIO - 1) + 1;
    const double x = (double)opacity;
    const double o = 1.0 / (1.0 + exp(-x));
    const double log_1mo = -log1p(exp(x));                // log(1 - o), without forming 1 - o
    const double op = -expm1(log_1mo / (double)N);        // 1 - (1 - o)^(1 / N)
    const double *row = kBinomials.c[N];
    double D = 0.0, pw = op;
    for (int k = 0; k < N; ++k) {
        const double term = row[k + 1] * pw / sqrt((double)(k + 1));
        D += (k & 1) ? -term : term;
        pw *= op;
    }
    const double shift = log(o / D);                      // log(scale') = log(o / D) + scaling
    const double oc = fmin(fmax(op, min_opacity), kMcmcOpacityMax);
    return make_float4((float)(log(oc) - log1p(-oc)), (float)(shift + (double)s0), (float)(shift + (double)s1), (float)(shift + (double)s2));
}

struct McmcTable {
    float *p;
    uint32_t width, role;
    uint32_t magic;         // ceil(2^32 / width) for width >= 2: x / width == umulhi(x, magic) for x < 2^20
    uint32_t first_block;   // of k_mcmc_dests' grid
};

struct McmcArgs {
    McmcTable t[LSR_MCMC_MAX_TABLES];
    int num_tables, growth;
    int64_t n, m;
    const int32_t *idx, *dest;
    const uint32_t *count;
    float *opacity, *scaling;   // the OPACITY and SCALING tables
    float4 *stage;              // [n], written at sources
    double min_opacity;
};

__global__ __launch_bounds__(kMcmcChunk) void k_mcmc_sources(McmcArgs a) {
    __shared__ uint32_t s_wave[kMcmcChunk / LSR_WAVE];
    __shared__ uint32_t s_rows[kMcmcChunk];
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * kMcmcChunk, g = g0 + tid;
    const uint32_t c = g < a.n ? a.count[g] : 0u;
    if (c > 0u) {
        float *sc = a.scaling + 3 * g;
        const float4 v = mcmc_new_values(a.opacity[g], sc[0], sc[1], sc[2], c, a.min_opacity);
        a.stage[g] = v;
        a.opacity[g] = v.x;
        sc[0] = v.y; sc[1] = v.z; sc[2] = v.w;
    }
    uint32_t sources;
    const uint32_t rank = block_exclusive_scan<kMcmcChunk>(c > 0u ? 1u : 0u, s_wave, sources);
    if (sources == 0u) return;                            // block-uniform
    if (c > 0u) s_rows[rank] = (uint32_t)tid;
    __syncthreads();
    for (int i = 0; i < a.num_tables; ++i) {
        const McmcTable tb = a.t[i];
        if (tb.role != (uint32_t)LSR_MCMC_MOMENT) continue;
        const uint32_t w = tb.width, elems = sources * w;  // <= 256 * 4096 = 2^20
        for (uint32_t e = tid; e < elems; e += kMcmcChunk) {
            const uint32_t r = w == 1u ? e : __umulhi(e, tb.magic);
            tb.p[(g0 + s_rows[r]) * (int64_t)w + (e - r * w)] = 0.0f;
        }
    }
}

__global__ __launch_bounds__(kMcmcThreads) void k_mcmc_dests(McmcArgs a) {
    __shared__ int32_t s_src[kMcmcApplyElems + 1];
    __shared__ int32_t s_dst[kMcmcApplyElems + 1];
    const int tid = threadIdx.x;
    McmcTable tb = a.t[0];
    for (int i = 1; i < a.num_tables; ++i)
        if (blockIdx.x >= a.t[i].first_block) tb = a.t[i];
    const uint32_t w = tb.width;
    const int64_t total = a.m * (int64_t)w;
    const int64_t e0 = (int64_t)(blockIdx.x - tb.first_block) * kMcmcApplyElems;
    if (e0 >= total) return;                              // (never: the grid is sized from the same numbers)
    const int count = total - e0 < (int64_t)kMcmcApplyElems ? (int)(total - e0) : kMcmcApplyElems;
    const int64_t r0 = e0 / w;
    const uint32_t off0 = (uint32_t)(e0 - r0 * w);
    // draws r0 .. r0 + rows - 1 hold this span; the last one is the draw of element e0 + count - 1 < m * w
    const int rows = (int)((off0 + (uint32_t)count - 1u) / w) + 1;          // <= kMcmcApplyElems + 1
    const int64_t limit = a.growth ? a.n + a.m : a.n;     // rows of the table
    for (int i = tid; i < rows; i += kMcmcThreads) {
        int64_t src = a.idx[r0 + i], dst = a.growth ? a.n + r0 + i : (int64_t)a.dest[r0 + i];
        if (src < 0 || src >= a.n || dst < 0 || dst >= limit) src = dst = -1;   // skipped
        s_src[i] = (int32_t)src; s_dst[i] = (int32_t)dst;
    }
    __syncthreads();
    for (int j = tid; j < count; j += kMcmcThreads) {
        const uint32_t x = off0 + (uint32_t)j;            // < width + kMcmcApplyElems <= 2^13
        const uint32_t q = w == 1u ? x : __umulhi(x, tb.magic);
        const uint32_t col = x - q * w;
        const int64_t src = s_src[q], dst = s_dst[q];
        if (src < 0) continue;
        float v = 0.0f;                                   // MOMENT (growth)
        if (tb.role == (uint32_t)LSR_MCMC_COPY) v = tb.p[src * w + col];
        else if (tb.role == (uint32_t)LSR_MCMC_OPACITY) v = a.stage[src].x;
        else if (tb.role == (uint32_t)LSR_MCMC_SCALING) { const float4 s = a.stage[src]; v = col == 0u ? s.y : col == 1u ? s.z : s.w; }
        tb.p[dst * w + col] = v;
    }
}

// ---- noise ----

__global__ __launch_bounds__(kMcmcThreads) void k_mcmc_noise(int64_t n, float *__restrict__ xyz, const float *__restrict__ opacity,
                                                            const float *__restrict__ scaling, const float *__restrict__ rotation,
                                                            const float *__restrict__ eps, float step_scale) {
    for (int64_t g = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x; g < n; g += (int64_t)gridDim.x * kMcmcThreads) {
        const float4 q = reinterpret_cast<const float4 *>(rotation)[g];
        const float *ls = scaling + 3 * g, *e = eps + 3 * g;
        float *p = xyz + 3 * g;
        const float op = opacity[g];
        const float l0 = ls[0], l1 = ls[1], l2 = ls[2], e0 = e[0], e1 = e[1], e2 = e[2];
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        // (1 - sigmoid(op)) - 0.995 = (0.005 - 0.995 ex) / (1 + ex) with ex = exp(op): the subtraction happens between numbers of
        // the size of 0.005, not of 1, which is worth two digits where the factor turns (it is multiplied by 100 and
        // exponentiated).  ex is kept finite (beyond op = 80 the factor is 0 either way: the outer exponential overflows).
        const float ex = expf(fminf(op, 80.0f));
        const float f = step_scale / (1.0f + expf(-100.0f * ((0.005f - 0.995f * ex) / (1.0f + ex))));
        const float inv = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        const float w = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
        const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
        const float r10 = 2.0f * (x * y + w * z), r11 = 1.0f - 2.0f * (x * x + z * z), r12 = 2.0f * (y * z - w * x);
        const float r20 = 2.0f * (x * z - w * y), r21 = 2.0f * (y * z + w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
        const float v0 = e0 * f, v1 = e1 * f, v2 = e2 * f;
        const float s0 = expf(l0), s1 = expf(l1), s2 = expf(l2);
        // Sigma v = R (s^2 * (R^T v))
        const float t0 = (r00 * v0 + r10 * v1 + r20 * v2) * (s0 * s0);
        const float t1 = (r01 * v0 + r11 * v1 + r21 * v2) * (s1 * s1);
        const float t2 = (r02 * v0 + r12 * v1 + r22 * v2) * (s2 * s2);
        const float i0 = r00 * t0 + r01 * t1 + r02 * t2;
        const float i1 = r10 * t0 + r11 * t1 + r12 * t2;
        const float i2 = r20 * t0 + r21 * t1 + r22 * t2;
        if (fabsf(i0) + fabsf(i1) + fabsf(i2) < INFINITY) {   // false for an infinite or NaN component
            p[0] = p0 + i0; p[1] = p1 + i1; p[2] = p2 + i2;
        }
    }
}

static int launched() {
    return launch_status();
}

}  // namespace lsr

using namespace lsr;

static_assert(LSR_MCMC_MAX_WIDTH + kMcmcApplyElems <= (1 << 13), "the reciprocal division of k_mcmc_dests");
static_assert((int64_t)kMcmcChunk * LSR_MCMC_MAX_WIDTH <= (1 << 20), "the reciprocal division of k_mcmc_sources");
static_assert(sizeof(McmcArgs) <= 4096, "kernel arguments");

extern "C" {

size_t lsr_mcmc_workspace_bytes(int64_t n, int64_t m) {
    (void)m;
    if (n <= 0) return 0;
    // sample: bases [chunks + 1] and cum [n] uint64; apply: stage [n] float4; classify: sums [chunks] uint32
    return (size_t)(mcmc_chunks(n) + 1) * sizeof(uint64_t) + (size_t)n * 16;
}

int lsr_mcmc_classify(int64_t n, const float *opacity, float dead_logit, float *weights, int32_t *dead, uint32_t *counts,
                      void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || n >= LSR_MCMC_MAX_ROWS || dead_logit != dead_logit || (dead == nullptr) != (counts == nullptr)) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!opacity || !weights || (dead && !workspace)) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = mcmc_chunks(n);                 // <= 2^20
    uint32_t *sums = dead ? (uint32_t *)workspace : nullptr;
    hipLaunchKernelGGL(k_mcmc_classify, dim3((unsigned)chunks), dim3(kMcmcChunk), 0, s, n, opacity, dead_logit, weights, sums);
    if (dead) {
        hipLaunchKernelGGL(k_mcmc_classify_scan, dim3(1), dim3(kMcmcScanThreads), 0, s, n, chunks, sums, counts);
        hipLaunchKernelGGL(k_mcmc_classify_emit, dim3((unsigned)chunks), dim3(kMcmcChunk), 0, s, n, opacity, dead_logit,
                           (const uint32_t *)sums, dead);
    }
    return launched();
}

int lsr_mcmc_sample(int64_t n, const float *weights, int64_t m, const double *uniforms, int32_t *idx, uint32_t *count,
                    uint64_t *total, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || n >= LSR_MCMC_MAX_ROWS || m < 0 || m >= (1ll << 31) || (n == 0 && m > 0)) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!weights || !count || !workspace || (m > 0 && (!uniforms || !idx))) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = mcmc_chunks(n);
    const SampleWorkspace ws = sample_workspace(workspace, n);
    hipLaunchKernelGGL(k_mcmc_sums, dim3((unsigned)chunks), dim3(kMcmcChunk), 0, s, n, weights, count, ws.bases);
    hipLaunchKernelGGL(k_mcmc_scan, dim3(1), dim3(kMcmcScanThreads), 0, s, chunks, ws.bases, total);
    hipLaunchKernelGGL(k_mcmc_cum, dim3((unsigned)chunks), dim3(kMcmcChunk), 0, s, n, weights, ws);
    if (m > 0)
        hipLaunchKernelGGL(k_mcmc_draw, dim3((unsigned)((m + kMcmcThreads - 1) / kMcmcThreads)), dim3(kMcmcThreads), 0, s, n, chunks, m,
                           uniforms, ws, idx, count);
    return launched();
}

int lsr_mcmc_apply(int64_t n, int64_t m, const int32_t *idx, const uint32_t *count, const int32_t *dest,
                   const lsr_mcmc_table *tables, int32_t num_tables, float min_opacity, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || m < 0 || n + m >= LSR_MCMC_MAX_ROWS || num_tables < 0 || num_tables > LSR_MCMC_MAX_TABLES) return LSR_EINVAL;
    if (!(min_opacity >= 0.0f && min_opacity < 1.0f)) return LSR_EINVAL;
    if (num_tables > 0 && !tables) return n > 0 ? LSR_ENULL : LSR_OK;
    int n_opacity = 0, n_scaling = 0;
    for (int i = 0; i < num_tables; ++i) {
        const lsr_mcmc_table &t = tables[i];
        if (t.role < LSR_MCMC_COPY || t.role > LSR_MCMC_MOMENT || t.width < 1 || t.width > LSR_MCMC_MAX_WIDTH) return LSR_EINVAL;
        if ((t.role == LSR_MCMC_OPACITY && t.width != 1) || (t.role == LSR_MCMC_SCALING && t.width != 3)) return LSR_EINVAL;
        n_opacity += t.role == LSR_MCMC_OPACITY;
        n_scaling += t.role == LSR_MCMC_SCALING;
    }
    if (n_opacity != 1 || n_scaling != 1) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!count || !workspace || (m > 0 && !idx)) return LSR_ENULL;
    McmcArgs a{};
    const bool growth = dest == nullptr;
    int64_t blocks = 0;
    for (int i = 0; i < num_tables; ++i) {
        const lsr_mcmc_table &t = tables[i];
        if (!t.table) return LSR_ENULL;
        McmcTable &d = a.t[i];
        d.p = t.table; d.width = (uint32_t)t.width; d.role = (uint32_t)t.role;
        d.magic = t.width >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)t.width - 1) / (uint64_t)t.width) : 0u;
        d.first_block = (uint32_t)blocks;
        if (growth || t.role != LSR_MCMC_MOMENT)          // a relocated row keeps its own moments
            blocks += (m * t.width + kMcmcApplyElems - 1) / kMcmcApplyElems;
        if (blocks > 0x7FFFFFFFll) return LSR_EINVAL;      // beyond one grid
        if (t.role == LSR_MCMC_OPACITY) a.opacity = t.table;
        if (t.role == LSR_MCMC_SCALING) a.scaling = t.table;
    }
    a.num_tables = num_tables; a.growth = growth ? 1 : 0; a.n = n; a.m = m; a.idx = idx; a.dest = dest; a.count = count;
    a.stage = (float4 *)workspace; a.min_opacity = (double)min_opacity;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mcmc_sources, dim3((unsigned)mcmc_chunks(n)), dim3(kMcmcChunk), 0, s, a);
    if (blocks > 0) hipLaunchKernelGGL(k_mcmc_dests, dim3((unsigned)blocks), dim3(kMcmcThreads), 0, s, a);
    return launched();
}

int lsr_mcmc_noise(int64_t n, float *xyz, const float *opacity, const float *scaling, const float *rotation,
                   const float *eps, float step_scale, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || n >= LSR_MCMC_MAX_ROWS || !std::isfinite(step_scale)) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!xyz || !opacity || !scaling || !rotation || !eps) return LSR_ENULL;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kMcmcThreads - 1) / kMcmcThreads, kMcmcMaxBlocks);
    hipLaunchKernelGGL(k_mcmc_noise, dim3(blocks), dim3(kMcmcThreads), 0, (hipStream_t)stream, n, xyz, opacity, scaling, rotation,
                       eps, step_scale);
    return launched();
}

}  // extern "C"
