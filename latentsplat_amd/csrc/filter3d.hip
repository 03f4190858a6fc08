// filter3d.hip — the 3D smoothing filter of Mip-Splatting (include/lsr_filter3d.h): per Gaussian the smallest size the
// training cameras can resolve, sqrt(variance) over the highest sampling rate (focal length over depth) among the cameras
// that see it.  A (Gaussians x cameras) pass: 3 M x 200 is 6e8 pairs, and all a pair needs from memory is 12 bytes of
// position, once per Gaussian, so the pass is bound by its vector instructions, not by bandwidth.
//
// k_filter3d_cameras, one workgroup: everything that depends on the camera alone is evaluated once, in double, and stored
// as a compacted record of kCamFloats floats: the three rows of W diag(s) (so that p is three FMAs per component, with
// the scene scale folded in), the two frustum limits (1 + 2 margin) tanfov, and the factor k that turns p.z into the
// quantity to minimise: 1 / s (PUBLISHED) or 1 / (s focal_v) (PER_VIEW).  The final factor c (sqrt(variance) / F, or
// sqrt(variance)) and the cleared maximum go into the workspace header.  The mode lives here alone.
// k_filter3d_pass: a lane owns kFilterRows Gaussians (rows tid, tid + 256, ... of its workgroup's 1024: each access of a
// wave is contiguous), their positions in registers for the whole camera loop; one workgroup per 1024 rows, no grid cap
// (at most 2^18 workgroups, which the hardware balances).  The loop index is wave-uniform and the records are read through
// a const __restrict__ pointer: they arrive as scalar loads, one 64-byte s_load_dwordx16 per camera and wave, never as
// per-lane loads, and one record serves the 4 x 64 pairs of the wave (one row per lane, the record fetched in five
// pieces and a capped strided grid took 0.378 ms at 3 M x 200 with the same vector work per pair; the figure of this
// version is in DESIGN.md section 2.16).  Per pair: nine FMAs, two
// products for the limits, four compares, one product and one select, with no branch.  A seen Gaussian writes min * c; an
// unseen one writes the sentinel -1.  Each wave reduces the bit patterns of its seen filters (non-negative floats order as unsigned
// integers) and issues one integer atomicMax: order-independent, so two calls give the same bits.
// k_filter3d_unseen replaces the sentinels by the maximum (0 when nothing was seen: the header starts at 0).
#include <math.h>

#include <algorithm>
#include <cmath>

#include "lsr_filter3d.h"
#include "lsr_wave.h"

namespace lsr {

constexpr int kFilterThreads = 256;
constexpr int kFilterRows = 4;             // Gaussians per lane of the pass: one camera record serves 4 x 64 pairs of a wave
constexpr int kFilterMaxBlocks = 2048;     // k_filter3d_unseen: 256 CUs x 8 resident workgroups, rows strided over the grid
constexpr int kCamFloats = 16;             // ax[3] tx  ay[3] ty  az[3] tz  limit_x limit_y k 0
constexpr int kHeaderBytes = 64;           // uint32 max bits, float c

struct FilterHeader {
    uint32_t max_bits;     // the largest filter among the seen Gaussians, as the bits of a non-negative float
    float c;               // filter = (min over valid v of p.z k_v) * c
};

__global__ __launch_bounds__(kFilterThreads) void k_filter3d_cameras(int num_views, const float *__restrict__ views, int width,
                                                                     float margin, float variance, int mode,
                                                                     FilterHeader *__restrict__ header, float *__restrict__ cams) {
    __shared__ double s_focal[kFilterThreads];
    const int tid = threadIdx.x;
    const double spread = 1.0 + 2.0 * (double)margin;
    const float nan = __builtin_nanf("");
    double focal_max = 0.0;
    for (int v = tid; v < num_views; v += kFilterThreads) {
        const float *view = views + (size_t)v * LSR_VIEW_FLOATS;
        float *rec = cams + (size_t)v * kCamFloats;
        const float s = view[40], tx = view[35], ty = view[36];
        const bool usable = s > 0.0f && tx > 0.0f && ty > 0.0f && isfinite(s) && isfinite(tx) && isfinite(ty);
        if (!usable) {                                   // sees nothing: every compare with a NaN fails
#pragma unroll
            for (int i = 0; i < kCamFloats; ++i) rec[i] = nan;
            continue;
        }
        const double focal = (double)width / (2.0 * (double)tx);
        focal_max = focal > focal_max ? focal : focal_max;
#pragma unroll
        for (int r = 0; r < 3; ++r) {                    // row r of W: slots r, 4 + r, 8 + r, 12 + r
            rec[4 * r + 0] = view[r] * s;
            rec[4 * r + 1] = view[4 + r] * s;
            rec[4 * r + 2] = view[8 + r] * s;
            rec[4 * r + 3] = view[12 + r];
        }
        rec[12] = (float)(spread * (double)tx);
        rec[13] = (float)(spread * (double)ty);
        rec[14] = (float)(mode == LSR_FILTER3D_PER_VIEW ? 1.0 / ((double)s * focal) : 1.0 / (double)s);
        rec[15] = 0.0f;
    }
    s_focal[tid] = focal_max;
    __syncthreads();
    for (int step = kFilterThreads / 2; step > 0; step >>= 1) {
        if (tid < step) s_focal[tid] = s_focal[tid] > s_focal[tid + step] ? s_focal[tid] : s_focal[tid + step];
        __syncthreads();
    }
    if (tid == 0) {
        const double F = s_focal[0], sd = sqrt((double)variance);
        header->max_bits = 0u;
        header->c = mode == LSR_FILTER3D_PER_VIEW ? (float)sd : (F > 0.0 ? (float)(sd / F) : 0.0f);
    }
}

// One compacted camera as the pass reads it: 64 bytes, one scalar load.
struct alignas(64) FilterCam {
    float ax[4], ay[4], az[4];     // rows of W diag(s) with the translation in [3]
    float limit_x, limit_y, k, pad;
};
static_assert(sizeof(FilterCam) == kCamFloats * sizeof(float), "a camera record is kCamFloats floats");

__global__ __launch_bounds__(kFilterThreads) void k_filter3d_pass(int n, const float *__restrict__ xyz, int num_views,
                                                                  const FilterCam *__restrict__ cams, const FilterHeader *header,
                                                                  uint32_t *max_bits, float *__restrict__ filter,
                                                                  uint8_t *__restrict__ seen) {
    constexpr int R = kFilterRows;
    const float c = header->c;
    const int g0 = blockIdx.x * (kFilterThreads * R) + threadIdx.x;      // rows g0 + j * kFilterThreads: coalesced per j
    float x[R], y[R], z[R], best[R];
    bool any[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int g = g0 + j * kFilterThreads;
        const bool in = g < n;                           // a row past the end is a NaN: never valid, never stored
        x[j] = in ? xyz[3 * (size_t)g] : __builtin_nanf("");
        y[j] = in ? xyz[3 * (size_t)g + 1] : 0.0f;
        z[j] = in ? xyz[3 * (size_t)g + 2] : 0.0f;
        best[j] = INFINITY;
        any[j] = false;
    }
#pragma unroll 2
    for (int v = 0; v < num_views; ++v) {
        const FilterCam r = cams[v];                     // wave-uniform: one 64-byte scalar load
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const float px = fmaf(r.ax[0], x[j], fmaf(r.ax[1], y[j], fmaf(r.ax[2], z[j], r.ax[3])));
            const float py = fmaf(r.ay[0], x[j], fmaf(r.ay[1], y[j], fmaf(r.ay[2], z[j], r.ay[3])));
            const float pz = fmaf(r.az[0], x[j], fmaf(r.az[1], y[j], fmaf(r.az[2], z[j], r.az[3])));
            const float t = pz * r.k;
            // (no short circuit: the body has no branch)
            const bool ok = (int)(pz > 0.2f) & (int)(fabsf(px) <= r.limit_x * pz) & (int)(fabsf(py) <= r.limit_y * pz);
            best[j] = ((int)ok & (int)(t < best[j])) ? t : best[j];
            any[j] |= ok;
        }
    }
    uint32_t mine = 0u;                                  // bits of the largest seen filter of this lane
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int g = g0 + j * kFilterThreads;
        const bool is_seen = any[j] && best[j] < INFINITY;       // a smallest depth that is not finite (an infinite position): unseen
        const float f = best[j] * c;
        if (g < n) {
            filter[g] = is_seen ? f : -1.0f;
            if (seen) seen[g] = is_seen ? 1 : 0;
        }
        const uint32_t bits = is_seen ? __float_as_uint(f) : 0u;
        mine = bits > mine ? bits : mine;
    }
    mine = wave_all(mine, Max());
    if ((threadIdx.x & (LSR_WAVE - 1)) == 0 && mine) atomicMax(max_bits, mine);
}

__global__ __launch_bounds__(kFilterThreads) void k_filter3d_unseen(int n, const FilterHeader *__restrict__ header, float *filter) {
    const float fallback = __uint_as_float(header->max_bits);
    for (int g = blockIdx.x * kFilterThreads + threadIdx.x; g < n; g += gridDim.x * kFilterThreads)
        if (__float_as_uint(filter[g]) == 0xbf800000u) filter[g] = fallback;      // the sentinel -1: no seen filter is negative
}

static bool views_in_range(int32_t num_views) { return num_views >= 1 && num_views <= LSR_FILTER3D_MAX_VIEWS; }

}  // namespace lsr

using namespace lsr;

extern "C" {

size_t lsr_filter3d_workspace_bytes(int64_t n, int32_t num_views) {
    if (n <= 0 || !views_in_range(num_views)) return 0;
    return (size_t)kHeaderBytes + (size_t)num_views * kCamFloats * sizeof(float);
}

int lsr_filter3d_compute(int64_t n, const float *xyz, int32_t num_views, const float *views, int32_t width, float margin,
                         float variance, int32_t mode, float *filter, uint8_t *seen, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || n >= LSR_FILTER3D_MAX_ROWS || !views_in_range(num_views) || width < 1) return LSR_EINVAL;
    if (!std::isfinite(margin) || margin < 0.0f || !std::isfinite(variance) || !(variance > 0.0f)) return LSR_EINVAL;
    if (mode != LSR_FILTER3D_PUBLISHED && mode != LSR_FILTER3D_PER_VIEW) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!xyz || !views || !filter || !workspace) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    FilterHeader *header = (FilterHeader *)workspace;
    float *cams = (float *)((char *)workspace + kHeaderBytes);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kFilterThreads - 1) / kFilterThreads, kFilterMaxBlocks);
    constexpr int kPassRows = kFilterThreads * kFilterRows;
    const unsigned pass_blocks = (unsigned)((n + kPassRows - 1) / kPassRows);      // <= 2^18: no cap, the hardware balances them
    hipLaunchKernelGGL(k_filter3d_cameras, dim3(1), dim3(kFilterThreads), 0, s, (int)num_views, views, (int)width, margin, variance,
                       (int)mode, header, cams);
    hipLaunchKernelGGL(k_filter3d_pass, dim3(pass_blocks), dim3(kFilterThreads), 0, s, (int)n, xyz, (int)num_views, (const FilterCam *)cams,
                       (const FilterHeader *)header, &header->max_bits, filter, seen);
    hipLaunchKernelGGL(k_filter3d_unseen, dim3(blocks), dim3(kFilterThreads), 0, s, (int)n, (const FilterHeader *)header, filter);
    return launch_status();
}

}  // extern "C"
