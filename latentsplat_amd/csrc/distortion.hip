// distortion.hip — the depth distortion regulariser (include/lsr_distortion.h): the depth moments (m', m'^2) of every
// (view, Gaussian) pair on one side of the unchanged rasterizer, the image-space loss alpha M2 - M1^2 on the other.
//
// A, k_dist_cameras + k_dist_fwd / k_dist_bwd, shaped like operator A of normals.hip: one workgroup compacts what depends
// on the camera alone, in double, into a 48-byte record: z = <a, x> + a3 with a = row 2 of the view matrix and
// a3 = its translation / s (the view-space z of the scaled mean, divided by s, with the division folded into the record),
// kept as doubles; m = c0 + c1 u with u = z (LINEAR: c = (0, 1)), 1 / z (DISPARITY: (0, 1); NDC: (f / (f - n),
// -f n / (f - n))), and the pivot, as floats.  A lane owns a Gaussian (grid-stride beyond LSR_DIST_MAX_BLOCKS workgroups),
// loads xyz once and loops over the records, which arrive as scalar loads (the loop index is wave-uniform and the pointer
// const __restrict__).  Per pair: z is three double FMAs rounded to float32 ONCE (the dot product of a depth of several
// units is where a float32 chain loses its last bits, and everything after it magnifies them: m' = m - pivot is small
// by design; four double FMAs per 8 bytes stored are a twelfth of the card's double rate at the HBM rate), then in
// float32 at most one division, one FMA, one subtraction, one product, and one 8-byte store; the pass is bound by that
// store.  The backward walks the same loop, adds (g0 + 2 m' g1) dm/dz per view in order into one double per axis of the
// row: written, no atomics.
//
// B, k_distl_fwd + k_image_mean_finish / k_distl_bwd, shaped like depth_loss.hip: a workgroup of 256 lanes owns LSR_DIST_CHUNK
// consecutive pixels of one view, a lane groups of 4 consecutive pixels counted from the start of the VIEW: one 16-byte
// load per plane where the plane is 16-byte aligned and the group whole, single floats elsewhere; the assignment of
// pixels to lanes is the same either way, so a view gives the same bits alone and in a batch.  d = alpha M2 - M1^2 is
// formed in double (two products of float32 values are exact in double: the difference carries ONE rounding, whatever it
// cancels), summed per chunk in a fixed order (the lane's pixels in order, the wave butterfly, the four waves in order)
// into the chunk's own slot; the finish of lsr_image_sum.h adds the slots of an image.
#include <math.h>

#include <cmath>

#include "lsr_distortion.h"
#include "lsr_image_sum.h"

namespace lsr {

// ---------------------------------------------------------------- A ----

constexpr int kDistThreads = LSR_DIST_THREADS;
constexpr int kDistCamBytes = 48;

// One compacted camera as the passes read it: 48 bytes, scalar loads.
struct alignas(16) DistCam {
    double a0, a1, a2, a3;     // z = a0 x + a1 y + a2 z + a3
    float c0, c1;              // m = c0 + c1 u
    float pivot, pad;
};
static_assert(sizeof(DistCam) == kDistCamBytes, "a camera record is kDistCamBytes bytes");

__global__ __launch_bounds__(kDistThreads) void k_dist_cameras(int num_views, const float *__restrict__ views,
                                                               const float *__restrict__ pivot, int space,
                                                               DistCam *__restrict__ cams) {
    for (int v = threadIdx.x; v < num_views; v += kDistThreads) {
        const float *view = views + (size_t)v * LSR_VIEW_FLOATS;
        DistCam rec;
        rec.a0 = view[2]; rec.a1 = view[6]; rec.a2 = view[10];
        rec.a3 = (double)view[14] / (double)view[40];               // s = 0: not finite, the pairs write (0, 0)
        double c0 = 0.0, c1 = 1.0;
        if (space == LSR_DIST_NDC) {
            const double n = view[42], f = view[43];
            c0 = f / (f - n);                                       // n == f: not finite, the pairs write (0, 0)
            c1 = -c0 * n;
        }
        rec.c0 = (float)c0; rec.c1 = (float)c1;
        rec.pivot = pivot ? pivot[v] : 0.0f;
        rec.pad = 0.0f;
        cams[v] = rec;
    }
}

// One (view, Gaussian) pair: m' and dm/dz; false when the pair writes (0, 0).
template <bool LINEAR>
__device__ __forceinline__ bool dist_pair(const DistCam &c, float x, float y, float z, float &mp, float &dmdz) {
    const float zc = (float)fma(c.a0, (double)x, fma(c.a1, (double)y, fma(c.a2, (double)z, c.a3)));
    float m;
    if (LINEAR) {
        m = zc;
        dmdz = 1.0f;
    } else {
        const float u = 1.0f / zc;
        m = fmaf(c.c1, u, c.c0);
        dmdz = -c.c1 * u * u;
    }
    mp = m - c.pivot;
    // (m'^2 finite implies m' finite; zc > 0 is false for a NaN)
    return zc > 0.0f && isfinite(zc) && isfinite(mp * mp) && isfinite(dmdz);
}

template <bool LINEAR>
__global__ __launch_bounds__(kDistThreads) void k_dist_fwd(int n, const float *__restrict__ xyz, int num_views,
                                                           const DistCam *__restrict__ cams, float *__restrict__ moments) {
    const int64_t stride = (int64_t)gridDim.x * kDistThreads;
    for (int64_t g = (int64_t)blockIdx.x * kDistThreads + threadIdx.x; g < n; g += stride) {
        const float x = xyz[3 * g], y = xyz[3 * g + 1], z = xyz[3 * g + 2];
        for (int v = 0; v < num_views; ++v) {
            const DistCam c = cams[v];                   // wave-uniform: scalar loads
            float mp, dmdz;
            const bool ok = dist_pair<LINEAR>(c, x, y, z, mp, dmdz);
            reinterpret_cast<float2 *>(moments)[(size_t)v * (size_t)n + (size_t)g] = ok ? make_float2(mp, mp * mp) : make_float2(0.0f, 0.0f);
        }
    }
}

template <bool LINEAR>
__global__ __launch_bounds__(kDistThreads) void k_dist_bwd(int n, const float *__restrict__ xyz, int num_views,
                                                           const DistCam *__restrict__ cams,
                                                           const float *__restrict__ grad_moments, float *__restrict__ grad_xyz) {
    const int64_t stride = (int64_t)gridDim.x * kDistThreads;
    for (int64_t g = (int64_t)blockIdx.x * kDistThreads + threadIdx.x; g < n; g += stride) {
        const float x = xyz[3 * g], y = xyz[3 * g + 1], z = xyz[3 * g + 2];
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;             // dL/dxyz, the views added in order
        for (int v = 0; v < num_views; ++v) {
            const DistCam c = cams[v];
            float mp, dmdz;
            const bool ok = dist_pair<LINEAR>(c, x, y, z, mp, dmdz);
            const float2 up = reinterpret_cast<const float2 *>(grad_moments)[(size_t)v * (size_t)n + (size_t)g];
            const double k = ok ? ((double)up.x + 2.0 * (double)mp * (double)up.y) * (double)dmdz : 0.0;
            g0 += k * c.a0; g1 += k * c.a1; g2 += k * c.a2;
        }
        grad_xyz[3 * g] = (float)g0; grad_xyz[3 * g + 1] = (float)g1; grad_xyz[3 * g + 2] = (float)g2;
    }
}

static int dist_check(int64_t n, int32_t num_views, int32_t space) {
    if (n < 0 || n >= LSR_DIST_MAX_ROWS || num_views < 1 || num_views > LSR_DIST_MAX_VIEWS) return LSR_EINVAL;
    if (space != LSR_DIST_LINEAR && space != LSR_DIST_NDC && space != LSR_DIST_DISPARITY) return LSR_EINVAL;
    return LSR_OK;
}

static unsigned dist_blocks(int64_t n) {
    const int64_t b = (n + kDistThreads - 1) / kDistThreads;
    return (unsigned)(b < LSR_DIST_MAX_BLOCKS ? b : LSR_DIST_MAX_BLOCKS);
}

// ---------------------------------------------------------------- B ----

constexpr int kDistlThreads = 256;
constexpr int kDistlGroups = LSR_DIST_CHUNK / (4 * kDistlThreads);      // groups of 4 pixels per lane
static_assert(kDistlGroups * 4 * kDistlThreads == LSR_DIST_CHUNK, "a chunk is whole groups for every lane");

struct DistlShape {
    int64_t pixels;            // H W
    int chunks;                // per view
};

// four consecutive floats of a plane from pixel `at` (a multiple of 4), `left` = pixels of the plane from `at` on;
// entries past the plane read 0
__device__ __forceinline__ float4 distl_load4(const float *__restrict__ plane, int64_t at, int64_t left, bool aligned) {
    if (aligned && left >= 4) return *reinterpret_cast<const float4 *>(plane + at);
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (left > 0) r.x = plane[at];
    if (left > 1) r.y = plane[at + 1];
    if (left > 2) r.z = plane[at + 2];
    if (left > 3) r.w = plane[at + 3];
    return r;
}

__device__ __forceinline__ void distl_store4(float *__restrict__ plane, int64_t at, int64_t left, bool aligned, float4 v) {
    if (aligned && left >= 4) { *reinterpret_cast<float4 *>(plane + at) = v; return; }
    if (left > 0) plane[at] = v.x;
    if (left > 1) plane[at + 1] = v.y;
    if (left > 2) plane[at + 2] = v.z;
    if (left > 3) plane[at + 3] = v.w;
}

__device__ __forceinline__ bool distl_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct DistlFwdArgs {
    DistlShape s;
    const float *moment_map, *alpha, *weight;      // weight optional
    double *slots;                                  // [V][chunks]
    float *distortion;                              // optional
};

__global__ __launch_bounds__(kDistlThreads) void k_distl_fwd(DistlFwdArgs a) {
    __shared__ double s_red[kDistlThreads / LSR_WAVE][1];
    const int image = (int)(blockIdx.x / (uint32_t)a.s.chunks), chunk = (int)(blockIdx.x % (uint32_t)a.s.chunks);
    const int64_t P = a.s.pixels;
    const float *M1 = a.moment_map + 2 * P * image, *M2 = M1 + P, *A = a.alpha + P * image;
    const float *Wt = a.weight ? a.weight + P * image : nullptr;
    float *Dm = a.distortion ? a.distortion + P * image : nullptr;
    const bool al1 = distl_aligned(M1), al2 = distl_aligned(M2), ala = distl_aligned(A), alw = distl_aligned(Wt), ald = distl_aligned(Dm);
    double sum[1] = {0.0};
#pragma unroll
    for (int k = 0; k < kDistlGroups; ++k) {
        const int64_t at = (int64_t)chunk * LSR_DIST_CHUNK + ((int64_t)k * kDistlThreads + threadIdx.x) * 4;
        const int64_t left = P - at;
        if (left <= 0) continue;
        const float4 m1 = distl_load4(M1, at, left, al1), m2 = distl_load4(M2, at, left, al2), al = distl_load4(A, at, left, ala);
        const float4 w = Wt ? distl_load4(Wt, at, left, alw) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        const double d0 = (double)al.x * (double)m2.x - (double)m1.x * (double)m1.x;
        const double d1 = (double)al.y * (double)m2.y - (double)m1.y * (double)m1.y;
        const double d2 = (double)al.z * (double)m2.z - (double)m1.z * (double)m1.z;
        const double d3 = (double)al.w * (double)m2.w - (double)m1.w * (double)m1.w;
        // (entries past the plane hold 0 and add 0)
        sum[0] += (double)w.x * d0; sum[0] += (double)w.y * d1; sum[0] += (double)w.z * d2; sum[0] += (double)w.w * d3;
        if (Dm) distl_store4(Dm, at, left, ald, make_float4((float)d0, (float)d1, (float)d2, (float)d3));
    }
    block_sum<kDistlThreads, 1>(sum, s_red, a.slots + blockIdx.x);
}

struct DistlUnit {};       // this unit's k_image_mean_finish

struct DistlBwdArgs {
    DistlShape s;
    double inv_count;          // 1 / (V H W)
    const float *moment_map, *alpha, *weight, *grad_loss;
    float *grad_moment_map, *grad_alpha;           // each optional
};

__global__ __launch_bounds__(kDistlThreads) void k_distl_bwd(DistlBwdArgs a) {
    const int image = (int)(blockIdx.x / (uint32_t)a.s.chunks), chunk = (int)(blockIdx.x % (uint32_t)a.s.chunks);
    const int64_t P = a.s.pixels;
    const float *M1 = a.moment_map + 2 * P * image, *M2 = M1 + P, *A = a.alpha + P * image;
    const float *Wt = a.weight ? a.weight + P * image : nullptr;
    float *G1 = a.grad_moment_map ? a.grad_moment_map + 2 * P * image : nullptr, *G2 = G1 ? G1 + P : nullptr;
    float *GA = a.grad_alpha ? a.grad_alpha + P * image : nullptr;
    const bool al1 = distl_aligned(M1), al2 = distl_aligned(M2), ala = distl_aligned(A), alw = distl_aligned(Wt);
    const bool alg1 = distl_aligned(G1), alg2 = distl_aligned(G2), alga = distl_aligned(GA);
    const double up = (double)*a.grad_loss * a.inv_count;
#pragma unroll
    for (int k = 0; k < kDistlGroups; ++k) {
        const int64_t at = (int64_t)chunk * LSR_DIST_CHUNK + ((int64_t)k * kDistlThreads + threadIdx.x) * 4;
        const int64_t left = P - at;
        if (left <= 0) continue;
        const float4 w = Wt ? distl_load4(Wt, at, left, alw) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        const double g0 = up * (double)w.x, g1 = up * (double)w.y, g2 = up * (double)w.z, g3 = up * (double)w.w;
        if (G1) {
            const float4 m1 = distl_load4(M1, at, left, al1), al = distl_load4(A, at, left, ala);
            distl_store4(G1, at, left, alg1, make_float4((float)(-2.0 * g0 * (double)m1.x), (float)(-2.0 * g1 * (double)m1.y),
                                                      (float)(-2.0 * g2 * (double)m1.z), (float)(-2.0 * g3 * (double)m1.w)));
            distl_store4(G2, at, left, alg2, make_float4((float)(g0 * (double)al.x), (float)(g1 * (double)al.y),
                                                      (float)(g2 * (double)al.z), (float)(g3 * (double)al.w)));
        }
        if (GA) {
            const float4 m2 = distl_load4(M2, at, left, al2);
            distl_store4(GA, at, left, alga, make_float4((float)(g0 * (double)m2.x), (float)(g1 * (double)m2.y),
                                                      (float)(g2 * (double)m2.z), (float)(g3 * (double)m2.w)));
        }
    }
}

// LSR_OK, or why these dims are refused
static int distl_check(const lsr_distortion_dims *d) {
    if (d->num_images < 1 || d->height < 1 || d->width < 1) return LSR_EINVAL;
    if (d->reserved0 || d->reserved1 || d->reserved2) return LSR_EINVAL;
    if (2 * (int64_t)d->num_images * d->height * d->width >= ((int64_t)1 << 31)) return LSR_EUNSUPPORTED;
    return LSR_OK;
}

static DistlShape distl_shape(const lsr_distortion_dims &d) {
    const int64_t pixels = (int64_t)d.height * d.width;
    return DistlShape{pixels, (int)((pixels + LSR_DIST_CHUNK - 1) / LSR_DIST_CHUNK)};
}

}  // namespace lsr

using namespace lsr;

extern "C" {

size_t lsr_scene_depth_moments_workspace_bytes(int64_t n, int32_t num_views) {
    if (n <= 0 || dist_check(n, num_views, LSR_DIST_LINEAR) != LSR_OK) return 0;
    return (size_t)num_views * kDistCamBytes;
}

int lsr_scene_depth_moments_forward(int64_t n, const float *xyz, int32_t num_views, const float *views, const float *pivot,
                                    int32_t space, float *moments, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    const int rc = dist_check(n, num_views, space);
    if (rc) return rc;
    if (n == 0) return LSR_OK;
    if (!xyz || !views || !moments || !workspace) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(moments) & 7)) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dist_cameras, dim3(1), dim3(kDistThreads), 0, s, (int)num_views, views, pivot, (int)space,
                       (DistCam *)workspace);
    if (space == LSR_DIST_LINEAR)
        hipLaunchKernelGGL(k_dist_fwd<true>, dim3(dist_blocks(n)), dim3(kDistThreads), 0, s, (int)n, xyz, (int)num_views,
                           (const DistCam *)workspace, moments);
    else
        hipLaunchKernelGGL(k_dist_fwd<false>, dim3(dist_blocks(n)), dim3(kDistThreads), 0, s, (int)n, xyz, (int)num_views,
                           (const DistCam *)workspace, moments);
    return launch_status();
}

int lsr_scene_depth_moments_backward(int64_t n, const float *xyz, int32_t num_views, const float *views, const float *pivot,
                                     int32_t space, const float *grad_moments, float *grad_xyz, void *workspace,
                                     lsr_stream_t stream) {
    note_hip_error(0);
    const int rc = dist_check(n, num_views, space);
    if (rc) return rc;
    if (n == 0) return LSR_OK;
    if (!xyz || !views || !grad_moments || !grad_xyz || !workspace) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(grad_moments) & 7)) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dist_cameras, dim3(1), dim3(kDistThreads), 0, s, (int)num_views, views, pivot, (int)space,
                       (DistCam *)workspace);
    if (space == LSR_DIST_LINEAR)
        hipLaunchKernelGGL(k_dist_bwd<true>, dim3(dist_blocks(n)), dim3(kDistThreads), 0, s, (int)n, xyz, (int)num_views,
                           (const DistCam *)workspace, grad_moments, grad_xyz);
    else
        hipLaunchKernelGGL(k_dist_bwd<false>, dim3(dist_blocks(n)), dim3(kDistThreads), 0, s, (int)n, xyz, (int)num_views,
                           (const DistCam *)workspace, grad_moments, grad_xyz);
    return launch_status();
}

size_t lsr_distortion_loss_workspace_bytes(const lsr_distortion_dims *dims) {
    if (!dims || distl_check(dims) != LSR_OK) return 0;
    return align_up((size_t)dims->num_images * (size_t)distl_shape(*dims).chunks * sizeof(double));
}

int lsr_distortion_loss_forward(const lsr_distortion_dims *dims, const float *moment_map, const float *alpha,
                                const float *weight, void *workspace, float *loss, float *per_view, float *distortion,
                                lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !moment_map || !alpha || !workspace) return LSR_ENULL;
    const int rc = distl_check(dims);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const DistlShape shape = distl_shape(*dims);
    DistlFwdArgs a{shape, moment_map, alpha, weight, (double *)workspace, distortion};
    // (blocks: at most V H W / 2048 + V < 2^21)
    hipLaunchKernelGGL(k_distl_fwd, dim3((unsigned)dims->num_images * (unsigned)shape.chunks), dim3(kDistlThreads), 0, s, a);
    if (loss || per_view)
        hipLaunchKernelGGL(k_image_mean_finish<DistlUnit>, dim3(1), dim3(kFinishThreads), 0, s, (const double *)workspace, dims->num_images,
                           shape.chunks, 1.0 / (double)shape.pixels, loss, per_view);
    return launch_status();
}

int lsr_distortion_loss_backward(const lsr_distortion_dims *dims, const float *moment_map, const float *alpha,
                                 const float *weight, const float *grad_loss, float *grad_moment_map, float *grad_alpha,
                                 lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !moment_map || !alpha || !grad_loss) return LSR_ENULL;
    const int rc = distl_check(dims);
    if (rc) return rc;
    if (!grad_moment_map && !grad_alpha) return LSR_OK;
    const DistlShape shape = distl_shape(*dims);
    DistlBwdArgs a{shape, 1.0 / ((double)dims->num_images * (double)shape.pixels), moment_map, alpha, weight, grad_loss,
                grad_moment_map, grad_alpha};
    hipLaunchKernelGGL(k_distl_bwd, dim3((unsigned)dims->num_images * (unsigned)shape.chunks), dim3(kDistlThreads), 0,
                       (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
