// depth_loss.hip — the inverse-depth loss of a trainable 3DGS scene (include/lsr_depth_loss.h is the contract): an L1
// between s alpha / depth of the rendered pair and an affine image of a target, per view, and its gradient.
//
// A streaming operator: 12 bytes per pixel forward (depth, alpha, target; 16 with a weight; 4 more when the map is wanted),
// 8 more written backward.  Shape of every pass:
//   * a workgroup of 256 lanes owns kChunk = 2048 consecutive pixels of ONE view: blockIdx.x = view * chunks + chunk;
//   * a lane owns the groups of 4 pixels g = lane, lane + 256 of the chunk, counted from the start of the view.  Whether a
//     group moves as 16-byte accesses or as floats is decided per view from the planes' addresses (dl_load_group; every
//     output plane for itself, dl_store): the assignment of pixels to lanes, and with it the order of every sum, is the
//     same either way, so a view gives the same bits alone, in a batch, and from a misaligned plane (H W % 4 != 0);
//   * the per-pixel arithmetic is in double (the division included: the pass stays bound by its loads);
//   * a lane adds its pixels in index order; the workgroup's sums are block_sum of lsr_wave.h (the wave butterfly, then
//     the four waves in order), written to the workgroup's own slot;
//   * a finishing launch gives a wave to a view (lsr_image_sum.h: lane l adds the slots l, l + 64, ... in order, then the
//     butterfly).
// The per-view table (a, b, 1 / N_v) is written by the finishing launches and read by the main pass (FIT) and the backward.
// No atomics, no allocation, nothing read back.
#include <float.h>
#include <math.h>

#include <cmath>

#include "lsr_depth_loss.h"
#include "lsr_image_sum.h"

namespace lsr {

constexpr int kDlThreads = 256;
constexpr int kDlChunk = LSR_DEPTH_LOSS_CHUNK;
constexpr int kDlGroups = kDlChunk / 4 / kDlThreads;     // groups of 4 pixels per lane: 2
constexpr int kDlWaves = kDlThreads / LSR_WAVE;
constexpr int kDlTable = 4;                              // doubles per view: a, b, 1 / N_v (0: the row gives nothing), N_v
constexpr int kDlMoments = 6;                            // count of w > 0, sums of w, w t, w I, w t^2, w t I
static_assert(kDlChunk == 4 * kDlThreads * kDlGroups, "a chunk is whole groups for every lane");

struct DlShape {
    int V, pixels, chunks;     // pixels = H W; chunks = workgroups per view
};

typedef float f32x4 __attribute__((ext_vector_type(4)));     // a native 128-bit value (float4 is a struct: no register constraint takes it)

// The n <= 4 floats from p + i (i counted in the plane p, a multiple of 4), one at a time; lanes beyond n read nothing and
// hold 0.
__device__ __forceinline__ float4 dl_load_single(const float *__restrict__ p, int i, int n) {
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (n > 0) r.x = p[i];
    if (n > 1) r.y = p[i + 1];
    if (n > 2) r.z = p[i + 2];
    if (n > 3) r.w = p[i + 3];
    return r;
}

// One group of 4 pixels of the three or four input planes.
struct DlGroup {
    float4 depth, alpha, target, weight;
};

// vec (the same in every lane of the workgroup): every input plane of this view is 16-byte aligned.  A whole group then
// moves as one 16-byte load per array, all of them issued before the first is waited for; elsewhere single loads.
// (The empty asm keeps each quad one 128-bit value, and being ONE statement it waits for the loads together.  Without it
// the compiler splits every 16-byte access into four, merges them with the single accesses of the other branch, and the
// pass moves 4 bytes per lane everywhere.)
__device__ __forceinline__ DlGroup dl_load_group(const float *__restrict__ depth, const float *__restrict__ alpha,
                                                 const float *__restrict__ target, const float *__restrict__ weight, bool vec,
                                                 int i, int n) {
    DlGroup g;
    if (vec && n == 4) {
        f32x4 d = *reinterpret_cast<const f32x4 *>(depth + i), a = *reinterpret_cast<const f32x4 *>(alpha + i),
              t = *reinterpret_cast<const f32x4 *>(target + i), w = {0.0f, 0.0f, 0.0f, 0.0f};
        if (weight) w = *reinterpret_cast<const f32x4 *>(weight + i);
        asm("" : "+v"(d), "+v"(a), "+v"(t), "+v"(w));
        g.depth = make_float4(d.x, d.y, d.z, d.w);
        g.alpha = make_float4(a.x, a.y, a.z, a.w);
        g.target = make_float4(t.x, t.y, t.z, t.w);
        g.weight = make_float4(w.x, w.y, w.z, w.w);
    } else {
        g.depth = dl_load_single(depth, i, n);
        g.alpha = dl_load_single(alpha, i, n);
        g.target = dl_load_single(target, i, n);
        g.weight = weight ? dl_load_single(weight, i, n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return g;
}

__device__ __forceinline__ void dl_store(float *__restrict__ p, bool aligned, int i, int n, float4 v) {
    if (aligned && n == 4) {
        f32x4 q = {v.x, v.y, v.z, v.w};
        asm("" : "+v"(q));
        *reinterpret_cast<f32x4 *>(p + i) = q;
        return;
    }
    if (n > 0) p[i] = v.x;
    if (n > 1) p[i + 1] = v.y;
    if (n > 2) p[i + 2] = v.z;
    if (n > 3) p[i + 3] = v.w;
}

__device__ __forceinline__ bool dl_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// I of one pixel, in double; *defined: the pixel passes the gate
__device__ __forceinline__ double dl_inverse(float depth, float alpha, float alpha_min, double s, bool *defined) {
    // (NaN fails every comparison; +inf fails the upper bounds)
    const bool ok = alpha > alpha_min && alpha <= FLT_MAX && depth > 0.0f && depth <= FLT_MAX;
    *defined = ok;
    return ok ? s * (double)alpha / (double)depth : 0.0;
}

__device__ __forceinline__ double dl_weight(bool has_weight, float weight, float target) {
    return has_weight ? (double)weight : (target > 0.0f ? 1.0 : 0.0);
}

// the view, the first pixel of this workgroup's chunk in it
__device__ __forceinline__ void dl_chunk(const DlShape &s, int &view, int &first) {
    const uint32_t b = blockIdx.x, per = (uint32_t)s.chunks;
    const uint32_t v = b / per;
    view = (int)v;
    first = (int)(b - v * per) * kDlChunk;
}

struct DlArgs {
    DlShape s;
    float alpha_min;
    int fit;                       // the main pass: (a, b) from the table; else from affine_in (NULL: 1, 0)
    const float *depth, *alpha, *views, *target, *weight, *affine_in;
    double *table;                 // [V][kDlTable]
    double *slots;                 // [V * chunks][2 or kDlMoments]
    float *inverse_depth;          // optional
};

// FIT, first pass: the moments of (w, target, I) per chunk.
__global__ __launch_bounds__(kDlThreads) void k_dl_moments(DlArgs a) {
    __shared__ double s_red[kDlWaves][kDlMoments];
    int view, first;
    dl_chunk(a.s, view, first);
    const int64_t base = (int64_t)view * a.s.pixels;
    const float *depth = a.depth + base, *alpha = a.alpha + base, *target = a.target + base;
    const float *weight = a.weight ? a.weight + base : nullptr;
    const bool vec = dl_aligned(depth) && dl_aligned(alpha) && dl_aligned(target) && dl_aligned(weight);
    const double s = (double)a.views[(size_t)view * LSR_VIEW_FLOATS + 40];
    double m[kDlMoments] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < kDlGroups; ++g) {
        const int i = first + 4 * (g * kDlThreads + (int)threadIdx.x);
        const int n = min(4, a.s.pixels - i);
        if (n <= 0) continue;
        const DlGroup q = dl_load_group(depth, alpha, target, weight, vec, i, n);
        const float d[4] = {q.depth.x, q.depth.y, q.depth.z, q.depth.w}, al[4] = {q.alpha.x, q.alpha.y, q.alpha.z, q.alpha.w},
                    t[4] = {q.target.x, q.target.y, q.target.z, q.target.w}, wt[4] = {q.weight.x, q.weight.y, q.weight.z, q.weight.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= n) break;
            bool defined;
            const double I = dl_inverse(d[k], al[k], a.alpha_min, s, &defined);
            const double w = dl_weight(weight != nullptr, wt[k], t[k]), tt = (double)t[k];
            m[0] += w > 0.0 ? 1.0 : 0.0;
            m[1] += w;
            m[2] += w * tt;
            m[3] += w * I;
            m[4] += w * tt * tt;
            m[5] += w * tt * I;
        }
    }
    block_sum<kDlThreads, kDlMoments>(m, s_red, a.slots + (size_t)blockIdx.x * kDlMoments);
}

// FIT, second pass: a wave per view adds the view's moment slots and solves the 2 x 2 system.
__global__ __launch_bounds__(kDlThreads) void k_dl_fit(const double *__restrict__ slots, DlShape s, double *__restrict__ table,
                                                      float *__restrict__ affine_out) {
    const int view = (int)blockIdx.x * kDlWaves + (int)(threadIdx.x / LSR_WAVE), lane = threadIdx.x & (LSR_WAVE - 1);
    if (view >= s.V) return;                       // (a whole wave leaves: the butterfly below has all its lanes)
    double m[kDlMoments];
    image_slot_sums<kDlMoments>(slots + (size_t)view * s.chunks * kDlMoments, s.chunks, m);
    if (lane != 0) return;
    const double count = m[0], Sw = m[1], St = m[2], SI = m[3], Stt = m[4], StI = m[5];
    double fa = 0.0, fb = 0.0;
    // det / Sw^2 is the weighted variance of the target, Stt / Sw its weighted mean square
    const double det = Sw * Stt - St * St;
    if (count >= 2.0 && Sw > 0.0 && det > 0x1p-24 * (Sw * Stt)) {
        fa = (Sw * StI - St * SI) / det;
        fb = (SI - fa * St) / Sw;
        if (!(isfinite(fa) && isfinite(fb))) { fa = 0.0; fb = 0.0; }
    }
    if (fa == 0.0) fb = 0.0;
    table[(size_t)view * kDlTable] = fa;
    table[(size_t)view * kDlTable + 1] = fb;
    if (affine_out) { affine_out[2 * view] = (float)fa; affine_out[2 * view + 1] = (float)fb; }
}

// The main pass: sums of |r| and of w per chunk, and the map.
__global__ __launch_bounds__(kDlThreads) void k_dl_fwd(DlArgs a) {
    __shared__ double s_red[kDlWaves][2];
    int view, first;
    dl_chunk(a.s, view, first);
    const int64_t base = (int64_t)view * a.s.pixels;
    const float *depth = a.depth + base, *alpha = a.alpha + base, *target = a.target + base;
    const float *weight = a.weight ? a.weight + base : nullptr;
    float *map = a.inverse_depth ? a.inverse_depth + base : nullptr;
    const bool vec = dl_aligned(depth) && dl_aligned(alpha) && dl_aligned(target) && dl_aligned(weight), al_m = dl_aligned(map);
    const double s = (double)a.views[(size_t)view * LSR_VIEW_FLOATS + 40];
    double fa = 1.0, fb = 0.0;
    if (a.fit) { fa = a.table[(size_t)view * kDlTable]; fb = a.table[(size_t)view * kDlTable + 1]; }
    else if (a.affine_in) { fa = (double)a.affine_in[2 * view]; fb = (double)a.affine_in[2 * view + 1]; }
    double sums[2] = {0.0, 0.0};
#pragma unroll
    for (int g = 0; g < kDlGroups; ++g) {
        const int i = first + 4 * (g * kDlThreads + (int)threadIdx.x);
        const int n = min(4, a.s.pixels - i);
        if (n <= 0) continue;
        const DlGroup q = dl_load_group(depth, alpha, target, weight, vec, i, n);
        const float d[4] = {q.depth.x, q.depth.y, q.depth.z, q.depth.w}, al[4] = {q.alpha.x, q.alpha.y, q.alpha.z, q.alpha.w},
                    t[4] = {q.target.x, q.target.y, q.target.z, q.target.w}, wt[4] = {q.weight.x, q.weight.y, q.weight.z, q.weight.w};
        float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= n) break;
            bool defined;
            const double I = dl_inverse(d[k], al[k], a.alpha_min, s, &defined);
            const double w = dl_weight(weight != nullptr, wt[k], t[k]);
            sums[0] += fabs(w * (I - (fa * (double)t[k] + fb)));
            sums[1] += w;
            out[k] = (float)I;
        }
        if (map) dl_store(map, al_m, i, n, make_float4(out[0], out[1], out[2], out[3]));
    }
    block_sum<kDlThreads, 2>(sums, s_red, a.slots + (size_t)blockIdx.x * 2);
}

// The finish of lsr_image_sum.h in its order, with the loop written out here: wave w finishes the views w, w + 16, ...
// (image_slot_sums), reads and writes the view's table row and per_view; thread 0 then adds the waves' totals in order
// for the loss.
__global__ __launch_bounds__(kFinishThreads) void k_dl_finish(const double *__restrict__ slots, DlShape s, int fit, int by_weights,
                                                              const float *__restrict__ affine_in, double *__restrict__ table,
                                                              float *loss, float *per_view, float *affine_out) {
    constexpr int kWaves = kFinishThreads / LSR_WAVE;
    __shared__ double s_tot[kWaves];
    const int wave = threadIdx.x / LSR_WAVE, lane = threadIdx.x & (LSR_WAVE - 1);
    double tot = 0.0;
    for (int v = wave; v < s.V; v += kWaves) {
        double sum[2];                              // of |r|, of w
        image_slot_sums<2>(slots + (size_t)v * s.chunks * 2, s.chunks, sum);
        double fa = 1.0, fb = 0.0;
        if (fit) { fa = table[(size_t)v * kDlTable]; fb = table[(size_t)v * kDlTable + 1]; }
        else if (affine_in) { fa = (double)affine_in[2 * v]; fb = (double)affine_in[2 * v + 1]; }
        const double N = by_weights ? sum[1] : (double)s.pixels;
        const double inv = fa != 0.0 && N > 0.0 ? 1.0 / N : 0.0;
        const double pv = inv != 0.0 ? sum[0] * inv : 0.0;
        if (lane == 0) {
            double *row = table + (size_t)v * kDlTable;
            if (!fit) { row[0] = fa; row[1] = fb; }
            row[2] = inv;
            row[3] = N;
            if (per_view) per_view[v] = (float)pv;
            if (affine_out && !fit) { affine_out[2 * v] = (float)fa; affine_out[2 * v + 1] = (float)fb; }
        }
        tot += pv;
    }
    if (lane == 0) s_tot[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0 && loss) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += s_tot[w];
        *loss = (float)(t / s.V);
    }
}

struct DlBwdArgs {
    DlShape s;
    float alpha_min;
    const float *depth, *alpha, *views, *target, *weight, *grad_loss, *grad_per_view;
    const double *table;
    float *grad_depth, *grad_alpha;        // each optional
};

__global__ __launch_bounds__(kDlThreads) void k_dl_bwd(DlBwdArgs a) {
    int view, first;
    dl_chunk(a.s, view, first);
    const int64_t base = (int64_t)view * a.s.pixels;
    const float *depth = a.depth + base, *alpha = a.alpha + base, *target = a.target + base;
    const float *weight = a.weight ? a.weight + base : nullptr;
    float *gd = a.grad_depth ? a.grad_depth + base : nullptr, *ga = a.grad_alpha ? a.grad_alpha + base : nullptr;
    const bool vec = dl_aligned(depth) && dl_aligned(alpha) && dl_aligned(target) && dl_aligned(weight);
    const bool al_gd = dl_aligned(gd), al_ga = dl_aligned(ga);
    const double s = (double)a.views[(size_t)view * LSR_VIEW_FLOATS + 40];
    const double *row = a.table + (size_t)view * kDlTable;
    const double fa = row[0], fb = row[1];
    double up = 0.0;
    if (a.grad_loss) up += (double)*a.grad_loss / (double)a.s.V;
    if (a.grad_per_view) up += (double)a.grad_per_view[view];
    const double scale = row[2] != 0.0 ? up * row[2] : 0.0;     // u_v / N_v; 0 for a row that gives nothing
#pragma unroll
    for (int g = 0; g < kDlGroups; ++g) {
        const int i = first + 4 * (g * kDlThreads + (int)threadIdx.x);
        const int n = min(4, a.s.pixels - i);
        if (n <= 0) continue;
        const DlGroup q = dl_load_group(depth, alpha, target, weight, vec, i, n);
        const float d[4] = {q.depth.x, q.depth.y, q.depth.z, q.depth.w}, al[4] = {q.alpha.x, q.alpha.y, q.alpha.z, q.alpha.w},
                    t[4] = {q.target.x, q.target.y, q.target.z, q.target.w}, wt[4] = {q.weight.x, q.weight.y, q.weight.z, q.weight.w};
        float od[4] = {0.0f, 0.0f, 0.0f, 0.0f}, oa[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= n) break;
            bool defined;
            const double I = dl_inverse(d[k], al[k], a.alpha_min, s, &defined);
            if (defined && scale != 0.0) {
                const double w = dl_weight(weight != nullptr, wt[k], t[k]);
                const double r = w * (I - (fa * (double)t[k] + fb));
                const double sign = r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0);
                const double gI = scale * w * sign, inv_d = 1.0 / (double)d[k];
                od[k] = (float)(-gI * I * inv_d);
                oa[k] = (float)(gI * s * inv_d);
            }
        }
        if (gd) dl_store(gd, al_gd, i, n, make_float4(od[0], od[1], od[2], od[3]));
        if (ga) dl_store(ga, al_ga, i, n, make_float4(oa[0], oa[1], oa[2], oa[3]));
    }
}

// LSR_OK, or why these dims are refused
static int dl_check(const lsr_depth_loss_dims *d) {
    if (d->num_views < 1 || d->height < 1 || d->width < 1) return LSR_EINVAL;
    if (d->align != LSR_DEPTH_ALIGN_GIVEN && d->align != LSR_DEPTH_ALIGN_FIT) return LSR_EINVAL;
    if (d->normalize != LSR_DEPTH_NORM_PIXELS && d->normalize != LSR_DEPTH_NORM_WEIGHTS) return LSR_EINVAL;
    if (!std::isfinite(d->alpha_min) || d->alpha_min < 0.0f) return LSR_EINVAL;
    if (d->reserved0 || d->reserved1) return LSR_EINVAL;
    if ((int64_t)d->num_views * d->height * d->width >= ((int64_t)1 << 31)) return LSR_EUNSUPPORTED;
    return LSR_OK;
}

// (V H W < 2^31: H W and V * chunks fit an int)
static DlShape dl_shape(const lsr_depth_loss_dims &d) {
    const int pixels = d.height * d.width;
    return DlShape{d.num_views, pixels, (pixels + kDlChunk - 1) / kDlChunk};
}

struct DlLayout {
    size_t table, main_slots, moment_slots, total;
};

static DlLayout dl_layout(const lsr_depth_loss_dims &d) {
    const DlShape s = dl_shape(d);
    const size_t groups = (size_t)s.V * (size_t)s.chunks;
    DlLayout L;
    L.table = 0;
    L.main_slots = align_up((size_t)s.V * kDlTable * sizeof(double));
    L.moment_slots = L.main_slots + align_up(groups * 2 * sizeof(double));
    L.total = L.moment_slots + (d.align == LSR_DEPTH_ALIGN_FIT ? align_up(groups * kDlMoments * sizeof(double)) : 0);
    return L;
}

}  // namespace lsr

using namespace lsr;

extern "C" {

size_t lsr_depth_loss_workspace_bytes(const lsr_depth_loss_dims *dims) {
    if (!dims || dl_check(dims) != LSR_OK) return 0;
    return dl_layout(*dims).total;
}

int lsr_depth_loss_forward(const lsr_depth_loss_dims *dims, const float *depth, const float *alpha, const float *views,
                           const float *target, const float *weight, const float *affine_in, void *workspace, float *loss,
                           float *per_view, float *inverse_depth, float *affine_out, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !depth || !alpha || !views || !target || !workspace) return LSR_ENULL;
    const int rc = dl_check(dims);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return LSR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const DlShape s = dl_shape(*dims);
    const DlLayout L = dl_layout(*dims);
    char *ws = (char *)workspace;
    const int fit = dims->align == LSR_DEPTH_ALIGN_FIT;
    const unsigned blocks = (unsigned)s.V * (unsigned)s.chunks;
    DlArgs a{s, dims->alpha_min, fit, depth, alpha, views, target, weight, fit ? nullptr : affine_in, (double *)(ws + L.table),
             nullptr, inverse_depth};
    if (fit) {
        a.slots = (double *)(ws + L.moment_slots);
        hipLaunchKernelGGL(k_dl_moments, dim3(blocks), dim3(kDlThreads), 0, st, a);
        hipLaunchKernelGGL(k_dl_fit, dim3((unsigned)((s.V + kDlWaves - 1) / kDlWaves)), dim3(kDlThreads), 0, st,
                           (const double *)a.slots, s, a.table, affine_out);
    }
    a.slots = (double *)(ws + L.main_slots);
    hipLaunchKernelGGL(k_dl_fwd, dim3(blocks), dim3(kDlThreads), 0, st, a);
    hipLaunchKernelGGL(k_dl_finish, dim3(1), dim3(kFinishThreads), 0, st, (const double *)a.slots, s, fit,
                       (int)(dims->normalize == LSR_DEPTH_NORM_WEIGHTS), a.affine_in, a.table, loss, per_view, affine_out);
    return launch_status();
}

int lsr_depth_loss_backward(const lsr_depth_loss_dims *dims, const float *depth, const float *alpha, const float *views,
                            const float *target, const float *weight, const void *workspace, const float *grad_loss,
                            const float *grad_per_view, float *grad_depth, float *grad_alpha, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !depth || !alpha || !views || !target || !workspace || (!grad_loss && !grad_per_view)) return LSR_ENULL;
    const int rc = dl_check(dims);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return LSR_EINVAL;
    if (!grad_depth && !grad_alpha) return LSR_OK;
    const DlShape s = dl_shape(*dims);
    DlBwdArgs a{s, dims->alpha_min, depth, alpha, views, target, weight, grad_loss, grad_per_view,
                (const double *)((const char *)workspace + dl_layout(*dims).table), grad_depth, grad_alpha};
    hipLaunchKernelGGL(k_dl_bwd, dim3((unsigned)s.V * (unsigned)s.chunks), dim3(kDlThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
