// depth_head.hip — fused depth head (include/lsr_depth_head.h): the encoder's depth logits to sampled depths, opacities
// and bucket indices in one launch, and their gradient back to the logits in one more.
//
// Reference behaviour restated (no code taken): DepthPredictorMonocular.forward behind its projection
// (src/model/encoder/epipolar/depth_predictor_monocular.py:37-81), sample_discrete_distribution / gather_discrete_topk
// (src/misc/discrete_probability_distribution.py:7-33), relative_disparity_to_depth (epipolar/conversions.py:5-14) and
// the encoder's map_pdf_to_opacity / gaussians_per_pixel (encoder_epipolar.py:113-126,190).
//
// Decomposition.  A GROUP of L lanes (L = 16, 32 or 64: the power of two at or above S) owns one (row, surface); lane b
// of the group holds bucket b as ONE float2 load (pdf logit, offset logit) of the interleaved row, so nothing is
// de-interleaved across lanes and every lane does useful work on both channels.  A wave holds 64 / L groups, consecutive
// (row, surface) pairs: at the reference's shape (S = 32, F = 1: L = 32) a wave reads two rows = 512 contiguous bytes;
// any S F = 32 (2 S F = 64 floats) takes the same L <= 32 instance, the surfaces of a row side by side in one wave.
//   max / sums   all-reduce butterflies inside the group: DPP quad_perm, row_half_mirror, row_mirror up to 16 lanes
//                (no LDS), one ds_swizzle for 32, one bpermute for 64; every lane ends with the same bits
//   prefix sum   DPP row_shr 1, 2, 4, 8 and row_bcast15 / row_bcast31 across the 16-lane rows
//   sampling     lane j < k of the group owns sample j: binary search of its uniform over the group's cumulative sums
//                (log2 L bpermute probes serve all samples of all groups of the wave at once), then two bpermute gathers
//   backward     recomputes p, o and the sums from the logits, broadcasts the k samples' (index, three coefficients)
//                to the group in sample order and accumulates per bucket: one owner per element, fixed order, no atomics
// No LDS allocation, no scratch.  Lanes b >= S and the groups past the end of the last wave stay enabled (DPP reads
// them) with neutral values and store nothing.
#include <float.h>
#include <math.h>

#include "lsr_wave.h"
#include "lsr_depth_head.h"

namespace lsr {

constexpr int kDhThreads = 256;

struct DhArgs {
    int64_t groups;            // rows * F
    int64_t row_stride, grad_row_stride;
    int rays, S, F, k;
    int deterministic, transmittance, vec2, gvec2;   // vec2 / gvec2: rows of logits / d_logits are 8-byte aligned
    float e, inv_e, scale;
};

// all-reduce over the L lanes of a group; the operands of every step are the same pair on both sides, so all lanes
// return identical bits
template <int L, class Op>
__device__ __forceinline__ float dh_all(float x, Op op) {
    x = row_all(x, op);
    if (L >= 32) x = op(x, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x401F)));   // lane ^ 16
    if (L >= 64) x = op(x, __shfl_xor(x, 32));
    return x;
}

// inclusive prefix sum over the L lanes of a group
template <int L>
__device__ __forceinline__ float dh_scan(float x) {
    x += dpp<0x111>(x);              // row_shr:1 (lanes without a source, or in a masked row, add 0)
    x += dpp<0x112>(x);              // row_shr:2
    x += dpp<0x114>(x);              // row_shr:4
    x += dpp<0x118>(x);              // row_shr:8
    if (L >= 32) x += dpp<0x142, 0xA>(x);         // row_bcast15 into rows 1 and 3
    if (L >= 64) x += dpp<0x143, 0xC>(x);         // row_bcast31 into rows 2 and 3
    return x;
}

// What both directions compute per lane from the logits.
struct DhLane {
    float p, o, n, z;          // softmax, sigmoid, normalised pdf; z = FLT_EPSILON + sum p (group-uniform)
    float den, xsel;           // transmittance denominator 1 - E + 1e-10 (1 otherwise); the value step 8 gathers
    float cdf;                 // inclusive cumulative sum of n; +inf on lanes b >= S
};

template <int L>
__device__ __forceinline__ DhLane dh_lane(const DhArgs &a, const float *__restrict__ logits, int64_t row, int f, int b,
                                          bool active) {
    float l = -INFINITY, off = 0.0f;
    if (active) {
        const float *src = logits + row * a.row_stride + (size_t)(b * a.F + f) * 2;
        if (a.vec2) {
            const float2 v = *reinterpret_cast<const float2 *>(src);
            l = v.x; off = v.y;
        } else {
            l = src[0]; off = src[1];
        }
    }
    DhLane r;
    const float m = dh_all<L>(l, Max());
    const float e = active ? expf(l - m) : 0.0f;
    const float s = dh_all<L>(e, Add());
    r.p = e / s;
    r.z = FLT_EPSILON + dh_all<L>(r.p, Add());
    r.n = r.p / r.z;
    r.o = 1.0f / (1.0f + expf(-off));
    const float c = dh_scan<L>(r.n);
    r.cdf = active ? c : INFINITY;
    r.den = 1.0f;
    r.xsel = r.n;
    if (a.transmittance) {
        const float incl = dh_scan<L>(r.p);
        const float before = __shfl_up(incl, 1);
        r.den = 1.0f - (b == 0 ? 0.0f : before) + 1e-10f;
        r.xsel = r.p / r.den;
    }
    return r;
}

__device__ __forceinline__ float dh_depth(const DhArgs &a, int idx, float o_at, float near, float far, float *slope) {
    const float rd = ((float)idx + o_at) / (float)a.S;
    const float dn = 1.0f / (near + 1e-10f), df = 1.0f / (far + 1e-10f);
    const float depth = 1.0f / ((1.0f - rd) * (dn - df) + df + 1e-10f);
    *slope = depth * depth * (dn - df) / (float)a.S;      // d depth / d o[index]
    return depth;
}

template <int L>
__global__ __launch_bounds__(kDhThreads) void k_depth_head_fwd(DhArgs a, const float *__restrict__ logits,
                                                               const float *__restrict__ near, const float *__restrict__ far,
                                                               const float *__restrict__ uniforms, float *__restrict__ depth,
                                                               float *__restrict__ opacity, int32_t *__restrict__ index) {
    const int lane = (int)(threadIdx.x & (LSR_WAVE - 1));
    const int b = lane & (L - 1), base = lane - b;
    const int64_t g = (int64_t)blockIdx.x * (kDhThreads / L) + (int)(threadIdx.x / L);
    const bool live = g < a.groups;
    const int64_t gc = live ? g : a.groups - 1;
    const int64_t row = gc / a.F;
    const int f = (int)(gc - row * a.F);
    const bool active = b < a.S, sample = b < a.k;
    const DhLane r = dh_lane<L>(a, logits, row, f, b, active);

    int idx = 0;
    if (a.deterministic) {
        // k rounds: the largest remaining p, then the lowest lane that holds it
        float pv = active ? r.p : -1.0f;
        for (int j = 0; j < a.k; ++j) {
            const float m = dh_all<L>(pv, Max());
            const int win = (int)dh_all<L>(pv == m ? (float)b : (float)L, Min());
            if (b == j) idx = win;
            if (b == win) pv = -1.0f;
        }
    } else {
        // #{ i : cdf_i <= u } clipped to S - 1: the last edge is never probed (lanes b >= S hold +inf)
        const float u = sample ? uniforms[gc * a.k + b] : -1.0f;
#pragma unroll
        for (int step = L / 2; step >= 1; step >>= 1) {
            const float probe = __shfl(r.cdf, base + idx + step - 1);
            if (probe <= u) idx += step;
        }
    }
    idx = max(0, min(idx, a.S - 1));
    const float o_at = __shfl(r.o, base + idx), x = __shfl(r.xsel, base + idx);
    if (!(live && sample)) return;      // (no cross-lane operation follows)
    const int64_t cam = row / a.rays;
    float slope;
    const float dep = dh_depth(a, idx, o_at, near[cam], far[cam], &slope);
    const float op = a.e == 1.0f ? a.scale * x : a.scale * 0.5f * (1.0f - powf(1.0f - x, a.e) + powf(x, a.inv_e));
    const int64_t at = gc * a.k + b;
    depth[at] = dep;
    opacity[at] = op;
    index[at] = idx;
}

template <int L>
__global__ __launch_bounds__(kDhThreads) void k_depth_head_bwd(DhArgs a, const float *__restrict__ logits,
                                                               const float *__restrict__ near, const float *__restrict__ far,
                                                               const int32_t *__restrict__ index, const float *__restrict__ g_depth,
                                                               const float *__restrict__ g_opacity, float *__restrict__ d_logits) {
    const int lane = (int)(threadIdx.x & (LSR_WAVE - 1));
    const int b = lane & (L - 1), base = lane - b;
    const int64_t g = (int64_t)blockIdx.x * (kDhThreads / L) + (int)(threadIdx.x / L);
    const bool live = g < a.groups;
    const int64_t gc = live ? g : a.groups - 1;
    const int64_t row = gc / a.F;
    const int f = (int)(gc - row * a.F);
    const bool active = b < a.S, sample = b < a.k;
    const DhLane r = dh_lane<L>(a, logits, row, f, b, active);

    // lane j < k: sample j's index and its three coefficients
    //   ca: dL/do[index];  cg: dL/dx;  ct: cg x (plain: the normalisation term) or cg x / den[index] (transmittance:
    //   the term every earlier bucket receives through the cumulative sum)
    const int64_t at = gc * a.k + b;
    int idx = sample ? index[at] : 0;
    idx = max(0, min(idx, a.S - 1));
    const float gd = sample && g_depth ? g_depth[at] : 0.0f, go = sample && g_opacity ? g_opacity[at] : 0.0f;
    const float o_at = __shfl(r.o, base + idx), x = __shfl(r.xsel, base + idx), den_at = __shfl(r.den, base + idx);
    const int64_t cam = row / a.rays;
    float slope;
    dh_depth(a, idx, o_at, near[cam], far[cam], &slope);
    const float dop = a.e == 1.0f ? a.scale
                                  : a.scale * 0.5f * (a.e * powf(1.0f - x, a.e - 1.0f) + a.inv_e * powf(x, a.inv_e - 1.0f));
    const float ca = sample ? gd * slope : 0.0f;
    const float cg = sample ? go * dop : 0.0f;
    const float ct = sample ? (a.transmittance ? cg * x / den_at : cg * x) : 0.0f;

    float acc_a = 0.0f, acc_g = 0.0f, acc_t = 0.0f;
    for (int j = 0; j < a.k; ++j) {       // sample order: the sums of a bucket are reproducible
        const int ij = __shfl(idx, base + j);
        const float aj = __shfl(ca, base + j), gj = __shfl(cg, base + j), tj = __shfl(ct, base + j);
        if (ij == b) { acc_a += aj; acc_g += gj; }
        if (!a.transmittance || ij > b) acc_t += tj;
    }
    float dp = a.transmittance ? acc_g / r.den + acc_t : (acc_g - acc_t) / r.z;
    if (!active) dp = 0.0f;
    const float dot = dh_all<L>(r.p * dp, Add());
    const float dl = r.p * (dp - dot), da = acc_a * r.o * (1.0f - r.o);
    if (!(live && active)) return;
    float *dst = d_logits + row * a.grad_row_stride + (size_t)(b * a.F + f) * 2;
    if (a.gvec2) {
        *reinterpret_cast<float2 *>(dst) = make_float2(dl, da);
    } else {
        dst[0] = dl; dst[1] = da;
    }
}

}  // namespace lsr

using namespace lsr;

// dims validation shared by both directions, host only
static int depth_head_check(const lsr_depth_head_dims *d, bool backward) {
    if (!d) return LSR_ENULL;
    if (d->num_cameras < 1 || d->rays < 0) return LSR_EINVAL;
    if (d->buckets < 1 || d->buckets > LSR_DEPTH_HEAD_MAX_BUCKETS || d->surfaces < 1) return LSR_EINVAL;
    if (d->samples < 1 || d->samples > LSR_DEPTH_HEAD_MAX_SAMPLES) return LSR_EINVAL;
    if (d->flags & ~(LSR_DEPTH_HEAD_DETERMINISTIC | LSR_DEPTH_HEAD_TRANSMITTANCE)) return LSR_EINVAL;
    if ((d->flags & LSR_DEPTH_HEAD_DETERMINISTIC) && d->samples > d->buckets) return LSR_EINVAL;
    if (!(d->opacity_exponent > 0.0f) || !isfinite(d->opacity_exponent) || !isfinite(d->opacity_scale)) return LSR_EINVAL;
    const int64_t W = 2 * (int64_t)d->buckets * d->surfaces;
    if (W > LSR_DEPTH_HEAD_MAX_ROW_FLOATS) return LSR_EUNSUPPORTED;
    if (d->row_stride < W || (backward && d->grad_row_stride < W)) return LSR_EINVAL;
    const int L = d->buckets <= 16 ? 16 : (d->buckets <= 32 ? 32 : 64);
    // (rows * F) groups, kDhThreads / L of them per workgroup, in a 31-bit grid; tested without forming a product that could overflow
    const int64_t rows = (int64_t)d->num_cameras * d->rays, max_groups = 0x7FFFFFFFll * (kDhThreads / L);
    if (rows > max_groups / d->surfaces) return LSR_EUNSUPPORTED;
    return LSR_OK;
}

static DhArgs depth_head_args(const lsr_depth_head_dims &d, const float *logits, const float *d_logits) {
    DhArgs a{};
    a.groups = (int64_t)d.num_cameras * d.rays * d.surfaces;
    a.row_stride = d.row_stride;
    a.grad_row_stride = d.grad_row_stride;
    a.rays = d.rays; a.S = d.buckets; a.F = d.surfaces; a.k = d.samples;
    a.deterministic = (d.flags & LSR_DEPTH_HEAD_DETERMINISTIC) != 0;
    a.transmittance = (d.flags & LSR_DEPTH_HEAD_TRANSMITTANCE) != 0;
    a.vec2 = (reinterpret_cast<uintptr_t>(logits) & 7) == 0 && (d.row_stride & 1) == 0;
    a.gvec2 = (reinterpret_cast<uintptr_t>(d_logits) & 7) == 0 && (d.grad_row_stride & 1) == 0;
    a.e = d.opacity_exponent; a.inv_e = 1.0f / d.opacity_exponent; a.scale = d.opacity_scale;
    return a;
}

extern "C" {

int lsr_depth_head_forward(const lsr_depth_head_dims *d, const float *logits, const float *near, const float *far,
                           const float *uniforms, float *depth, float *opacity, int32_t *index, lsr_stream_t stream) {
    note_hip_error(0);
    const int rc = depth_head_check(d, false);
    if (rc) return rc;
    if (d->rays == 0) return LSR_OK;
    if (!logits || !near || !far || !depth || !opacity || !index) return LSR_ENULL;
    if (!uniforms && !(d->flags & LSR_DEPTH_HEAD_DETERMINISTIC)) return LSR_ENULL;
    const DhArgs a = depth_head_args(*d, logits, nullptr);
    hipStream_t s = (hipStream_t)stream;
    if (a.S <= 16) {
        const unsigned blocks = (unsigned)((a.groups + kDhThreads / 16 - 1) / (kDhThreads / 16));
        hipLaunchKernelGGL(k_depth_head_fwd<16>, dim3(blocks), dim3(kDhThreads), 0, s, a, logits, near, far, uniforms, depth, opacity, index);
    } else if (a.S <= 32) {
        const unsigned blocks = (unsigned)((a.groups + kDhThreads / 32 - 1) / (kDhThreads / 32));
        hipLaunchKernelGGL(k_depth_head_fwd<32>, dim3(blocks), dim3(kDhThreads), 0, s, a, logits, near, far, uniforms, depth, opacity, index);
    } else {
        const unsigned blocks = (unsigned)((a.groups + kDhThreads / 64 - 1) / (kDhThreads / 64));
        hipLaunchKernelGGL(k_depth_head_fwd<64>, dim3(blocks), dim3(kDhThreads), 0, s, a, logits, near, far, uniforms, depth, opacity, index);
    }
    return launch_status();
}

int lsr_depth_head_backward(const lsr_depth_head_dims *d, const float *logits, const float *near, const float *far,
                            const int32_t *index, const float *g_depth, const float *g_opacity, float *d_logits,
                            lsr_stream_t stream) {
    note_hip_error(0);
    const int rc = depth_head_check(d, true);
    if (rc) return rc;
    if (d->rays == 0) return LSR_OK;
    if (!logits || !near || !far || !index || !d_logits) return LSR_ENULL;
    const DhArgs a = depth_head_args(*d, logits, d_logits);
    hipStream_t s = (hipStream_t)stream;
    if (a.S <= 16) {
        const unsigned blocks = (unsigned)((a.groups + kDhThreads / 16 - 1) / (kDhThreads / 16));
        hipLaunchKernelGGL(k_depth_head_bwd<16>, dim3(blocks), dim3(kDhThreads), 0, s, a, logits, near, far, index, g_depth, g_opacity, d_logits);
    } else if (a.S <= 32) {
        const unsigned blocks = (unsigned)((a.groups + kDhThreads / 32 - 1) / (kDhThreads / 32));
        hipLaunchKernelGGL(k_depth_head_bwd<32>, dim3(blocks), dim3(kDhThreads), 0, s, a, logits, near, far, index, g_depth, g_opacity, d_logits);
    } else {
        const unsigned blocks = (unsigned)((a.groups + kDhThreads / 64 - 1) / (kDhThreads / 64));
        hipLaunchKernelGGL(k_depth_head_bwd<64>, dim3(blocks), dim3(kDhThreads), 0, s, a, logits, near, far, index, g_depth, g_opacity, d_logits);
    }
    return launch_status();
}

}  // extern "C"
