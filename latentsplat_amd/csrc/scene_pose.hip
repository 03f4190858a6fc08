// scene_pose.hip — the pose gradient of a 3DGS scene's rigid parts (include/lsr_pose.h): the similarity transform of
// scene_transform.hip, differentiated in the transforms.  A pose is a raw quaternion p, a translation t and a log-scale l;
// for the world-frame perturbation R -> exp([w]x) R every output's derivative needs only that output, the upstream
// gradient and constants, so a Gaussian contributes 7 numbers (w, t, l) to its transform and no (2l+1)^2 outer product is
// ever formed: the colour term is the bilinear form g^T J_a c' with the constant sparse generators of
// lsr_sh_generator_table.h (42 (i, j, v) triples in all, 7 FMAs each over the three channels).
//
// Three kernels.
//   k_pose_matrices: (p, t, l) -> (T, 4, 4) float32 similarities, one lane per transform, in double.
//   k_scene_pose_grad<K>: the pass over the scene, shaped like k_scene_transform: a workgroup owns chunks of consecutive
//     Gaussians, the grid capped at kPgMaxBlocks so that the partial table stays small.
//       * c' and g_c: the chunk's two spans are read lane j element j, kPgBatch independent dwords per lane and tensor in
//         flight, into LDS at an odd row stride; then one Gaussian per lane reads its own two rows (conflict-free).
//       * one Gaussian per lane forms its 7 float32 contributions (colour first, then quaternion, then position).
//       * reduction by transform, without atomics: per wave, while any lane is unclaimed, the id of the first unclaimed
//         lane is taken as a uniform value, the 7 values of the matching lanes are summed over the wave in six levels of a
//         fixed lane order (DPP exchanges within rows of 16, then the four rows: no LDS round trips) and lane k < 7 adds component k, in double, into the wave's private LDS table [T][7].  Entry
//         [id][k] is only ever touched by lane k of its wave, and chunks are visited in order.  Contiguous parts take one
//         or two trips per wave.  A trip costs about 260 instructions, so after kPgTrips of them the lanes still unclaimed
//         (shuffled rows: most of the wave) are walked in lane order instead: lane k < 7 reads component k of that lane
//         (v_readlane) and adds it to the table entry of its id, about 25 instructions per lane.
//       * at the end the workgroup sums its waves' tables in wave order and writes partial[block][T][7] (double), all of it.
//   k_pose_grad_finish: a workgroup per transform; 32 lanes per component sum partial over the blocks (lane j the blocks
//     j, j + 32, ... in order; then the 32 sums in order), in double: one lane walking up to 2048 blocks serially took
//     longer than the pass over 393 216 Gaussians.  Then it applies the quaternion chain dL/dp = (2 / |p|) (0, G_w) (x) p / |p| in double and writes float32.
// No atomics anywhere and every order fixed: the same bits every call.  LDS: two row sets of a chunk plus the waves' tables
// (T <= LSR_POSE_MAX_TRANSFORMS = 256: 14 KB per wave) stay within 64 KB with 128 Gaussians per chunk up to K = 9 and 64
// from K = 16 (K = 25: 36.5 KB of rows and one table).
#include <math.h>

#include <algorithm>

#include "lsr_wave.h"
#include "lsr_sh_shape.h"
#include "lsr_pose.h"
#include "lsr_sh_generator_table.h"

namespace lsr {

constexpr int kPgMaxBlocks = 2048;        // grid cap: partial is at most 2048 x T x 7 doubles (29 MB at T = 256)
constexpr int kPgBatch = 16;              // dword loads in flight per lane and tensor
constexpr int kPgLdsBytes = 65536;
constexpr int kPgTrips = 4;               // ids of a wave reduced by a wave sum each, before the lane-by-lane walk
constexpr int kPgFinishPhases = 32;       // lanes per (transform, component) of k_pose_grad_finish

__host__ __device__ constexpr int pg_chunk(int K) { return K >= 16 ? 64 : 128; }     // Gaussians per chunk = lanes per workgroup
__host__ __device__ constexpr int pg_rows_bytes(int K) { return K > 1 ? 2 * pg_chunk(K) * sh_rest_stride(K) * 4 : 32; }
__host__ __device__ constexpr int pg_tables_bytes(int K, int T) { return pg_chunk(K) / 64 * T * 7 * 8; }
static_assert(pg_rows_bytes(25) + pg_tables_bytes(25, LSR_POSE_MAX_TRANSFORMS) <= kPgLdsBytes, "LDS budget, K = 25");
static_assert(pg_rows_bytes(16) + pg_tables_bytes(16, LSR_POSE_MAX_TRANSFORMS) <= kPgLdsBytes, "LDS budget, K = 16");
static_assert(pg_rows_bytes(9) + pg_tables_bytes(9, LSR_POSE_MAX_TRANSFORMS) <= kPgLdsBytes, "LDS budget, K = 9");
static_assert(pg_rows_bytes(4) + pg_tables_bytes(4, LSR_POSE_MAX_TRANSFORMS) <= kPgLdsBytes, "LDS budget, K = 4");

static int64_t pg_blocks(int64_t n, int K) {
    const int G = pg_chunk(K);
    return std::min<int64_t>((n + G - 1) / G, kPgMaxBlocks);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pose_matrices(int T, const float *__restrict__ quat, const float *__restrict__ trans,
                                                      const float *__restrict__ log_scale, float *__restrict__ mats) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= T) return;
    double w = quat[4 * k], x = quat[4 * k + 1], y = quat[4 * k + 2], z = quat[4 * k + 3];
    const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= inv; x *= inv; y *= inv; z *= inv;
    const double s = log_scale ? exp((double)log_scale[k]) : 1.0;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    float *m = mats + 16 * (size_t)k;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) m[4 * a + b] = (float)(s * R[3 * a + b]);
        m[4 * a + 3] = trans[3 * k + a];
    }
    m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = 1.0f;
}

// ---------------------------------------------------------------------------------------------------------------------
// sum over the entries E.. of axis A, band L of  v (g_i . c_j - g_j . c_i)  (the dots over the three channels), added to acc
template <int A, int L, int E = 0>
__device__ __forceinline__ float pg_axis_band(const float *__restrict__ c, const float *__restrict__ g, float acc) {
    if constexpr (E < kShGenCount[A][L]) {
        constexpr int base = 3 * (L * L - 1);
        constexpr int i = base + 3 * kShGenRow[A][L][E], j = base + 3 * kShGenCol[A][L][E];
        constexpr float v = (float)kShGenVal[A][L][E];
        float d = g[i] * c[j];
        d = fmaf(g[i + 1], c[j + 1], d);
        d = fmaf(g[i + 2], c[j + 2], d);
        d = fmaf(-g[j], c[i], d);
        d = fmaf(-g[j + 1], c[i + 1], d);
        d = fmaf(-g[j + 2], c[i + 2], d);
        return pg_axis_band<A, L, E + 1>(c, g, fmaf(v, d, acc));
    } else {
        return acc;
    }
}

template <int K, int A>
__device__ __forceinline__ float pg_axis(const float *__restrict__ c, const float *__restrict__ g) {
    float acc = pg_axis_band<A, 1>(c, g, 0.0f);
    if constexpr (K > 4) acc = pg_axis_band<A, 2>(c, g, acc);
    if constexpr (K > 9) acc = pg_axis_band<A, 3>(c, g, acc);
    if constexpr (K > 16) acc = pg_axis_band<A, 4>(c, g, acc);
    return acc;
}

// the sum of v over the 64 lanes as a uniform value, in a fixed order: within each row of 16 lanes by row_all (every lane
// of a row ends with the same sum), then the four rows as (r0 + r1) + (r2 + r3).  Six levels; no LDS traffic (a __shfl
// butterfly is six dependent LDS round trips).
__device__ __forceinline__ float pg_wave_sum(float v) {
    v = row_all<true>(v, Add());
    return (readlane(v, 0) + readlane(v, 16)) + (readlane(v, 32) + readlane(v, 48));
}

template <int K>
__global__ __launch_bounds__(pg_chunk(K)) void k_scene_pose_grad(int64_t n, int T, const float *__restrict__ records,
                                                                 const int32_t *__restrict__ idx, lsr_pose_grad_in in,
                                                                 double *__restrict__ partial) {
    constexpr int G = pg_chunk(K), W = sh_rest_floats(K), WP = sh_rest_stride(K), PAD = WP - W, WAVES = G / 64;
    constexpr int RF = LSR_TRANSFORM_RECORD_FLOATS(sh_degree_of(K));
    __shared__ float s_c[K > 1 ? G * WP : 4], s_g[K > 1 ? G * WP : 4];
    extern __shared__ double pg_tab[];                   // [WAVES][T][7]
    const int tid = threadIdx.x, lane = tid & 63;
    const int cells = T * 7;
    double *tab = pg_tab + (size_t)(tid >> 6) * cells;
    for (int i = lane; i < cells; i += 64) tab[i] = 0.0;
    __syncthreads();
    const bool rest = K > 1 && in.g_features_rest != nullptr;
    const int64_t chunks = (n + G - 1) / G;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t g0 = c * G;
        const int nr = (int)(n - g0 < (int64_t)G ? n - g0 : (int64_t)G);
        if constexpr (K > 1) {
            if (rest) {
                const int total = W * nr;
                const float *src_c = in.features_rest + g0 * W, *src_g = in.g_features_rest + g0 * W;
                for (int j0 = tid; j0 < total; j0 += kPgBatch * G) {
                    float vc[kPgBatch], vg[kPgBatch];
#pragma unroll
                    for (int u = 0; u < kPgBatch; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) { vc[u] = src_c[j]; vg[u] = src_g[j]; }
                    }
#pragma unroll
                    for (int u = 0; u < kPgBatch; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) {
                            const int at = j + (j / W) * PAD;
                            s_c[at] = vc[u]; s_g[at] = vg[u];
                        }
                    }
                }
            }
        }
        const int64_t gi = g0 + tid;
        bool valid = tid < nr;
        int id = 0;
        if (idx) {
            if (valid) {
                id = idx[gi];
                valid = (unsigned)id < (unsigned)T;
            }
            if (!valid) id = 0;
        }
        __syncthreads();

        // the lane's 7 contributions: w (3), t (3), l
        float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, ls = 0.0f;
        if (valid) {
            if constexpr (K > 1) {
                if (rest) {
                    const float *rc = s_c + tid * WP, *rg = s_g + tid * WP;
                    w0 = pg_axis<K, 0>(rc, rg);
                    w1 = pg_axis<K, 1>(rc, rg);
                    w2 = pg_axis<K, 2>(rc, rg);
                }
            }
            if (in.g_rotation) {
                const float4 q = reinterpret_cast<const float4 *>(in.rotation)[gi];
                const float4 g = reinterpret_cast<const float4 *>(in.g_rotation)[gi];
                // (w g_v - g_w v + v x g_v) / 2, q = (q.x; q.y q.z q.w)
                const float h0 = fmaf(q.x, g.y, fmaf(-g.x, q.y, fmaf(q.z, g.w, -q.w * g.z)));
                const float h1 = fmaf(q.x, g.z, fmaf(-g.x, q.z, fmaf(q.w, g.y, -q.y * g.w)));
                const float h2 = fmaf(q.x, g.w, fmaf(-g.x, q.w, fmaf(q.y, g.z, -q.z * g.y)));
                w0 = fmaf(0.5f, h0, w0); w1 = fmaf(0.5f, h1, w1); w2 = fmaf(0.5f, h2, w2);
            }
            if (in.g_scaling) {
                const float *p = in.g_scaling + 3 * gi;
                ls = (p[0] + p[1]) + p[2];
            }
            if (in.g_xyz) {
                const float *rec = records + (size_t)id * RF;
                const float *p = in.xyz + 3 * gi, *gp = in.g_xyz + 3 * gi;
                const float x0 = p[0], x1 = p[1], x2 = p[2], g0x = gp[0], g1x = gp[1], g2x = gp[2];
                const float y0 = fmaf(rec[0], x0, fmaf(rec[1], x1, rec[2] * x2));
                const float y1 = fmaf(rec[3], x0, fmaf(rec[4], x1, rec[5] * x2));
                const float y2 = fmaf(rec[6], x0, fmaf(rec[7], x1, rec[8] * x2));
                w0 += fmaf(y1, g2x, -y2 * g1x);
                w1 += fmaf(y2, g0x, -y0 * g2x);
                w2 += fmaf(y0, g1x, -y1 * g0x);
                t0 = g0x; t1 = g1x; t2 = g2x;
                ls += fmaf(g0x, y0, fmaf(g1x, y1, g2x * y2));
            }
        }

        // by transform: up to kPgTrips ids by one wave sum each, whatever is left lane by lane
        bool open = valid;
        unsigned long long todo = __ballot(open);
        for (int trip = 0; todo && trip < kPgTrips; ++trip) {
            const int cur = readlane(id, __ffsll((long long)todo) - 1);
            const bool mine = open && id == cur;
            const float r[7] = {pg_wave_sum(mine ? w0 : 0.0f), pg_wave_sum(mine ? w1 : 0.0f), pg_wave_sum(mine ? w2 : 0.0f),
                                pg_wave_sum(mine ? t0 : 0.0f), pg_wave_sum(mine ? t1 : 0.0f), pg_wave_sum(mine ? t2 : 0.0f),
                                pg_wave_sum(mine ? ls : 0.0f)};
            float x = r[0];
#pragma unroll
            for (int k = 1; k < 7; ++k) x = lane == k ? r[k] : x;
            if (lane < 7) tab[cur * 7 + lane] += (double)x;
            open = open && !mine;
            todo = __ballot(open);
        }
        while (todo) {                                   // in lane order; uniform: todo lives in scalar registers
            const int src = __ffsll((long long)todo) - 1;
            const int cur = readlane(id, src);
            float x = readlane(w0, src);
            x = lane == 1 ? readlane(w1, src) : x;
            x = lane == 2 ? readlane(w2, src) : x;
            x = lane == 3 ? readlane(t0, src) : x;
            x = lane == 4 ? readlane(t1, src) : x;
            x = lane == 5 ? readlane(t2, src) : x;
            x = lane == 6 ? readlane(ls, src) : x;
            if (lane < 7) tab[cur * 7 + lane] += (double)x;
            todo &= todo - 1;
        }
        if constexpr (K > 1) {
            if (rest) __syncthreads();                   // the rows are the next chunk's
        }
    }
    __syncthreads();
    double *out = partial + (size_t)blockIdx.x * cells;
    for (int i = tid; i < cells; i += G) {
        double s = pg_tab[i];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += pg_tab[(size_t)w * cells + i];
        out[i] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// one workgroup per transform, lane = (phase, component): the lane sums the blocks phase, phase + 32, ... in that order, then
// lane (0, component) adds the 32 phase sums in phase order: a fixed order whatever the grid, and 32 loads deep per
// component instead of one serial walk over up to kPgMaxBlocks blocks
__global__ __launch_bounds__(7 * kPgFinishPhases) void k_pose_grad_finish(int T, int blocks, const double *__restrict__ partial,
                                                                          const float *__restrict__ quat,
                                                                          float *__restrict__ grad_q, float *__restrict__ grad_t,
                                                                          float *__restrict__ grad_l) {
    __shared__ double s_part[7 * kPgFinishPhases], s_sum[8];
    const int tid = threadIdx.x, phase = tid / 7, comp = tid - 7 * phase, k = blockIdx.x;
    double s = 0.0;
    const double *p = partial + (size_t)k * 7 + comp;
    for (int b = phase; b < blocks; b += kPgFinishPhases) s += p[(size_t)b * T * 7];
    s_part[tid] = s;
    __syncthreads();
    if (tid < 7) {
        double total = s_part[tid];
        for (int j = 1; j < kPgFinishPhases; ++j) total += s_part[7 * j + tid];
        s_sum[tid] = total;
    }
    __syncthreads();
    if (tid >= 8) return;
    if (tid >= 4) {
        if (tid < 7 && grad_t) grad_t[3 * k + tid - 4] = (float)s_sum[tid - 1];
        if (tid == 7 && grad_l) grad_l[k] = (float)s_sum[6];
    } else if (grad_q) {
        // (2 / |p|) (0, a) (x) (w, v) / |p| = (2 / |p|^2) (-a . v, w a + a x v)
        const double a0 = s_sum[0], a1 = s_sum[1], a2 = s_sum[2];
        const double w = quat[4 * k], x = quat[4 * k + 1], y = quat[4 * k + 2], z = quat[4 * k + 3];
        const double f = 2.0 / (w * w + x * x + y * y + z * z);
        double r;
        if (tid == 0) r = -(a0 * x + a1 * y + a2 * z);
        else if (tid == 1) r = w * a0 + (a1 * z - a2 * y);
        else if (tid == 2) r = w * a1 + (a2 * x - a0 * z);
        else r = w * a2 + (a0 * y - a1 * x);
        grad_q[4 * k + tid] = (float)(f * r + 0.0);         // (+ 0.0: a transform that owns nothing gets +0, not -0)
    }
}

template <int K>
static void pg_launch(const lsr_transform_dims &d, const float *records, const int32_t *idx, const lsr_pose_grad_in &in,
                      double *partial, hipStream_t s) {
    const size_t dyn = (size_t)pg_tables_bytes(K, d.num_transforms);
    hipLaunchKernelGGL((k_scene_pose_grad<K>), dim3((unsigned)pg_blocks(d.n, K)), dim3(pg_chunk(K)), dyn, s, d.n,
                       d.num_transforms, records, idx, in, partial);
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_pose_matrices(int32_t T, const float *quaternions, const float *translations, const float *log_scales,
                      float *matrices, lsr_stream_t stream) {
    note_hip_error(0);
    if (T < 0) return LSR_EINVAL;
    if (T == 0) return LSR_OK;
    if (!quaternions || !translations || !matrices) return LSR_ENULL;
    hipLaunchKernelGGL(k_pose_matrices, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (int)T, quaternions,
                       translations, log_scales, matrices);
    return launch_status();
}

size_t lsr_pose_grad_workspace_bytes(int64_t n, int32_t sh_coeffs, int32_t T) {
    if (n < 0 || !sh_valid_coeffs(sh_coeffs) || T < 0 || T > LSR_POSE_MAX_TRANSFORMS) return 0;
    return (size_t)pg_blocks(n, sh_coeffs) * (size_t)T * 7 * sizeof(double);
}

int lsr_scene_pose_grad(const lsr_transform_dims *dims, const float *records, const int32_t *idx,
                        const float *quaternions, const lsr_pose_grad_in *in, void *workspace, size_t workspace_bytes,
                        float *grad_quaternion, float *grad_translation, float *grad_log_scale, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !in) return LSR_ENULL;
    const int K = dims->sh_coeffs, T = dims->num_transforms;
    if (dims->n < 0 || !sh_valid_coeffs(K) || T < 0) return LSR_EINVAL;
    if (dims->reserved0 || dims->reserved1) return LSR_EINVAL;
    if (K == 1 && (in->features_rest || in->g_features_rest)) return LSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in->rotation) | reinterpret_cast<uintptr_t>(in->g_rotation)) & 15) return LSR_EINVAL;
    if (T > LSR_POSE_MAX_TRANSFORMS) return LSR_EUNSUPPORTED;
    if (workspace_bytes < lsr_pose_grad_workspace_bytes(dims->n, K, T)) return LSR_EINVAL;
    if (T == 0 || (!grad_quaternion && !grad_translation && !grad_log_scale)) return LSR_OK;
    if (grad_quaternion && !quaternions) return LSR_ENULL;
    if (dims->n > 0) {
        if (!records || !workspace) return LSR_ENULL;
        if ((in->g_xyz && !in->xyz) || (in->g_rotation && !in->rotation) || (in->g_features_rest && !in->features_rest))
            return LSR_ENULL;
    }
    hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(workspace);
    if (dims->n > 0) dispatch_sh_coeffs(K, [&](auto k) { pg_launch<decltype(k)::value>(*dims, records, idx, *in, partial, s); });
    hipLaunchKernelGGL(k_pose_grad_finish, dim3((unsigned)T), dim3(7 * kPgFinishPhases), 0, s, (int)T, (int)pg_blocks(dims->n, K), partial, quaternions, grad_quaternion, grad_translation,
                       grad_log_scale);
    return launch_status();
}

}  // extern "C"
