// scene_transform.hip — similarity transforms of a 3DGS scene (include/lsr_transform.h): x' = s R x + t applied to the raw
// parameters a trainer holds.  Positions, log-scales and quaternions are a few flops per Gaussian; the view-dependent
// colour is the part that is easy to get wrong: band l of f_rest goes through T_l(R) = A_l D_l(R) A_l^T, with D_l the
// matrices of sh_rotate.hip (exact polynomials of R) and A_l the constant change of basis between that kernel's SH basis
// and the "3dgs" one of a scene file (lsr_sh_basis_table.h).
//
// Two kernels.  k_transform_records: one 64-lane workgroup per 4x4 matrix, in double, writes the per-transform record
// (linear part, translation, log s, q_R, band blocks; or the constants of the adjoint map).  k_scene_transform: one pass
// over the raw parameters, forward and backward alike (the mode is in the records).
//
// k_scene_transform is a streaming kernel shaped like scene_params.hip: a workgroup owns chunks of kXfChunk consecutive
// Gaussians (grid capped at a few rounds of the resident workgroups, chunks strided over it).
//   * f_rest: the chunk's span (3 (K-1) floats per Gaussian, contiguous) is read lane j element j, sixteen independent
//     dwords per lane in flight, into LDS at an odd row stride; then one Gaussian per lane runs the band mat-vecs on its
//     own LDS row (conflict-free: odd stride), in place; then the span is written back out densely.  A row whose index is
//     out of range is never touched in LDS: it leaves with the bits it came with.
//   * xyz, scaling, rotation: one Gaussian per lane, as in scene_params.hip (the quaternion is one 16-byte access; the
//     3-float rows are strided dwords that together cover whole lines).
//   * the records: without idx the record is uniform over the grid, read through a const __restrict__ pointer at constant
//     offsets (scalar loads, the entries sit in scalar registers); with idx the T records are staged in LDS when they fit
//     beside the rows (64 KB in all), and gathered from global memory otherwise.
// In place (out == in): a chunk has one owner, which reads the chunk's f_rest whole into LDS before the barrier behind
// which it writes; a lane reads its own geometry rows before it writes them.  No atomics: the same bits every call.
#include <math.h>

#include <algorithm>

#include "lsr_internal.h"
#include "lsr_sh_shape.h"
#include "lsr_transform.h"
#include "lsr_sh_rotate.h"
#include "lsr_sh_rotate_basis.h"
#include "lsr_sh_rotate_tables.h"
#include "lsr_sh_basis_table.h"

namespace lsr {

constexpr int kXfChunk = 128;             // Gaussians per chunk = lanes per workgroup
constexpr int kXfLdsBytes = 65536;        // rows + staged records of one workgroup
constexpr int kXfCuLdsBytes = 160 * 1024;
constexpr int kXfCus = 256, kXfMaxBlocksPerCu = 16;   // (two-wave workgroups: 32 waves per CU)
constexpr int kXfRounds = 4;              // grid cap in rounds of resident workgroups (uniform and gathered records)
constexpr int kXfBatch = 16;              // dword loads in flight per lane
enum { kXfUniform = 0, kXfStaged = 1, kXfGather = 2 };

__host__ __device__ constexpr int xf_record_band(int l) { return LSR_TRANSFORM_HEADER_FLOATS + sh_band_offset(l) - 1; }
__host__ __device__ constexpr int xf_rows_bytes(int K) { return K > 1 ? kXfChunk * sh_rest_stride(K) * 4 : 16; }

// X <- (X + X^-T) / 2: one Newton step towards the orthogonal factor of X (X^-T = cofactors / det)
__device__ static void xf_polar_step(double (&X)[9]) {
    const double c[9] = {X[4] * X[8] - X[5] * X[7], X[5] * X[6] - X[3] * X[8], X[3] * X[7] - X[4] * X[6],
                         X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                         X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};
    const double det = X[0] * c[0] + X[1] * c[1] + X[2] * c[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) X[k] = 0.5 * (X[k] + c[k] / det);
}

// ---------------------------------------------------------------------------------------------------------------------
// Records.  One workgroup of 64 lanes per matrix; lane e < (degree+1)^2 is (band l, index e - l^2), as in
// k_sh_rotation_matrices: Y_l at the rotated sample directions, D_l = Y B^-1, E = D A^T, T = A E.
__global__ __launch_bounds__(64) void k_transform_records(int num, const float *__restrict__ mats, int degree, int adjoint,
                                                          float *__restrict__ records) {
    constexpr int full = LSR_SH_ROTATE_TABLE_FLOATS(LSR_TRANSFORM_MAX_DEGREE);
    __shared__ double sY[full], sD[full], sE[full];
    const int e = threadIdx.x;
    const float *m = mats + (size_t)blockIdx.x * 16;
    float *out = records + (size_t)blockIdx.x * LSR_TRANSFORM_RECORD_FLOATS(degree);
    double A[9], R[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) A[3 * a + b] = (double)m[4 * a + b];
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    const double s = cbrt(det);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = A[k] / s;
    // A / s is a rotation only to the rounding of the float32 entries (1e-7), and T_l and q_R are defined for rotations:
    // R is the rotation nearest to A / s, by three Newton steps of the polar decomposition (quadratic: 1e-5 -> 1e-20).
    for (int it = 0; it < 3; ++it) xf_polar_step(R);

    if (e == 0) {
        // the linear part is the matrix's own floats; the unit quaternion of R by the largest of the four pivots
        double w, x, y, z;
        const double tr = R[0] + R[4] + R[8];
        if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
            w = 0.5 * sqrt(1.0 + tr);
            const double f = 0.25 / w;
            x = (R[7] - R[5]) * f; y = (R[2] - R[6]) * f; z = (R[3] - R[1]) * f;
        } else if (R[0] >= R[4] && R[0] >= R[8]) {
            x = 0.5 * sqrt(1.0 + R[0] - R[4] - R[8]);
            const double f = 0.25 / x;
            w = (R[7] - R[5]) * f; y = (R[1] + R[3]) * f; z = (R[2] + R[6]) * f;
        } else if (R[4] >= R[8]) {
            y = 0.5 * sqrt(1.0 - R[0] + R[4] - R[8]);
            const double f = 0.25 / y;
            w = (R[2] - R[6]) * f; x = (R[1] + R[3]) * f; z = (R[5] + R[7]) * f;
        } else {
            z = 0.5 * sqrt(1.0 - R[0] - R[4] + R[8]);
            const double f = 0.25 / z;
            w = (R[3] - R[1]) * f; x = (R[2] + R[6]) * f; y = (R[5] + R[7]) * f;
        }
        const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
        w *= inv; x *= inv; y *= inv; z *= inv;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) out[3 * a + b] = adjoint ? m[4 * b + a] : m[4 * a + b];
#pragma unroll
        for (int a = 0; a < 3; ++a) out[9 + a] = adjoint ? 0.0f : m[4 * a + 3];
        out[12] = adjoint ? 0.0f : (float)log(s);
        out[13] = (float)w;
        out[14] = (float)(adjoint ? -x : x);
        out[15] = (float)(adjoint ? -y : y);
        out[16] = (float)(adjoint ? -z : z);
        out[17] = out[18] = out[19] = 0.0f;
    }

    int l = 0;
    while (l < LSR_TRANSFORM_MAX_DEGREE && (l + 1) * (l + 1) <= e) ++l;
    const int idx = e - l * l, n = 2 * l + 1, off = sh_band_offset(l);
    const bool active = e >= 1 && e < (degree + 1) * (degree + 1);
    if (active) {
        const double *x = kShRotDirs[l * l + idx];
        double y[9];
        sh_band_all(l, R[0] * x[0] + R[1] * x[1] + R[2] * x[2], R[3] * x[0] + R[4] * x[1] + R[5] * x[2],
                    R[6] * x[0] + R[7] * x[1] + R[8] * x[2], y);
#pragma unroll
        for (int i = 0; i < 9; ++i)
            if (i < n) sY[off + i * n + idx] = y[i];
    }
    __syncthreads();
    if (active) {        // row idx of D_l
        for (int j = 0; j < n; ++j) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += sY[off + idx * n + k] * kShRotBinv[off + k * n + j];
            sD[off + idx * n + j] = acc;
        }
        for (int j = 0; j < n; ++j) {     // row idx of E = D A^T (reads only this lane's row of D)
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += sD[off + idx * n + k] * kShBasisA[off + j * n + k];
            sE[off + idx * n + j] = acc;
        }
    }
    __syncthreads();
    if (active) {        // row idx of T = A E; the adjoint record holds the transpose
        float *band = out + xf_record_band(l);
        for (int j = 0; j < n; ++j) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += kShBasisA[off + idx * n + k] * sE[off + k * n + j];
            band[adjoint ? j * n + idx : idx * n + j] = (float)acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The pass over the parameters.

// band L of one Gaussian, all three channels, in place on the lane's LDS row: o_i = sum_j T[i][j] c_j
template <int L>
__device__ __forceinline__ void xf_band(const float *__restrict__ rec, float *row) {
    constexpr int n = 2 * L + 1, base = 3 * (L * L - 1);
    const float *T = rec + xf_record_band(L);
    float c[3 * n], o[3 * n];
#pragma unroll
    for (int k = 0; k < 3 * n; ++k) c[k] = row[base + k];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const float t0 = T[i * n];
        float a0 = t0 * c[0], a1 = t0 * c[1], a2 = t0 * c[2];
#pragma unroll
        for (int j = 1; j < n; ++j) {
            const float t = T[i * n + j];
            a0 = fmaf(t, c[3 * j], a0); a1 = fmaf(t, c[3 * j + 1], a1); a2 = fmaf(t, c[3 * j + 2], a2);
        }
        o[3 * i] = a0; o[3 * i + 1] = a1; o[3 * i + 2] = a2;
    }
#pragma unroll
    for (int k = 0; k < 3 * n; ++k) row[base + k] = o[k];
}

template <int K, int MODE>
__global__ __launch_bounds__(kXfChunk) void k_scene_transform(int64_t n, int T, const float *__restrict__ records,
                                                              const int32_t *__restrict__ idx, lsr_transform_in in,
                                                              lsr_transform_out out) {
    constexpr int G = kXfChunk, W = sh_rest_floats(K), WP = sh_rest_stride(K), PAD = WP - W;
    constexpr int RF = LSR_TRANSFORM_RECORD_FLOATS(sh_degree_of(K));
    __shared__ float s_rows[K > 1 ? G * WP : 4];
    extern __shared__ float4 xf_dyn[];                   // kXfStaged: the T records
    float *s_rec = reinterpret_cast<float *>(xf_dyn);
    const int tid = threadIdx.x;
    if constexpr (MODE == kXfStaged) {
        for (int i = tid; i < T * RF; i += G) s_rec[i] = records[i];    // (visible after the first barrier below)
    }
    const bool rest = K > 1 && out.features_rest != nullptr;
    const int64_t chunks = (n + G - 1) / G;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t g0 = c * G;
        const int nr = (int)(n - g0 < (int64_t)G ? n - g0 : (int64_t)G);
        const int total = W * nr;
        if constexpr (K > 1) {
            if (rest) {
                const float *src = in.features_rest + g0 * W;
                for (int j0 = tid; j0 < total; j0 += kXfBatch * G) {
                    float v[kXfBatch];
#pragma unroll
                    for (int u = 0; u < kXfBatch; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) v[u] = src[j];
                    }
#pragma unroll
                    for (int u = 0; u < kXfBatch; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) s_rows[j + (j / W) * PAD] = v[u];
                    }
                }
            }
        }
        // the lane's Gaussian and its record; out of range: the Gaussian passes through
        const int64_t gi = g0 + tid;
        bool valid = tid < nr;
        int id = 0;
        if constexpr (MODE != kXfUniform) {
            if (valid) {
                id = idx[gi];
                valid = (unsigned)id < (unsigned)T;
            }
            if (!valid) id = 0;
        }
        const float *rec = MODE == kXfUniform ? records : (MODE == kXfStaged ? s_rec + id * RF : records + (size_t)id * RF);
        __syncthreads();

        if constexpr (K > 1) {
            if (rest && valid) {
                float *row = s_rows + tid * WP;
                xf_band<1>(rec, row);
                if constexpr (K > 4) xf_band<2>(rec, row);
                if constexpr (K > 9) xf_band<3>(rec, row);
                if constexpr (K > 16) xf_band<4>(rec, row);
            }
        }
        if (tid < nr) {
            if (out.xyz) {
                const float *p = in.xyz + 3 * gi;
                float x0 = p[0], x1 = p[1], x2 = p[2];
                if (valid) {
                    const float y0 = fmaf(rec[0], x0, fmaf(rec[1], x1, fmaf(rec[2], x2, rec[9])));
                    const float y1 = fmaf(rec[3], x0, fmaf(rec[4], x1, fmaf(rec[5], x2, rec[10])));
                    const float y2 = fmaf(rec[6], x0, fmaf(rec[7], x1, fmaf(rec[8], x2, rec[11])));
                    x0 = y0; x1 = y1; x2 = y2;
                }
                float *o = out.xyz + 3 * gi;
                o[0] = x0; o[1] = x1; o[2] = x2;
            }
            if (out.scaling) {
                const float *p = in.scaling + 3 * gi;
                float s0 = p[0], s1 = p[1], s2 = p[2];
                if (valid) {
                    const float ls = rec[12];
                    s0 += ls; s1 += ls; s2 += ls;
                }
                float *o = out.scaling + 3 * gi;
                o[0] = s0; o[1] = s1; o[2] = s2;
            }
            if (out.rotation) {
                float4 q = reinterpret_cast<const float4 *>(in.rotation)[gi];
                if (valid) {
                    const float aw = rec[13], ax = rec[14], ay = rec[15], az = rec[16];
                    const float bw = q.x, bx = q.y, by = q.z, bz = q.w;
                    q.x = fmaf(aw, bw, fmaf(-ax, bx, fmaf(-ay, by, -az * bz)));
                    q.y = fmaf(aw, bx, fmaf(ax, bw, fmaf(ay, bz, -az * by)));
                    q.z = fmaf(aw, by, fmaf(-ax, bz, fmaf(ay, bw, az * bx)));
                    q.w = fmaf(aw, bz, fmaf(ax, by, fmaf(-ay, bx, az * bw)));
                }
                reinterpret_cast<float4 *>(out.rotation)[gi] = q;
            }
        }
        __syncthreads();

        if constexpr (K > 1) {
            if (rest) {
                float *dst = out.features_rest + g0 * W;
                for (int j0 = tid; j0 < total; j0 += kXfBatch * G) {
                    float v[kXfBatch];
#pragma unroll
                    for (int u = 0; u < kXfBatch; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) v[u] = s_rows[j + (j / W) * PAD];
                    }
#pragma unroll
                    for (int u = 0; u < kXfBatch; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) dst[j] = v[u];
                    }
                }
                __syncthreads();                         // s_rows is the next chunk's
            }
        }
    }
}

static int xf_mode(const lsr_transform_dims &d, const int32_t *idx) {
    if (!idx) return kXfUniform;
    const int64_t bytes = (int64_t)d.num_transforms * LSR_TRANSFORM_RECORD_FLOATS(sh_degree_of(d.sh_coeffs)) * 4;
    return xf_rows_bytes(d.sh_coeffs) + bytes + 64 <= kXfLdsBytes ? kXfStaged : kXfGather;
}

template <int K>
static void xf_launch(const lsr_transform_dims &d, const float *records, const int32_t *idx, const lsr_transform_in &in,
                      const lsr_transform_out &out, hipStream_t s) {
    const int mode = xf_mode(d, idx);
    const size_t dyn = mode == kXfStaged ? (size_t)d.num_transforms * LSR_TRANSFORM_RECORD_FLOATS(sh_degree_of(K)) * 4 : 0;
    // as many workgroups as are resident (by LDS, at most 16 two-wave workgroups per CU) when each stages the records;
    // otherwise up to kXfRounds times as many, so that a scene of a few rounds is handed out chunk by chunk as workgroups
    // retire instead of two chunks to some workgroups and one to the others
    const int per_cu = std::max(1, std::min<int>(kXfMaxBlocksPerCu, kXfCuLdsBytes / (int)(xf_rows_bytes(K) + dyn + 64)));
    const int64_t cap = (int64_t)kXfCus * per_cu * (mode == kXfStaged ? 1 : kXfRounds);
    const dim3 grid((unsigned)std::min<int64_t>((d.n + kXfChunk - 1) / kXfChunk, cap)), block(kXfChunk);
    if (mode == kXfUniform) hipLaunchKernelGGL((k_scene_transform<K, kXfUniform>), grid, block, 0, s, d.n, d.num_transforms, records, idx, in, out);
    else if (mode == kXfStaged) hipLaunchKernelGGL((k_scene_transform<K, kXfStaged>), grid, block, dyn, s, d.n, d.num_transforms, records, idx, in, out);
    else hipLaunchKernelGGL((k_scene_transform<K, kXfGather>), grid, block, 0, s, d.n, d.num_transforms, records, idx, in, out);
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_transform_records(int32_t T, const float *matrices, int32_t degree, int32_t adjoint, float *records,
                          lsr_stream_t stream) {
    note_hip_error(0);
    if (T < 0 || degree < 0 || degree > LSR_TRANSFORM_MAX_DEGREE || (adjoint != 0 && adjoint != 1)) return LSR_EINVAL;
    if (T == 0) return LSR_OK;
    if (!matrices || !records) return LSR_ENULL;
    hipLaunchKernelGGL(k_transform_records, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, (int)T, matrices, (int)degree,
                       (int)adjoint, records);
    return launch_status();
}

int lsr_scene_transform(const lsr_transform_dims *dims, const float *records, const int32_t *idx,
                        const lsr_transform_in *in, const lsr_transform_out *out, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !in || !out) return LSR_ENULL;
    const int K = dims->sh_coeffs;
    if (dims->n < 0 || !sh_valid_coeffs(K) || dims->num_transforms < 1) return LSR_EINVAL;
    if (dims->reserved0 || dims->reserved1) return LSR_EINVAL;
    if (K == 1 && (in->features_rest || out->features_rest)) return LSR_EINVAL;
    if (K > 1 && out->features_rest && !in->features_rest) return LSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in->rotation) | reinterpret_cast<uintptr_t>(out->rotation)) & 15) return LSR_EINVAL;
    if (dims->n == 0) return LSR_OK;
    if (!records || (out->xyz && !in->xyz) || (out->scaling && !in->scaling) || (out->rotation && !in->rotation)) return LSR_ENULL;
    if (!out->xyz && !out->features_rest && !out->scaling && !out->rotation) return LSR_OK;
    hipStream_t s = (hipStream_t)stream;
    dispatch_sh_coeffs(K, [&](auto k) { xf_launch<decltype(k)::value>(*dims, records, idx, *in, *out, s); });
    return launch_status();
}

}  // extern "C"
