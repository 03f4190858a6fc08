// ply.hip — 3DGS .ply export (include/lsr_ply.h): per-Gaussian vertex packing on the device and
// the binary file writer on the host.  Restates /root/reference/src/model/ply_export.py:26-92
// (no code taken); the quaternion <-> matrix conversions follow scipy's documented
// Rotation.from_quat / from_matrix (largest-of-diagonal-and-trace branch) in double precision so
// that the exported quaternion has the same sign as the reference's.
#include <stdio.h>

#include <algorithm>

#include "lsr_eig3.h"
#include "lsr_internal.h"
#include "lsr_ply.h"
#include "lsr_sh_shape.h"
#define LSR_SH_AXES_TABLE_QUALIFIER __device__
#include "lsr_sh_axes_table.h"

namespace lsr {

__global__ __launch_bounds__(256) void k_ply_pack(int64_t n, int d_sh, lsr_ply_inputs in, float *__restrict__ out) {
    __shared__ double Rv[9];                             // viewer rotation
    if (threadIdx.x == 0) {
        double m[9], inv[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m[3 * r + c] = in.extrinsics[4 * r + c];
        const double A = m[4] * m[8] - m[5] * m[7], B = -(m[3] * m[8] - m[5] * m[6]), C = m[3] * m[7] - m[4] * m[6];
        const double id = 1.0 / (m[0] * A + m[1] * B + m[2] * C);
        inv[0] = A * id; inv[1] = -(m[1] * m[8] - m[2] * m[7]) * id; inv[2] = (m[1] * m[5] - m[2] * m[4]) * id;
        inv[3] = B * id; inv[4] = (m[0] * m[8] - m[2] * m[6]) * id;  inv[5] = -(m[0] * m[5] - m[2] * m[3]) * id;
        inv[6] = C * id; inv[7] = -(m[0] * m[7] - m[1] * m[6]) * id; inv[8] = (m[0] * m[4] - m[1] * m[3]) * id;
        const double s = 0.70710678118654752440;
        // Rz(-45 deg) @ [[0,0,1],[-1,0,0],[0,-1,0]]
        const double base[9] = {-s, 0, s, -s, 0, -s, 0, -1, 0};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                Rv[3 * r + c] = base[3 * r] * inv[c] + base[3 * r + 1] * inv[3 + c] + base[3 * r + 2] * inv[6 + c];
    }
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const float sf = in.scale_factor[0];
    float p[3];
    for (int k = 0; k < 3; ++k) p[k] = (in.means[3 * g + k] - in.center[k]) / sf;
    float *v = out + g * LSR_PLY_VERTEX_FLOATS;
    for (int r = 0; r < 3; ++r)
        v[r] = (float)Rv[3 * r] * p[0] + (float)Rv[3 * r + 1] * p[1] + (float)Rv[3 * r + 2] * p[2];
    v[3] = v[4] = v[5] = 0.0f;
    for (int c = 0; c < 3; ++c) v[6 + c] = in.harmonics[(3 * g + c) * (int64_t)d_sh];
    v[9] = in.opacities[g];
    for (int k = 0; k < 3; ++k) v[10 + k] = logf(in.scales[3 * g + k] / sf);
    // orientation: normalise, to matrix, rotate, back to a quaternion
    double x = in.rotations[4 * g], y = in.rotations[4 * g + 1], z = in.rotations[4 * g + 2], w = in.rotations[4 * g + 3];
    const double nq = 1.0 / sqrt(x * x + y * y + z * z + w * w);
    x *= nq; y *= nq; z *= nq; w *= nq;
    const double Q[9] = {x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w),
                         2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w};
    double M[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[3 * r + c] = Rv[3 * r] * Q[c] + Rv[3 * r + 1] * Q[3 + c] + Rv[3 * r + 2] * Q[6 + c];
    const double tr = M[0] + M[4] + M[8];
    const double dec[4] = {M[0], M[4], M[8], tr};
    int choice = 0;
    for (int k = 1; k < 4; ++k)
        if (dec[k] > dec[choice]) choice = k;
    double q[4];
    if (choice != 3) {
        const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1.0 - tr + 2.0 * M[4 * i];
        q[j] = M[3 * j + i] + M[3 * i + j];
        q[k] = M[3 * k + i] + M[3 * i + k];
        q[3] = M[3 * k + j] - M[3 * j + k];
    } else {
        q[0] = M[7] - M[5];
        q[1] = M[2] - M[6];
        q[2] = M[3] - M[1];
        q[3] = 1.0 + tr;
    }
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    v[13] = (float)(q[3] * qn);
    v[14] = (float)(q[0] * qn);
    v[15] = (float)(q[1] * qn);
    v[16] = (float)(q[2] * qn);
}

// ---- import: rows of a standard 3DGS scene file -> the rasterizer's tensors (lsr_ply_unpack) ----
// A workgroup owns `rpb` consecutive rows.  Rows are 17 ... 89 floats (more with extra properties), so a lane that
// walked its own row in global memory would touch one dword of every cache line per load; instead the workgroup's
// block of rows — one contiguous span of rpb * stride floats — is copied into LDS with lane-dense loads (dwordx4
// from the first 16-byte boundary of the span on, single dwords before it and behind the last full quad: neither a
// row nor a block starts aligned in general), and every output is produced by a loop over OUTPUT elements, lane j
// element j, reading its source from LDS.  means / shs / opacities / scales are elementwise, so those loops are all
// there is; rotations are one dwordx4 store per lane; the covariance (one quaternion -> 6 values per Gaussian) is
// computed per Gaussian, staged in LDS and stored by such a loop as well.
// LDS layout (floats): [pad: (address of the span / 4) % 4][rpb * stride rows][cov staging 6 * rpb].  The pad gives the
// LDS copy the global span's 16-byte phase, so that the quad loads are stored as aligned quads.
// (the loops below step by the workgroup size; without this the loop vectoriser adds a second copy of each for a
// workgroup of one lane)
#define PLY_NO_VECTORIZE _Pragma("clang loop vectorize(disable) interleave(disable)")
constexpr int kPlyMaxThreads = 256;
constexpr int kPlyLdsBytes = 64 * 1024 - 512;      // dynamic LDS a launch may ask for next to the offset table

template <int K>
__global__ __launch_bounds__(kPlyMaxThreads) void k_ply_unpack(lsr_ply_layout L, int rpb, int flags,
                                                              const float *__restrict__ rows, lsr_ply_outputs out) {
    extern __shared__ float4 ply_lds4[];
    __shared__ int sh_off[3 * K];                        // row offset of shs[g][k][c] at [3 k + c]
    float *const lds = reinterpret_cast<float *>(ply_lds4);
    const int tid = threadIdx.x, nt = blockDim.x, stride = L.stride;
    const int64_t g0 = (int64_t)blockIdx.x * rpb;
    const int nr = (int)(L.n - g0 < (int64_t)rpb ? L.n - g0 : (int64_t)rpb);
    const float *const src = rows + g0 * stride;
    const int total = nr * stride;
    const int phase = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    float *const tile = lds + phase;
    float *const stage = lds + 4 + rpb * stride;

    for (int e = tid; e < 3 * K; e += nt) {
        const int k = e / 3, c = e - 3 * k;
        sh_off[e] = k == 0 ? (c == 0 ? L.f_dc[0] : (c == 1 ? L.f_dc[1] : L.f_dc[2])) : L.f_rest[c * (K - 1) + k - 1];
    }
    // the span into LDS
    const int head = min((4 - phase) & 3, total);
    const int nquad = (total - head) >> 2;
    if (tid < head) tile[tid] = src[tid];
    {
        const float4 *const s4 = reinterpret_cast<const float4 *>(src + head);
        float4 *const t4 = reinterpret_cast<float4 *>(tile + head);
        for (int i = tid; i < nquad; i += nt) t4[i] = s4[i];
    }
    for (int i = head + 4 * nquad + tid; i < total; i += nt) tile[i] = src[i];
    __syncthreads();

    // one Gaussian per lane: quaternion, covariance
    if (out.rotations || out.cov3D) {
        for (int r = tid; r < nr; r += nt) {
            const float *row = tile + r * stride;
            float w = row[L.rot[0]], x = row[L.rot[1]], y = row[L.rot[2]], z = row[L.rot[3]];
            const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
            w *= inv; x *= inv; y *= inv; z *= inv;
            if (out.rotations) reinterpret_cast<float4 *>(out.rotations)[g0 + r] = make_float4(w, x, y, z);
            if (out.cov3D) {
                const float s0 = expf(row[L.scale[0]]), s1 = expf(row[L.scale[1]]), s2 = expf(row[L.scale[2]]);
                // M = R diag(s); Sigma = M M^T
                const float m00 = (1.0f - 2.0f * (y * y + z * z)) * s0, m01 = 2.0f * (x * y - w * z) * s1, m02 = 2.0f * (x * z + w * y) * s2;
                const float m10 = 2.0f * (x * y + w * z) * s0, m11 = (1.0f - 2.0f * (x * x + z * z)) * s1, m12 = 2.0f * (y * z - w * x) * s2;
                const float m20 = 2.0f * (x * z - w * y) * s0, m21 = 2.0f * (y * z + w * x) * s1, m22 = (1.0f - 2.0f * (x * x + y * y)) * s2;
                float *st = stage + 6 * r;
                st[0] = m00 * m00 + m01 * m01 + m02 * m02;
                st[1] = m00 * m10 + m01 * m11 + m02 * m12;
                st[2] = m00 * m20 + m01 * m21 + m02 * m22;
                st[3] = m10 * m10 + m11 * m11 + m12 * m12;
                st[4] = m10 * m20 + m11 * m21 + m12 * m22;
                st[5] = m20 * m20 + m21 * m21 + m22 * m22;
            }
        }
    }
    if (out.means) {
        float *dst = out.means + g0 * 3;
        PLY_NO_VECTORIZE
        for (int j = tid; j < 3 * nr; j += nt) {
            const int r = j / 3, c = j - 3 * r;
            dst[j] = tile[r * stride + (c == 0 ? L.xyz[0] : (c == 1 ? L.xyz[1] : L.xyz[2]))];
        }
    }
    if (out.scales) {
        float *dst = out.scales + g0 * 3;
        PLY_NO_VECTORIZE
        for (int j = tid; j < 3 * nr; j += nt) {
            const int r = j / 3, c = j - 3 * r;
            dst[j] = expf(tile[r * stride + (c == 0 ? L.scale[0] : (c == 1 ? L.scale[1] : L.scale[2]))]);
        }
    }
    if (out.opacities) {
        for (int r = tid; r < nr; r += nt) {
            const float v = tile[r * stride + L.opacity];
            out.opacities[g0 + r] = (flags & LSR_PLY_OPACITY_RAW) ? v : 1.0f / (1.0f + expf(-v));
        }
    }
    if (out.shs) {
        float *dst = out.shs + g0 * (3 * K);
        PLY_NO_VECTORIZE
        for (int j = tid; j < 3 * K * nr; j += nt) {
            const int r = j / (3 * K), e = j - 3 * K * r;
            dst[j] = tile[r * stride + sh_off[e]];
        }
    }
    if (out.cov3D) {
        __syncthreads();
        float *dst = out.cov3D + g0 * 6;
        PLY_NO_VECTORIZE
        for (int j = tid; j < 6 * nr; j += nt) dst[j] = stage[j];
    }
}

template <int K>
static void launch_ply_unpack(const lsr_ply_layout &L, int rpb, int threads, size_t lds, int flags, const float *rows,
                              const lsr_ply_outputs &out, hipStream_t s) {
    const int64_t blocks = (L.n + rpb - 1) / rpb;
    hipLaunchKernelGGL(k_ply_unpack<K>, dim3((unsigned)blocks), dim3(threads), lds, s, L, rpb, flags, rows, out);
}


// ---- scene export: the rasterizer's tensors -> rows of a standard 3DGS scene file (lsr_ply_pack_scene) ----
// The unpack run backwards.  A workgroup owns `rpb` consecutive Gaussians; their rows are one contiguous span of
// rpb * STRIDE floats of the output table, which is assembled in LDS and leaves with lane-dense dwordx4 stores (single
// dwords up to the span's first 16-byte boundary and behind its last full quad; the LDS image has the span's 16-byte
// phase).  Every input is read by a loop over INPUT elements, lane j element j, and scattered into the image; the
// covariances (or scales and rotations) are staged in LDS the same way and then decomposed one Gaussian per lane
// (lsr_eig3.h: 6 + 9 floats in registers).  Colour SH is first re-laid out as it is — for LSR_SH_AXES_3DGS that is all,
// bit for bit — and for LSR_SH_AXES_REFERENCE each (Gaussian, channel) lane then multiplies its bands by M_l in place,
// M as floats in LDS (every lane reads the same entry: a broadcast).  Band 0 is left alone: M_0 rounds to 1.0f.
// LDS layout (floats): [pad: (address of the span / 4) % 4][rpb * STRIDE image][geometry staging 9 * rpb] + the table.
// No atomics; one owner per row.
constexpr int kPlyPackRows = 128;                    // 128 * (89 + 9) floats = 49 KiB at degree 4

constexpr int sh_axes_table_floats(int deg) { return (deg + 1) * (2 * deg + 1) * (2 * deg + 3) / 3; }

// f[0 .. 2L] <- M_L f, M row-major in LDS
template <int L>
__device__ __forceinline__ void sh_axes_band(float *f, const float *M) {
    constexpr int N = 2 * L + 1;
    float v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = f[j];
#pragma unroll 1                                         // (unrolled, band 4 holds its 81 entries in registers: 225 VGPRs)
    for (int i = 0; i < N; ++i) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) acc = fmaf(M[N * i + j], v[j], acc);
        f[i] = acc;
    }
}

template <int K>
__global__ __launch_bounds__(kPlyMaxThreads) void k_ply_pack_scene(int64_t n, int rpb, int reference, lsr_ply_scene_inputs in,
                                                                  float *__restrict__ rows) {
    constexpr int STRIDE = LSR_PLY_SCENE_ROW_FLOATS(K), OPA = 6 + 3 * K, DEG = sh_degree_of(K);
    constexpr int TABLE = sh_axes_table_floats(DEG);
    extern __shared__ float4 ply_lds4[];
    __shared__ float shM[TABLE];
    float *const lds = reinterpret_cast<float *>(ply_lds4);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t g0 = (int64_t)blockIdx.x * rpb;
    const int nr = (int)(n - g0 < (int64_t)rpb ? n - g0 : (int64_t)rpb);
    float *const dst = rows + g0 * STRIDE;
    const int total = nr * STRIDE;
    const int phase = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    float *const tile = lds + phase;
    float *const geo = lds + 4 + rpb * STRIDE;
    const int Kin = in.sh_coeffs, ce = in.cov_elems;
    const bool basis_change = reference && K > 1;

    // geometry inputs into the staging area, lane-dense
    if (in.cov) {
        const float *src = in.cov + g0 * ce;
        PLY_NO_VECTORIZE
        for (int j = tid; j < ce * nr; j += nt) geo[j] = src[j];
    } else {
        const float *ss = in.scales + g0 * 3, *sq = in.rotations + g0 * 4;
        PLY_NO_VECTORIZE
        for (int j = tid; j < 3 * nr; j += nt) geo[j] = ss[j];
        PLY_NO_VECTORIZE
        for (int j = tid; j < 4 * nr; j += nt) geo[3 * rpb + j] = sq[j];
    }
    if (basis_change)
        for (int i = tid; i < TABLE; i += nt) shM[i] = (float)kShAxesM[i];
    {   // means, normals
        const float *src = in.means + g0 * 3;
        PLY_NO_VECTORIZE
        for (int j = tid; j < 3 * nr; j += nt) {
            const int r = j / 3, c = j - 3 * r;
            tile[r * STRIDE + c] = src[j];
            tile[r * STRIDE + 3 + c] = 0.0f;
        }
    }
    for (int r = tid; r < nr; r += nt) {                     // opacity -> logit in [-20, 20]; a NaN passes through
        const float p = in.opacities[g0 + r];
        const float v = logf(p / (1.0f - p));
        tile[r * STRIDE + OPA] = v < -20.0f ? -20.0f : (v > 20.0f ? 20.0f : v);
    }
    {   // colour SH: shs[g][k][c] (or [g][c][k]) -> f_dc_c, f_rest_{c (K - 1) + k - 1}; coefficients k >= K are dropped
        const float *src = in.shs + g0 * 3 * Kin;
        if (in.sh_channel_major) {
            PLY_NO_VECTORIZE
            for (int j = tid; j < 3 * K * nr; j += nt) {
                const int r = j / (3 * K), e = j - 3 * K * r, c = e / K, k = e - K * c;
                tile[r * STRIDE + (k == 0 ? 6 + c : 8 + c * (K - 1) + k)] = src[r * 3 * Kin + c * Kin + k];
            }
        } else {
            PLY_NO_VECTORIZE
            for (int j = tid; j < 3 * K * nr; j += nt) {
                const int r = j / (3 * K), e = j - 3 * K * r, k = e / 3, c = e - 3 * k;
                tile[r * STRIDE + (k == 0 ? 6 + c : 8 + c * (K - 1) + k)] = src[r * 3 * Kin + e];
            }
        }
    }
    __syncthreads();

    // one Gaussian per lane: log-scales and the quaternion
    for (int r = tid; r < nr; r += nt) {
        float ls[3], q[4];
        if (in.cov) {
            const float *c = geo + r * ce;
            float c6[6];
            if (ce == 6) {
#pragma unroll
                for (int k = 0; k < 6; ++k) c6[k] = c[k];
            } else {
                c6[0] = c[0]; c6[1] = c[1]; c6[2] = c[2]; c6[3] = c[4]; c6[4] = c[5]; c6[5] = c[8];
            }
            eig3_scale_rotation(c6, ls, q);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) ls[k] = logf(geo[3 * r + k]);
            const float *qs = geo + 3 * rpb + 4 * r;
            const float w = qs[0], x = qs[1], y = qs[2], z = qs[3];
            float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
            if (w < 0.0f) inv = -inv;
            q[0] = w * inv; q[1] = x * inv; q[2] = y * inv; q[3] = z * inv;
        }
        float *o = tile + r * STRIDE + OPA + 1;
        o[0] = ls[0]; o[1] = ls[1]; o[2] = ls[2];
        o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
    }
    // reference -> 3dgs basis, in place: one (Gaussian, channel) per lane
    if (basis_change) {
        for (int j = tid; j < 3 * nr; j += nt) {
            const int r = j / 3, c = j - 3 * r;
            float *f = tile + r * STRIDE + 9 + c * (K - 1);     // f[k - 1]: coefficient k of this channel
            if constexpr (DEG >= 1) sh_axes_band<1>(f, shM + sh_axes_table_floats(0));
            if constexpr (DEG >= 2) sh_axes_band<2>(f + 3, shM + sh_axes_table_floats(1));
            if constexpr (DEG >= 3) sh_axes_band<3>(f + 8, shM + sh_axes_table_floats(2));
            if constexpr (DEG >= 4) sh_axes_band<4>(f + 15, shM + sh_axes_table_floats(3));
        }
    }
    __syncthreads();

    // the image out
    const int head = min((4 - phase) & 3, total);
    const int nquad = (total - head) >> 2;
    if (tid < head) dst[tid] = tile[tid];
    {
        float4 *const d4 = reinterpret_cast<float4 *>(dst + head);
        const float4 *const t4 = reinterpret_cast<const float4 *>(tile + head);
        for (int i = tid; i < nquad; i += nt) d4[i] = t4[i];
    }
    for (int i = head + 4 * nquad + tid; i < total; i += nt) dst[i] = tile[i];
}

template <int K>
static void launch_ply_pack_scene(int64_t n, int reference, const lsr_ply_scene_inputs &in, float *rows, hipStream_t s) {
    const int rpb = kPlyPackRows;
    const size_t lds = sizeof(float) * (4 + (size_t)rpb * (LSR_PLY_SCENE_ROW_FLOATS(K) + 9));
    static_assert(sizeof(float) * (4 + (size_t)kPlyPackRows * (LSR_PLY_SCENE_ROW_FLOATS(K) + 9)) + 165 * sizeof(float) <= 64 * 1024,
                  "a block of rows, its geometry staging and the table fit the per-workgroup LDS");
    hipLaunchKernelGGL(k_ply_pack_scene<K>, dim3((unsigned)((n + rpb - 1) / rpb)), dim3(kPlyMaxThreads), lds, s, n, rpb,
                       reference, in, rows);
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_ply_pack(int64_t n, int32_t d_sh, const lsr_ply_inputs *in, float *vertices, lsr_stream_t stream) {
    note_hip_error(0);
    if (n < 0 || d_sh < 1) return LSR_EINVAL;
    if (!in) return LSR_ENULL;
    if (n == 0) return LSR_OK;
    if (!in->extrinsics || !in->means || !in->scales || !in->rotations || !in->harmonics || !in->opacities ||
        !in->center || !in->scale_factor || !vertices)
        return LSR_ENULL;
    if ((n + 255) / 256 > 0x7fffffffLL) return LSR_EUNSUPPORTED;
    hipLaunchKernelGGL(k_ply_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, d_sh, *in, vertices);
    return launch_status();
}

int lsr_ply_unpack(const lsr_ply_layout *layout, const float *rows, int32_t flags, const lsr_ply_outputs *out,
                   lsr_stream_t stream) {
    note_hip_error(0);
    if (!layout || !out) return LSR_ENULL;
    const lsr_ply_layout &L = *layout;
    const int K = L.sh_coeffs;
    if (L.n < 0 || L.stride < 1 || L.stride > LSR_PLY_MAX_STRIDE || (flags & ~LSR_PLY_OPACITY_RAW)) return LSR_EINVAL;
    if (!sh_valid_coeffs(K)) return LSR_EINVAL;
    // every offset the kernel may read lies inside the row (and with it inside the workgroup's LDS block)
    const auto inside = [&](const int32_t *o, int count) {
        for (int k = 0; k < count; ++k)
            if (o[k] < 0 || o[k] >= L.stride) return false;
        return true;
    };
    if (!inside(L.xyz, 3) || !inside(L.f_dc, 3) || !inside(&L.opacity, 1) || !inside(L.scale, 3) || !inside(L.rot, 4) ||
        !inside(L.f_rest, 3 * (K - 1)))
        return LSR_EINVAL;
    if (L.n == 0) return LSR_OK;
    if (!rows) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) || (reinterpret_cast<uintptr_t>(out->rotations) & 15)) return LSR_EINVAL;
    // rows per workgroup: 128 (LSR_PLY_UNPACK_ROWS, a development knob, takes any 1 ... 256; multiples of 64 are what
    // tools/bench_ply_import.py --rows compares: DESIGN.md section 2.8), or as many as the LDS budget holds
    const int per_row = (L.stride + 6) * (int)sizeof(float);
    int rpb = std::min(std::max(env_int("LSR_PLY_UNPACK_ROWS", 128), 1), kPlyMaxThreads);
    rpb = std::min(rpb, (kPlyLdsBytes - 16) / per_row);
    if (rpb >= 64) rpb &= ~63;
    const int threads = std::min(kPlyMaxThreads, (rpb + 63) & ~63);
    const size_t lds = 16 + (size_t)rpb * per_row;
    if ((L.n + rpb - 1) / rpb > 0x7fffffffLL) return LSR_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    dispatch_sh_coeffs(K, [&](auto k) { launch_ply_unpack<decltype(k)::value>(L, rpb, threads, lds, flags, rows, *out, s); });
    return launch_status();
}

int lsr_ply_pack_scene(int64_t n, const lsr_ply_scene_inputs *in, const lsr_ply_scene_opts *opts, float *rows,
                       lsr_stream_t stream) {
    note_hip_error(0);
    if (!in || !opts) return LSR_ENULL;
    const int K = opts->sh_coeffs_out;
    if (n < 0 || !sh_valid_coeffs(in->sh_coeffs) || !sh_valid_coeffs(K) || K > in->sh_coeffs) return LSR_EINVAL;
    if (opts->sh_convention != LSR_SH_AXES_3DGS && opts->sh_convention != LSR_SH_AXES_REFERENCE) return LSR_EINVAL;
    if ((in->sh_channel_major & ~1) || in->reserved0 || opts->reserved0 || opts->reserved1) return LSR_EINVAL;
    if (in->cov && in->cov_elems != 6 && in->cov_elems != 9) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!in->means || !in->opacities || !in->shs || !rows) return LSR_ENULL;
    if (!in->cov && (!in->scales || !in->rotations)) return LSR_ENULL;
    const uintptr_t align = reinterpret_cast<uintptr_t>(in->means) | reinterpret_cast<uintptr_t>(in->opacities) |
                            reinterpret_cast<uintptr_t>(in->shs) | reinterpret_cast<uintptr_t>(in->cov) |
                            reinterpret_cast<uintptr_t>(in->scales) | reinterpret_cast<uintptr_t>(in->rotations) |
                            reinterpret_cast<uintptr_t>(rows);
    if (align & 3) return LSR_EINVAL;
    if ((n + kPlyPackRows - 1) / kPlyPackRows > 0x7fffffffLL) return LSR_EUNSUPPORTED;
    const int reference = opts->sh_convention == LSR_SH_AXES_REFERENCE;
    hipStream_t s = (hipStream_t)stream;
    dispatch_sh_coeffs(K, [&](auto k) { launch_ply_pack_scene<decltype(k)::value>(n, reference, *in, rows, s); });
    return launch_status();
}

int lsr_ply_write_host(const char *path, const float *vertices_host, int64_t n) {
    if (!path || (n > 0 && !vertices_host)) return LSR_ENULL;
    if (n < 0) return LSR_EINVAL;
    FILE *f = fopen(path, "wb");
    if (!f) return LSR_EINVAL;
    static const char *props[LSR_PLY_VERTEX_FLOATS] = {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2",
                                                       "opacity", "scale_0", "scale_1", "scale_2",
                                                       "rot_0", "rot_1", "rot_2", "rot_3"};
    bool ok = fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\n", (long long)n) > 0;
    for (int k = 0; k < LSR_PLY_VERTEX_FLOATS && ok; ++k) ok = fprintf(f, "property float %s\n", props[k]) > 0;
    ok = ok && fprintf(f, "end_header\n") > 0;
    if (ok && n > 0) ok = fwrite(vertices_host, sizeof(float) * LSR_PLY_VERTEX_FLOATS, (size_t)n, f) == (size_t)n;
    ok = (fclose(f) == 0) && ok;
    return ok ? LSR_OK : LSR_EINVAL;
}

}  // extern "C"
