// scene_params.hip — the 3DGS activation map (include/lsr_scene.h): the raw parameters a trainer holds (f_dc, f_rest,
// opacity logits, log-scales, unnormalised quaternions) -> the rasterizer's shs / opacities / cov3D, and the backward of
// that map, one launch each.  The forward arithmetic is k_ply_unpack's (ply.hip), taken from live tensors instead of a row
// table, with the scale modifier folded into the scale before it enters M = R diag(s).
//
// A streaming kernel: of the 3 K + 8 floats per Gaussian, 3 K are a pure copy.  A workgroup owns chunks of kSceneChunk
// consecutive Gaussians (grid capped at kSceneMaxBlocks, chunks strided over it); the spans of features_dc, features_rest
// and shs that belong to a chunk are each contiguous, so
//   * the SH concat (forward) / split (backward) is a loop over the elements of the big span, lane j element j, four
//     independent elements per lane in flight.  The three dc floats per Gaussian — 12 bytes every 12 K — would be the one
//     sparse access; they cross through LDS instead (their span is read / written densely on its own);
//   * the geometry runs one Gaussian per lane: the quaternion is one 16-byte access; the 3- and 6-float rows are
//     accessed directly by their lane: the three / six strided dword accesses of a wave together cover whole cache
//     lines, and the lines stay in the vector cache between them (DESIGN.md section 2.10 has the measurement against
//     staging them through LDS as ply.hip does).
// Indices are 64-bit from the chunk base on (3 K n passes 2^31 near 30 M Gaussians); inside a chunk they are ints
// (at most 75 * 256).  One owner per output element, no atomics: two calls give the same bits.
//
// The filtered pair (lsr_scene_activate_filtered_*) is the same two kernel bodies instantiated with FILTERED = true: with
// the 3D smoothing filter f of the Gaussian (lsr_filter3d.h), s_k = exp(scaling_k) and v_k = s_k^2 + f^2, the scale that
// enters M is m sqrt(v_k) and the opacity is multiplied by c = prod_k s_k / sqrt(v_k): three ratios, each at most 1, never
// sqrt(det / det) (a product of six small scales leaves float32 long before a ratio does).  4 bytes more per Gaussian
// each way.  Every statement of the unfiltered instantiation is the one it was: the same bits.
#include <math.h>

#include <algorithm>

#include "lsr_internal.h"
#include "lsr_sh_shape.h"
#include "lsr_scene.h"

namespace lsr {

constexpr int kSceneChunk = 256;        // Gaussians per chunk = lanes per workgroup
constexpr int kSceneMaxBlocks = 2048;   // 256 CUs x 8 resident workgroups
#define SCENE_NO_VECTORIZE _Pragma("clang loop vectorize(disable) interleave(disable)")

// dst[j] = src[j] (or 0 when src is NULL) for j < count, lane j element j
__device__ __forceinline__ void scene_copy(float *__restrict__ dst, const float *__restrict__ src, int count, int tid) {
    SCENE_NO_VECTORIZE
    for (int j = tid; j < count; j += kSceneChunk) dst[j] = src ? src[j] : 0.0f;
}

// The filtered scales of one Gaussian: r_k = sqrt(s_k^2 + f^2) and the ratios s_k / r_k (each <= 1), s_k = exp(ls[k]).
__device__ __forceinline__ void scene_filtered_scales(const float *ls, float f, float (&s)[3], float (&v)[3], float (&r)[3],
                                                      float (&ratio)[3]) {
    const float f2 = f * f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = expf(ls[k]);
        v[k] = fmaf(s[k], s[k], f2);
        r[k] = sqrtf(v[k]);
        ratio[k] = s[k] / r[k];
    }
}

template <int K, bool FILTERED>
__global__ __launch_bounds__(kSceneChunk) void k_scene_fwd(int64_t n, float m, lsr_scene_params p, lsr_scene_outputs o,
                                                          const float *filter3d) {
    constexpr int E = 3 * K, G = kSceneChunk;
    __shared__ float s_dc[3 * G];
    const int tid = threadIdx.x;
    const int64_t chunks = (n + G - 1) / G;
    const bool geo = o.cov3D || o.scales || o.rotations;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t g0 = c * G;
        const int nr = (int)(n - g0 < (int64_t)G ? n - g0 : (int64_t)G);
        if (o.shs && K > 1) scene_copy(s_dc, p.features_dc + g0 * 3, 3 * nr, tid);
        __syncthreads();

        if (o.shs) {
            float *dst = o.shs + g0 * E;
            const int total = E * nr;
            if constexpr (K == 1) {
                scene_copy(dst, p.features_dc + g0 * 3, total, tid);
            } else {
                const float *rest = p.features_rest + g0 * (E - 3);
                for (int j0 = tid; j0 < total; j0 += 4 * G) {
                    float v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) {
                            const int g = j / E, e = j - E * g;
                            v[u] = e < 3 ? s_dc[3 * g + e] : rest[j - 3 * g - 3];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) dst[j] = v[u];
                    }
                }
            }
        }
        if constexpr (FILTERED) {
            if (o.opacities && tid < nr) {
                float s[3], v[3], r[3], ratio[3];
                scene_filtered_scales(p.scaling + 3 * (g0 + tid), filter3d[g0 + tid], s, v, r, ratio);
                o.opacities[g0 + tid] = (1.0f / (1.0f + expf(-p.opacity[g0 + tid]))) * (ratio[0] * ratio[1] * ratio[2]);
            }
        } else {
            if (o.opacities && tid < nr) o.opacities[g0 + tid] = 1.0f / (1.0f + expf(-p.opacity[g0 + tid]));
        }

        // one Gaussian per lane: quaternion, scales, covariance
        if (geo && tid < nr) {
            const int64_t gi = g0 + tid;
            const float4 q = reinterpret_cast<const float4 *>(p.rotation)[gi];
            float w = q.x, x = q.y, y = q.z, z = q.w;
            const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
            w *= inv; x *= inv; y *= inv; z *= inv;
            if (o.rotations) reinterpret_cast<float4 *>(o.rotations)[gi] = make_float4(w, x, y, z);
            const float *ls = p.scaling + 3 * gi;
            float s0, s1, s2;
            if constexpr (FILTERED) {
                float s[3], v[3], r[3], ratio[3];
                scene_filtered_scales(ls, filter3d[gi], s, v, r, ratio);
                s0 = m * r[0]; s1 = m * r[1]; s2 = m * r[2];
            } else {
                s0 = m * expf(ls[0]); s1 = m * expf(ls[1]); s2 = m * expf(ls[2]);
            }
            if (o.scales) {
                float *sc = o.scales + 3 * gi;
                sc[0] = s0; sc[1] = s1; sc[2] = s2;
            }
            if (o.cov3D) {
                // M = R diag(s); Sigma = M M^T
                const float m00 = (1.0f - 2.0f * (y * y + z * z)) * s0, m01 = 2.0f * (x * y - w * z) * s1, m02 = 2.0f * (x * z + w * y) * s2;
                const float m10 = 2.0f * (x * y + w * z) * s0, m11 = (1.0f - 2.0f * (x * x + z * z)) * s1, m12 = 2.0f * (y * z - w * x) * s2;
                const float m20 = 2.0f * (x * z - w * y) * s0, m21 = 2.0f * (y * z + w * x) * s1, m22 = (1.0f - 2.0f * (x * x + y * y)) * s2;
                float *st = o.cov3D + 6 * gi;
                st[0] = m00 * m00 + m01 * m01 + m02 * m02;
                st[1] = m00 * m10 + m01 * m11 + m02 * m12;
                st[2] = m00 * m20 + m01 * m21 + m02 * m22;
                st[3] = m10 * m10 + m11 * m11 + m12 * m12;
                st[4] = m10 * m20 + m11 * m21 + m12 * m22;
                st[5] = m20 * m20 + m21 * m21 + m22 * m22;
            }
        }
        __syncthreads();                                 // s_dc is the next chunk's
    }
}

template <int K, bool FILTERED>
__global__ __launch_bounds__(kSceneChunk) void k_scene_bwd(int64_t n, float m, lsr_scene_params p, lsr_scene_out_grads g,
                                                          lsr_scene_in_grads d, const float *filter3d) {
    constexpr int E = 3 * K, G = kSceneChunk;
    __shared__ float s_dc[3 * G];
    const int tid = threadIdx.x;
    const int64_t chunks = (n + G - 1) / G;
    const bool geo = d.scaling || d.rotation;
    float *const d_rest_all = K > 1 ? d.features_rest : nullptr;
    // the dc gradients cross through LDS when the pass over the shs gradient runs anyway (for the rest gradients)
    const bool dc_via_lds = d.features_dc && d_rest_all && g.shs;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t g0 = c * G;
        const int nr = (int)(n - g0 < (int64_t)G ? n - g0 : (int64_t)G);
        // colour SH: the forward's re-layout run backwards
        if (d_rest_all) {
            float *drest = d_rest_all + g0 * (E - 3);
            if (!g.shs) {
                scene_copy(drest, nullptr, (E - 3) * nr, tid);
            } else {
                const float *src = g.shs + g0 * E;
                const int total = E * nr;
                for (int j0 = tid; j0 < total; j0 += 4 * G) {
                    float v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) v[u] = src[j];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + u * G;
                        if (j < total) {
                            const int gg = j / E, e = j - E * gg;
                            if (e >= 3) drest[j - 3 * gg - 3] = v[u];
                            else if (dc_via_lds) s_dc[3 * gg + e] = v[u];
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (d.features_dc) {
            float *ddc = d.features_dc + g0 * 3;
            if (dc_via_lds) {
                scene_copy(ddc, s_dc, 3 * nr, tid);
            } else if (!g.shs) {
                scene_copy(ddc, nullptr, 3 * nr, tid);
            } else {                                     // dc alone (or K == 1, where this is dense): gathered
                const float *src = g.shs + g0 * E;
                SCENE_NO_VECTORIZE
                for (int j = tid; j < 3 * nr; j += G) {
                    const int gg = j / 3;
                    ddc[j] = src[j + (E - 3) * gg];
                }
            }
        }
        if constexpr (FILTERED) {
            if (d.opacity && tid < nr) {
                float s[3], v[3], r[3], ratio[3];
                scene_filtered_scales(p.scaling + 3 * (g0 + tid), filter3d[g0 + tid], s, v, r, ratio);
                const float o = 1.0f / (1.0f + expf(-p.opacity[g0 + tid]));
                d.opacity[g0 + tid] = g.opacities ? g.opacities[g0 + tid] * (ratio[0] * ratio[1] * ratio[2]) * (o * (1.0f - o)) : 0.0f;
            }
        } else {
            if (d.opacity && tid < nr) {
                const float o = 1.0f / (1.0f + expf(-p.opacity[g0 + tid]));
                d.opacity[g0 + tid] = g.opacities ? g.opacities[g0 + tid] * o * (1.0f - o) : 0.0f;
            }
        }

        // one Gaussian per lane
        if (geo && tid < nr) {
            const int64_t gi = g0 + tid;
            const float4 q = reinterpret_cast<const float4 *>(p.rotation)[gi];
            float w = q.x, x = q.y, y = q.z, z = q.w;
            const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
            w *= inv; x *= inv; y *= inv; z *= inv;
            const float *ls = p.scaling + 3 * gi;
            // s: the scale that enters M; FILTERED: chain[k] = d log s_k / d scaling_k = exp(2 scaling_k) / v_k, and
            // extra[k] = g_o o c f^2 / v_k, the opacity coefficient's share
            float s[3], chain[3], extra[3];
            if constexpr (FILTERED) {
                float e[3], v[3], r[3], ratio[3];
                const float f = filter3d[gi];
                scene_filtered_scales(ls, f, e, v, r, ratio);
                const float go = g.opacities ? g.opacities[gi] : 0.0f;
                const float goc = go * (1.0f / (1.0f + expf(-p.opacity[gi]))) * (ratio[0] * ratio[1] * ratio[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    s[k] = m * r[k];
                    chain[k] = ratio[k] * ratio[k];
                    extra[k] = goc * ((f * f) / v[k]);
                }
            } else {
                s[0] = m * expf(ls[0]); s[1] = m * expf(ls[1]); s[2] = m * expf(ls[2]);
            }
            float gc[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) gc[k] = g.cov3D ? g.cov3D[6 * gi + k] : 0.0f;
            // G: the diagonal as given, each off-diagonal entry half of its packed value
            const float Gm[9] = {gc[0], 0.5f * gc[1], 0.5f * gc[2],
                                 0.5f * gc[1], gc[3], 0.5f * gc[4],
                                 0.5f * gc[2], 0.5f * gc[4], gc[5]};
            const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - w * z), 2.0f * (x * z + w * y),
                                2.0f * (x * y + w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - w * x),
                                2.0f * (x * z - w * y), 2.0f * (y * z + w * x), 1.0f - 2.0f * (x * x + y * y)};
            // dM = 2 G M with M = R diag(s); d s_k = sum_i dM_ik R_ik; dR_ik = dM_ik s_k
            float dR[9], dls[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float m0 = R[k] * s[k], m1 = R[3 + k] * s[k], m2 = R[6 + k] * s[k];
                const float dm0 = 2.0f * (Gm[0] * m0 + Gm[1] * m1 + Gm[2] * m2);
                const float dm1 = 2.0f * (Gm[3] * m0 + Gm[4] * m1 + Gm[5] * m2);
                const float dm2 = 2.0f * (Gm[6] * m0 + Gm[7] * m1 + Gm[8] * m2);
                dls[k] = (dm0 * R[k] + dm1 * R[3 + k] + dm2 * R[6 + k]) * s[k];
                if constexpr (FILTERED) dls[k] = fmaf(dls[k], chain[k], extra[k]);
                dR[k] = dm0 * s[k]; dR[3 + k] = dm1 * s[k]; dR[6 + k] = dm2 * s[k];
            }
            if (d.scaling) {
                float *o3 = d.scaling + 3 * gi;
                o3[0] = dls[0]; o3[1] = dls[1]; o3[2] = dls[2];
            }
            if (d.rotation) {
                // R(q_hat) as the forward writes it, q_hat's four components independent
                const float s01 = dR[1] + dR[3], s02 = dR[2] + dR[6], s12 = dR[5] + dR[7];
                const float a10 = dR[3] - dR[1], a02 = dR[2] - dR[6], a21 = dR[7] - dR[5];
                const float dw = 2.0f * (z * a10 + y * a02 + x * a21);
                const float dx = 2.0f * (y * s01 + z * s02 + w * a21 - 2.0f * x * (dR[4] + dR[8]));
                const float dy = 2.0f * (x * s01 + z * s12 + w * a02 - 2.0f * y * (dR[0] + dR[8]));
                const float dz = 2.0f * (x * s02 + y * s12 + w * a10 - 2.0f * z * (dR[0] + dR[4]));
                // q_hat = q / |q|
                const float dot = dw * w + dx * x + dy * y + dz * z;
                reinterpret_cast<float4 *>(d.rotation)[gi] =
                    make_float4((dw - dot * w) * inv, (dx - dot * x) * inv, (dy - dot * y) * inv, (dz - dot * z) * inv);
            }
        }
        __syncthreads();                                 // s_dc is the next chunk's
    }
}

static int scene_check(const lsr_scene_dims *dims, const lsr_scene_params *p) {
    if (!dims || !p) return LSR_ENULL;
    const int K = dims->sh_coeffs;
    if (dims->n < 0 || !sh_valid_coeffs(K)) return LSR_EINVAL;
    if ((K == 1) != (p->features_rest == nullptr)) return LSR_EINVAL;
    if (!std::isfinite(dims->scale_modifier) || !(dims->scale_modifier > 0.0f)) return LSR_EINVAL;
    if (dims->reserved0 || dims->reserved1) return LSR_EINVAL;
    return LSR_OK;
}

static unsigned scene_blocks(int64_t n) {
    return (unsigned)std::min<int64_t>((n + kSceneChunk - 1) / kSceneChunk, kSceneMaxBlocks);
}

// filter3d NULL: the unfiltered instantiation
static void launch_scene_fwd(const lsr_scene_dims &d, const lsr_scene_params &p, const lsr_scene_outputs &o, const float *filter3d,
                             hipStream_t s) {
    const dim3 grid(scene_blocks(d.n)), block(kSceneChunk);
    dispatch_sh_coeffs(d.sh_coeffs, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (filter3d) hipLaunchKernelGGL((k_scene_fwd<K, true>), grid, block, 0, s, d.n, d.scale_modifier, p, o, filter3d);
        else hipLaunchKernelGGL((k_scene_fwd<K, false>), grid, block, 0, s, d.n, d.scale_modifier, p, o, (const float *)nullptr);
    });
}

static void launch_scene_bwd(const lsr_scene_dims &d, const lsr_scene_params &p, const lsr_scene_out_grads &g,
                             const lsr_scene_in_grads &o, const float *filter3d, hipStream_t s) {
    const dim3 grid(scene_blocks(d.n)), block(kSceneChunk);
    dispatch_sh_coeffs(d.sh_coeffs, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (filter3d) hipLaunchKernelGGL((k_scene_bwd<K, true>), grid, block, 0, s, d.n, d.scale_modifier, p, g, o, filter3d);
        else hipLaunchKernelGGL((k_scene_bwd<K, false>), grid, block, 0, s, d.n, d.scale_modifier, p, g, o, (const float *)nullptr);
    });
}

}  // namespace lsr

using namespace lsr;

static int scene_forward(const lsr_scene_dims *dims, const lsr_scene_params *params, const float *filter3d, bool filtered,
                         const lsr_scene_outputs *out, lsr_stream_t stream) {
    note_hip_error(0);
    if (!out) return LSR_ENULL;
    const int rc = scene_check(dims, params);
    if (rc) return rc;
    if (dims->n == 0) return LSR_OK;
    if (!params->features_dc || !params->opacity || !params->scaling || !params->rotation || (filtered && !filter3d)) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(params->rotation) | reinterpret_cast<uintptr_t>(out->rotations)) & 15) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    launch_scene_fwd(*dims, *params, *out, filtered ? filter3d : nullptr, s);
    return launch_status();
}

static int scene_backward(const lsr_scene_dims *dims, const lsr_scene_params *params, const float *filter3d, bool filtered,
                          const lsr_scene_out_grads *dout, const lsr_scene_in_grads *din, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dout || !din) return LSR_ENULL;
    const int rc = scene_check(dims, params);
    if (rc) return rc;
    if (dims->n == 0) return LSR_OK;
    if (!params->opacity || !params->scaling || !params->rotation || (filtered && !filter3d)) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(params->rotation) | reinterpret_cast<uintptr_t>(din->rotation)) & 15) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    launch_scene_bwd(*dims, *params, *dout, *din, filtered ? filter3d : nullptr, s);
    return launch_status();
}

extern "C" {

int lsr_scene_activate_forward(const lsr_scene_dims *dims, const lsr_scene_params *params, const lsr_scene_outputs *out,
                               lsr_stream_t stream) {
    return scene_forward(dims, params, nullptr, false, out, stream);
}

int lsr_scene_activate_backward(const lsr_scene_dims *dims, const lsr_scene_params *params,
                                const lsr_scene_out_grads *dout, const lsr_scene_in_grads *din, lsr_stream_t stream) {
    return scene_backward(dims, params, nullptr, false, dout, din, stream);
}

int lsr_scene_activate_filtered_forward(const lsr_scene_dims *dims, const lsr_scene_params *params, const float *filter3d,
                                        const lsr_scene_outputs *out, lsr_stream_t stream) {
    return scene_forward(dims, params, filter3d, true, out, stream);
}

int lsr_scene_activate_filtered_backward(const lsr_scene_dims *dims, const lsr_scene_params *params, const float *filter3d,
                                         const lsr_scene_out_grads *dout, const lsr_scene_in_grads *din, lsr_stream_t stream) {
    return scene_backward(dims, params, filter3d, true, dout, din, stream);
}

}  // extern "C"
