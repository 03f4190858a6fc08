// views.hip — builds the per-view camera table (LSR_VIEW_FLOATS floats per view) on the device in
// one tiny launch.  Replaces ~40 launch-bound PyTorch ops per render call (measured 0.66 ms per
// call on MI355X, more than the rasterizer's own forward at 4 views) that the reference performs
// in /root/reference/src/model/decoder/cuda_splatting.py:75-82 (1/near scale invariance),
// :111-113 (get_fov, tan), :115-118 (projection, inverse extrinsics, full projection) and
// src/geometry/projection.py:233-247 (get_fov).  One thread per view, double precision inside.
#include "lsr_wave.h"

namespace lsr {

__device__ static void inv3(const double m[9], double o[9]) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C, id = 1.0 / det;
    o[0] = A * id; o[1] = -(b * i - c * h) * id; o[2] = (b * f - c * e) * id;
    o[3] = B * id; o[4] = (a * i - c * g) * id;  o[5] = -(a * f - c * d) * id;
    o[6] = C * id; o[7] = -(a * h - b * g) * id; o[8] = (a * e - b * d) * id;
}

// general 4x4 inverse by cofactors (camera-to-world matrices are affine, but keep it general)
__device__ static void inv4(const double m[16], double inv[16]) {
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12], id = 1.0 / det;
    for (int k = 0; k < 16; ++k) inv[k] *= id;
}

__global__ void k_build_views(int V, const float *__restrict__ extrinsics, const float *__restrict__ intrinsics,
                              const float *__restrict__ near, const float *__restrict__ far,
                              const float *__restrict__ bg, int bg_stride, int scale_invariant, int depth_mode,
                              float *__restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    double E[16], K[9], Ki[9], Vw[16];
    for (int k = 0; k < 16; ++k) E[k] = extrinsics[16 * v + k];
    for (int k = 0; k < 9; ++k) K[k] = intrinsics[9 * v + k];
    const float scale_f = scale_invariant ? 1.0f / near[v] : 1.0f;   // float, as the reference computes it
    const double scale = scale_f;
    E[3] *= scale; E[7] *= scale; E[11] *= scale;
    const double nr = (double)(near[v] * scale_f), fr = (double)(far[v] * scale_f);
    // field of view: angle between the rays through opposite image-edge midpoints
    inv3(K, Ki);
    const double pts[4][3] = {{0, 0.5, 1}, {1, 0.5, 1}, {0.5, 0, 1}, {0.5, 1, 1}};
    double ray[4][3];
    for (int e = 0; e < 4; ++e) {
        double r[3], n = 0;
        for (int i = 0; i < 3; ++i) { r[i] = Ki[3 * i] * pts[e][0] + Ki[3 * i + 1] * pts[e][1] + Ki[3 * i + 2] * pts[e][2]; n += r[i] * r[i]; }
        n = sqrt(n);
        for (int i = 0; i < 3; ++i) ray[e][i] = r[i] / n;
    }
    auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double tan_x = tan(0.5 * acos(fmin(1.0, fmax(-1.0, dot(ray[0], ray[1])))));
    const double tan_y = tan(0.5 * acos(fmin(1.0, fmax(-1.0, dot(ray[2], ray[3])))));
    // perspective matrix (x,y -> (-1,1), z -> (0,1), +z forward)
    double P[16] = {0};
    const double right = tan_x * nr, top = tan_y * nr;
    P[0] = 2 * nr / (2 * right); P[5] = 2 * nr / (2 * top);
    P[10] = fr / (fr - nr); P[11] = -(fr * nr) / (fr - nr); P[14] = 1;
    inv4(E, Vw);   // world -> view
    float *o = out + (size_t)v * LSR_VIEW_FLOATS;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            o[4 * c + r] = (float)Vw[4 * r + c];                    // memory = transposed matrix
            double f = 0;
            for (int k = 0; k < 4; ++k) f += P[4 * r + k] * Vw[4 * k + c];   // (P * view)[r][c]
            o[16 + 4 * c + r] = (float)f;
        }
    o[32] = (float)E[3]; o[33] = (float)E[7]; o[34] = (float)E[11];
    o[35] = (float)tan_x; o[36] = (float)tan_y;
    o[37] = bg[(size_t)v * bg_stride]; o[38] = bg[(size_t)v * bg_stride + 1]; o[39] = bg[(size_t)v * bg_stride + 2];
    // depth mode (lsr_build_views_depth) and the caller's near / far, which only the modes read
    o[40] = scale_f; o[41] = (float)depth_mode;
    o[42] = depth_mode != LSR_DEPTH_NATIVE ? near[v] : 0.0f; o[43] = depth_mode != LSR_DEPTH_NATIVE ? far[v] : 0.0f;
}

hipError_t launch_build_views(int V, const float *extrinsics, const float *intrinsics, const float *near,
                              const float *far, const float *bg, int bg_stride, int scale_invariant,
                              float *out, hipStream_t s, int depth_mode) {
    hipLaunchKernelGGL(k_build_views, dim3((V + 63) / 64), dim3(64), 0, s, V, extrinsics, intrinsics, near, far,
                       bg, bg_stride, scale_invariant, depth_mode, out);
    return hipGetLastError();
}

// One view record from the 12-field settings tuple of the reference API (the per-view call pattern of
// cuda_splatting.py:132-158): a single 64-thread launch instead of ~8 small PyTorch ops per view.
__global__ void __launch_bounds__(64)
k_pack_view(const float *__restrict__ viewmatrix, const float *__restrict__ projmatrix, const float *__restrict__ campos,
            const float *__restrict__ bg, float tanfovx, float tanfovy, const float *tanfovx_dev, const float *tanfovy_dev,
            float *__restrict__ out) {
    const int t = threadIdx.x;
    float v = 0.0f;
    if (t < 16) v = viewmatrix[t];
    else if (t < 32) v = projmatrix[t - 16];
    else if (t < 35) v = campos[t - 32];
    else if (t == 35) v = tanfovx_dev ? tanfovx_dev[0] : tanfovx;
    else if (t == 36) v = tanfovy_dev ? tanfovy_dev[0] : tanfovy;
    else if (t < 40) v = bg[t - 37];
    else if (t == 40) v = 1.0f;     // scene scale: the caller of this API has scaled the scene itself
    if (t < LSR_VIEW_FLOATS) out[t] = v;
}

hipError_t launch_pack_view(const float *viewmatrix, const float *projmatrix, const float *campos, const float *bg,
                            float tanfovx, float tanfovy, const float *tanfovx_dev, const float *tanfovy_dev, float *out,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_pack_view, dim3(1), dim3(64), 0, s, viewmatrix, projmatrix, campos, bg, tanfovx, tanfovy,
                       tanfovx_dev, tanfovy_dev, out);
    return hipGetLastError();
}

// ---- camera gradient: the fixed-order sum of the partial records (lsr_backward_views) ----
// Step 1, workgroup (s, v): chunks and pixels of slice s of view v.  Thread (q, j) adds slot j of every 8th partial record
// of the slice (coalesced 128-byte rows); the 8 row sums and the background sums (dL/dcolour * final T over the slice's
// pixels) are combined in a fixed order and stored as one second-level record.
constexpr int kCamThreads = 256;
__global__ void __launch_bounds__(kCamThreads)
k_view_grad_partial(const float *__restrict__ part, const float *__restrict__ dpart, int chunks, int sh,
                    const float *__restrict__ final_T, const float *__restrict__ g_color, int HW, float *__restrict__ l2) {
    const int s = blockIdx.x, v = blockIdx.y, tid = threadIdx.x;
    __shared__ float s_row[kCamThreads / kCamSlots][kCamSlots];
    __shared__ float s_bg[kCamThreads / LSR_WAVE][5];
    const int j = tid & (kCamSlots - 1), q = tid / kCamSlots;
    // slots a kernel of this call wrote: the geometry's always, the SH direction's when the SH backward ran
    const bool used = j <= kCamScaleGeo || (sh && j < kCamScaleSh + 1);
    const int per = (chunks + kCamSplit - 1) / kCamSplit, c0 = s * per, c1 = min(chunks, c0 + per);
    float a = 0.0f;
    if (used) {
#pragma unroll 4
        for (int c = c0 + q; c < c1; c += kCamThreads / kCamSlots) a += part[((size_t)v * chunks + c) * kCamSlots + j];
    }
    s_row[q][j] = a;
    float b[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // background (3), then near / far of the depth modes
    if (dpart) {   // (nullptr: no Gaussians, nothing wrote the pairs)
        for (int c = c0 + tid; c < c1; c += kCamThreads) {
            const float2 t = *(const float2 *)(dpart + ((size_t)v * chunks + c) * 2);
            b[3] += t.x; b[4] += t.y;
        }
    }
    if (g_color) {
        const int pper = (HW + kCamSplit - 1) / kCamSplit, p0 = s * pper, p1 = min(HW, p0 + pper);
#pragma unroll 4
        for (int px = p0 + tid; px < p1; px += kCamThreads) {
            const float T = final_T ? final_T[(size_t)v * HW + px] : 1.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c] += g_color[((size_t)v * 3 + c) * HW + px] * T;
        }
    }
    wave_all_each(Add(), b[0], b[1], b[2], b[3], b[4]);
    if ((tid & (LSR_WAVE - 1)) == 0)
        for (int c = 0; c < 5; ++c) s_bg[tid / LSR_WAVE][c] = b[c];
    __syncthreads();
    float *o = l2 + ((size_t)v * kCamSplit + s) * kCamL2;
    if (tid < kCamSlots) {
        float t = 0.0f;
        for (int r = 0; r < kCamThreads / kCamSlots; ++r) t += s_row[r][tid];
        o[tid] = t;
    } else if (tid < kCamSlots + 5) {
        float t = 0.0f;
        for (int w = 0; w < kCamThreads / LSR_WAVE; ++w) t += s_bg[w][tid - kCamSlots];
        o[tid] = t;
    }
}

// Step 2, one 64-thread workgroup per view: the kCamSplit second-level records in order -> the 44 slots of dL/d(view record)
__global__ void __launch_bounds__(LSR_WAVE)
k_view_grad_final(const float *__restrict__ l2, float *__restrict__ grad_views) {
    const int v = blockIdx.x, t = threadIdx.x;
    if (t >= LSR_VIEW_FLOATS) return;
    int a = -1, b = -1;      // second-level slots summed into record slot t (-1: none)
    if (t < 16) { if ((t & 3) != 3) a = kCamVm + 3 * (t >> 2) + (t & 3); }
    else if (t < 32) { const int k = t - 16, jj = k & 3; if (jj != 2) a = kCamPm + 3 * (k >> 2) + (jj == 3 ? 2 : jj); }
    else if (t < 35) a = kCamPos + (t - 32);
    else if (t == 35) a = kCamTanX;
    else if (t == 36) a = kCamTanY;
    else if (t < 40) a = kCamSlots + (t - 37);
    else if (t == 40) { a = kCamScaleGeo; b = kCamScaleSh; }
    else if (t >= 42) a = kCamSlots + 3 + (t - 42);     // near / far of the depth modes
    float x = 0.0f, y = 0.0f;
    for (int s = 0; s < kCamSplit; ++s) {
        const float *r = l2 + ((size_t)v * kCamSplit + s) * kCamL2;
        if (a >= 0) x += r[a];
        if (b >= 0) y += r[b];
    }
    grad_views[(size_t)v * LSR_VIEW_FLOATS + t] = x + y;
}

hipError_t launch_view_grad_reduce(const lsr_dims &d, char *ws, bool sh, const float *final_T, const float *g_color,
                                   float *grad_views, hipStream_t s) {
    const ViewGradLayout L = view_grad_layout(d);
    float *l2 = (float *)(ws + L.l2);
    prof_begin(kStViewGrad, s);
    hipLaunchKernelGGL(k_view_grad_partial, dim3(kCamSplit, d.num_views), dim3(kCamThreads), 0, s, (const float *)(ws + L.part),
                       d.num_gaussians > 0 ? (const float *)(ws + L.dpart) : nullptr, cam_chunks(d), sh ? 1 : 0, final_T, g_color,
                       d.height * d.width, l2);
    hipLaunchKernelGGL(k_view_grad_final, dim3(d.num_views), dim3(LSR_WAVE), 0, s, (const float *)l2, grad_views);
    prof_end(kStViewGrad, s);
    return hipGetLastError();
}

}  // namespace lsr
