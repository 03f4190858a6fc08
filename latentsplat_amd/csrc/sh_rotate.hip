// sh_rotate.hip — SH coefficient rotation of the Gaussian adapter (include/lsr_sh_rotate.h): the colour and
// latent-feature harmonics go from camera space to world space, fused with the degree masks and the broadcast over the
// depth samples; forward and backward are one launch each, the rotation matrices one tiny launch before them.
//
// Reference behaviour restated (no code taken): /root/reference/src/model/encoder/common/gaussian_adapter.py:90-93
// (sample broadcast, masks) and :107-108 with src/misc/sh_utils.py:100-120 (rotate_sh: e3nn Wigner-D matrices from Euler
// angles, one batched matmul per band, cat).  Here the matrices come straight from the 3x3 rotation (see
// k_sh_rotation_matrices), so e3nn is not involved.
//
// Decomposition of the two hot kernels.  A workgroup owns a tile of consecutive rows of ONE camera, so the rotation
// tables are uniform over it: they are staged once per workgroup in LDS (with the masks folded in).  Everything
// that touches HBM is a flat copy between global memory and LDS with consecutive lanes on consecutive floats (dwordx4
// wherever the global address allows it: the LDS image is shifted by the address's misalignment so both sides agree);
// the per-Gaussian block-diagonal mat-vec runs out of LDS, one thread per (row, channel) coefficient vector:
//   forward   rows -> LDS, mat-vec, result written S times into the LDS image of the output tile, flat copy out;
//   backward  the two gradient tiles -> LDS, sum over S, transposed mat-vec, mask, LDS image of the dense rows, copy out.
// HBM traffic per row is the minimum: 4 W bytes in and 4 S W out (forward), the reverse (backward); W = 3 Kc + C Kf.
#include "lsr_internal.h"
#include "lsr_sh_shape.h"
#include "lsr_sh_rotate.h"
#include "lsr_sh_rotate_basis.h"
#include "lsr_sh_rotate_tables.h"

namespace lsr {

constexpr int kShRotThreads = 256;
constexpr int kShRotLdsFloats = 12288;    // staging budget of a workgroup: 48 KB, three workgroups per CU
constexpr int kShRotLdsMaxFloats = 15360; // (with the tables: the 64 KB a workgroup gets without opting in to more)
constexpr int kShRotLdsSlack = 16;        // alignment shifts of the (up to three) LDS images

// ---------------------------------------------------------------------------------------------------------------------
// Rotation matrices.  Y_l(R x) = D_l(R) Y_l(x) for all x, so with n = 2l+1 fixed directions x_k and the constant
// B_l^-1 (B_l[i][k] = Y_{l,i}(x_k); tools/gen_sh_rotation_tables.py):  D_l[i][j] = sum_k Y_{l,i}(R x_k) B_l^-1[k][j].
// Y in homogeneous form (1 -> x.x): a polynomial of degree l in R, also for an R that is only nearly orthogonal.

// Two rotations per 64-thread workgroup, 32 lanes each; lane e < (degree+1)^2 is (band l, index e - l^2).  First as
// (l, direction k): the band's components at R x_k into LDS (the lanes diverge over the five bands only); then as (l, row i):
// row i of D_l.  The constant tables go through LDS too: one round of global loads per workgroup.
constexpr int kShRotMatPerBlock = 2;
__global__ __launch_bounds__(64) void k_sh_rotation_matrices(int num_rot, const float *__restrict__ rot, int64_t row_stride,
                                                             int64_t mat_stride, int degree, float *__restrict__ tables) {
    constexpr int full = LSR_SH_ROTATE_TABLE_FLOATS(LSR_SH_ROTATE_MAX_DEGREE);
    __shared__ double sBinv[full];
    __shared__ double sDirs[25 * 3];
    __shared__ double sA[kShRotMatPerBlock][full];      // [l-block][i][k] = Y_{l,i}(R x_k)
    const int local = threadIdx.x >> 5, e = threadIdx.x & 31;
    const int rr = blockIdx.x * kShRotMatPerBlock + local;
    const bool active = rr < num_rot && e < (degree + 1) * (degree + 1);
    const int r = min(rr, num_rot - 1);
    const float *m = rot + (size_t)r * mat_stride;
    double R[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) R[3 * a + b] = (double)m[a * row_stride + b];
    for (int k = threadIdx.x; k < full; k += 64) sBinv[k] = kShRotBinv[k];
    for (int k = threadIdx.x; k < 25 * 3; k += 64) sDirs[k] = kShRotDirs[k / 3][k % 3];
    __syncthreads();
    int l = 0;
    while (l < LSR_SH_ROTATE_MAX_DEGREE && (l + 1) * (l + 1) <= e) ++l;
    const int idx = e - l * l, n = 2 * l + 1, off = sh_band_offset(l);     // (e >= 25: idle lanes, kept in range)
    if (active) {
        const double *x = sDirs + 3 * (l * l + idx);
        double y[9];
        sh_band_all(l, R[0] * x[0] + R[1] * x[1] + R[2] * x[2], R[3] * x[0] + R[4] * x[1] + R[5] * x[2],
                    R[6] * x[0] + R[7] * x[1] + R[8] * x[2], y);
#pragma unroll
        for (int i = 0; i < 9; ++i)
            if (i < n) sA[local][off + i * n + idx] = y[i];
    }
    __syncthreads();
    if (!active) return;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < n; ++k) {
        const double a = sA[local][off + idx * n + k];
#pragma unroll
        for (int j = 0; j < 9; ++j)
            if (j < n) acc[j] += a * sBinv[off + k * n + j];
    }
    float *out = tables + (size_t)r * LSR_SH_ROTATE_TABLE_FLOATS(degree) + off + idx * n;
#pragma unroll
    for (int j = 0; j < 9; ++j)
        if (j < n) out[j] = (float)acc[j];
}

// ---------------------------------------------------------------------------------------------------------------------
// Hot path.

struct ShRotTiling {
    int tile_rows;        // rows of one camera per workgroup; tile_rows * channels <= kShRotThreads
    int chunk_samples;    // samples staged at a time: S, unless one row's S W floats exceed the LDS budget (then tile_rows = 1)
    int tiles_per_cam;
};

// The rotation tables of the workgroup's camera live in LDS, one copy per tensor with that tensor's mask folded in
// (T = D diag(mask): forward o = T c, backward d = T^T g), bands padded to multiples of four floats so that the
// fully unrolled reads below merge into ds_read_b128.
constexpr int kShRotTablePad = 180;
__host__ __device__ constexpr int sh_band_pad_offset(int l) { return l == 0 ? 0 : (l == 1 ? 4 : (l == 2 ? 16 : (l == 3 ? 44 : 96))); }

__device__ __forceinline__ void sh_rot_load_tables(float (*sT)[kShRotTablePad], const lsr_sh_rotate_dims &d,
                                                   const float *__restrict__ D, const float *__restrict__ cmask,
                                                   const float *__restrict__ fmask) {
    constexpr int full = LSR_SH_ROTATE_TABLE_FLOATS(LSR_SH_ROTATE_MAX_DEGREE);
    for (int e = threadIdx.x; e < 2 * full; e += kShRotThreads) {
        const int which = e >= full, f = e - which * full;
        const int K = which ? d.feat_coeffs : d.color_coeffs;
        const float *mask = which ? fmask : cmask;
        int l = 0;
        while (l < LSR_SH_ROTATE_MAX_DEGREE && sh_band_offset(l + 1) <= f) ++l;
        const int within = f - sh_band_offset(l), k = l * l + within % (2 * l + 1);   // k: the column's coefficient
        if (k < K) sT[which][sh_band_pad_offset(l) + within] = D[f] * (mask ? mask[k] : 1.0f);
    }
}

// o_l = T_l c_l (TRANSPOSED: T_l^T c_l) for the bands l <= deg, fully unrolled
template <int L, bool TRANSPOSED>
__device__ __forceinline__ void sh_rotate_band(const float *T, const float (&c)[25], float (&o)[25]) {
    constexpr int n = 2 * L + 1, off = L * L, toff = sh_band_pad_offset(L);
    float t[n * n];
#pragma unroll
    for (int e = 0; e < n * n; ++e) t[e] = T[toff + e];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < n; ++j) acc = fmaf(TRANSPOSED ? t[j * n + i] : t[i * n + j], c[off + j], acc);
        o[off + i] = acc;
    }
}
template <bool TRANSPOSED>
__device__ __forceinline__ void sh_rotate_vector(const float *T, int deg, const float (&c)[25], float (&o)[25]) {
    sh_rotate_band<0, TRANSPOSED>(T, c, o);
    if (deg >= 1) sh_rotate_band<1, TRANSPOSED>(T, c, o);
    if (deg >= 2) sh_rotate_band<2, TRANSPOSED>(T, c, o);
    if (deg >= 3) sh_rotate_band<3, TRANSPOSED>(T, c, o);
    if (deg >= 4) sh_rotate_band<4, TRANSPOSED>(T, c, o);
}

__device__ __forceinline__ int misalign4(const float *p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// Flat copies of n floats between global memory and an LDS image whose index has the same residue mod 4 as the global
// address (then the body moves as aligned dwordx4 on both sides); any other pairing falls back to dwords.
__device__ __forceinline__ void copy_out(float *__restrict__ dst, const float *lds, int lds_index, int n) {
    const int tid = threadIdx.x;
    const float *src = lds + lds_index;
    const int mis = misalign4(dst);
    if (mis == (lds_index & 3)) {
        const int head = min(n, (4 - mis) & 3);
        const int nv = (n - head) >> 2;
        if (tid < head) dst[tid] = src[tid];
        float4 *dv = reinterpret_cast<float4 *>(dst + head);
        const float4 *sv = reinterpret_cast<const float4 *>(src + head);
        for (int v = tid; v < nv; v += kShRotThreads) dv[v] = sv[v];
        const int done = head + 4 * nv;
        if (tid < n - done) dst[done + tid] = src[done + tid];
    } else {
        for (int i = tid; i < n; i += kShRotThreads) dst[i] = src[i];
    }
}
// (global loads in batches of kShRotBatch per thread, all issued before the first is stored: the loop would otherwise wait
// out one HBM latency per iteration.  The batch is straight-line code: a slot past the end re-reads the last element and
// stores it to `dump`, a float4 of LDS nobody reads.)
constexpr int kShRotBatch = 8;         // float4 loads in flight per thread (gradient tiles)
constexpr int kShRotRowBatch = 16;     // dword loads in flight per thread (raw rows: a 36-row tile of the encoder shape in one batch)
__device__ __forceinline__ void copy_in(float *lds, int lds_index, const float *__restrict__ srcg, int n, float4 *dump) {
    const int tid = threadIdx.x;
    float *dst = lds + lds_index;
    const int mis = misalign4(srcg);
    if (mis == (lds_index & 3)) {
        const int head = min(n, (4 - mis) & 3);
        const int nv = (n - head) >> 2;
        if (tid < head) dst[tid] = srcg[tid];
        const float4 *sv = reinterpret_cast<const float4 *>(srcg + head);
        float4 *dv = reinterpret_cast<float4 *>(dst + head);
        for (int v0 = tid; v0 < nv; v0 += kShRotBatch * kShRotThreads) {
            float4 x[kShRotBatch];
#pragma unroll
            for (int u = 0; u < kShRotBatch; ++u) x[u] = sv[min(v0 + u * kShRotThreads, nv - 1)];
#pragma unroll
            for (int u = 0; u < kShRotBatch; ++u) *(v0 + u * kShRotThreads < nv ? dv + v0 + u * kShRotThreads : dump) = x[u];
        }
        const int done = head + 4 * nv;
        if (tid < n - done) dst[done + tid] = srcg[done + tid];
    } else {
        for (int i = tid; i < n; i += kShRotThreads) dst[i] = srcg[i];
    }
}

// The coefficient vector a thread owns: (row of the tile, channel) of the colour tensor first, then of the feature tensor.
struct ShRotTask {
    bool active, color;
    int row, ch;      // row of the tile, channel of its tensor
    int K, deg;       // coefficients, degree
    int width, col;   // floats of the tensor per row (3 Kc or C Kf); first column of the vector inside the W-float row
};
__device__ __forceinline__ ShRotTask sh_rot_task(const lsr_sh_rotate_dims &d, int nr) {
    ShRotTask t;
    const int tid = threadIdx.x;
    const int ncol = d.color_coeffs > 0 ? 3 * nr : 0, nfeat = d.feat_coeffs > 0 ? d.feat_channels * nr : 0;
    t.color = tid < ncol;
    t.active = tid < ncol + nfeat;
    const int u = t.color ? tid : tid - ncol, nch = t.color ? 3 : max(d.feat_channels, 1);
    t.row = u / nch;
    t.ch = u - t.row * nch;
    t.K = t.color ? d.color_coeffs : d.feat_coeffs;
    t.deg = (t.K > 16) + (t.K > 9) + (t.K > 4) + (t.K > 1);
    t.width = t.color ? 3 * d.color_coeffs : d.feat_channels * d.feat_coeffs;
    t.col = (t.color ? 0 : 3 * d.color_coeffs) + t.ch * t.K;
    return t;
}

__global__ __launch_bounds__(kShRotThreads) void k_sh_rotate_fwd(lsr_sh_rotate_dims d, ShRotTiling tl,
                                                                 const float *__restrict__ tables, const float *__restrict__ rows,
                                                                 const float *__restrict__ cmask, const float *__restrict__ fmask,
                                                                 float *__restrict__ color_out, float *__restrict__ feature_out) {
    extern __shared__ float4 sh_rot_lds[];
    float *lds = reinterpret_cast<float *>(sh_rot_lds);
    const int tid = threadIdx.x;
    const int cam = blockIdx.x / tl.tiles_per_cam, tile = blockIdx.x - cam * tl.tiles_per_cam;
    const int row0 = tile * tl.tile_rows, nr = min(tl.tile_rows, d.rays - row0);
    const int S = d.samples, Sc = tl.chunk_samples;
    const int Wc = 3 * d.color_coeffs, Wf = d.feat_coeffs > 0 ? d.feat_channels * d.feat_coeffs : 0, W = Wc + Wf;
    const size_t grow = (size_t)cam * d.rays + row0;      // first global row of the tile
    __shared__ __attribute__((aligned(16))) float sT[2][kShRotTablePad];
    __shared__ float4 sDump;

    // 1. the tile's raw rows, [nr][W] at LDS index 0: consecutive lanes on consecutive floats of the (strided) rows,
    //    kShRotRowBatch loads in flight per thread
    {
        const float *src = rows + grow * (size_t)d.row_stride;
        int r = tid / W, c = tid - r * W;
        const int dr = kShRotThreads / W, dc = kShRotThreads - dr * W;
        const int n = nr * W;
        for (int i0 = tid; i0 < n; i0 += kShRotRowBatch * kShRotThreads) {
            float x[kShRotRowBatch];
            int at[kShRotRowBatch];
#pragma unroll
            for (int u = 0; u < kShRotRowBatch; ++u) {     // straight-line: a slot past the end re-reads the tile's first float
                const bool in = i0 + u * kShRotThreads < n;
                x[u] = src[(size_t)(in ? r : 0) * d.row_stride + (in ? c : 0)];
                at[u] = in ? i0 + u * kShRotThreads : -1;
                r += dr; c += dc;
                if (c >= W) { c -= W; ++r; }
            }
#pragma unroll
            for (int u = 0; u < kShRotRowBatch; ++u) *(at[u] >= 0 ? lds + at[u] : &sDump.x) = x[u];
        }
    }
    sh_rot_load_tables(sT, d, tables + (size_t)cam * d.table_stride, cmask, fmask);
    __syncthreads();

    // 2. coefficients -> registers, rotate (the masks are part of the LDS tables)
    const ShRotTask t = sh_rot_task(d, nr);
    float c[25], o[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) c[k] = (t.active && k < t.K) ? lds[t.row * W + t.col + k] : 0.0f;
    sh_rotate_vector<false>(sT[t.color ? 0 : 1], t.deg, c, o);
    __syncthreads();     // every raw row has been read: the output images may overwrite them

    // 3. LDS images of the two output tiles, [nr][Sc][3 Kc] and [nr][Sc][C Kf], each shifted to its global alignment
    float *gc = color_out + grow * (size_t)S * Wc, *gf = feature_out + grow * (size_t)S * Wf;
    const int bc = Wc > 0 ? misalign4(gc) : 0;
    const int bf = ((bc + nr * Sc * Wc + 3) & ~3) + (Wf > 0 ? misalign4(gf) : 0);
    if (t.active) {
        const int base = (t.color ? bc : bf) + t.row * Sc * t.width + t.ch * t.K;
        for (int s = 0; s < Sc; ++s) {
#pragma unroll
            for (int k = 0; k < 25; ++k)
                if (k < t.K) lds[base + s * t.width + k] = o[k];
        }
    }
    __syncthreads();

    // 4. flat copies out.  (S > Sc only with one row per tile: its samples leave in chunks of the same periodic image)
    for (int s0 = 0; s0 < S; s0 += Sc) {
        const int ns = min(Sc, S - s0);
        if (Wc > 0) copy_out(gc + (size_t)s0 * Wc, lds, bc, nr * ns * Wc);
        if (Wf > 0) copy_out(gf + (size_t)s0 * Wf, lds, bf, nr * ns * Wf);
    }
}

__global__ __launch_bounds__(kShRotThreads) void k_sh_rotate_bwd(lsr_sh_rotate_dims d, ShRotTiling tl,
                                                                 const float *__restrict__ tables, const float *__restrict__ g_color,
                                                                 const float *__restrict__ g_feature, const float *__restrict__ cmask,
                                                                 const float *__restrict__ fmask, float *__restrict__ d_rows) {
    extern __shared__ float4 sh_rot_lds[];
    float *lds = reinterpret_cast<float *>(sh_rot_lds);
    const int cam = blockIdx.x / tl.tiles_per_cam, tile = blockIdx.x - cam * tl.tiles_per_cam;
    const int row0 = tile * tl.tile_rows, nr = min(tl.tile_rows, d.rays - row0);
    const int S = d.samples, Sc = tl.chunk_samples;
    const int Wc = 3 * d.color_coeffs, Wf = d.feat_coeffs > 0 ? d.feat_channels * d.feat_coeffs : 0, W = Wc + Wf;
    const size_t grow = (size_t)cam * d.rays + row0;
    __shared__ __attribute__((aligned(16))) float sT[2][kShRotTablePad];
    __shared__ float4 sDump;
    sh_rot_load_tables(sT, d, tables + (size_t)cam * d.table_stride, cmask, fmask);     // (visible after the first barrier below)
    const ShRotTask t = sh_rot_task(d, nr);
    const bool have = t.active && (t.color ? g_color != nullptr : g_feature != nullptr);

    // 1. sum of the upstream gradients over the samples, staged [nr][ns][3 Kc] / [nr][ns][C Kf] through LDS
    float c[25], o[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) c[k] = 0.0f;
    for (int s0 = 0; s0 < S; s0 += Sc) {
        const int ns = min(Sc, S - s0);
        const float *gc = g_color ? g_color + (grow * (size_t)S + s0) * Wc : nullptr;
        const float *gf = g_feature ? g_feature + (grow * (size_t)S + s0) * Wf : nullptr;
        const int bc = gc ? misalign4(gc) : 0;
        const int bf = ((bc + nr * ns * Wc + 3) & ~3) + (gf ? misalign4(gf) : 0);
        if (s0 > 0) __syncthreads();     // the previous chunk has been summed
        if (gc && Wc > 0) copy_in(lds, bc, gc, nr * ns * Wc, &sDump);
        if (gf && Wf > 0) copy_in(lds, bf, gf, nr * ns * Wf, &sDump);
        __syncthreads();
        if (have) {
            const int base = (t.color ? bc : bf) + t.row * ns * t.width + t.ch * t.K;
            for (int s = 0; s < ns; ++s) {
#pragma unroll
                for (int k = 0; k < 25; ++k)
                    if (k < t.K) c[k] += lds[base + s * t.width + k];
            }
        }
    }

    // 2. transposed rotation (mask folded into the table)
    sh_rotate_vector<true>(sT[t.color ? 0 : 1], t.deg, c, o);
    __syncthreads();     // every staged gradient has been read

    // 3. LDS image of the dense rows [nr][W], flat copy out
    float *gd = d_rows + grow * (size_t)W;
    const int bo = misalign4(gd);
    if (t.active) {
#pragma unroll
        for (int k = 0; k < 25; ++k)
            if (k < t.K) lds[bo + t.row * W + t.col + k] = o[k];
    }
    __syncthreads();
    copy_out(gd, lds, bo, nr * W);
}

}  // namespace lsr

using namespace lsr;

static int sh_degree_or_none(int coeffs) { return sh_valid_coeffs(coeffs) ? sh_degree_of(coeffs) : -1; }

// dims validation shared by both directions; fills in the tiling.  LSR_OK with tiles_per_cam == 0: nothing to launch.
static int sh_rotate_check(const lsr_sh_rotate_dims *d, bool forward, ShRotTiling *tl) {
    if (!d) return LSR_ENULL;
    if (d->num_cameras < 1 || d->rays < 0 || d->samples < 1 || d->reserved0 != 0) return LSR_EINVAL;
    const int lc = d->color_coeffs == 0 ? -1 : sh_degree_or_none(d->color_coeffs);
    const int lf = d->feat_coeffs == 0 ? -1 : sh_degree_or_none(d->feat_coeffs);
    if ((d->color_coeffs != 0 && lc < 0) || (d->feat_coeffs != 0 && lf < 0) || (lc < 0 && lf < 0)) return LSR_EINVAL;
    if (lf >= 0 && (d->feat_channels < 1 || d->feat_channels > LSR_MAX_FEAT_CHANNELS)) return LSR_EINVAL;
    const int lmax = lc > lf ? lc : lf;
    if (d->table_stride < LSR_SH_ROTATE_TABLE_FLOATS(lmax)) return LSR_EINVAL;
    const int channels = (lc >= 0 ? 3 : 0) + (lf >= 0 ? d->feat_channels : 0);
    const int W = 3 * d->color_coeffs + (lf >= 0 ? d->feat_channels * d->feat_coeffs : 0);
    if (forward && d->row_stride < W) return LSR_EINVAL;
    // (LSR_SHROT_LDS_FLOATS: development knob, read once per process — a smaller staging budget trades tile size for
    // more resident workgroups; same results)
    int budget = env_int("LSR_SHROT_LDS_FLOATS", kShRotLdsFloats);
    budget = budget < 1024 ? 1024 : (budget > kShRotLdsMaxFloats ? kShRotLdsMaxFloats : budget);
    const int64_t SW = (int64_t)d->samples * W;
    if (SW <= budget) {
        tl->chunk_samples = d->samples;
        const int by_lds = (int)(budget / SW), by_threads = kShRotThreads / channels;
        tl->tile_rows = by_lds < by_threads ? by_lds : by_threads;
    } else {
        tl->chunk_samples = budget / W;
        tl->tile_rows = 1;
    }
    const int64_t tiles = ((int64_t)d->rays + tl->tile_rows - 1) / tl->tile_rows;
    if (tiles * d->num_cameras > 0x7FFFFFFFll) return LSR_EUNSUPPORTED;
    tl->tiles_per_cam = (int)tiles;
    return LSR_OK;
}

static size_t sh_rotate_lds_bytes(const lsr_sh_rotate_dims &d, const ShRotTiling &tl) {
    const size_t W = 3 * (size_t)d.color_coeffs + (d.feat_coeffs > 0 ? (size_t)d.feat_channels * d.feat_coeffs : 0);
    return ((size_t)tl.tile_rows * tl.chunk_samples * W + kShRotLdsSlack) * sizeof(float);
}

extern "C" {

int lsr_sh_rotation_matrices(int32_t num_rot, const float *rotations, int64_t row_stride, int64_t mat_stride,
                             int32_t degree, float *tables, lsr_stream_t stream) {
    note_hip_error(0);
    if (num_rot < 0 || degree < 0 || degree > LSR_SH_ROTATE_MAX_DEGREE) return LSR_EINVAL;
    if (row_stride < 3 || mat_stride < 2 * row_stride + 3) return LSR_EINVAL;
    if (num_rot == 0) return LSR_OK;
    if (!rotations || !tables) return LSR_ENULL;
    hipLaunchKernelGGL(k_sh_rotation_matrices, dim3((unsigned)((num_rot + kShRotMatPerBlock - 1) / kShRotMatPerBlock)), dim3(64), 0, (hipStream_t)stream,
                       (int)num_rot, rotations, row_stride, mat_stride, (int)degree, tables);
    return launch_status();
}

int lsr_sh_rotate_forward(const lsr_sh_rotate_dims *d, const float *tables, const float *rows,
                          const float *color_mask, const float *feature_mask,
                          float *color_out, float *feature_out, lsr_stream_t stream) {
    note_hip_error(0);
    ShRotTiling tl{};
    const int rc = sh_rotate_check(d, true, &tl);
    if (rc) return rc;
    if (d->rays == 0) return LSR_OK;
    if (!tables || !rows || (d->color_coeffs > 0 && !color_out) || (d->feat_coeffs > 0 && !feature_out)) return LSR_ENULL;
    hipLaunchKernelGGL(k_sh_rotate_fwd, dim3((unsigned)(tl.tiles_per_cam * d->num_cameras)), dim3(kShRotThreads),
                       sh_rotate_lds_bytes(*d, tl), (hipStream_t)stream, *d, tl, tables, rows, color_mask, feature_mask,
                       color_out, feature_out);
    return launch_status();
}

int lsr_sh_rotate_backward(const lsr_sh_rotate_dims *d, const float *tables, const float *g_color,
                           const float *g_feature, const float *color_mask, const float *feature_mask,
                           float *d_rows, lsr_stream_t stream) {
    note_hip_error(0);
    ShRotTiling tl{};
    const int rc = sh_rotate_check(d, false, &tl);
    if (rc) return rc;
    if (d->rays == 0) return LSR_OK;
    if (!tables || !d_rows) return LSR_ENULL;
    hipLaunchKernelGGL(k_sh_rotate_bwd, dim3((unsigned)(tl.tiles_per_cam * d->num_cameras)), dim3(kShRotThreads),
                       sh_rotate_lds_bytes(*d, tl), (hipStream_t)stream, *d, tl, tables,
                       d->color_coeffs > 0 ? g_color : nullptr, d->feat_coeffs > 0 ? g_feature : nullptr, color_mask,
                       feature_mask, d_rows);
    return launch_status();
}

}  // extern "C"
