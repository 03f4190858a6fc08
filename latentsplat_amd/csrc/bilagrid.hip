// bilagrid.hip — bilateral-grid appearance compensation (include/lsr_bilagrid.h): slicing a 3-D table of 3 x 4 colour affines
// by pixel position and luminance and applying the interpolated affine, its gradients, and the table's total variation.
//
// Slice kernels.  A workgroup of 256 lanes owns one T x T tile of pixels of one view (T = 32: a lane owns one column and four
// consecutive rows; T = 16: one pixel), lanes of a wave on consecutive columns.  The grid nodes a tile can reach in x and y
// follow from its first and last pixel alone (the coordinate is a monotone function of the pixel index, bg_coord); the
// luminance can reach every level.  That footprint, nx x ny x L nodes, goes to LDS cell-major, 12 contiguous floats per node,
// from the channel-major parameter, so that a pixel reads each of its 8 nodes as three 16-byte LDS reads instead of 12
// scattered global ones.  The backward keeps a second, zeroed copy of the footprint for the grid gradient and flushes its
// non-zero entries once per workgroup with global float atomics (runs of nx floats along x): the gradient leaves the CU as
// the footprint, not as 96 floats per pixel.  Into that copy go wave sums, not pixels: neighbouring pixels share their
// nodes, and one LDS float atomic per contribution (96 per pixel) made forward + backward of 16 x 3 x 256 x 256 take 0.65 ms,
// and still 0.54 ms with up to 64 accumulators per entry so that no two lanes of an instruction named one address: the
// LDS atomic unit's own rate.  So a wave takes its pixels one distinct lower node at a time, sums the 96 products of the lanes that
// share it with the transposing exchange of wave_sum32 (lsr_wave.h), and adds each non-zero sum with one LDS atomic.
// bg_path picks T: the largest of 32 and 16 whose worst-case footprint is at most kBgMaxNodes; when neither fits (a grid much
// finer than the image), path 0 runs the same per-pixel code on 16 x 16 tiles against the parameter in global memory, one
// global float atomic per contribution.  The bound behind the LDS sizes: a coordinate is the correctly rounded
// (i + 0.5) (size - 1) / extent, off by at most 2^-24 x 64 = 4e-6, so two pixels Teff - 1 apart lie at most
// span + 8e-6 apart, span = (Teff - 1)(size - 1) / extent, their lower nodes at most floor(span + 1e-4) + 1 apart, and the
// nodes from the first pixel's lower one to the last pixel's upper one number at most floor(span + 1e-4) + 3.
// A view whose grid_idx is outside [0, N) is copied (workgroup-uniform branch ahead of every barrier).
// Luminance indexing is safe for NaN and +-Inf: fminf(fmaxf(z, 0), L - 1) sends a NaN to node 0.
//
// Total variation.  Forward: every workgroup walks a fixed share of the elements (grid-stride), adds the squared forward
// differences of the three axes in double, and leaves three sums in its own slot; one workgroup adds the slots in a fixed
// order.  Backward: a gather over each element's six neighbours.  No atomics in either.
#include <math.h>

#include "lsr_bilagrid.h"
#include "lsr_wave.h"

namespace lsr {

constexpr int kBgThreads = 256;
constexpr int kBgEntries = 12;                    // floats per node: a 3 x 4 matrix
constexpr int kBgMaxNodes = 640;                  // footprint limit: 30 KiB forward, twice that backward (below the 64 KiB a workgroup gets unasked)
constexpr int kBgDirectTile = 16;                 // tile of path 0
constexpr int kBgZeroPerThread = 8;
constexpr int kTvPerThread = 8, kTvMaxBlocks = 1024;
constexpr float kLumaR = 0.299f, kLumaG = 0.587f, kLumaB = 0.114f;

struct BgShape {
    int V, H, W, N, L, Y, X;
    int tiles_x, tiles_y;
    int nx_max, ny_max;       // LDS paths: the bound the dynamic LDS was sized by
};

struct BgArgs {
    BgShape s;
    const float *grids, *image;
    const int32_t *grid_idx;
    const float *grad_out;    // backward only
    float *out;               // forward: out; backward: grad_image
    float *grad_grids;        // backward only; nullptr: not wanted
};

// Grid coordinate of pixel index i on an axis of `extent` pixels and `size` nodes: (i + 0.5) (size - 1) / extent, one
// rounding (the product is exact below 2^24), clamped above (it is never negative).  Monotone in i.
__device__ __forceinline__ float bg_coord(int i, int extent, int size) {
    const float u = __fdiv_rn(((float)i + 0.5f) * (float)(size - 1), (float)extent);
    return fminf(u, (float)(size - 1));
}
// lower node of a clamped coordinate: the upper one is min(lower + 1, size - 1)
__device__ __forceinline__ int bg_lower(float u, int size) { return min((int)u, max(size - 2, 0)); }

// the 12 floats of one node: `off` counts nodes; LDS: cell-major; direct: channel-major, `stride` = L Y X
template <bool kLds>
__device__ __forceinline__ void bg_node(const float *__restrict__ base, int off, int stride, float (&m)[kBgEntries]) {
    if (kLds) {
        const float4 *q = reinterpret_cast<const float4 *>(base + off * kBgEntries);
        const float4 a = q[0], b = q[1], c = q[2];
        m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w; m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
        m[8] = c.x; m[9] = c.y; m[10] = c.z; m[11] = c.w;
    } else {
#pragma unroll
        for (int c = 0; c < kBgEntries; ++c) m[c] = base[off + c * stride];
    }
}

// What a workgroup knows about its tile.
struct BgTile {
    int v, y0, x0;            // view, first pixel
    int ix_lo, iy_lo, nx, ny; // footprint: first node and node count per axis
};

template <int T>
__device__ __forceinline__ BgTile bg_tile(const BgShape &s) {
    BgTile t;
    const uint32_t per_view = (uint32_t)(s.tiles_x * s.tiles_y);
    const uint32_t b = blockIdx.x, v = b / per_view, r = b - v * per_view;
    t.v = (int)v;
    t.y0 = (int)(r / (uint32_t)s.tiles_x) * T;
    t.x0 = (int)(r % (uint32_t)s.tiles_x) * T;
    const int xe = min(t.x0 + T, s.W) - 1, ye = min(t.y0 + T, s.H) - 1;
    t.ix_lo = bg_lower(bg_coord(t.x0, s.W, s.X), s.X);
    t.iy_lo = bg_lower(bg_coord(t.y0, s.H, s.Y), s.Y);
    t.nx = min(bg_lower(bg_coord(xe, s.W, s.X), s.X) + 1, s.X - 1) - t.ix_lo + 1;
    t.ny = min(bg_lower(bg_coord(ye, s.H, s.Y), s.Y) + 1, s.Y - 1) - t.iy_lo + 1;
    return t;
}

// footprint entry j (x fastest, then y, luminance, channel) -> LDS float index and offset inside the grid
__device__ __forceinline__ void bg_entry(const BgShape &s, const BgTile &t, int j, int &lds, int &glob) {
    const int lx = j % t.nx;
    int r = j / t.nx;
    const int ly = r % t.ny;
    r /= t.ny;
    const int l = r % s.L, c = r / s.L;
    lds = ((l * t.ny + ly) * t.nx + lx) * kBgEntries + c;
    glob = ((c * s.L + l) * s.Y + t.iy_lo + ly) * s.X + t.ix_lo + lx;
}

// The 8 nodes of one pixel: offsets (in nodes) of the four xy corners at the lower luminance level, the step to the upper
// level, and the weights.
struct BgPixel {
    int off[4];
    int dz;
    float wxy[4], fz;
    bool inside;              // 0 < unclamped u_z < L - 1
};

template <bool kLds>
__device__ __forceinline__ BgPixel bg_pixel(const BgShape &s, const BgTile &t, int ix0, float fx, int iy0, float fy, float p0, float p1,
                                            float p2) {
    BgPixel q;
    const float lz = (float)(s.L - 1);
    const float z = (kLumaR * p0 + kLumaG * p1 + kLumaB * p2) * lz;
    q.inside = z > 0.0f && z < lz;
    const float uz = fminf(fmaxf(z, 0.0f), lz);          // a NaN lands on node 0
    const int iz0 = bg_lower(uz, s.L);
    q.fz = uz - (float)iz0;
    const int ix1 = min(ix0 + 1, s.X - 1), iy1 = min(iy0 + 1, s.Y - 1), iz1 = min(iz0 + 1, s.L - 1);
    if (kLds) {
        const int row0 = (iz0 * t.ny + (iy0 - t.iy_lo)) * t.nx - t.ix_lo, row1 = (iz0 * t.ny + (iy1 - t.iy_lo)) * t.nx - t.ix_lo;
        q.off[0] = row0 + ix0; q.off[1] = row0 + ix1; q.off[2] = row1 + ix0; q.off[3] = row1 + ix1;
        q.dz = (iz1 - iz0) * t.ny * t.nx;
    } else {
        const int row0 = (iz0 * s.Y + iy0) * s.X, row1 = (iz0 * s.Y + iy1) * s.X;
        q.off[0] = row0 + ix0; q.off[1] = row0 + ix1; q.off[2] = row1 + ix0; q.off[3] = row1 + ix1;
        q.dz = (iz1 - iz0) * s.Y * s.X;
    }
    q.wxy[0] = (1.0f - fx) * (1.0f - fy); q.wxy[1] = fx * (1.0f - fy); q.wxy[2] = (1.0f - fx) * fy; q.wxy[3] = fx * fy;
    return q;
}

template <int T, bool kLds>
__global__ __launch_bounds__(kBgThreads) void k_bg_slice_fwd(BgArgs a) {
    extern __shared__ float4 s_dyn[];
    float *s_nodes = reinterpret_cast<float *>(s_dyn);
    constexpr int kRows = T * T / kBgThreads;
    const BgShape s = a.s;
    const BgTile t = bg_tile<T>(s);
    const int64_t plane = (int64_t)s.H * s.W, base = (int64_t)t.v * 3 * plane;
    const int col = threadIdx.x % T, row0 = threadIdx.x / T * kRows;
    const int gx = t.x0 + col;
    const int gi = a.grid_idx[t.v];
    if (gi < 0 || gi >= s.N) {                            // no grid: the view passes through
        for (int o = 0; o < kRows; ++o) {
            const int gy = t.y0 + row0 + o;
            if (gy < s.H && gx < s.W) {
                const int64_t at = base + (int64_t)gy * s.W + gx;
                a.out[at] = a.image[at]; a.out[at + plane] = a.image[at + plane]; a.out[at + 2 * plane] = a.image[at + 2 * plane];
            }
        }
        return;
    }
    const int lyx = s.L * s.Y * s.X;
    const float *grid = a.grids + (int64_t)gi * kBgEntries * lyx;
    if (kLds) {
        const int total = kBgEntries * s.L * t.ny * t.nx;
        for (int j = threadIdx.x; j < total; j += kBgThreads) {
            int lds, glob;
            bg_entry(s, t, j, lds, glob);
            s_nodes[lds] = grid[glob];
        }
        __syncthreads();
    }
    if (gx >= s.W) return;
    const float ux = bg_coord(gx, s.W, s.X);
    const int ix0 = bg_lower(ux, s.X);
    const float fx = ux - (float)ix0;
    const float *nodes = kLds ? s_nodes : grid;
    for (int o = 0; o < kRows; ++o) {
        const int gy = t.y0 + row0 + o;
        if (gy >= s.H) break;
        const float uy = bg_coord(gy, s.H, s.Y);
        const int iy0 = bg_lower(uy, s.Y);
        const int64_t at = base + (int64_t)gy * s.W + gx;
        const float p0 = a.image[at], p1 = a.image[at + plane], p2 = a.image[at + 2 * plane];
        const BgPixel q = bg_pixel<kLds>(s, t, ix0, fx, iy0, uy - (float)iy0, p0, p1, p2);
        float A[kBgEntries];
#pragma unroll
        for (int c = 0; c < kBgEntries; ++c) A[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float lo[kBgEntries], hi[kBgEntries];
            bg_node<kLds>(nodes, q.off[k], lyx, lo);
            bg_node<kLds>(nodes, q.off[k] + q.dz, lyx, hi);
            const float w0 = q.wxy[k] * (1.0f - q.fz), w1 = q.wxy[k] * q.fz;
#pragma unroll
            for (int c = 0; c < kBgEntries; ++c) A[c] = fmaf(w1, hi[c], fmaf(w0, lo[c], A[c]));
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
            a.out[at + r * plane] = fmaf(A[4 * r], p0, fmaf(A[4 * r + 1], p1, fmaf(A[4 * r + 2], p2, A[4 * r + 3])));
    }
}

template <int T, bool kLds>
__global__ __launch_bounds__(kBgThreads) void k_bg_slice_bwd(BgArgs a) {
    extern __shared__ float4 s_dyn[];
    constexpr int kRows = T * T / kBgThreads;
    const BgShape s = a.s;
    const BgTile t = bg_tile<T>(s);
    float *s_nodes = reinterpret_cast<float *>(s_dyn);
    float *s_acc = s_nodes + kBgEntries * s.L * s.ny_max * s.nx_max;
    const int64_t plane = (int64_t)s.H * s.W, base = (int64_t)t.v * 3 * plane;
    const int col = threadIdx.x % T, row0 = threadIdx.x / T * kRows;
    const int gx = t.x0 + col;
    const int gi = a.grid_idx[t.v];
    if (gi < 0 || gi >= s.N) {                            // no grid: the gradient passes through
        for (int o = 0; o < kRows; ++o) {
            const int gy = t.y0 + row0 + o;
            if (gy < s.H && gx < s.W) {
                const int64_t at = base + (int64_t)gy * s.W + gx;
                a.out[at] = a.grad_out[at]; a.out[at + plane] = a.grad_out[at + plane]; a.out[at + 2 * plane] = a.grad_out[at + 2 * plane];
            }
        }
        return;
    }
    const int lyx = s.L * s.Y * s.X;
    const float *grid = a.grids + (int64_t)gi * kBgEntries * lyx;
    const bool want_grids = a.grad_grids != nullptr;      // (uniform over the launch)
    float *ggrid = a.grad_grids + (want_grids ? (int64_t)gi * kBgEntries * lyx : 0);
    const int total = kBgEntries * s.L * t.ny * t.nx;
    if (kLds) {
        for (int j = threadIdx.x; j < total; j += kBgThreads) {
            int lds, glob;
            bg_entry(s, t, j, lds, glob);
            s_nodes[lds] = grid[glob];
            s_acc[lds] = 0.0f;
        }
        __syncthreads();
    }
    const float lz = (float)(s.L - 1);
    const float *nodes = kLds ? s_nodes : grid;
    const int lane = (int)(threadIdx.x & (LSR_WAVE - 1));
    const float ux = bg_coord(min(gx, s.W - 1), s.W, s.X);
    const int ix0 = bg_lower(ux, s.X);
    const float fx = ux - (float)ix0;
    for (int o = 0; o < kRows; ++o) {                     // (every lane of the wave walks the loop: the sums below are the wave's)
        const int gy = t.y0 + row0 + o;
        const bool active = gx < s.W && gy < s.H;
        int key = -1, off[4] = {0, 0, 0, 0}, dzo = 0;     // key: the pixel's lower node in the footprint, which names all eight
        float wc[8], outer[kBgEntries];
#pragma unroll
        for (int k = 0; k < 8; ++k) wc[k] = 0.0f;
#pragma unroll
        for (int c = 0; c < kBgEntries; ++c) outer[c] = 0.0f;
        if (active) {
            const float uy = bg_coord(gy, s.H, s.Y);
            const int iy0 = bg_lower(uy, s.Y);
            const int64_t at = base + (int64_t)gy * s.W + gx;
            const float p0 = a.image[at], p1 = a.image[at + plane], p2 = a.image[at + 2 * plane];
            const float g0 = a.grad_out[at], g1 = a.grad_out[at + plane], g2 = a.grad_out[at + 2 * plane];
            const BgPixel q = bg_pixel<kLds>(s, t, ix0, fx, iy0, uy - (float)iy0, p0, p1, p2);
            const float w0z = 1.0f - q.fz, w1z = q.fz;
            float A[kBgEntries], D[kBgEntries];           // the interpolated matrix and its derivative along luminance
#pragma unroll
            for (int c = 0; c < kBgEntries; ++c) A[c] = D[c] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float lo[kBgEntries], hi[kBgEntries];
                bg_node<kLds>(nodes, q.off[k], lyx, lo);
                bg_node<kLds>(nodes, q.off[k] + q.dz, lyx, hi);
                const float w0 = q.wxy[k] * w0z, w1 = q.wxy[k] * w1z;
#pragma unroll
                for (int c = 0; c < kBgEntries; ++c) {
                    A[c] = fmaf(w1, hi[c], fmaf(w0, lo[c], A[c]));
                    D[c] = fmaf(q.wxy[k], hi[c] - lo[c], D[c]);
                }
                off[k] = q.off[k];
                wc[k] = w0; wc[k + 4] = w1;
            }
            key = q.off[0]; dzo = q.dz;
            float d0 = fmaf(A[0], g0, fmaf(A[4], g1, A[8] * g2));
            float d1 = fmaf(A[1], g0, fmaf(A[5], g1, A[9] * g2));
            float d2 = fmaf(A[2], g0, fmaf(A[6], g1, A[10] * g2));
            if (q.inside) {
                const float e0 = fmaf(D[0], p0, fmaf(D[1], p1, fmaf(D[2], p2, D[3])));
                const float e1 = fmaf(D[4], p0, fmaf(D[5], p1, fmaf(D[6], p2, D[7])));
                const float e2 = fmaf(D[8], p0, fmaf(D[9], p1, fmaf(D[10], p2, D[11])));
                const float dz = lz * fmaf(g0, e0, fmaf(g1, e1, g2 * e2));
                d0 = fmaf(dz, kLumaR, d0); d1 = fmaf(dz, kLumaG, d1); d2 = fmaf(dz, kLumaB, d2);
            }
            a.out[at] = d0; a.out[at + plane] = d1; a.out[at + 2 * plane] = d2;
            outer[0] = g0 * p0; outer[1] = g0 * p1; outer[2] = g0 * p2; outer[3] = g0;
            outer[4] = g1 * p0; outer[5] = g1 * p1; outer[6] = g1 * p2; outer[7] = g1;
            outer[8] = g2 * p0; outer[9] = g2 * p1; outer[10] = g2 * p2; outer[11] = g2;
        }
        if (!want_grids) continue;
        if (kLds) {
            // One round per distinct lower node among the wave's pixels: its 8 x 12 sums over the lanes that share it, 32 at
            // a time (wave_sum32 leaves the sum of slot l mod 32 in lane l), then one LDS atomic per non-zero sum.
            unsigned long long pending = __ballot(active);
            while (pending) {
                const int leader = __ffsll(pending) - 1;
                const bool mine = active && key == __shfl(key, leader);
                pending &= ~__ballot(mine);
                const int o0 = __shfl(off[0], leader), o1 = __shfl(off[1], leader), o2 = __shfl(off[2], leader), o3 = __shfl(off[3], leader);
                const int dzl = __shfl(dzo, leader);
#pragma unroll
                for (int part = 0; part < 3; ++part) {
                    float v[32];
#pragma unroll
                    for (int i = 0; i < 32; ++i) v[i] = mine ? wc[(32 * part + i) / kBgEntries] * outer[(32 * part + i) % kBgEntries] : 0.0f;
                    const float sum = wave_sum32(v);
                    const int slot = 32 * part + (lane & 31), corner = slot / kBgEntries, c = slot - corner * kBgEntries;
                    const int xy = corner & 3;
                    const int node = (xy == 0 ? o0 : xy == 1 ? o1 : xy == 2 ? o2 : o3) + (corner >= 4 ? dzl : 0);
                    if (lane < 32 && sum != 0.0f) atomicAdd(s_acc + node * kBgEntries + c, sum);   // (a NaN is not 0)
                }
            }
        } else if (active) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (wc[k] == 0.0f) continue;              // the far node of a clamped coordinate, the twin of a size-1 axis
                const int node = off[k & 3] + (k < 4 ? 0 : dzo);
#pragma unroll
                for (int c = 0; c < kBgEntries; ++c) unsafeAtomicAdd(ggrid + node + c * lyx, wc[k] * outer[c]);
            }
        }
    }
    if (kLds && want_grids) {
        __syncthreads();
        for (int j = threadIdx.x; j < total; j += kBgThreads) {
            int lds, glob;
            bg_entry(s, t, j, lds, glob);
            const float v = s_acc[lds];
            if (v != 0.0f) unsafeAtomicAdd(ggrid + glob, v);   // (a NaN is not 0: it is flushed)
        }
    }
}

__global__ __launch_bounds__(kBgThreads) void k_bg_zero(float *__restrict__ p, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kBgThreads;
    for (int64_t i = (int64_t)blockIdx.x * kBgThreads + threadIdx.x; i < n; i += stride) p[i] = 0.0f;
}

// ---- total variation ----

struct TvShape {
    int L, Y, X;
    int64_t total;            // N 12 L Y X
};

__global__ __launch_bounds__(kBgThreads) void k_bg_tv_fwd(TvShape s, const float *__restrict__ g, double *__restrict__ slots) {
    __shared__ double s_red[kBgThreads / LSR_WAVE][3];
    double sum[3] = {0.0, 0.0, 0.0};                 // squared differences along x, y, l
    const int64_t stride = (int64_t)gridDim.x * kBgThreads;
    const int yx = s.Y * s.X;
    for (int64_t e = (int64_t)blockIdx.x * kBgThreads + threadIdx.x; e < s.total; e += stride) {
        const int cell = (int)(e % ((int64_t)s.L * yx));
        const int x = cell % s.X, y = cell / s.X % s.Y, l = cell / yx;
        const float v = g[e];
        if (x + 1 < s.X) { const float d = g[e + 1] - v; sum[0] += (double)d * (double)d; }
        if (y + 1 < s.Y) { const float d = g[e + s.X] - v; sum[1] += (double)d * (double)d; }
        if (l + 1 < s.L) { const float d = g[e + yx] - v; sum[2] += (double)d * (double)d; }
    }
    block_sum<kBgThreads, 3>(sum, s_red, slots + 3 * (int64_t)blockIdx.x);
}

// one workgroup: lane i adds the slots i, i + 256, ... of each axis, the lanes' sums are added in a fixed order
__global__ __launch_bounds__(kBgThreads) void k_bg_tv_finish(const double *__restrict__ slots, int blocks, double inv_x, double inv_y,
                                                             double inv_l, float *tv) {
    __shared__ double s_red[kBgThreads / LSR_WAVE][3];
    double sum[3] = {0.0, 0.0, 0.0}, t[3];
    for (int b = threadIdx.x; b < blocks; b += kBgThreads) { sum[0] += slots[3 * b]; sum[1] += slots[3 * b + 1]; sum[2] += slots[3 * b + 2]; }
    block_sum<kBgThreads, 3, 1>(sum, s_red, t);
    if (threadIdx.x == 0) *tv = (float)(t[0] * inv_x + t[1] * inv_y + t[2] * inv_l);
}

__global__ __launch_bounds__(kBgThreads) void k_bg_tv_bwd(TvShape s, const float *__restrict__ g, const float *__restrict__ grad_tv,
                                                          float kx, float ky, float kl, float *__restrict__ grad) {
    const int64_t stride = (int64_t)gridDim.x * kBgThreads;
    const int yx = s.Y * s.X;
    const float up = *grad_tv;
    for (int64_t e = (int64_t)blockIdx.x * kBgThreads + threadIdx.x; e < s.total; e += stride) {
        const int cell = (int)(e % ((int64_t)s.L * yx));
        const int x = cell % s.X, y = cell / s.X % s.Y, l = cell / yx;
        const float v = g[e];
        float dx = 0.0f, dy = 0.0f, dl = 0.0f;            // (v - previous) - (next - v), each where it exists
        if (x > 0) dx += v - g[e - 1];
        if (x + 1 < s.X) dx -= g[e + 1] - v;
        if (y > 0) dy += v - g[e - s.X];
        if (y + 1 < s.Y) dy -= g[e + s.X] - v;
        if (l > 0) dl += v - g[e - yx];
        if (l + 1 < s.L) dl -= g[e + yx] - v;
        grad[e] = up * fmaf(kx, dx, fmaf(ky, dy, kl * dl));
    }
}

// ---- host ----

// LSR_OK, or why these dims are refused (slice: the call reads the image sizes)
static int bg_check(const lsr_bilagrid_dims *d, bool slice) {
    if (d->num_grids < 1 || d->grid_l < 1 || d->grid_y < 1 || d->grid_x < 1) return LSR_EINVAL;
    if (slice && (d->num_views < 1 || d->height < 1 || d->width < 1)) return LSR_EINVAL;
    if (d->reserved0) return LSR_EINVAL;
    if (d->grid_x > LSR_BILAGRID_MAX_XY || d->grid_y > LSR_BILAGRID_MAX_XY || d->grid_l > LSR_BILAGRID_MAX_L) return LSR_EUNSUPPORTED;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)d->num_grids * kBgEntries * d->grid_l * d->grid_y * d->grid_x >= lim) return LSR_EUNSUPPORTED;
    if (slice) {
        const int64_t n = (int64_t)d->num_views * 3;
        if (n >= lim || n * d->height >= lim || n * d->height * d->width >= lim) return LSR_EUNSUPPORTED;
    }
    return LSR_OK;
}

// most nodes a tile of edge T reaches on an axis of `extent` pixels and `size` nodes (the file header has the argument)
static int bg_axis_nodes(int T, int extent, int size) {
    if (size == 1) return 1;
    const int edge = T < extent ? T : extent;
    const double span = (double)(edge - 1) * (double)(size - 1) / (double)extent;
    const int n = (int)(span + 1e-4) + 3;
    return n < size ? n : size;
}

// 32, 16 or 0 (lsr_bilagrid.h), and the footprint bound of an LDS path
static int bg_path(const lsr_bilagrid_dims &d, int &nx_max, int &ny_max) {
    for (int T = 32; T >= 16; T /= 2) {
        nx_max = bg_axis_nodes(T, d.width, d.grid_x);
        ny_max = bg_axis_nodes(T, d.height, d.grid_y);
        if (nx_max * ny_max * d.grid_l <= kBgMaxNodes) return T;
    }
    nx_max = ny_max = 0;
    return 0;
}

static BgShape bg_shape(const lsr_bilagrid_dims &d, int path, int nx_max, int ny_max) {
    const int T = path ? path : kBgDirectTile;
    return BgShape{d.num_views, d.height, d.width, d.num_grids, d.grid_l, d.grid_y, d.grid_x,
                   (d.width + T - 1) / T, (d.height + T - 1) / T, nx_max, ny_max};
}

static TvShape tv_shape(const lsr_bilagrid_dims &d) {
    return TvShape{d.grid_l, d.grid_y, d.grid_x, (int64_t)d.num_grids * kBgEntries * d.grid_l * d.grid_y * d.grid_x};
}

static int tv_blocks(int64_t total) {
    const int64_t b = (total + kBgThreads * kTvPerThread - 1) / (kBgThreads * kTvPerThread);
    return (int)(b < kTvMaxBlocks ? b : kTvMaxBlocks);
}

// 1 / (number of differences along an axis of `size` nodes); 0 for an axis of one node
static double tv_inv_count(const lsr_bilagrid_dims &d, int size) {
    if (size < 2) return 0.0;
    const double cells = (double)d.num_grids * kBgEntries * d.grid_l * d.grid_y * d.grid_x;
    return 1.0 / (cells / size * (size - 1));
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_bilagrid_slice_path(const lsr_bilagrid_dims *dims) {
    if (!dims) return LSR_ENULL;
    const int rc = bg_check(dims, true);
    if (rc) return rc;
    int nx, ny;
    return bg_path(*dims, nx, ny);
}

int lsr_bilagrid_slice_forward(const lsr_bilagrid_dims *dims, const float *grids, const float *image, const int32_t *grid_idx,
                               float *out, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !grids || !image || !grid_idx || !out) return LSR_ENULL;
    const int rc = bg_check(dims, true);
    if (rc) return rc;
    int nx, ny;
    const int path = bg_path(*dims, nx, ny);
    const BgShape s = bg_shape(*dims, path, nx, ny);
    const BgArgs a{s, grids, image, grid_idx, nullptr, out, nullptr};
    const dim3 blocks((unsigned)((int64_t)s.V * s.tiles_x * s.tiles_y));
    const size_t lds = (size_t)nx * ny * s.L * kBgEntries * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (path == 32) hipLaunchKernelGGL((k_bg_slice_fwd<32, true>), blocks, dim3(kBgThreads), lds, st, a);
    else if (path == 16) hipLaunchKernelGGL((k_bg_slice_fwd<16, true>), blocks, dim3(kBgThreads), lds, st, a);
    else hipLaunchKernelGGL((k_bg_slice_fwd<kBgDirectTile, false>), blocks, dim3(kBgThreads), 0, st, a);
    return launch_status();
}

int lsr_bilagrid_slice_backward(const lsr_bilagrid_dims *dims, const float *grids, const float *image, const int32_t *grid_idx,
                                const float *grad_out, float *grad_image, float *grad_grids, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !grids || !image || !grid_idx || !grad_out || !grad_image) return LSR_ENULL;
    const int rc = bg_check(dims, true);
    if (rc) return rc;
    int nx, ny;
    const int path = bg_path(*dims, nx, ny);
    const BgShape s = bg_shape(*dims, path, nx, ny);
    const BgArgs a{s, grids, image, grid_idx, grad_out, grad_image, grad_grids};
    const dim3 blocks((unsigned)((int64_t)s.V * s.tiles_x * s.tiles_y));
    const size_t lds = 2 * (size_t)nx * ny * s.L * kBgEntries * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = tv_shape(*dims).total;
    const int64_t zb = (cells + kBgThreads * kBgZeroPerThread - 1) / (kBgThreads * kBgZeroPerThread);
    if (grad_grids) hipLaunchKernelGGL(k_bg_zero, dim3((unsigned)zb), dim3(kBgThreads), 0, st, grad_grids, cells);
    if (path == 32) hipLaunchKernelGGL((k_bg_slice_bwd<32, true>), blocks, dim3(kBgThreads), lds, st, a);
    else if (path == 16) hipLaunchKernelGGL((k_bg_slice_bwd<16, true>), blocks, dim3(kBgThreads), lds, st, a);
    else hipLaunchKernelGGL((k_bg_slice_bwd<kBgDirectTile, false>), blocks, dim3(kBgThreads), 0, st, a);
    return launch_status();
}

size_t lsr_bilagrid_tv_workspace_bytes(const lsr_bilagrid_dims *dims) {
    if (!dims || bg_check(dims, false) != LSR_OK) return 0;
    return align_up((size_t)tv_blocks(tv_shape(*dims).total) * 3 * sizeof(double));
}

int lsr_bilagrid_tv_forward(const lsr_bilagrid_dims *dims, const float *grids, void *workspace, float *tv, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !grids || !workspace || !tv) return LSR_ENULL;
    const int rc = bg_check(dims, false);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return LSR_EINVAL;
    const TvShape s = tv_shape(*dims);
    const int blocks = tv_blocks(s.total);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bg_tv_fwd, dim3(blocks), dim3(kBgThreads), 0, st, s, grids, (double *)workspace);
    hipLaunchKernelGGL(k_bg_tv_finish, dim3(1), dim3(kBgThreads), 0, st, (const double *)workspace, blocks,
                       tv_inv_count(*dims, dims->grid_x), tv_inv_count(*dims, dims->grid_y), tv_inv_count(*dims, dims->grid_l), tv);
    return launch_status();
}

int lsr_bilagrid_tv_backward(const lsr_bilagrid_dims *dims, const float *grids, const float *grad_tv, float *grad_grids,
                             lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !grids || !grad_tv || !grad_grids) return LSR_ENULL;
    const int rc = bg_check(dims, false);
    if (rc) return rc;
    const TvShape s = tv_shape(*dims);
    hipLaunchKernelGGL(k_bg_tv_bwd, dim3(tv_blocks(s.total)), dim3(kBgThreads), 0, (hipStream_t)stream, s, grids, grad_tv,
                       (float)(2.0 * tv_inv_count(*dims, dims->grid_x)), (float)(2.0 * tv_inv_count(*dims, dims->grid_y)),
                       (float)(2.0 * tv_inv_count(*dims, dims->grid_l)), grad_grids);
    return launch_status();
}

}  // extern "C"
