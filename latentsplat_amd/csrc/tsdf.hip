// tsdf.hip — mesh extraction (include/lsr_mesh.h): fusion of rendered depth maps into a truncated signed distance volume,
// and marching tetrahedra on the Kuhn subdivision of its lattice.
//
// A, k_tsdf_cameras + k_tsdf_integrate, shaped like filter3d.hip and normals.hip: one workgroup compacts what depends on
// the camera alone, in double, into a 192-byte record: the affine map from the lattice index (i, j, k) to (clip.x, clip.y,
// clip.w, z) with origin, voxel size and the scene scale folded in (four rows of four floats), and the six half-space
// functions of the frustum (w, z, w + x, w - x, w + y, w - y; a point is accepted only where all six are >= 0) with, added
// to their constants, their largest increase over a brick and a margin for the float arithmetic of both sides.  A wave
// owns a brick of 64 x 4 x 1 lattice points, lanes along x, four rows per lane: 20 floats of state held in registers across
// all V views, so that the volume is read once and written once per CALL.  The records reach the wave as scalar loads (the
// loop index is wave-uniform and the pointer const __restrict__); six three-FMA evaluations at the brick's low corner
// reject a view for the whole brick before any per-lane work.  Accepted views: the terms in i and k of the four rows once per
// lane, one FMA per row and lattice row, one reciprocal to the pixel, two gathers that land on neighbouring pixels for
// neighbouring lanes (no LDS), one true division (D = depth / alpha), and the quotients by s, trunc and w' as a residual
// correction on reciprocals that are formed once (divide_by: correctly rounded by s and trunc, whose reciprocals are rounded
// from double; by w' after one Newton step on the hardware's estimate).  No atomics, no static state.
//
// B, k_mesh_classify + k_mesh_scan + k_mesh_bases / k_mesh_emit, shaped like the plan of density.hip: a thread owns one
// lattice point, which is both the owner of up to 7 edges and the low corner of one cube.  Classify reads the 8 corners,
// writes the edge mask and block-scans the two counts of its chunk of 256 points; one workgroup scans the chunk sums in int64
// and writes the counts; k_mesh_bases adds the chunk bases.  Emit reads the corners again, writes its own vertices (the
// interpolation in double: one rounding per coordinate) and the faces of its cube, whose vertex ids are the owner's base
// plus the popcount of the lower mask bits.
#include <float.h>
#include <math.h>

#include <cmath>

#include "lsr_mesh.h"
#include "lsr_wave.h"

namespace lsr {

// ---------------------------------------------------------------- A ----

constexpr int kTsdfThreads = 256;
constexpr int kTsdfRows = 4;                 // lattice rows (y) per lane
constexpr int kTsdfCamFloats = 48;
constexpr double kTsdfCullMargin = 1e-3;     // of the size of the four rows over the grid: far above float rounding

// One compacted camera as the main kernel reads it: 192 bytes, scalar loads.
struct alignas(64) TsdfCam {
    float x[4], y[4], w[4], z[4];            // clip.x, clip.y, clip.w, view z: (ci, cj, ck, constant) over the lattice index
    float cull[6][4];                        // the half-space functions: negative at a brick's low corner = reject the brick
    float s, inv_s;                          // view[40] and its reciprocal, rounded once from double
    float pad[6];
};
static_assert(sizeof(TsdfCam) == kTsdfCamFloats * sizeof(float), "a camera record is kTsdfCamFloats floats");

struct TsdfGrid {
    int nx, ny, nz;
    float origin[3], voxel_size, trunc;
};

__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_cameras(int num_views, const float *__restrict__ views, TsdfGrid g,
                                                               float *__restrict__ cams) {
    for (int v = threadIdx.x; v < num_views; v += kTsdfThreads) {
        const float *view = views + (size_t)v * LSR_VIEW_FLOATS;
        float *rec = cams + (size_t)v * kTsdfCamFloats;
        const double s = view[40], step = s * (double)g.voxel_size;
        // rows of the two matrices (transposed as stored: M(r, c) = m[4 c + r]): clip.x, clip.y, clip.w, view z
        const int at[4] = {16 + 0, 16 + 1, 16 + 3, 2};
        double row[4][4], size = 0.0;
        for (int r = 0; r < 4; ++r) {
            const float *m = view + at[r];
            double c = m[12];
            for (int k = 0; k < 3; ++k) {
                row[r][k] = (double)m[4 * k] * step;
                c += (double)m[4 * k] * s * (double)g.origin[k];
            }
            row[r][3] = c;
            for (int k = 0; k < 4; ++k) rec[4 * r + k] = (float)row[r][k];
            size += fabs(row[r][0]) * g.nx + fabs(row[r][1]) * g.ny + fabs(row[r][2]) * g.nz + fabs(c);
        }
        // w, z, w + x, w - x, w + y, w - y: over a brick an affine function is largest at the low corner's value plus its
        // positive increments
        const double sign[6][4] = {{0, 0, 1, 0}, {0, 0, 0, 1}, {1, 0, 1, 0}, {-1, 0, 1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}};
        const double extent[3] = {LSR_WAVE - 1, kTsdfRows - 1, 0};
        for (int f = 0; f < 6; ++f) {
            double c[4];
            for (int k = 0; k < 4; ++k) {
                c[k] = 0.0;
                for (int r = 0; r < 4; ++r) c[k] += sign[f][r] * row[r][k];
            }
            for (int k = 0; k < 3; ++k) c[3] += fmax(0.0, c[k] * extent[k]);
            c[3] += kTsdfCullMargin * size;
            for (int k = 0; k < 4; ++k) rec[16 + 4 * f + k] = (float)c[k];
        }
        rec[40] = view[40];
        rec[41] = (float)(1.0 / s);
        for (int k = 42; k < kTsdfCamFloats; ++k) rec[k] = 0.0f;
    }
}

struct TsdfArgs {
    TsdfGrid g;
    int bricks_x, bricks_y;
    int V, H, W;
    float alpha_min, depth_max, max_weight;
    float inv_trunc;                         // 1 / trunc, rounded once from double
    float *tsdf, *weight, *color;            // color NULL: no colour
    const float *depth, *alpha, *image_color;
    const TsdfCam *cams;
};

__device__ __forceinline__ float affine(const float (&c)[4], float i, float j, float k) {
    return fmaf(c[0], i, fmaf(c[1], j, fmaf(c[2], k, c[3])));
}

// x / y with r the correctly rounded 1 / y: the quotient estimate and one residual correction, which is the correctly
// rounded quotient (Markstein) wherever nothing leaves the normal range: three operations in place of the division's ten
__device__ __forceinline__ float divide_by(float x, float y, float r) {
    const float q = x * r;
    return fmaf(fmaf(-q, y, x), r, q);
}

__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_integrate(TsdfArgs a) {
    // the brick of this wave: wave-uniform
    const uint32_t brick = blockIdx.x * (kTsdfThreads / LSR_WAVE) + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / LSR_WAVE);
    const uint32_t per_slab = (uint32_t)(a.bricks_x * a.bricks_y);
    const int k = (int)(brick / per_slab);
    if (k >= a.g.nz) return;
    const uint32_t in_slab = brick - (uint32_t)k * per_slab;
    const int j0 = (int)(in_slab / (uint32_t)a.bricks_x) * kTsdfRows, i0 = (int)(in_slab % (uint32_t)a.bricks_x) * LSR_WAVE;
    const int i = i0 + (int)(threadIdx.x & (LSR_WAVE - 1));
    const bool in_x = i < a.g.nx;
    const size_t plane = (size_t)a.g.nx * a.g.ny * a.g.nz;
    const int64_t pixels = (int64_t)a.H * a.W;
    const bool has_color = a.color != nullptr;

    float t[kTsdfRows], w[kTsdfRows], c0[kTsdfRows], c1[kTsdfRows], c2[kTsdfRows];
    size_t at[kTsdfRows];
    bool in[kTsdfRows];
    uint32_t touched = 0;
#pragma unroll
    for (int r = 0; r < kTsdfRows; ++r) {
        in[r] = in_x && j0 + r < a.g.ny;
        at[r] = ((size_t)k * a.g.ny + (size_t)(j0 + r)) * a.g.nx + (size_t)i;
        t[r] = w[r] = c0[r] = c1[r] = c2[r] = 0.0f;
        if (in[r]) {
            t[r] = a.tsdf[at[r]];
            w[r] = a.weight[at[r]];
            if (has_color) { c0[r] = a.color[at[r]]; c1[r] = a.color[plane + at[r]]; c2[r] = a.color[2 * plane + at[r]]; }
        }
    }

    const float fi0 = (float)i0, fj0 = (float)j0, fk = (float)k, fi = (float)i;
    const float fW = (float)a.W, fH = (float)a.H;
    for (int v = 0; v < a.V; ++v) {
        const TsdfCam cam = a.cams[v];                   // wave-uniform: scalar loads
        bool reject = false;
#pragma unroll
        for (int f = 0; f < 6; ++f) reject |= affine(cam.cull[f], fi0, fj0, fk) < 0.0f;      // (a NaN record rejects nothing)
        if (reject) continue;
        const float *depth = a.depth + (size_t)v * (size_t)pixels, *alpha = a.alpha + (size_t)v * (size_t)pixels;
        const float *image = has_color ? a.image_color + 3 * (size_t)v * (size_t)pixels : nullptr;
        // what the rows of this lane share: the terms in i and k
        const float bx = fmaf(cam.x[0], fi, fmaf(cam.x[2], fk, cam.x[3])), by = fmaf(cam.y[0], fi, fmaf(cam.y[2], fk, cam.y[3]));
        const float bw = fmaf(cam.w[0], fi, fmaf(cam.w[2], fk, cam.w[3])), bz = fmaf(cam.z[0], fi, fmaf(cam.z[2], fk, cam.z[3]));
#pragma unroll
        for (int r = 0; r < kTsdfRows; ++r) {
            const float fj = (float)(j0 + r);
            const float z = fmaf(cam.z[1], fj, bz), cw = fmaf(cam.w[1], fj, bw);
            if (!in[r] || !(z > 0.0f) || !(cw > 0.0f)) continue;
            const float inv = __builtin_amdgcn_rcpf(cw);
            const float px = floorf(fmaf(fmaf(fmaf(cam.x[1], fj, bx), inv, 1.0f), fW, -1.0f) * 0.5f + 0.5f);
            const float py = floorf(fmaf(fmaf(fmaf(cam.y[1], fj, by), inv, 1.0f), fH, -1.0f) * 0.5f + 0.5f);
            if (!(px >= 0.0f && px < fW && py >= 0.0f && py < fH)) continue;          // (NaN: outside)
            const int pixel = (int)py * a.W + (int)px;
            const float al = alpha[pixel];
            if (!(al > a.alpha_min)) continue;
            const float D = depth[pixel] / al;
            if (!(D > 0.0f && D <= FLT_MAX)) continue;
            if (a.depth_max > 0.0f && divide_by(D, cam.s, cam.inv_s) > a.depth_max) continue;
            const float sdf = divide_by(D - z, cam.s, cam.inv_s);
            if (sdf < -a.g.trunc) continue;
            const float d = fminf(1.0f, divide_by(sdf, a.g.trunc, a.inv_trunc));
            // the four quotients by w' share its reciprocal: the hardware's estimate, one Newton step, then divide_by
            const float w1 = w[r] + 1.0f, r0 = __builtin_amdgcn_rcpf(w1);
            const float rw = fmaf(fmaf(-w1, r0, 1.0f), r0, r0);
            t[r] = divide_by(fmaf(t[r], w[r], d), w1, rw);
            if (has_color) {
                c0[r] = divide_by(fmaf(c0[r], w[r], image[pixel]), w1, rw);
                c1[r] = divide_by(fmaf(c1[r], w[r], image[pixels + pixel]), w1, rw);
                c2[r] = divide_by(fmaf(c2[r], w[r], image[2 * pixels + pixel]), w1, rw);
            }
            w[r] = a.max_weight > 0.0f ? fminf(w1, a.max_weight) : w1;
            touched |= 1u << r;
        }
    }
#pragma unroll
    for (int r = 0; r < kTsdfRows; ++r)
        if (touched >> r & 1u) {                         // (only rows inside the grid are ever touched)
            a.tsdf[at[r]] = t[r];
            a.weight[at[r]] = w[r];
            if (has_color) { a.color[at[r]] = c0[r]; a.color[plane + at[r]] = c1[r]; a.color[2 * plane + at[r]] = c2[r]; }
        }
}

// LSR_OK, or why these dims are refused
static int tsdf_check(const lsr_tsdf_dims *d) {
    if (d->nx < LSR_TSDF_MIN_EXTENT || d->ny < LSR_TSDF_MIN_EXTENT || d->nz < LSR_TSDF_MIN_EXTENT) return LSR_EINVAL;
    if (!std::isfinite(d->voxel_size) || !(d->voxel_size > 0.0f) || !std::isfinite(d->trunc) || !(d->trunc > 0.0f)) return LSR_EINVAL;
    if (!std::isfinite(d->origin[0]) || !std::isfinite(d->origin[1]) || !std::isfinite(d->origin[2])) return LSR_EINVAL;
    if ((d->has_color != 0 && d->has_color != 1) || d->reserved0 || d->reserved1 || d->reserved2) return LSR_EINVAL;
    if (d->nx > LSR_TSDF_MAX_EXTENT || d->ny > LSR_TSDF_MAX_EXTENT || d->nz > LSR_TSDF_MAX_EXTENT) return LSR_EUNSUPPORTED;
    if ((int64_t)d->nx * d->ny * d->nz > LSR_TSDF_MAX_VOXELS) return LSR_EUNSUPPORTED;
    return LSR_OK;
}

static TsdfGrid tsdf_grid(const lsr_tsdf_dims &d) {
    return TsdfGrid{d.nx, d.ny, d.nz, {d.origin[0], d.origin[1], d.origin[2]}, d.voxel_size, d.trunc};
}

// ---------------------------------------------------------------- B ----

constexpr int kMeshChunk = 256;              // lattice points per workgroup
constexpr int kMeshScanThreads = 256;        // the one workgroup that scans the chunk sums
constexpr int64_t kMeshMaxCount = (int64_t)1 << 31;

// The six tetrahedra of a cube, corners as 3-bit cube-corner numbers (dx + 2 dy + 4 dz), v0 in bits 0..2 up to v3 in bits
// 9..11, in the order of the header; kTetOdd: bit t set = permutation t is odd (the tetrahedron is negatively oriented).
__device__ constexpr uint32_t kTets[6] = {0 | 1 << 3 | 3 << 6 | 7 << 9, 0 | 1 << 3 | 5 << 6 | 7 << 9, 0 | 2 << 3 | 3 << 6 | 7 << 9,
                                          0 | 2 << 3 | 6 << 6 | 7 << 9, 0 | 4 << 3 | 5 << 6 | 7 << 9, 0 | 4 << 3 | 6 << 6 | 7 << 9};
constexpr uint32_t kTetOdd = 0b100110;

struct MeshWorkspace {
    uint32_t *vbase, *fbase;       // [N]
    uint8_t *mask;                 // [N]
    int64_t *vsum, *fsum;          // [chunks]
    size_t total;
};

static MeshWorkspace mesh_workspace(const lsr_tsdf_dims &d, void *base) {
    const size_t n = (size_t)d.nx * d.ny * d.nz, chunks = (n + kMeshChunk - 1) / kMeshChunk;
    char *p = (char *)base;
    MeshWorkspace ws;
    size_t o = 0;
    ws.vbase = (uint32_t *)(p + o); o = align_up(o + n * 4);
    ws.fbase = (uint32_t *)(p + o); o = align_up(o + n * 4);
    ws.mask = (uint8_t *)(p + o); o = align_up(o + n);
    ws.vsum = (int64_t *)(p + o); o = align_up(o + chunks * 8);
    ws.fsum = (int64_t *)(p + o); o = align_up(o + chunks * 8);
    ws.total = o;
    return ws;
}

// What a thread knows of its lattice point and the cube above it: per cube corner, bit = valid / inside; which corners
// lie inside the grid.
struct MeshCorners {
    uint32_t exists, valid, inside;
    int i, j, k;
};

__device__ __forceinline__ MeshCorners mesh_corners(const TsdfGrid &g, int64_t n, const float *__restrict__ tsdf,
                                                    const float *__restrict__ weight, float min_weight, float (&f)[8]) {
    MeshCorners c;
    const int64_t row = n / g.nx;
    c.i = (int)(n - row * g.nx); c.j = (int)(row % g.ny); c.k = (int)(row / g.ny);
    c.exists = c.valid = c.inside = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const bool there = c.i + (q & 1) < g.nx && c.j + (q >> 1 & 1) < g.ny && c.k + (q >> 2) < g.nz;
        f[q] = 0.0f;
        if (there) {
            const int64_t m = n + (q & 1) + (int64_t)(q >> 1 & 1) * g.nx + (int64_t)(q >> 2) * g.nx * g.ny;
            f[q] = tsdf[m];
            c.exists |= 1u << q;
            if (weight[m] >= min_weight) c.valid |= 1u << q;
            if (f[q] < 0.0f) c.inside |= 1u << q;
        }
    }
    return c;
}

// bit e = edge e of the point carries a vertex
__device__ __forceinline__ uint32_t mesh_edge_mask(const MeshCorners &c) {
    if (!(c.valid & 1u)) return 0;
    const uint32_t differs = (c.inside & 1u) ? ~c.inside : c.inside;
    return (c.exists & c.valid & differs) >> 1 & 0x7fu;
}

// inside bits of tetrahedron t's corners v0..v3 (bits 0..3), or false when a corner is not valid
__device__ __forceinline__ bool mesh_tet(const MeshCorners &c, int t, uint32_t &in4) {
    in4 = 0;
    bool ok = true;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t q = kTets[t] >> (3 * m) & 7u;
        ok = ok && (c.valid >> q & 1u);
        in4 |= (c.inside >> q & 1u) << m;
    }
    return ok;
}

__device__ __forceinline__ uint32_t mesh_cube_faces(const MeshCorners &c) {
    if (c.exists != 0xffu) return 0;
    uint32_t faces = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        uint32_t in4;
        if (mesh_tet(c, t, in4)) {
            const int inside = __popc(in4);
            faces += inside == 2 ? 2u : (inside == 1 || inside == 3) ? 1u : 0u;
        }
    }
    return faces;
}

__global__ __launch_bounds__(kMeshChunk) void k_mesh_classify(TsdfGrid g, int64_t total, const float *__restrict__ tsdf,
                                                              const float *__restrict__ weight, float min_weight, MeshWorkspace ws) {
    __shared__ uint32_t s_wave[kMeshChunk / LSR_WAVE];
    const int64_t n = (int64_t)blockIdx.x * kMeshChunk + threadIdx.x;
    uint32_t mask = 0, faces = 0;
    if (n < total) {
        float f[8];
        const MeshCorners c = mesh_corners(g, n, tsdf, weight, min_weight, f);
        mask = mesh_edge_mask(c);
        faces = mesh_cube_faces(c);
    }
    // both counts of a chunk in one scan: vertices (<= 7 x 256) in bits 0..15, faces (<= 12 x 256) above
    uint32_t sum;
    const uint32_t base = block_exclusive_scan<kMeshChunk>((uint32_t)__popc(mask) | faces << 16, s_wave, sum);
    if (n < total) {
        ws.mask[n] = (uint8_t)mask;
        ws.vbase[n] = base & 0xffffu;
        ws.fbase[n] = base >> 16;
    }
    if (threadIdx.x == 0) { ws.vsum[blockIdx.x] = sum & 0xffffu; ws.fsum[blockIdx.x] = sum >> 16; }
}

__global__ __launch_bounds__(kMeshScanThreads) void k_mesh_scan(int64_t chunks, MeshWorkspace ws, int64_t *__restrict__ counts) {
    __shared__ int64_t s_wave[kMeshScanThreads / LSR_WAVE];
    int64_t vertices, faces;
    scan_chunk_sums<kMeshScanThreads>(ws.vsum, chunks, s_wave, vertices);
    scan_chunk_sums<kMeshScanThreads>(ws.fsum, chunks, s_wave, faces);
    if (threadIdx.x == 0) { counts[0] = vertices; counts[1] = faces; }
}

// (beyond 2^32 the bases wrap; the counts say so and k_mesh_emit writes nothing)
__global__ __launch_bounds__(kMeshChunk) void k_mesh_bases(int64_t total, MeshWorkspace ws) {
    const int64_t n = (int64_t)blockIdx.x * kMeshChunk + threadIdx.x;
    if (n >= total) return;
    ws.vbase[n] += (uint32_t)ws.vsum[blockIdx.x];
    ws.fbase[n] += (uint32_t)ws.fsum[blockIdx.x];
}

struct MeshEmitArgs {
    TsdfGrid g;
    int64_t total;
    const float *tsdf, *weight, *color;
    float min_weight;
    MeshWorkspace ws;
    const int64_t *counts;
    int64_t capacity_vertices, capacity_faces;
    float *vertices, *vertex_colors;
    int32_t *faces;
};

__global__ __launch_bounds__(kMeshChunk) void k_mesh_emit(MeshEmitArgs a) {
    const int64_t n = (int64_t)blockIdx.x * kMeshChunk + threadIdx.x;
    if (n >= a.total || a.counts[0] >= kMeshMaxCount || a.counts[1] >= kMeshMaxCount) return;
    const TsdfGrid g = a.g;
    float f[8];
    const MeshCorners c = mesh_corners(g, n, a.tsdf, a.weight, a.min_weight, f);
    const int64_t stride[3] = {1, g.nx, (int64_t)g.nx * g.ny};

    // the vertices this point owns
    const uint32_t mask = a.ws.mask[n];
    int64_t id = a.ws.vbase[n];
    for (uint32_t left = mask; left; left &= left - 1, ++id) {
        if (id >= a.capacity_vertices) break;
        const int q = __ffs(left);                       // edge e = q - 1 ends at cube corner q
        const double t = (double)f[0] / ((double)f[0] - (double)f[q]);
        const int at[3] = {c.i, c.j, c.k};
#pragma unroll
        for (int x = 0; x < 3; ++x)
            a.vertices[3 * id + x] = (float)((double)g.origin[x] + (double)g.voxel_size * ((double)at[x] + ((q >> x & 1) ? t : 0.0)));
        if (a.vertex_colors) {
            const int64_t m = n + (q & 1) * stride[0] + (q >> 1 & 1) * stride[1] + (q >> 2) * stride[2];
#pragma unroll
            for (int p = 0; p < 3; ++p)
                a.vertex_colors[3 * id + p] = (float)((1.0 - t) * (double)a.color[p * a.total + n] + t * (double)a.color[p * a.total + m]);
        }
    }

    // the faces of the cube above this point
    if (c.exists != 0xffu) return;
    int64_t face = a.ws.fbase[n];
    // the vertex on the edge between cube corners p and q: owned by the lower one (p is a subset of q along a chain)
    auto vertex = [&](uint32_t p, uint32_t q) -> int32_t {
        if (p > q) { const uint32_t x = p; p = q; q = x; }
        const int64_t owner = n + (p & 1) * stride[0] + (p >> 1 & 1) * stride[1] + (p >> 2) * stride[2];
        const uint32_t e = (q ^ p) - 1u;
        return (int32_t)(a.ws.vbase[owner] + (uint32_t)__popc(a.ws.mask[owner] & ((1u << e) - 1u)));
    };
    auto emit = [&](int32_t v0, int32_t v1, int32_t v2) {      // rotated so that the lowest number comes first
        if (face < a.capacity_faces) {
            int32_t *dst = a.faces + 3 * face;
            if (v1 < v0 && v1 < v2) { dst[0] = v1; dst[1] = v2; dst[2] = v0; }
            else if (v2 < v0 && v2 < v1) { dst[0] = v2; dst[1] = v0; dst[2] = v1; }
            else { dst[0] = v0; dst[1] = v1; dst[2] = v2; }
        }
        ++face;
    };
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        uint32_t in4;
        if (!mesh_tet(c, t, in4)) continue;
        const int inside = __popc(in4);
        if (inside == 0 || inside == 4) continue;
        auto corner = [&](int m) -> uint32_t { return kTets[t] >> (3 * m) & 7u; };
        bool flip = (kTetOdd >> t & 1u) != 0;
        if (inside != 2) {
            // one corner A alone on its side, at chain position m; B, C, D the others in chain order.  (AB, AC, AD) faces
            // away from A when det[B - A, C - A, D - A] > 0: the tetrahedron's orientation times (-1)^m.
            const uint32_t lone = inside == 1 ? in4 : ~in4 & 15u;
            const int m = __ffs(lone) - 1;
            flip ^= (m & 1) != 0;
            flip ^= inside == 3;                         // A is the outside corner: the triangle faces toward it
            const uint32_t A = corner(m), B = corner(m == 0 ? 1 : 0), C = corner(m <= 1 ? 2 : 1), D = corner(m <= 2 ? 3 : 2);
            const int32_t v0 = vertex(A, B), v1 = vertex(A, C), v2 = vertex(A, D);
            if (flip) emit(v0, v2, v1); else emit(v0, v1, v2);
        } else {
            // inside A, B at chain positions p < q, outside C, D at r < s: the cycle AC, AD, BD, BC faces C and D when the
            // tetrahedron (A, B, C, D) is positively oriented: its own orientation times the parity of (p, q, r, s),
            // which is odd for the inside pairs {0, 2} and {1, 3}
            const int p = __ffs(in4) - 1, q = 31 - __clz(in4);
            const uint32_t out = ~in4 & 15u;
            const int r = __ffs(out) - 1, s = 31 - __clz(out);
            flip ^= in4 == 0b0101u || in4 == 0b1010u;
            const uint32_t A = corner(p), B = corner(q), C = corner(r), D = corner(s);
            int32_t cyc[4] = {vertex(A, C), vertex(A, D), vertex(B, D), vertex(B, C)};
            if (flip) { const int32_t x = cyc[1]; cyc[1] = cyc[3]; cyc[3] = x; }
            // split along the diagonal from the lowest number
            int32_t q0 = cyc[0], q1 = cyc[1], q2 = cyc[2], q3 = cyc[3];
#pragma unroll
            for (int turn = 0; turn < 3; ++turn)
                if (q1 < q0 || q2 < q0 || q3 < q0) { const int32_t x = q0; q0 = q1; q1 = q2; q2 = q3; q3 = x; }
            emit(q0, q1, q2);
            emit(q0, q2, q3);
        }
    }
}

}  // namespace lsr

using namespace lsr;

extern "C" {

size_t lsr_tsdf_workspace_bytes(int32_t num_views) {
    if (num_views < 1 || num_views > LSR_TSDF_MAX_VIEWS) return 0;
    return align_up((size_t)num_views * sizeof(TsdfCam));
}

int lsr_tsdf_integrate(const lsr_tsdf_dims *dims, float *tsdf, float *weight, float *color, int32_t num_views, int32_t height,
                       int32_t width, const float *depth, const float *alpha, const float *image_color, const float *views,
                       float alpha_min, float depth_max, float max_weight, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !tsdf || !weight || !depth || !alpha || !views || !workspace) return LSR_ENULL;
    const int rc = tsdf_check(dims);
    if (rc) return rc;
    if (dims->has_color && (!color || !image_color)) return LSR_ENULL;
    if (!dims->has_color && image_color) return LSR_EINVAL;
    if (num_views < 1 || num_views > LSR_TSDF_MAX_VIEWS || height < 1 || width < 1) return LSR_EINVAL;
    if (!std::isfinite(alpha_min) || !std::isfinite(depth_max) || depth_max < 0.0f || !std::isfinite(max_weight) || max_weight < 0.0f)
        return LSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return LSR_EINVAL;
    if ((int64_t)num_views * height * width >= ((int64_t)1 << 31)) return LSR_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    TsdfArgs a;
    a.g = tsdf_grid(*dims);
    a.bricks_x = (dims->nx + LSR_WAVE - 1) / LSR_WAVE;
    a.bricks_y = (dims->ny + kTsdfRows - 1) / kTsdfRows;
    a.V = num_views; a.H = height; a.W = width;
    a.alpha_min = alpha_min; a.depth_max = depth_max; a.max_weight = max_weight;
    a.inv_trunc = (float)(1.0 / (double)dims->trunc);
    a.tsdf = tsdf; a.weight = weight; a.color = dims->has_color ? color : nullptr;
    a.depth = depth; a.alpha = alpha; a.image_color = image_color;
    a.cams = (const TsdfCam *)workspace;
    // bricks: at most 32 x 512 x 2048 / (what 2^30 points allow) < 2^25
    const int64_t bricks = (int64_t)a.bricks_x * a.bricks_y * dims->nz;
    const unsigned blocks = (unsigned)((bricks + kTsdfThreads / LSR_WAVE - 1) / (kTsdfThreads / LSR_WAVE));
    hipLaunchKernelGGL(k_tsdf_cameras, dim3(1), dim3(kTsdfThreads), 0, s, (int)num_views, views, a.g, (float *)workspace);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(blocks), dim3(kTsdfThreads), 0, s, a);
    return launch_status();
}

size_t lsr_mesh_workspace_bytes(const lsr_tsdf_dims *dims) {
    if (!dims || tsdf_check(dims) != LSR_OK) return 0;
    return mesh_workspace(*dims, nullptr).total;
}

int lsr_mesh_count(const lsr_tsdf_dims *dims, const float *tsdf, const float *weight, float min_weight, void *workspace,
                   int64_t *counts, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !tsdf || !weight || !workspace || !counts) return LSR_ENULL;
    const int rc = tsdf_check(dims);
    if (rc) return rc;
    if (min_weight != min_weight) return LSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(counts) & 7)) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const TsdfGrid g = tsdf_grid(*dims);
    const MeshWorkspace ws = mesh_workspace(*dims, workspace);
    const int64_t total = (int64_t)dims->nx * dims->ny * dims->nz, chunks = (total + kMeshChunk - 1) / kMeshChunk;     // <= 2^22
    hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)chunks), dim3(kMeshChunk), 0, s, g, total, tsdf, weight, min_weight, ws);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMeshScanThreads), 0, s, chunks, ws, counts);
    hipLaunchKernelGGL(k_mesh_bases, dim3((unsigned)chunks), dim3(kMeshChunk), 0, s, total, ws);
    return launch_status();
}

int lsr_mesh_emit(const lsr_tsdf_dims *dims, const float *tsdf, const float *weight, const float *color, float min_weight,
                  void *workspace, const int64_t *counts, int64_t capacity_vertices, int64_t capacity_faces, float *vertices,
                  float *vertex_colors, int32_t *faces, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !tsdf || !weight || !workspace || !counts) return LSR_ENULL;
    const int rc = tsdf_check(dims);
    if (rc) return rc;
    if (capacity_vertices < 0 || capacity_faces < 0 || min_weight != min_weight) return LSR_EINVAL;
    if ((capacity_vertices > 0 && !vertices) || (capacity_faces > 0 && !faces) || (vertex_colors && !color)) return LSR_ENULL;
    if (vertex_colors && !dims->has_color) return LSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(counts) & 7)) return LSR_EINVAL;
    if (capacity_vertices >= kMeshMaxCount || capacity_faces >= kMeshMaxCount) return LSR_EUNSUPPORTED;
    if (capacity_vertices == 0 && capacity_faces == 0) return LSR_OK;
    MeshEmitArgs a;
    a.g = tsdf_grid(*dims);
    a.total = (int64_t)dims->nx * dims->ny * dims->nz;
    a.tsdf = tsdf; a.weight = weight; a.color = color; a.min_weight = min_weight;
    a.ws = mesh_workspace(*dims, workspace);
    a.counts = counts;
    a.capacity_vertices = capacity_vertices; a.capacity_faces = capacity_faces;
    a.vertices = vertices; a.vertex_colors = vertex_colors; a.faces = faces;
    const int64_t chunks = (a.total + kMeshChunk - 1) / kMeshChunk;
    hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)chunks), dim3(kMeshChunk), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
