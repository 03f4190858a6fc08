// normals.hip — the depth-normal consistency regulariser (include/lsr_normals.h): per-(view, Gaussian) normals on one side
// of the unchanged rasterizer, the image-space loss against the normals of the rendered depth map on the other.
//
// A, k_normals_cameras + k_normals_fwd / k_normals_bwd, shaped like filter3d.hip: one workgroup compacts what depends on
// the camera alone, in double, into a 64-byte record (the rows of the upper 3 x 3 of the view matrix with its uniform
// scale divided out, the camera position, the scene scale); a lane owns one Gaussian, forms its shortest axis once (the
// quaternion normalised and the column of R evaluated in double: a handful of operations per Gaussian against 12 bytes
// stored per pair) and loops over the records, which arrive as scalar loads (the loop index is wave-uniform and the
// pointer const __restrict__).  Per pair: three FMAs for the sign, nine for the rotation, three selects and one 12-byte
// store; the pass is bound by that store.  The backward walks the same loop, adds sign W^T g per view in order into three
// doubles and runs the quaternion chain once: written, no atomics.
//
// B, k_nc_fwd + k_image_mean_finish / k_nc_bwd, shaped like photometric.hip: a workgroup of 256 lanes owns one 32 x 32 tile of one
// image.  Thread 0 derives the view's ray (six affine coefficients and the sign) in double while the others stage
// D = depth / alpha (NaN where alpha <= alpha_min or outside the image, so that "usable" is "finite") with its halo in
// LDS, as doubles: the per-pixel arithmetic (two differences of D r, their cross product, its norm) is a few dozen double
// operations against 36 bytes moved, and in double the outputs carry one rounding each, whatever the cross product cancels.
// The forward sums e per tile in a fixed order (wave butterfly, then the four waves in order) into the tile's own
// workspace slot and the finish of lsr_image_sum.h adds the slots of an image; the backward computes, per stencil centre of the tile and a
// 1-pixel ring around it, the four scalars its neighbours will want (dL/dP of that neighbour dotted with the neighbour's
// ray), and every pixel then gathers four of them.  No atomics, no static state.
#include <float.h>
#include <math.h>

#include <cmath>

#include "lsr_image_sum.h"
#include "lsr_normals.h"

namespace lsr {

// ---------------------------------------------------------------- A ----

constexpr int kNrmThreads = 256;
constexpr int kNrmCamFloats = 16;

// One compacted camera as the passes read it: 64 bytes, one scalar load.
struct alignas(64) NormalCam {
    float wx[4], wy[4], wz[4];     // rows of W3 / c ([3] unused)
    float cx, cy, cz, s;           // camera position (scaled space), scene scale
};
static_assert(sizeof(NormalCam) == kNrmCamFloats * sizeof(float), "a camera record is kNrmCamFloats floats");

__global__ __launch_bounds__(kNrmThreads) void k_normals_cameras(int num_views, const float *__restrict__ views,
                                                                 float *__restrict__ cams) {
    for (int v = threadIdx.x; v < num_views; v += kNrmThreads) {
        const float *view = views + (size_t)v * LSR_VIEW_FLOATS;
        float *rec = cams + (size_t)v * kNrmCamFloats;
        double sq = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) sq += (double)view[4 * c + r] * (double)view[4 * c + r];
        const double inv = 1.0 / sqrt(sq / 3.0);       // a zero block: infinite, the rows NaN or infinite, the pairs write 0
#pragma unroll
        for (int r = 0; r < 3; ++r) {                  // row r of W: slots r, 4 + r, 8 + r
            rec[4 * r + 0] = (float)((double)view[r] * inv);
            rec[4 * r + 1] = (float)((double)view[4 + r] * inv);
            rec[4 * r + 2] = (float)((double)view[8 + r] * inv);
            rec[4 * r + 3] = 0.0f;
        }
        rec[12] = view[32]; rec[13] = view[33]; rec[14] = view[34]; rec[15] = view[40];
    }
}

// What a lane keeps of its Gaussian: the position, the unit quaternion (double), the index of the shortest axis and that axis.
struct NormalRow {
    float x, y, z;
    double qw, qx, qy, qz, inv_len;
    int k;
    float a[3];
};

__device__ __forceinline__ NormalRow normal_row(int64_t g, const float *__restrict__ xyz, const float *__restrict__ scaling,
                                                const float *__restrict__ rotation) {
    NormalRow r;
    r.x = xyz[3 * g]; r.y = xyz[3 * g + 1]; r.z = xyz[3 * g + 2];
    const float s0 = scaling[3 * g], s1 = scaling[3 * g + 1], s2 = scaling[3 * g + 2];
    int k = s1 < s0 ? 1 : 0;                             // ties go to the lowest index
    k = s2 < (k ? s1 : s0) ? 2 : k;
    r.k = k;
    const float4 q = reinterpret_cast<const float4 *>(rotation)[g];
    const double w = q.x, x = q.y, y = q.z, z = q.w;
    r.inv_len = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    r.qw = w * r.inv_len; r.qx = x * r.inv_len; r.qy = y * r.inv_len; r.qz = z * r.inv_len;
    const double W = r.qw, X = r.qx, Y = r.qy, Z = r.qz;
    double a0, a1, a2;
    if (k == 0) { a0 = 1.0 - 2.0 * (Y * Y + Z * Z); a1 = 2.0 * (X * Y + W * Z); a2 = 2.0 * (X * Z - W * Y); }
    else if (k == 1) { a0 = 2.0 * (X * Y - W * Z); a1 = 1.0 - 2.0 * (X * X + Z * Z); a2 = 2.0 * (Y * Z + W * X); }
    else { a0 = 2.0 * (X * Z + W * Y); a1 = 2.0 * (Y * Z - W * X); a2 = 1.0 - 2.0 * (X * X + Y * Y); }
    r.a[0] = (float)a0; r.a[1] = (float)a1; r.a[2] = (float)a2;
    return r;
}

// One (view, Gaussian) pair: the sign and the camera-space normal before the sign; false when the row is not finite.
__device__ __forceinline__ bool normal_pair(const NormalCam &c, const NormalRow &r, float &sign, float (&o)[3]) {
    const float d = fmaf(r.a[0], fmaf(-c.s, r.x, c.cx), fmaf(r.a[1], fmaf(-c.s, r.y, c.cy), r.a[2] * fmaf(-c.s, r.z, c.cz)));
    sign = d < 0.0f ? -1.0f : 1.0f;
    o[0] = fmaf(c.wx[0], r.a[0], fmaf(c.wx[1], r.a[1], c.wx[2] * r.a[2]));
    o[1] = fmaf(c.wy[0], r.a[0], fmaf(c.wy[1], r.a[1], c.wy[2] * r.a[2]));
    o[2] = fmaf(c.wz[0], r.a[0], fmaf(c.wz[1], r.a[1], c.wz[2] * r.a[2]));
    return isfinite(d) && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]);
}

__global__ __launch_bounds__(kNrmThreads) void k_normals_fwd(int n, const float *__restrict__ xyz, const float *__restrict__ scaling,
                                                             const float *__restrict__ rotation, int num_views,
                                                             const NormalCam *__restrict__ cams, float *__restrict__ normals) {
    const int64_t g = (int64_t)blockIdx.x * kNrmThreads + threadIdx.x;
    const bool in = g < n;
    const NormalRow row = normal_row(in ? g : 0, xyz, scaling, rotation);      // a lane past the end reads row 0, stores nothing
    for (int v = 0; v < num_views; ++v) {
        const NormalCam c = cams[v];                     // wave-uniform: one 64-byte scalar load
        float sign, o[3];
        const bool ok = normal_pair(c, row, sign, o);
        if (in) {
            float *dst = normals + ((size_t)v * (size_t)n + (size_t)g) * 3;
            dst[0] = ok ? sign * o[0] : 0.0f;
            dst[1] = ok ? sign * o[1] : 0.0f;
            dst[2] = ok ? sign * o[2] : 0.0f;
        }
    }
}

__global__ __launch_bounds__(kNrmThreads) void k_normals_bwd(int n, const float *__restrict__ xyz, const float *__restrict__ scaling,
                                                             const float *__restrict__ rotation, int num_views,
                                                             const NormalCam *__restrict__ cams,
                                                             const float *__restrict__ grad_normals,
                                                             float *__restrict__ grad_rotation) {
    const int64_t g = (int64_t)blockIdx.x * kNrmThreads + threadIdx.x;
    const bool in = g < n;
    const NormalRow row = normal_row(in ? g : 0, xyz, scaling, rotation);
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;               // dL/da in world space, the views added in order
    for (int v = 0; v < num_views; ++v) {
        const NormalCam c = cams[v];
        float sign, o[3];
        const bool ok = normal_pair(c, row, sign, o);
        const float *src = grad_normals + ((size_t)v * (size_t)n + (size_t)(in ? g : 0)) * 3;
        const double u = ok ? (double)sign : 0.0;
        const double n0 = (double)src[0] * u, n1 = (double)src[1] * u, n2 = (double)src[2] * u;
        g0 += (double)c.wx[0] * n0 + (double)c.wy[0] * n1 + (double)c.wz[0] * n2;      // W^T g
        g1 += (double)c.wx[1] * n0 + (double)c.wy[1] * n1 + (double)c.wz[1] * n2;
        g2 += (double)c.wx[2] * n0 + (double)c.wy[2] * n1 + (double)c.wz[2] * n2;
    }
    if (!in) return;
    const double W = row.qw, X = row.qx, Y = row.qy, Z = row.qz;
    double dw, dx, dy, dz;                              // dL/d(unit quaternion) through column k of R
    if (row.k == 0) {
        dw = 2.0 * (Z * g1 - Y * g2); dx = 2.0 * (Y * g1 + Z * g2);
        dy = -4.0 * Y * g0 + 2.0 * X * g1 - 2.0 * W * g2; dz = -4.0 * Z * g0 + 2.0 * W * g1 + 2.0 * X * g2;
    } else if (row.k == 1) {
        dw = 2.0 * (X * g2 - Z * g0); dx = 2.0 * Y * g0 - 4.0 * X * g1 + 2.0 * W * g2;
        dy = 2.0 * (X * g0 + Z * g2); dz = -2.0 * W * g0 - 4.0 * Z * g1 + 2.0 * Y * g2;
    } else {
        dw = 2.0 * (Y * g0 - X * g1); dx = 2.0 * Z * g0 - 2.0 * W * g1 - 4.0 * X * g2;
        dy = 2.0 * W * g0 + 2.0 * Z * g1 - 4.0 * Y * g2; dz = 2.0 * (X * g0 + Y * g1);
    }
    const double along = W * dw + X * dx + Y * dy + Z * dz;          // through q / |q|: (d - q^ <q^, d>) / |q|
    float4 out = make_float4((float)((dw - W * along) * row.inv_len), (float)((dx - X * along) * row.inv_len),
                             (float)((dy - Y * along) * row.inv_len), (float)((dz - Z * along) * row.inv_len));
    if (!(isfinite(out.x) && isfinite(out.y) && isfinite(out.z) && isfinite(out.w))) out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    reinterpret_cast<float4 *>(grad_rotation)[g] = out;
}

static int normals_check(int64_t n, int32_t num_views) {
    if (n < 0 || n >= LSR_NORMALS_MAX_ROWS || num_views < 1 || num_views > LSR_NORMALS_MAX_VIEWS) return LSR_EINVAL;
    return LSR_OK;
}

// ---------------------------------------------------------------- B ----

constexpr int kNcTile = 32;                          // output pixels per tile, each way
constexpr int kNcThreads = 256;
constexpr int kNcRows = kNcTile * kNcTile / kNcThreads;      // 4 output rows per lane
constexpr int kNcFwdSpan = kNcTile + 2;              // the forward's D: a 1-pixel halo
constexpr int kNcBwdSpan = kNcTile + 4;              // the backward's D: a 2-pixel halo

struct NcShape {
    int H, W, tiles_x, tiles_y;
};

// The ray of one view, affine in the pixel: r = (x0 + xx px + xy py, y0 + yx px + yy py, 1); sign = sigma.
struct NcRay {
    double x0, xx, xy, y0, yx, yy, sign;
};

// (include/lsr_normals.h)  One thread, in double.
__device__ static void nc_derive_ray(const float *__restrict__ view, int H, int W, NcRay &ray) {
    // A = upper 3 x 3 of the view matrix, A(r, c) = view[4 c + r]; its inverse by cofactors
    const double a = view[0], b = view[4], c = view[8], d = view[1], e = view[5], f = view[9], g = view[2], h = view[6], i = view[10];
    const double C0 = e * i - f * h, C1 = -(d * i - f * g), C2 = d * h - e * g;
    const double id = 1.0 / (a * C0 + b * C1 + c * C2);
    const double inv[3][3] = {{C0 * id, -(b * i - c * h) * id, (b * f - c * e) * id},
                              {C1 * id, (a * i - c * g) * id, -(a * f - c * d) * id},
                              {C2 * id, -(a * h - b * g) * id, (a * e - b * d) * id}};
    double Q[3][3];                                    // rows 0, 1, 3 of projmatrix (M(r, c) = view[16 + 4 c + r]) times A^-1
    const int rows[3] = {0, 1, 3};
    for (int q = 0; q < 3; ++q)
        for (int j = 0; j < 3; ++j) {
            double t = 0.0;
            for (int k = 0; k < 3; ++k) t += (double)view[16 + 4 * k + rows[q]] * inv[k][j];
            Q[q][j] = t;
        }
    double rx[3], ry[3];                               // the rays through pixels (0, 0), (1, 0), (0, 1)
    for (int t = 0; t < 3; ++t) {
        const double px = t == 1 ? 1.0 : 0.0, py = t == 2 ? 1.0 : 0.0;
        const double nx = (2.0 * px + 1.0) / W - 1.0, ny = (2.0 * py + 1.0) / H - 1.0;
        const double m00 = Q[0][0] - nx * Q[2][0], m01 = Q[0][1] - nx * Q[2][1], b0 = nx * Q[2][2] - Q[0][2];
        const double m10 = Q[1][0] - ny * Q[2][0], m11 = Q[1][1] - ny * Q[2][1], b1 = ny * Q[2][2] - Q[1][2];
        const double det = m00 * m11 - m01 * m10;
        rx[t] = (b0 * m11 - m01 * b1) / det;
        ry[t] = (m00 * b1 - b0 * m10) / det;
    }
    ray.x0 = rx[0]; ray.xx = rx[1] - rx[0]; ray.xy = rx[2] - rx[0];
    ray.y0 = ry[0]; ray.yx = ry[1] - ry[0]; ray.yy = ry[2] - ry[0];
    ray.sign = ray.xx * ray.yy - ray.xy * ray.yx > 0.0 ? -1.0 : 1.0;
}

// dst[SPAN][SPAN] = depth / alpha around the tile with a HALO-pixel ring; NaN outside the image and where alpha <= alpha_min
template <int SPAN, int HALO>
__device__ __forceinline__ void nc_stage(double *__restrict__ dst, const float *__restrict__ depth, const float *__restrict__ alpha,
                                         const NcShape &s, int y0, int x0, float alpha_min) {
    for (int i = threadIdx.x; i < SPAN * SPAN; i += kNcThreads) {
        const int r = i / SPAN, c = i - r * SPAN;
        const int gy = y0 + r - HALO, gx = x0 + c - HALO;
        double D = __builtin_nan("");
        if (gy >= 0 && gy < s.H && gx >= 0 && gx < s.W) {
            const int64_t at = (int64_t)gy * s.W + gx;
            const float al = alpha[at];
            if (al > alpha_min) D = (double)depth[at] / (double)al;
        }
        dst[i] = D;
    }
}

// The stencil centred on pixel (px, py), whose D is *c in an LDS tile with rows `stride` apart.
struct NcStencil {
    double a[3], b[3], m[3], norm;
    bool valid;
};

__device__ __forceinline__ NcStencil nc_stencil(const double *c, int stride, int px, int py, const NcRay &ray) {
    NcStencil s;
    const double dc = c[0], dl = c[-1], dr = c[1], du = c[-stride], dd = c[stride];
    const double rx = ray.x0 + ray.xx * px + ray.xy * py, ry = ray.y0 + ray.yx * px + ray.yy * py;
    s.a[0] = dr * (rx + ray.xx) - dl * (rx - ray.xx); s.a[1] = dr * (ry + ray.yx) - dl * (ry - ray.yx); s.a[2] = dr - dl;
    s.b[0] = dd * (rx + ray.xy) - du * (rx - ray.xy); s.b[1] = dd * (ry + ray.yy) - du * (ry - ray.yy); s.b[2] = dd - du;
    s.m[0] = s.a[1] * s.b[2] - s.a[2] * s.b[1];
    s.m[1] = s.a[2] * s.b[0] - s.a[0] * s.b[2];
    s.m[2] = s.a[0] * s.b[1] - s.a[1] * s.b[0];
    s.norm = sqrt(s.m[0] * s.m[0] + s.m[1] * s.m[1] + s.m[2] * s.m[2]);
    // (the five D are finite exactly when their sum is: they are quotients of floats, far from double's range)
    s.valid = isfinite(dc + dl + dr + du + dd) && s.norm >= (double)FLT_MIN && s.norm <= (double)FLT_MAX;
    return s;
}

struct NcFwdArgs {
    NcShape s;
    float alpha_min;
    const float *normal_map, *depth, *alpha, *views;
    double *slots;             // [V][tiles_y][tiles_x]: sum of e
    float *depth_normals;      // optional
    uint8_t *valid;            // optional
};

__global__ __launch_bounds__(kNcThreads) void k_nc_fwd(NcFwdArgs a) {
    __shared__ double s_D[kNcFwdSpan * kNcFwdSpan];
    __shared__ double s_red[kNcThreads / LSR_WAVE][1];
    __shared__ NcRay s_ray;
    const NcShape s = a.s;
    int image, y0, x0;
    image_tile(s.tiles_x, s.tiles_y, kNcTile, image, y0, x0);
    const int64_t pixels = (int64_t)s.H * s.W, base = (int64_t)image * pixels;
    if (threadIdx.x == 0) nc_derive_ray(a.views + (size_t)image * LSR_VIEW_FLOATS, s.H, s.W, s_ray);
    nc_stage<kNcFwdSpan, 1>(s_D, a.depth + base, a.alpha + base, s, y0, x0, a.alpha_min);
    __syncthreads();
    const NcRay ray = s_ray;

    const int col = threadIdx.x % kNcTile, row0 = threadIdx.x / kNcTile * kNcRows;
    const int gx = x0 + col;
    double sum[1] = {0.0};
#pragma unroll
    for (int o = 0; o < kNcRows; ++o) {
        const int gy = y0 + row0 + o;
        if (gy < s.H && gx < s.W) {
            const int64_t at = (int64_t)gy * s.W + gx;
            const NcStencil st = nc_stencil(s_D + (row0 + o + 1) * kNcFwdSpan + col + 1, kNcFwdSpan, gx, gy, ray);
            double n0 = 0.0, n1 = 0.0, n2 = 0.0;
            if (st.valid) {
                const double k = ray.sign / st.norm;
                n0 = st.m[0] * k; n1 = st.m[1] * k; n2 = st.m[2] * k;
                if (a.normal_map) {                   // (NULL: the caller wants n~ and the mask alone)
                    const float *N = a.normal_map + 3 * base + at;
                    sum[0] += (double)a.alpha[base + at] - ((double)N[0] * n0 + (double)N[pixels] * n1 + (double)N[2 * pixels] * n2);
                }
            }
            if (a.depth_normals) {
                float *dn = a.depth_normals + 3 * base + at;
                dn[0] = (float)n0; dn[pixels] = (float)n1; dn[2 * pixels] = (float)n2;
            }
            if (a.valid) a.valid[base + at] = st.valid ? 1 : 0;
        }
    }
    block_sum<kNcThreads, 1>(sum, s_red, a.slots + blockIdx.x);
}

struct NcUnit {};          // this unit's k_image_mean_finish

struct NcBwdArgs {
    NcShape s;
    float alpha_min;
    double inv_count;          // 1 / (V H W)
    const float *normal_map, *depth, *alpha, *views, *grad_loss;
    float *grad_normal_map, *grad_depth, *grad_alpha;      // each optional
};

__global__ __launch_bounds__(kNcThreads) void k_nc_bwd(NcBwdArgs a) {
    constexpr int kCentres = kNcTile + 2;              // the tile's pixels and a 1-pixel ring: every stencil a tile pixel belongs to
    __shared__ double s_D[kNcBwdSpan * kNcBwdSpan];
    __shared__ float s_c[4][kCentres * kCentres];      // per centre: dL/dD of its right, left, lower and upper neighbour
    __shared__ NcRay s_ray;
    const NcShape s = a.s;
    int image, y0, x0;
    image_tile(s.tiles_x, s.tiles_y, kNcTile, image, y0, x0);
    const int64_t pixels = (int64_t)s.H * s.W, base = (int64_t)image * pixels;
    if (threadIdx.x == 0) nc_derive_ray(a.views + (size_t)image * LSR_VIEW_FLOATS, s.H, s.W, s_ray);
    nc_stage<kNcBwdSpan, 2>(s_D, a.depth + base, a.alpha + base, s, y0, x0, a.alpha_min);
    __syncthreads();
    const NcRay ray = s_ray;
    const double up = (double)*a.grad_loss * a.inv_count;

    for (int i = threadIdx.x; i < kCentres * kCentres; i += kNcThreads) {
        const int r = i / kCentres, c = i - r * kCentres;
        const int gy = y0 + r - 1, gx = x0 + c - 1;
        // (a centre outside the image has a NaN D of its own: never valid)
        const NcStencil st = nc_stencil(s_D + (r + 1) * kNcBwdSpan + c + 1, kNcBwdSpan, gx, gy, ray);
        double n0 = 0.0, n1 = 0.0, n2 = 0.0;
        float c_right = 0.0f, c_left = 0.0f, c_down = 0.0f, c_up = 0.0f;
        if (st.valid) {
            const int64_t at = (int64_t)gy * s.W + gx;
            const double inv = 1.0 / st.norm;
            const double u0 = st.m[0] * inv, u1 = st.m[1] * inv, u2 = st.m[2] * inv;      // m / |m|
            n0 = ray.sign * u0; n1 = ray.sign * u1; n2 = ray.sign * u2;
            const float *N = a.normal_map + 3 * base + at;
            const double N0 = N[0], N1 = N[pixels], N2 = N[2 * pixels];
            const double along = N0 * u0 + N1 * u1 + N2 * u2;
            const double k = -up * ray.sign * inv;                                        // dL/dm = k (N - u <N, u>)
            const double G0 = k * (N0 - u0 * along), G1 = k * (N1 - u1 * along), G2 = k * (N2 - u2 * along);
            // m = a x b:  dL/da = b x G,  dL/db = G x a
            const double A0 = st.b[1] * G2 - st.b[2] * G1, A1 = st.b[2] * G0 - st.b[0] * G2, A2 = st.b[0] * G1 - st.b[1] * G0;
            const double B0 = G1 * st.a[2] - G2 * st.a[1], B1 = G2 * st.a[0] - G0 * st.a[2], B2 = G0 * st.a[1] - G1 * st.a[0];
            const double rx = ray.x0 + ray.xx * gx + ray.xy * gy, ry = ray.y0 + ray.yx * gx + ray.yy * gy;
            // P = D r, a = P(x+1) - P(x-1), b = P(y+1) - P(y-1): dL/dD of a neighbour is +-<dL/da or dL/db, its ray>
            c_right = (float)(A0 * (rx + ray.xx) + A1 * (ry + ray.yx) + A2);
            c_left = (float)-(A0 * (rx - ray.xx) + A1 * (ry - ray.yx) + A2);
            c_down = (float)(B0 * (rx + ray.xy) + B1 * (ry + ray.yy) + B2);
            c_up = (float)-(B0 * (rx - ray.xy) + B1 * (ry - ray.yy) + B2);
        }
        s_c[0][i] = c_right; s_c[1][i] = c_left; s_c[2][i] = c_down; s_c[3][i] = c_up;
        if (a.grad_normal_map && r >= 1 && r <= kNcTile && c >= 1 && c <= kNcTile && gy < s.H && gx < s.W) {
            float *gn = a.grad_normal_map + 3 * base + (int64_t)gy * s.W + gx;
            gn[0] = (float)(-up * n0); gn[pixels] = (float)(-up * n1); gn[2 * pixels] = (float)(-up * n2);
        }
    }
    __syncthreads();
    if (!a.grad_depth && !a.grad_alpha) return;

    const int col = threadIdx.x % kNcTile, row0 = threadIdx.x / kNcTile * kNcRows;
    const int gx = x0 + col;
#pragma unroll
    for (int o = 0; o < kNcRows; ++o) {
        const int gy = y0 + row0 + o;
        if (gy < s.H && gx < s.W) {
            const int64_t at = base + (int64_t)gy * s.W + gx;
            const int rc = row0 + o + 1, cc = col + 1;                  // this pixel among the centres
            // the right neighbour of the centre to the left, the left neighbour of the centre to the right, the lower of
            // the one above, the upper of the one below: added in this order
            const double dD = (((double)s_c[0][rc * kCentres + cc - 1] + (double)s_c[1][rc * kCentres + cc + 1]) +
                               (double)s_c[2][(rc - 1) * kCentres + cc]) + (double)s_c[3][(rc + 1) * kCentres + cc];
            const double D = s_D[(rc + 1) * kNcBwdSpan + cc + 1];
            float g_depth = 0.0f, g_alpha = 0.0f;
            if (isfinite(D)) {                                          // alpha > alpha_min > 0 here; elsewhere no stencil uses the pixel
                const double al = a.alpha[at];
                g_depth = (float)(dD / al);
                g_alpha = (float)(-dD * D / al);
            }
            if (a.grad_depth) a.grad_depth[at] = g_depth;
            if (a.grad_alpha) a.grad_alpha[at] = g_alpha;
        }
    }
}

// LSR_OK, or why these dims are refused
static int nc_check(const lsr_normal_dims *d) {
    if (d->num_images < 1 || d->height < 1 || d->width < 1) return LSR_EINVAL;
    if (!std::isfinite(d->alpha_min) || !(d->alpha_min > 0.0f)) return LSR_EINVAL;
    if (d->reserved0 || d->reserved1) return LSR_EINVAL;
    const int64_t n = 3 * (int64_t)d->num_images;
    if (n * d->height >= ((int64_t)1 << 31) || n * d->height * d->width >= ((int64_t)1 << 31)) return LSR_EUNSUPPORTED;
    return LSR_OK;
}

static NcShape nc_shape(const lsr_normal_dims &d) {
    return NcShape{d.height, d.width, (d.width + kNcTile - 1) / kNcTile, (d.height + kNcTile - 1) / kNcTile};
}

// tiles of all images: below 2^31 whenever V H W is (a tile holds at least one pixel)
static int64_t nc_tiles(const lsr_normal_dims &d) {
    const NcShape s = nc_shape(d);
    return (int64_t)d.num_images * s.tiles_x * s.tiles_y;
}

}  // namespace lsr

using namespace lsr;

extern "C" {

size_t lsr_scene_normals_workspace_bytes(int64_t n, int32_t num_views) {
    if (n <= 0 || normals_check(n, num_views) != LSR_OK) return 0;
    return (size_t)num_views * kNrmCamFloats * sizeof(float);
}

int lsr_scene_normals_forward(int64_t n, const float *xyz, const float *scaling, const float *rotation, int32_t num_views,
                              const float *views, float *normals, void *workspace, lsr_stream_t stream) {
    note_hip_error(0);
    const int rc = normals_check(n, num_views);
    if (rc) return rc;
    if (n == 0) return LSR_OK;
    if (!xyz || !scaling || !rotation || !views || !normals || !workspace) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(rotation) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n + kNrmThreads - 1) / kNrmThreads);      // <= 2^20
    hipLaunchKernelGGL(k_normals_cameras, dim3(1), dim3(kNrmThreads), 0, s, (int)num_views, views, (float *)workspace);
    hipLaunchKernelGGL(k_normals_fwd, dim3(blocks), dim3(kNrmThreads), 0, s, (int)n, xyz, scaling, rotation, (int)num_views,
                       (const NormalCam *)workspace, normals);
    return launch_status();
}

int lsr_scene_normals_backward(int64_t n, const float *xyz, const float *scaling, const float *rotation, int32_t num_views,
                               const float *views, const float *grad_normals, float *grad_rotation, void *workspace,
                               lsr_stream_t stream) {
    note_hip_error(0);
    const int rc = normals_check(n, num_views);
    if (rc) return rc;
    if (n == 0) return LSR_OK;
    if (!xyz || !scaling || !rotation || !views || !grad_normals || !grad_rotation || !workspace) return LSR_ENULL;
    if ((reinterpret_cast<uintptr_t>(rotation) & 15) || (reinterpret_cast<uintptr_t>(grad_rotation) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15))
        return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n + kNrmThreads - 1) / kNrmThreads);
    hipLaunchKernelGGL(k_normals_cameras, dim3(1), dim3(kNrmThreads), 0, s, (int)num_views, views, (float *)workspace);
    hipLaunchKernelGGL(k_normals_bwd, dim3(blocks), dim3(kNrmThreads), 0, s, (int)n, xyz, scaling, rotation, (int)num_views,
                       (const NormalCam *)workspace, grad_normals, grad_rotation);
    return launch_status();
}

size_t lsr_normal_consistency_workspace_bytes(const lsr_normal_dims *dims) {
    if (!dims || nc_check(dims) != LSR_OK) return 0;
    return align_up((size_t)nc_tiles(*dims) * sizeof(double));
}

int lsr_normal_consistency_forward(const lsr_normal_dims *dims, const float *normal_map, const float *depth, const float *alpha,
                                   const float *views, void *workspace, float *loss, float *per_view, float *depth_normals,
                                   uint8_t *valid, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !depth || !alpha || !views || !workspace) return LSR_ENULL;
    if (!normal_map && (loss || per_view)) return LSR_ENULL;
    const int rc = nc_check(dims);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const NcShape shape = nc_shape(*dims);
    NcFwdArgs a{shape, dims->alpha_min, normal_map, depth, alpha, views, (double *)workspace, depth_normals, valid};
    hipLaunchKernelGGL(k_nc_fwd, dim3((unsigned)nc_tiles(*dims)), dim3(kNcThreads), 0, s, a);
    if (loss || per_view)
        hipLaunchKernelGGL(k_image_mean_finish<NcUnit>, dim3(1), dim3(kFinishThreads), 0, s, (const double *)workspace, dims->num_images,
                           shape.tiles_x * shape.tiles_y, 1.0 / ((double)dims->height * (double)dims->width), loss, per_view);
    return launch_status();
}

int lsr_normal_consistency_backward(const lsr_normal_dims *dims, const float *normal_map, const float *depth, const float *alpha,
                                    const float *views, const float *grad_loss, float *grad_normal_map, float *grad_depth,
                                    float *grad_alpha, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !normal_map || !depth || !alpha || !views || !grad_loss) return LSR_ENULL;
    const int rc = nc_check(dims);
    if (rc) return rc;
    if (!grad_normal_map && !grad_depth && !grad_alpha) return LSR_OK;
    const double count = (double)dims->num_images * (double)dims->height * (double)dims->width;
    NcBwdArgs a{nc_shape(*dims), dims->alpha_min, 1.0 / count, normal_map, depth, alpha, views, grad_loss, grad_normal_map,
                grad_depth, grad_alpha};
    hipLaunchKernelGGL(k_nc_bwd, dim3((unsigned)nc_tiles(*dims)), dim3(kNcThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
