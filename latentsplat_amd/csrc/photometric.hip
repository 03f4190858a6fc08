// photometric.hip — the 3DGS photometric loss (include/lsr_loss.h): (1 - lambda) L1 + lambda (1 - SSIM) of rendered images
// against their targets, and its gradient with respect to the rendered images.
//
// Both big kernels have one shape.  A workgroup of 256 lanes owns one 32 x 32 tile of output pixels of one plane:
//   1. the tile of every input map with its 5-pixel halo (42 x 42) goes to LDS, lane j element j;
//   2. the horizontal 11-tap pass runs over the 42 haloed rows and leaves 42 x 32 values per moment in LDS;
//   3. the vertical pass: a lane owns one column and four consecutive rows, reads the 14 rows those four windows span
//      once per moment and keeps the 4 x (moments) sums in registers.
// Lanes of a wave walk consecutive columns in every LDS access (rows of 42 or 32 floats): no bank conflicts.
// The forward's maps are x - c and y - c, -c outside the image: the variances w*x^2 - mu^2 do not change when one
// constant is subtracted from every pixel of the window, padding included, and the two terms that cancel in them shrink
// with the window's mean (the means get their c back).  c is one constant per call, 0.5 times the image's share of its
// padded extent (photo_shift: the mean of a padded image whose own mean is 0.5) to the nearest eighth, so that tiny
// images, whose windows are mostly padding, are not shifted away from it (theirs is 0: the padding then adds exact
// zeros) and x - c keeps the low bits of most pixel values.  The backward is written in the same shifted variables (lsr_loss.h).
// The pixel's own x and y (the L1 term, the backward's factors) come from global memory as they are.
// Reductions, all in double and in a fixed order: a tile sums its S and |x - y| (wave shuffles, then the four waves in
// order) into its own workspace slot; k_photo_finish adds the slots of an image (lsr_image_sum.h).  No float atomics, no
// static state.
#include <math.h>

#include <cmath>

#include "lsr_image_sum.h"
#include "lsr_loss.h"

namespace lsr {

constexpr int kPhTile = 32;                      // output pixels per tile, each way
constexpr int kPhR = 5;                          // window radius
constexpr int kPhTaps = 2 * kPhR + 1;
constexpr int kPhHalo = kPhTile + 2 * kPhR;      // 42
constexpr int kPhThreads = 256;
constexpr int kPhRows = kPhTile * kPhTile / kPhThreads;      // 4 output rows per lane
constexpr int kPhSpan = kPhRows + 2 * kPhR;                  // 14 rows of the horizontal pass per lane
constexpr float kPhC1 = 0.01f * 0.01f, kPhC2 = 0.03f * 0.03f;

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, k = 0..10, rounded from double
__device__ __forceinline__ constexpr float ph_tap(int k) {
    constexpr float g[kPhTaps] = {0.0010283801f, 0.0075987581f, 0.0360007721f, 0.1093606895f, 0.2130055377f, 0.2660117249f,
                                  0.2130055377f, 0.1093606895f, 0.0360007721f, 0.0075987581f, 0.0010283801f};
    return g[k];
}

struct PhotoShape {
    int H, W, tiles_x, tiles_y;
};

// dst[42][42] = src - shift around the tile, `outside` beyond the image
__device__ __forceinline__ void ph_stage(float *__restrict__ dst, const float *__restrict__ src, const PhotoShape &s, int y0,
                                         int x0, float shift, float outside) {
    for (int i = threadIdx.x; i < kPhHalo * kPhHalo; i += kPhThreads) {
        const int r = i / kPhHalo, c = i - r * kPhHalo;
        const int gy = y0 + r - kPhR, gx = x0 + c - kPhR;
        const bool in = gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
        dst[i] = in ? src[(int64_t)gy * s.W + gx] - shift : outside;
    }
}

struct PhotoFwdArgs {
    PhotoShape s;
    float cov_norm, shift;
    int crop;
    const float *image, *target;
    double2 *slots;          // [planes][tiles_y][tiles_x]: sum of S over the cropped region, sum of |x - y|
    float *ssim_map;         // optional
    float *saved;            // optional: three maps, `map_stride` apart
    int64_t map_stride;      // V C H W
};

__global__ __launch_bounds__(kPhThreads) void k_photo_fwd(PhotoFwdArgs a) {
    __shared__ float s_in[2][kPhHalo * kPhHalo];
    __shared__ float s_h[5][kPhHalo * kPhTile];
    __shared__ double s_red[kPhThreads / LSR_WAVE][2];
    const PhotoShape s = a.s;
    int64_t plane;                                   // v * C + c
    int y0, x0;
    image_tile(s.tiles_x, s.tiles_y, kPhTile, plane, y0, x0);
    const int64_t base = plane * s.H * s.W;
    ph_stage(s_in[0], a.image + base, s, y0, x0, a.shift, -a.shift);
    ph_stage(s_in[1], a.target + base, s, y0, x0, a.shift, -a.shift);
    __syncthreads();

    // horizontal pass: the five moments of every haloed row
    for (int i = threadIdx.x; i < kPhHalo * kPhTile; i += kPhThreads) {
        const int r = i / kPhTile, c = i - r * kPhTile;
        const float *px = s_in[0] + r * kPhHalo + c, *py = s_in[1] + r * kPhHalo + c;
        float mx = 0.0f, my = 0.0f, mxx = 0.0f, myy = 0.0f, mxy = 0.0f;
#pragma unroll
        for (int k = 0; k < kPhTaps; ++k) {
            const float g = ph_tap(k), x = px[k], y = py[k];
            const float gx = g * x, gy = g * y;
            mx += gx; my += gy;
            mxx = fmaf(gx, x, mxx); myy = fmaf(gy, y, myy); mxy = fmaf(gx, y, mxy);
        }
        s_h[0][i] = mx; s_h[1][i] = my; s_h[2][i] = mxx; s_h[3][i] = myy; s_h[4][i] = mxy;
    }
    __syncthreads();

    // vertical pass: one column, kPhRows rows per lane
    const int col = threadIdx.x % kPhTile, row0 = threadIdx.x / kPhTile * kPhRows;
    float acc[5][kPhRows];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
#pragma unroll
        for (int o = 0; o < kPhRows; ++o) acc[m][o] = 0.0f;
#pragma unroll
        for (int j = 0; j < kPhSpan; ++j) {
            const float v = s_h[m][(row0 + j) * kPhTile + col];
#pragma unroll
            for (int o = 0; o < kPhRows; ++o)
                if (j - o >= 0 && j - o < kPhTaps) acc[m][o] = fmaf(ph_tap(j - o), v, acc[m][o]);
        }
    }

    double sums[2] = {0.0, 0.0};                     // of S over the cropped region, of |x - y|
    const int gx = x0 + col;
#pragma unroll
    for (int o = 0; o < kPhRows; ++o) {
        const int gy = y0 + row0 + o;
        if (gy < s.H && gx < s.W) {
            const int64_t at = base + (int64_t)gy * s.W + gx;
            // from the ten float sums on in double (a few dozen operations per pixel): S and the maps carry the sums'
            // rounding and one more, whatever the expression cancels
            const double m1 = acc[0][o], m2 = acc[1][o], n = a.cov_norm;
            const double mu1 = m1 + (double)a.shift, mu2 = m2 + (double)a.shift;
            const double s1 = n * (acc[2][o] - m1 * m1), s2 = n * (acc[3][o] - m2 * m2), s12 = n * (acc[4][o] - m1 * m2);
            const double A1 = 2.0 * mu1 * mu2 + (double)kPhC1, A2 = 2.0 * s12 + (double)kPhC2;
            const double B1 = mu1 * mu1 + mu2 * mu2 + (double)kPhC1, B2 = s1 + s2 + (double)kPhC2;
            const double S = (A1 * A2) / (B1 * B2);
            if (gy >= a.crop && gy < s.H - a.crop && gx >= a.crop && gx < s.W - a.crop) sums[0] += S;
            sums[1] += (double)fabsf(a.image[at] - a.target[at]);
            if (a.ssim_map) a.ssim_map[at] = (float)S;
            if (a.saved) {
                const double dS1 = -S / B2;                        // dS/ds1 = -A1 A2 / (B1 B2^2)
                const double dS12 = 2.0 * A1 / (B1 * B2);
                const double direct = 2.0 * mu2 * A2 / (B1 * B2) - 2.0 * mu1 * S / B1;
                a.saved[at] = (float)(direct - 2.0 * m1 * dS1 - m2 * dS12);
                a.saved[a.map_stride + at] = (float)dS1;
                a.saved[2 * a.map_stride + at] = (float)dS12;
            }
        }
    }
    double tile[2];
    block_sum<kPhThreads, 2, 1>(sums, s_red, tile);
    if (threadIdx.x == 0) a.slots[blockIdx.x] = make_double2(tile[0], tile[1]);
}

// The finish (lsr_image_sum.h) over the slots' two sums: an image's mean S and mean |x - y|, the loss from their means.
__global__ __launch_bounds__(kFinishThreads) void k_photo_finish(const double *__restrict__ slots, int V, int slots_per_image,
                                                                 double inv_count_s, double inv_count_l, float lambda,
                                                                 float *loss, float *l1, float *ssim) {
    image_finish<2, 2>(slots, V, slots_per_image, loss != nullptr,
                       [=](int v, int lane, const double (&sum)[2], double (&part)[2]) {
                           part[0] = sum[0] * inv_count_s; part[1] = sum[1] * inv_count_l;
                           if (lane == 0) {
                               if (ssim) ssim[v] = (float)part[0];
                               if (l1) l1[v] = (float)part[1];
                           }
                       },
                       [=](const double (&t)[2]) {
                           const double a = t[0] / V, b = t[1] / V;
                           *loss = (float)((1.0 - (double)lambda) * b + (double)lambda * (1.0 - a));
                       });
}

struct PhotoBwdArgs {
    PhotoShape s;
    float lambda, inv_n, shift;
    const float *image, *target, *saved, *grad_loss;
    float *grad_image;
    int64_t map_stride;
};

__global__ __launch_bounds__(kPhThreads) void k_photo_bwd(PhotoBwdArgs a) {
    __shared__ float s_in[3][kPhHalo * kPhHalo];
    __shared__ float s_h[3][kPhHalo * kPhTile];
    const PhotoShape s = a.s;
    int64_t plane;                                   // v * C + c
    int y0, x0;
    image_tile(s.tiles_x, s.tiles_y, kPhTile, plane, y0, x0);
    const int64_t base = plane * s.H * s.W;
#pragma unroll
    for (int m = 0; m < 3; ++m) ph_stage(s_in[m], a.saved + m * a.map_stride + base, s, y0, x0, 0.0f, 0.0f);
    __syncthreads();

    for (int i = threadIdx.x; i < kPhHalo * kPhTile; i += kPhThreads) {
        const int r = i / kPhTile, c = i - r * kPhTile;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float *p = s_in[m] + r * kPhHalo + c;
            float t = 0.0f;
#pragma unroll
            for (int k = 0; k < kPhTaps; ++k) t = fmaf(ph_tap(k), p[k], t);
            s_h[m][i] = t;
        }
    }
    __syncthreads();

    const int col = threadIdx.x % kPhTile, row0 = threadIdx.x / kPhTile * kPhRows;
    float acc[3][kPhRows];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
        for (int o = 0; o < kPhRows; ++o) acc[m][o] = 0.0f;
#pragma unroll
        for (int j = 0; j < kPhSpan; ++j) {
            const float v = s_h[m][(row0 + j) * kPhTile + col];
#pragma unroll
            for (int o = 0; o < kPhRows; ++o)
                if (j - o >= 0 && j - o < kPhTaps) acc[m][o] = fmaf(ph_tap(j - o), v, acc[m][o]);
        }
    }

    const float up = *a.grad_loss;
    const float k_l1 = (1.0f - a.lambda) * a.inv_n, k_ssim = a.lambda * a.inv_n;
    const int gx = x0 + col;
#pragma unroll
    for (int o = 0; o < kPhRows; ++o) {
        const int gy = y0 + row0 + o;
        if (gy < s.H && gx < s.W) {
            const int64_t at = base + (int64_t)gy * s.W + gx;
            const float x = a.image[at], y = a.target[at];
            const float d = acc[0][o] + 2.0f * (x - a.shift) * acc[1][o] + (y - a.shift) * acc[2][o];
            const float sgn = x > y ? 1.0f : (x < y ? -1.0f : 0.0f);
            a.grad_image[at] = up * (k_l1 * sgn - k_ssim * d);
        }
    }
}

// LSR_OK, or why these dims are refused (saved: the call reads or writes the saved maps)
static int photo_check(const lsr_photometric_dims *d, bool saved) {
    if (d->num_images < 1 || d->channels < 1 || d->height < 1 || d->width < 1) return LSR_EINVAL;
    if (!(d->lambda_dssim >= 0.0f && d->lambda_dssim <= 1.0f)) return LSR_EINVAL;
    if (!std::isfinite(d->cov_norm) || !(d->cov_norm > 0.0f)) return LSR_EINVAL;
    if (d->crop != 0 && d->crop != kPhR) return LSR_EINVAL;
    if (d->crop == kPhR && (d->height < kPhTaps || d->width < kPhTaps)) return LSR_EINVAL;
    if (d->reserved0) return LSR_EINVAL;
    if (saved && (d->crop != 0 || d->cov_norm != 1.0f)) return LSR_EINVAL;
    const int64_t n = (int64_t)d->num_images * d->channels;
    if (n >= ((int64_t)1 << 31) || n * d->height >= ((int64_t)1 << 31) || n * d->height * d->width >= ((int64_t)1 << 31))
        return LSR_EUNSUPPORTED;
    return LSR_OK;
}

// the constant both kernels subtract from the images (file header; lsr_loss.h documents it: `saved` depends on it)
static float photo_shift(const lsr_photometric_dims &d) {
    const double share = (double)d.height * d.width / ((d.height + 2.0 * kPhR) * (d.width + 2.0 * kPhR));
    return (float)(std::floor(4.0 * share + 0.5) / 8.0);
}

static PhotoShape photo_shape(const lsr_photometric_dims &d) {
    return PhotoShape{d.height, d.width, (d.width + kPhTile - 1) / kPhTile, (d.height + kPhTile - 1) / kPhTile};
}

// tiles of all planes: below 2^31 / 1 whenever V C H W is (a tile holds at least one pixel)
static int64_t photo_tiles(const lsr_photometric_dims &d) {
    const PhotoShape s = photo_shape(d);
    return (int64_t)d.num_images * d.channels * s.tiles_x * s.tiles_y;
}

}  // namespace lsr

using namespace lsr;

extern "C" {

size_t lsr_photometric_workspace_bytes(const lsr_photometric_dims *dims) {
    if (!dims || photo_check(dims, false) != LSR_OK) return 0;
    return align_up((size_t)photo_tiles(*dims) * sizeof(double2));
}

int lsr_photometric_forward(const lsr_photometric_dims *dims, const float *image, const float *target, void *workspace,
                            float *loss, float *l1, float *ssim, float *ssim_map, float *saved, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !image || !target || !workspace) return LSR_ENULL;
    const int rc = photo_check(dims, saved != nullptr);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return LSR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const PhotoShape shape = photo_shape(*dims);
    const int64_t planes = (int64_t)dims->num_images * dims->channels, pixels = (int64_t)dims->height * dims->width;
    PhotoFwdArgs a{shape, dims->cov_norm, photo_shift(*dims), dims->crop, image, target, (double2 *)workspace, ssim_map, saved, planes * pixels};
    hipLaunchKernelGGL(k_photo_fwd, dim3((unsigned)photo_tiles(*dims)), dim3(kPhThreads), 0, s, a);
    if (loss || l1 || ssim) {
        const double cropped = (double)(dims->height - 2 * dims->crop) * (double)(dims->width - 2 * dims->crop);
        hipLaunchKernelGGL(k_photo_finish, dim3(1), dim3(kFinishThreads), 0, s, (const double *)workspace, dims->num_images,
                           dims->channels * shape.tiles_x * shape.tiles_y, 1.0 / (cropped * dims->channels),
                           1.0 / ((double)pixels * dims->channels), dims->lambda_dssim, loss, l1, ssim);
    }
    return launch_status();
}

int lsr_photometric_backward(const lsr_photometric_dims *dims, const float *image, const float *target, const float *saved,
                             const float *grad_loss, float *grad_image, lsr_stream_t stream) {
    note_hip_error(0);
    if (!dims || !image || !target || !saved || !grad_loss || !grad_image) return LSR_ENULL;
    const int rc = photo_check(dims, true);
    if (rc) return rc;
    const int64_t n = (int64_t)dims->num_images * dims->channels * dims->height * dims->width;
    PhotoBwdArgs a{photo_shape(*dims), dims->lambda_dssim, (float)(1.0 / (double)n), photo_shift(*dims), image, target, saved, grad_loss, grad_image, n};
    hipLaunchKernelGGL(k_photo_bwd, dim3((unsigned)photo_tiles(*dims)), dim3(kPhThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

}  // extern "C"
