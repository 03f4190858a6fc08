// image_prepare.hip — photographs onto the rasterizer's camera (include/lsr_image.h): one pass over the output pixels that
// undoes the principal-point offset and the lens distortion of the source camera and reduces to the training resolution
// by averaging S x S sub-samples, each a bilinear tap of the uint8 source.
//
// A byte-granular gather: what a sub-sample needs is 4 x C bytes at a computed address, so nothing is staged.  The layout
// makes the gather as dense as it can be: a workgroup is 64 x 4 threads, a wave is 64 consecutive output columns of one
// row, so that at every (a, b) of the sub-sample loop the wave's taps walk along one or two source rows with a stride of
// (fx / fx') C bytes and the cache lines a wave touches are shared by its lanes and reused by the next a.  The camera is
// a kernel argument by value: the waves read it as scalars.  The model is resolved on the host: (k1, k2, p1, p2) are
// filled from the model's own numbers, and the launch picks one of two kernels (DISTORT or not, C a template parameter),
// so no lane ever branches on the model.  Indices inside an image are 32-bit (the host refuses Hs Ws C >= 2^31); the
// image's base is the only 64-bit product.  Uncovered sub-samples skip their loads; their lanes idle for that tap only.
// Every output value has one owner and the sub-samples are summed in a fixed order: two calls give the same bits.
#include <math.h>

#include <cmath>

#include "lsr_image.h"
#include "lsr_internal.h"

namespace lsr {

constexpr int kImageCols = 64;      // one wave: 64 consecutive output columns
constexpr int kImageRows = 4;       // waves (output rows) per workgroup

struct ImageCam {                   // the source camera as the kernel takes it, by value
    float fx, fy, cx, cy;
    float k1, k2, p1, p2;
    float sx, sy;                   // fx / fx', fy / fy' (float32 quotients, formed once on the host)
    float fxo, fyo;                 // fx', fy'
};

template <bool DISTORT, int C>
__global__ __launch_bounds__(kImageCols * kImageRows) void k_image_prepare(const uint8_t *__restrict__ src, int Hs, int Ws, int H, int W,
                                                                           int S, ImageCam cam, const float *__restrict__ background,
                                                                           float *__restrict__ image, float *__restrict__ coverage) {
    const int j = blockIdx.x * kImageCols + threadIdx.x;
    const int i = blockIdx.y * kImageRows + threadIdx.y;
    if (j >= W || i >= H) return;
    const uint8_t *img = src + (size_t)blockIdx.z * ((size_t)Hs * (size_t)Ws * C);
    const float cxo = 0.5f * (float)W, cyo = 0.5f * (float)H;       // exact: W, H <= 65536
    const float fS = (float)S, fWs = (float)Ws, fHs = (float)Hs;
    const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
    float bg[3] = {0.0f, 0.0f, 0.0f};
    if (C == 4 && background) { bg[0] = 255.0f * background[0]; bg[1] = 255.0f * background[1]; bg[2] = 255.0f * background[2]; }
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int covered = 0;
    for (int b = 0; b < S; ++b) {
        const float vo = (float)i + ((float)b + 0.5f) / fS;
        const float dy = vo - cyo;
        const float y = DISTORT ? dy / cam.fyo : 0.0f;
        const float v_plain = dy * cam.sy + cam.cy;
        for (int a = 0; a < S; ++a) {
            const float uo = (float)j + ((float)a + 0.5f) / fS;
            const float dx = uo - cxo;
            float u, v;
            if (DISTORT) {
                const float x = dx / cam.fxo;
                const float r2 = x * x + y * y;
                const float radial = 1.0f + cam.k1 * r2 + cam.k2 * (r2 * r2);
                const float xd = x * radial + 2.0f * cam.p1 * (x * y) + cam.p2 * (r2 + 2.0f * (x * x));
                const float yd = y * radial + 2.0f * cam.p2 * (x * y) + cam.p1 * (r2 + 2.0f * (y * y));
                u = cam.fx * xd + cam.cx;
                v = cam.fy * yd + cam.cy;
            } else {
                u = dx * cam.sx + cam.cx;
                v = v_plain;
            }
            const bool in = u >= 0.0f && u <= fWs && v >= 0.0f && v <= fHs;       // false for a NaN
            if (!in) continue;
            const float xs = u - 0.5f, ys = v - 0.5f;
            const float xf = floorf(xs), yf = floorf(ys);
            const float wx = xs - xf, wy = ys - yf;
            // covered: xf in [-1, Ws - 1], yf in [-1, Hs - 1]; the clamps make every index one of the image's own
            const int x0 = (int)fminf(fmaxf(xf, 0.0f), xmax), x1 = (int)fminf(fmaxf(xf + 1.0f, 0.0f), xmax);
            const int y0 = (int)fminf(fmaxf(yf, 0.0f), ymax), y1 = (int)fminf(fmaxf(yf + 1.0f, 0.0f), ymax);
            const uint8_t *p00 = img + (y0 * Ws + x0) * C, *p01 = img + (y0 * Ws + x1) * C;
            const uint8_t *p10 = img + (y1 * Ws + x0) * C, *p11 = img + (y1 * Ws + x1) * C;
            float val[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t00 = (float)p00[c], t01 = (float)p01[c], t10 = (float)p10[c], t11 = (float)p11[c];
                const float top = t00 + wx * (t01 - t00), bot = t10 + wx * (t11 - t10);
                val[c] = top + wy * (bot - top);
            }
            if (C == 4) {
                const float alpha = val[C - 1] / 255.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) val[c] = val[c] * alpha + bg[c] * (1.0f - alpha);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += val[c];
            ++covered;
        }
    }
    const int plane = H * W;                                    // <= 2^32 would not fit: the host keeps 3 H W below 2^31
    const int at = i * W + j;
    float *out = image + (size_t)blockIdx.z * (3 * (size_t)plane);
    const float denom = 255.0f * (float)covered;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane + at] = covered ? acc[c] / denom : 0.0f;
    coverage[(size_t)blockIdx.z * (size_t)plane + at] = (float)covered / (float)(S * S);
}

static bool finite_all(const float *v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// The checks both entry points share, and the camera as the kernel takes it.  *distort: some distortion number is not 0.
static int resolve(const lsr_image_dims *d, const lsr_image_camera *c, ImageCam *cam, bool *distort, int *S) {
    if (!d || !c) return LSR_ENULL;
    if (c->reserved != 0 || c->model < LSR_IMAGE_SIMPLE_PINHOLE || c->model > LSR_IMAGE_OPENCV) return LSR_EINVAL;
    static const int used[] = {0, 0, 1, 2, 4};
    for (int k = used[c->model]; k < 4; ++k)
        if (c->dist[k] != 0.0f) return LSR_EINVAL;
    const float nums[] = {c->fx, c->fy, c->cx, c->cy, c->dist[0], c->dist[1], c->dist[2], c->dist[3], d->fx, d->fy};
    if (!finite_all(nums, 10) || !(c->fx > 0.0f) || !(c->fy > 0.0f) || !(d->fx > 0.0f) || !(d->fy > 0.0f)) return LSR_EINVAL;
    const float sx = c->fx / d->fx, sy = c->fy / d->fy;
    const float s = ceilf(fmaxf(fmaxf(sx, sy), 1.0f));
    if (!(s <= (float)LSR_IMAGE_MAX_SUBSAMPLES)) return LSR_EUNSUPPORTED;
    *S = (int)s;
    *cam = ImageCam{c->fx, c->fy, c->cx, c->cy, c->dist[0], c->dist[1], c->dist[2], c->dist[3], sx, sy, d->fx, d->fy};
    *distort = c->dist[0] != 0.0f || c->dist[1] != 0.0f || c->dist[2] != 0.0f || c->dist[3] != 0.0f;
    return LSR_OK;
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_image_subsamples(const lsr_image_dims *dims, const lsr_image_camera *camera) {
    ImageCam cam;
    bool distort;
    int S = 0;
    const int rc = resolve(dims, camera, &cam, &distort, &S);
    return rc == LSR_OK ? S : rc;
}

int lsr_image_prepare(const lsr_image_dims *dims, const lsr_image_camera *camera, const uint8_t *src, const float *background,
                      float *image, float *coverage, lsr_stream_t stream) {
    note_hip_error(0);
    ImageCam cam;
    bool distort;
    int S = 0;
    const int rc = resolve(dims, camera, &cam, &distort, &S);
    if (rc != LSR_OK) return rc;
    const lsr_image_dims &d = *dims;
    const auto extent_ok = [](int32_t e) { return e >= 1 && e <= LSR_IMAGE_MAX_EXTENT; };
    if (d.batch < 0 || !extent_ok(d.src_height) || !extent_ok(d.src_width) || !extent_ok(d.height) || !extent_ok(d.width)) return LSR_EINVAL;
    if (d.channels != 3 && d.channels != 4) return LSR_EINVAL;
    // 32-bit indices inside one image, source and output
    if ((int64_t)d.src_height * d.src_width * d.channels >= (int64_t)1 << 31 || (int64_t)d.height * d.width * 3 >= (int64_t)1 << 31) return LSR_EUNSUPPORTED;
    if (d.batch > 65535) return LSR_EUNSUPPORTED;
    if (d.batch == 0) return LSR_OK;
    if (!src || !image || !coverage) return LSR_ENULL;
    const dim3 block(kImageCols, kImageRows);
    const dim3 grid((unsigned)((d.width + kImageCols - 1) / kImageCols), (unsigned)((d.height + kImageRows - 1) / kImageRows), (unsigned)d.batch);
    hipStream_t s = (hipStream_t)stream;
#define LSR_IMAGE_LAUNCH(DISTORT, C)                                                                                              \
    hipLaunchKernelGGL((k_image_prepare<DISTORT, C>), grid, block, 0, s, src, (int)d.src_height, (int)d.src_width, (int)d.height, \
                       (int)d.width, S, cam, background, image, coverage)
    if (d.channels == 3) { if (distort) LSR_IMAGE_LAUNCH(true, 3); else LSR_IMAGE_LAUNCH(false, 3); }
    else                 { if (distort) LSR_IMAGE_LAUNCH(true, 4); else LSR_IMAGE_LAUNCH(false, 4); }
#undef LSR_IMAGE_LAUNCH
    return launch_status();
}

}  // extern "C"
