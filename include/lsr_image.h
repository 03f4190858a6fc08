/*
 * lsr_image.h — C ABI of the image preparation for captures: photographs, as a camera with an off-centre principal point
 * and lens distortion took them, resampled onto the centred, distortion-free pinhole camera the rasterizer implements, at
 * the training resolution, in one pass over the output pixels.  Same library (liblsr_hip.so) and conventions as
 * lsr_filter3d.h: device pointers, a stream, asynchronous, negative LSR_E* codes returned before any GPU work, an empty
 * batch launches nothing and returns LSR_OK, nothing is read back.  No atomics: every output value has one owner and two
 * calls give the same bits; the launch is graph-capturable.  Values only: targets need no gradient.
 */
#ifndef LSR_IMAGE_H
#define LSR_IMAGE_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_IMAGE_MAX_SUBSAMPLES 16     /* S, per axis */
#define LSR_IMAGE_MAX_EXTENT 65536      /* largest source or output width / height */

enum {                                  /* lsr_image_camera.model: COLMAP's ids */
    LSR_IMAGE_SIMPLE_PINHOLE = 0,       /* no distortion numbers */
    LSR_IMAGE_PINHOLE = 1,
    LSR_IMAGE_SIMPLE_RADIAL = 2,        /* dist = k */
    LSR_IMAGE_RADIAL = 3,               /* dist = k1 k2 */
    LSR_IMAGE_OPENCV = 4                /* dist = k1 k2 p1 p2 */
};

typedef struct lsr_image_camera {       /* the SOURCE camera, one per call, in source pixels */
    int32_t model;
    int32_t reserved;                   /* 0 */
    float fx, fy, cx, cy;               /* (the one-focal models give fx = fy = f) */
    float dist[4];                      /* the model's distortion numbers in its own order; the unused tail must be 0 */
} lsr_image_camera;

typedef struct lsr_image_dims {
    int32_t batch;                      /* B */
    int32_t src_height, src_width;      /* Hs, Ws */
    int32_t channels;                   /* C: 3 (RGB) or 4 (RGBA) */
    int32_t height, width;              /* H, W of the output */
    float fx, fy;                       /* focal lengths of the TARGET camera in output pixels: fx', fy' */
} lsr_image_dims;

/* S = ceil(max(fx / fx', fy / fy', 1)) in float32: the sub-samples per axis and output pixel.  Negative: LSR_EINVAL for a
 * focal length that is not finite and positive, LSR_EUNSUPPORTED for S > LSR_IMAGE_MAX_SUBSAMPLES.  Host only. */
int lsr_image_subsamples(const lsr_image_dims *dims, const lsr_image_camera *camera);

/* src [B][Hs][Ws][C] uint8; background [3] (NULL: black; read only for C = 4); image [B][3][H][W]; coverage [B][H][W].
 * Per output pixel (i, j), in float32.  The target camera is a centred pinhole, cx' = W / 2, cy' = H / 2, a pixel's
 * centre at j + 0.5.  The S x S sub-samples sit at u' = j + (a + 0.5) / S, v' = i + (b + 0.5) / S.
 *   Without distortion (models 0 and 1, or every distortion number zero) the source position is formed in pixel units:
 *     u = (u' - cx') (fx / fx') + cx,   v = (v' - cy') (fy / fy') + cy
 *   (exact for a power-of-two reduction and a half-integer principal-point shift).  With distortion, with (k1, k2, p1, p2)
 *   = (k, 0, 0, 0), (k1, k2, 0, 0) or the four numbers of OPENCV:
 *     x = (u' - cx') / fx',  y = (v' - cy') / fy',  r2 = x x + y y,  radial = 1 + k1 r2 + k2 r2 r2,
 *     x_d = x radial + 2 p1 x y + p2 (r2 + 2 x x),   y_d = y radial + 2 p2 x y + p1 (r2 + 2 y y),
 *     u = fx x_d + cx,  v = fy y_d + cy.
 *   A sub-sample is COVERED when 0 <= u <= Ws and 0 <= v <= Hs (a NaN is not).  Its value per channel is the bilinear
 *   interpolation of the raw 0..255 bytes at (u - 0.5, v - 0.5), indices clamped to the edge; for C = 4 all four channels
 *   are interpolated and the value is rgb a / 255 + 255 background (1 - a / 255).
 *   image = (sum of the covered values) / (255 n_covered), one IEEE division, 0 where nothing is covered;
 *   coverage = n_covered / S^2.
 * One launch: a wave owns 64 consecutive output columns of one row, the camera arrives by value and is read as scalars,
 * the model is resolved before the launch (two kernels: with and without distortion), indices are 32-bit inside an image.
 * LSR_EINVAL: a NULL or non-zero-reserved struct field, B < 0, an extent outside [1, LSR_IMAGE_MAX_EXTENT], C not 3 or 4,
 * an unknown model, a non-zero number in the unused tail of dist, a camera number that is not finite, a focal length that
 * is not positive.  LSR_EUNSUPPORTED: S > LSR_IMAGE_MAX_SUBSAMPLES, Hs Ws C >= 2^31, B > 65535.  LSR_ENULL: with B > 0 a
 * NULL src, image or coverage. */
int lsr_image_prepare(const lsr_image_dims *dims, const lsr_image_camera *camera, const uint8_t *src, const float *background,
                      float *image, float *coverage, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_IMAGE_H */
