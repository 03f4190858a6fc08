/*
 * lsr_loss.h — C ABI of the 3DGS photometric loss: (1 - lambda) * L1 + lambda * (1 - SSIM) between
 * rendered images and their targets, and its gradient with respect to the rendered images.  Same
 * library (liblsr_hip.so) and conventions as lsr_scene.h: device pointers, sizes, a stream,
 * negative LSR_E* codes, asynchronous on the caller's stream.
 *
 * Definition (per plane of [V][C][H][W] float32 images x = image, y = target, values as they are):
 * g is the normalised 11-tap Gaussian of sigma 1.5, w = g g^T, pixels outside the image count as 0;
 *   mu1 = w*x, mu2 = w*y, s1 = n (w*x^2 - mu1^2), s2 = n (w*y^2 - mu2^2), s12 = n (w*xy - mu1 mu2)
 *   S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  C1 = 0.01^2, C2 = 0.03^2
 * with n = cov_norm.  ssim[v] is the mean of S over the image's C (H - 2 crop)(W - 2 crop) values at
 * least `crop` pixels from every border, l1[v] the mean of |x - y| over all C H W values, and
 *   loss = (1 - lambda) mean_v l1[v] + lambda (1 - mean_v ssim[v]).
 * cov_norm = 1, crop = 0 is the loss every 3DGS trainer optimises; cov_norm = 121/120, crop = 5 is
 * the evaluation metric (sample covariance, interior pixels only: those windows never see the padding).
 */
#ifndef LSR_LOSS_H
#define LSR_LOSS_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsr_photometric_dims {
    int32_t num_images;    /* V >= 1 */
    int32_t channels;      /* C >= 1 */
    int32_t height;        /* H >= 1 */
    int32_t width;         /* W >= 1 */
    float lambda_dssim;    /* in [0, 1] */
    float cov_norm;        /* finite, > 0 */
    int32_t crop;          /* 0 or 5 (needs H, W >= 11) */
    int32_t reserved0;     /* 0 */
} lsr_photometric_dims;

/* Bytes of the workspace the forward needs (one pair of double partial sums per tile of every plane): a pure function of the dims,
 * host only.  0 for dims the forward would refuse. */
size_t lsr_photometric_workspace_bytes(const lsr_photometric_dims *dims);

/* Two launches: one over 32 x 32 tiles of output pixels of every plane (both images staged with their 5-pixel halo in LDS,
 * the five moments through the separable window, S and |x - y| formed and summed per tile into the tile's own workspace
 * slot), one that adds the slots per image in a fixed order.  No float atomics: two calls give the same bits.
 * Outputs, each optional (NULL = not wanted):
 *   loss [1], l1 [V], ssim [V]
 *   ssim_map [V][C][H][W]   S at every pixel (crop does not restrict the map)
 *   saved [3][V][C][H][W]   what lsr_photometric_backward reads: D, dS/ds1 and dS/ds12.  D is dS/dmu1 with the variances'
 *                           dependence on mu1 folded in, Dmu = dS/dmu1 - 2 mu1 dS/ds1 - mu2 dS/ds12, written for the
 *                           images shifted by -c: D = Dmu + c (2 dS/ds1 + dS/ds12).  The kernels convolve x - c and y - c
 *                           (-c outside the image), which leaves the variances as they are and shrinks the terms that
 *                           cancel in them; c = 0.5 H W / ((H + 10)(W + 10)) to the nearest eighth.  Needs crop == 0, cov_norm == 1.
 * image, target and workspace (lsr_photometric_workspace_bytes, 16-byte aligned) are required.  Nothing is allocated and the
 * host is never waited for.
 * LSR_ENULL: a NULL dims, image, target or workspace.  LSR_EINVAL (before any GPU work): a size < 1, lambda_dssim outside
 * [0, 1], a cov_norm that is not finite and positive, crop other than 0 or 5, crop 5 with H or W < 11, a non-zero reserved
 * field, `saved` with crop != 0 or cov_norm != 1.  LSR_EUNSUPPORTED: V C H W >= 2^31. */
int lsr_photometric_forward(const lsr_photometric_dims *dims, const float *image, const float *target, void *workspace,
                            float *loss, float *l1, float *ssim, float *ssim_map, float *saved, lsr_stream_t stream);

/* One launch: grad_image [V][C][H][W] = *grad_loss * d loss / d image, written, never accumulated.  `saved` is what the
 * forward wrote for the same dims, image and target; grad_loss is a DEVICE pointer to one float (the upstream gradient of
 * the scalar loss).  With N = V C H W and the three saved maps D, E, F:
 *   d loss / dx = ((1 - lambda) sign(x - y) - lambda (w*D + 2 (x - c) (w*E) + (y - c) (w*F))) / N,   sign(0) = 0,
 * the maps taken as zero outside the image.  Same codes as the forward; every pointer is required; crop must be 0 and
 * cov_norm 1. */
int lsr_photometric_backward(const lsr_photometric_dims *dims, const float *image, const float *target, const float *saved,
                             const float *grad_loss, float *grad_image, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_LOSS_H */
