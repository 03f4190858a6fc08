/*
 * lsr_vq.h — C ABI of the vector quantisation behind the codebook compression of a 3DGS scene: the two halves of a
 * weighted Lloyd iteration (k-means) over n rows of d floats and a codebook of k rows.  Same library (liblsr_hip.so)
 * and conventions as lsr_knn.h: device pointers, float32 row-major contiguous tensors, int32 indices, a stream,
 * asynchronous, negative LSR_E* codes returned before any GPU work, n == 0 launches nothing and returns LSR_OK.
 * No float atomics anywhere: both calls give the same bits every time.
 *
 * lsr_vq_assign   the nearest code of every row.  The n x k matrix of distances never exists: a workgroup keeps
 *                 LSR_VQ_ROWS rows in LDS, the codebook streams past it in tiles of LSR_VQ_CODES codes (double
 *                 buffered), the products run on the f32-input matrix instruction (v_mfma_f32_32x32x2_f32, bit for bit
 *                 a chain of fmaf) and every lane keeps the best (score, index) of the accumulator elements it has seen.
 * lsr_vq_update   the weighted mean of the rows of every code, summed in float64 in an order that depends on the
 *                 arguments only: a stable radix sort of (code, row), float64 sums over fixed blocks of the sorted order,
 *                 a code's block sums added in block order.
 */
#ifndef LSR_VQ_H
#define LSR_VQ_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_VQ_MAX_DIM 96
#define LSR_VQ_MAX_CODES 65536
#define LSR_VQ_MAX_ROWS (1 << 28) /* 32-bit sort sizes and row indices */
/* the tiling of lsr_vq_assign: rows per workgroup, codes per LDS tile, floats a row is zero-padded to a multiple of */
#define LSR_VQ_ROWS 128
#define LSR_VQ_CODES 64
#define LSR_VQ_KSTEP 4

typedef struct lsr_vq_dims {
    int64_t n;                    /* rows, 0 .. LSR_VQ_MAX_ROWS */
    int32_t k;                    /* codes, 1 .. LSR_VQ_MAX_CODES */
    int32_t d;                    /* floats per row, 1 .. LSR_VQ_MAX_DIM */
    int32_t reserved0, reserved1; /* 0 */
} lsr_vq_dims;

/* Bytes of device scratch either call needs (one figure serves both).  A pure function of its arguments, non-decreasing
 * in n and in k: it can be asked without a device.  0 for arguments outside the limits above (and for n == 0). */
size_t lsr_vq_workspace_bytes(int64_t n, int32_t k, int32_t d);

/* idx_out[i] = the j in [0, k) that minimises |x_i - c_j|^2, found as the largest  x_i . c_j - |c_j|^2 / 2  in float32:
 * the bias -|c_j|^2 / 2 (a chain of fmaf over d, then one multiplication) seeds the accumulator and the d products are
 * added to it one fmaf each.  Equal scores go to the lowest j.  The chosen code is within
 * 4 (d + 2) 2^-24 (|x_i| + max_j |c_j|)^2 of the smallest squared distance; where every product and sum is exact in
 * float32 (small integers) it is the exact lowest-index nearest code.
 * dist2_out (optional, NULL = not wanted): sum over d of (x - c)^2 for the chosen code, computed from the differences in
 * float32 (not from the score): exact zeros are exact.
 * Inputs are expected to be finite.  Rows or codes that are not give unspecified indices, still inside [0, k); nothing
 * is read or written out of bounds.
 * LSR_EINVAL: n, k or d outside the limits, a non-zero reserved field.  LSR_ENULL: dims NULL; with n > 0: x, codebook,
 * idx_out or workspace NULL. */
int lsr_vq_assign(const lsr_vq_dims *dims, const float *x, const float *codebook, int32_t *idx_out, float *dist2_out,
                  void *workspace, lsr_stream_t stream);

/* For every code j, over the rows i with idx[i] == j and the weights w (NULL = every weight 1):
 *   mass_out[j]        sum of w_i
 *   codebook_out[j][:] sum of w_i x_i / sum of w_i, or prev_codebook[j][:] bit for bit where the mass is not positive
 *                      (a code nothing chose, or only rows of weight 0).
 * Rows whose idx lies outside [0, k) are skipped.  The sums are float64 (every product w_i x_i is exact there), rounded
 * to float32 once after the division.  The order of every sum is fixed by the arguments: the same bits on every call.
 * Weights are expected to be finite and non-negative.  codebook_out must not overlap prev_codebook.
 * n == 0 launches nothing and writes nothing (the caller's codebook is then prev_codebook and every mass 0).
 * LSR_EINVAL as lsr_vq_assign.  LSR_ENULL: dims NULL; with n > 0: x, idx, prev_codebook, codebook_out, mass_out or
 * workspace NULL.  LSR_EUNSUPPORTED: the device's sort asks for more scratch than lsr_vq_workspace_bytes reserves for it
 * (checked on the host, before any launch). */
int lsr_vq_update(const lsr_vq_dims *dims, const float *x, const int32_t *idx, const float *weights,
                  const float *prev_codebook, float *codebook_out, float *mass_out, void *workspace, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_VQ_H */
