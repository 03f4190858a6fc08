/*
 * lsr_mcmc.h — C ABI of the MCMC densification strategy for a trainable 3DGS scene (lsr_scene.h), after "3D Gaussian
 * Splatting as Markov Chain Monte Carlo" (Kheradmand et al., 2024): the dead-row classification, sampling of rows in
 * proportion to a weight, the relocation / growth of the published relocate_gs / add_new_gs over every per-Gaussian table
 * (parameters and optimiser moments), and the per-step covariance-shaped noise on the positions.  Same library
 * (liblsr_hip.so) and conventions as lsr_density.h: device float32 pointers, a stream, asynchronous, negative LSR_E* codes
 * returned before any GPU work, n == 0 launches nothing and returns LSR_OK.  No float atomics; every output element has
 * one owner: two calls give the same bits.  The only atomics are integer increments of `count`, whose result does not
 * depend on their order.  Random numbers are the caller's.
 */
#ifndef LSR_MCMC_H
#define LSR_MCMC_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_MCMC_MAX_ROWS (1 << 28)    /* n, and n + m of a growth, stay below this */
#define LSR_MCMC_MAX_TABLES 24
#define LSR_MCMC_MAX_WIDTH 4096        /* floats per row of a table */
#define LSR_MCMC_MAX_RATIO 50          /* N = min(count + 1, 50): the published 51-row binomial table */
#define LSR_MCMC_WEIGHT_BITS 30        /* a weight is quantised to trunc(clamp(w, 0, 1) * 2^30) */

enum {                       /* lsr_mcmc_table.role */
    LSR_MCMC_COPY = 0,       /* a destination row copies its source's row; sources keep theirs */
    LSR_MCMC_OPACITY = 1,    /* width 1, logits: sources and destinations take the new opacity */
    LSR_MCMC_SCALING = 2,    /* width 3, logs: sources and destinations take the new scaling */
    LSR_MCMC_MOMENT = 3      /* an optimiser moment: rows of sources become 0; destinations see below */
};

/* Bytes of device scratch that any one call below needs for n rows and m draws (0 for n <= 0). */
size_t lsr_mcmc_workspace_bytes(int64_t n, int64_t m);

/* One pass over the opacity logits [n].  A row is dead when opacity[g] <= dead_logit (the host passes logit(min_opacity)
 * computed in double and rounded to float: the comparison is exact).  weights[g] = dead ? 0 : 1 / (1 + expf(-opacity[g])).
 * With `dead` and `counts` given, dead[0 .. counts[0]) are the indices of the dead rows in index order ([n] int32, the rest
 * is not written) and counts = {dead, alive}: a per-chunk count, a scan of the chunk sums and a per-chunk emission.  With
 * both NULL only the weights are written, in one launch (dead_logit = -inf: the weights of a growth, nothing is dead).
 * LSR_EINVAL: n < 0 or n >= 2^28, a NaN dead_logit, exactly one of dead / counts NULL.  LSR_ENULL: with n > 0 a NULL
 * opacity or weights, or a NULL workspace when dead is given.  With n == 0 counts is not written. */
int lsr_mcmc_classify(int64_t n, const float *opacity, float dead_logit, float *weights, int32_t *dead, uint32_t *counts,
                      void *workspace, lsr_stream_t stream);

/* m draws from n rows in proportion to their weights, by inverse CDF in exact integer arithmetic (the answer does not
 * depend on the shape of the scan):
 *   q[g]   = (uint32) trunc(clamp(weights[g], 0, 1) * 2^30), a NaN counting as 0;
 *   cum    = the inclusive prefix sum of q in uint64;  total = cum[n - 1];
 *   t[j]   = min((uint64)(clamp(uniforms[j], 0, 1 - 2^-53) * (double)total), total - 1), a NaN counting as 0;
 *   idx[j] = the smallest g with cum[g] > t[j]  (a row of weight 0 is never drawn);
 *   count[g] = the number of j that drew g.
 * uniforms [m] are the caller's float64 (float32 uniforms have 24 bits: too coarse for millions of rows); idx [m] int32;
 * count [n] uint32 is zeroed by the call; *total (device, may be NULL) receives the total.  With total == 0 every idx[j]
 * is -1 and count stays 0.  Chunk sums, one workgroup scanning them, the prefix sums, and one lane per draw searching
 * the chunk bases and then its chunk: four launches (three with m == 0), nothing read back.
 * LSR_EINVAL: n < 0, n >= 2^28, m < 0, m >= 2^31.  LSR_ENULL: with n > 0 a NULL weights, count or workspace, or with
 * m > 0 a NULL uniforms or idx.  n == 0 with m > 0 is LSR_EINVAL (there is nothing to draw from and nothing is launched). */
int lsr_mcmc_sample(int64_t n, const float *weights, int64_t m, const double *uniforms, int32_t *idx, uint32_t *count,
                    uint64_t *total, void *workspace, lsr_stream_t stream);

typedef struct lsr_mcmc_table {
    float *table;        /* [n][width] for a relocation, [n + m][width] for a growth; updated in place */
    int32_t width;       /* 1 .. LSR_MCMC_MAX_WIDTH; 1 for OPACITY, 3 for SCALING */
    int32_t role;        /* LSR_MCMC_* */
} lsr_mcmc_table;

/* The published relocate_gs (dest given) / add_new_gs (dest NULL), in place over every table, from the idx [m] and
 * count [n] of ONE lsr_mcmc_sample call.  A source is a row g < n with c = count[g] > 0; N = min(c + 1, 50).  With
 * o = sigmoid(opacity[g]):
 *   o'      = 1 - (1 - o)^(1 / N)
 *   D       = sum_{k=0..N-1} C(N, k+1) (-1)^k o'^(k+1) / sqrt(k+1)
 *             (the published double loop sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1), summed over i)
 *   scale'  = (o / D) * exp(scaling[g])
 *   o'      clamped to [min_opacity, 1 - 1.1920929e-7]
 * stored as logit(o') and log(scale'), evaluated in double with an exact binomial table and rounded once.
 *   Every source row: OPACITY and SCALING take the new values; its rows of every MOMENT table become 0.
 *   Every destination row d = dest[j] (dest NULL: d = n + j, the growth): COPY tables copy row idx[j]; OPACITY and SCALING
 *   take the new values of source idx[j], bit for bit.  MOMENT tables: in the growth the destination's rows are 0; in the
 *   relocation a destination KEEPS its own moments — what the published trainer does (its relocate_gs resets the
 *   optimiser state of the sampled rows only).  Entries with idx[j] < 0 are skipped.
 * A destination must not be a source (a dead row has weight 0 and is never drawn; a new row lies beyond n) and no row may
 * be a destination twice; entries that point outside their table are skipped.  Exactly one OPACITY and one SCALING table
 * are required.  Two launches: the sources (new values to scratch and to their own rows, moments zeroed), then the
 * destinations (which read scratch and columns no launch writes).
 * LSR_EINVAL: n < 0, m < 0, n + m >= 2^28, num_tables out of 0..24, a width or role out of range, not exactly one OPACITY
 * and one SCALING table, min_opacity not in [0, 1).  LSR_ENULL: with n > 0, a NULL count, tables, table pointer or
 * workspace, or with m > 0 a NULL idx.  n == 0 launches nothing. */
int lsr_mcmc_apply(int64_t n, int64_t m, const int32_t *idx, const uint32_t *count, const int32_t *dest,
                   const lsr_mcmc_table *tables, int32_t num_tables, float min_opacity, void *workspace, lsr_stream_t stream);

/* The per-step noise of the published trainer, in place, one launch, no host wait, graph-capturable:
 *   xyz[g] += Sigma_g (eps[g] * f_g),  Sigma = R S S^T R^T,  R from rotation[g] / |rotation[g]| (w, x, y, z),
 *   S = diag(expf(scaling[g])),  f = step_scale / (1 + expf(-100 ((1 - sigmoid(opacity[g])) - 0.995))),
 * step_scale = noise_lr * lr_xyz from the host, eps [n][3] the caller's standard normals.  Where the exponential
 * overflows the factor is 0.  The increment is rounded to float32 and then added (one rounding each); a row whose
 * increment is not finite is left unchanged.
 * LSR_EINVAL: n < 0, n >= 2^28, step_scale not finite.  LSR_ENULL: with n > 0 any NULL pointer. */
int lsr_mcmc_noise(int64_t n, float *xyz, const float *opacity, const float *scaling, const float *rotation,
                   const float *eps, float step_scale, lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_MCMC_H */
