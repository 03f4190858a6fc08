/*
 * lsr_optim.h — C ABI of the fused Adam step for a trainable 3DGS scene (lsr_scene.h): every per-Gaussian table of
 * every parameter group — parameter, gradient and the two moments — updated in ONE launch, densely or only on the rows
 * a visibility mask names.  Same library (liblsr_hip.so) and conventions as lsr_density.h: device float32 pointers, a
 * stream, asynchronous, negative LSR_E* codes returned before any GPU work, nothing launched when there is nothing to
 * do.  No atomics; every output element has one owner: two calls on the same inputs give the same bits.
 */
#ifndef LSR_OPTIM_H
#define LSR_OPTIM_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_ADAM_MAX_TABLES 24
#define LSR_ADAM_MAX_WIDTH 4096              /* floats per row of a table */
#define LSR_ADAM_MAX_ROWS (1ll << 40)        /* rows of a table */

/* One tensor of the optimizer: [rows][width] float32, row-major without padding, the four arrays of one table of the
 * same shape and not overlapping each other or any array of another table.  The scalars are the table's own (each
 * parameter group has its rate): the host folds the step count into step_size and inv_sqrt_bc2, in double, and passes
 * 1 - beta rounded from double as well.  The kernel does not subtract: 0.999 is 0.99900001287 as a float, and 1.0f minus
 * that differs from 0.001 by 1.3e-5 of itself — the weight torch.optim.Adam gives a new gradient is (float)(1 - 0.999),
 * and moments that are to move between the two optimizers (a state_dict) have to be built with the same weights. */
typedef struct lsr_adam_table {
    float *param;        /* [rows][width], updated in place */
    const float *grad;   /* [rows][width] */
    float *exp_avg;      /* [rows][width], in place */
    float *exp_avg_sq;   /* [rows][width], in place */
    int64_t rows;        /* 0 .. LSR_ADAM_MAX_ROWS; 0: the table is skipped */
    int32_t width;       /* 1 .. LSR_ADAM_MAX_WIDTH */
    int32_t reserved;    /* 0 */
    float beta1, beta2;                         /* in [0, 1) */
    float one_minus_beta1, one_minus_beta2;     /* (float)(1 - beta) of the host's double beta: in [0, 1] */
    float eps;           /* >= 0 */
    float step_size;     /* lr / (1 - beta1^t), or lr without bias correction: computed by the host in double */
    float inv_sqrt_bc2;  /* 1 / sqrt(1 - beta2^t), or 1 */
    float reserved_f;    /* 0 */
} lsr_adam_table;

/* One Adam step over num_tables tables in one launch.  Per element, in float32 and in this order (beta * x + y and
 * sqrtf(v) * inv_sqrt_bc2 + eps are each ONE fused multiply-add, on every path alike; sqrtf and the division are
 * correctly rounded), with (1 - beta) standing for the table's one_minus_beta:
 *     m = beta1 * m + (1 - beta1) * g
 *     v = beta2 * v + (1 - beta2) * g * g
 *     p = p - step_size * m / (sqrtf(v) * inv_sqrt_bc2 + eps)
 * with g, m, v, p the element of grad, exp_avg, exp_avg_sq and param.  This is torch.optim.Adam's step (no weight decay,
 * no amsgrad, not maximize) at step t with step_size = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t).
 *
 * Dense mode, visible == NULL: every row of every table is updated; visible_rows is not read.
 * Sparse mode, visible != NULL: `visible` holds visible_rows bytes, one per row, and every table with rows > 0 must have
 * rows == visible_rows.  Row r of every table is updated when visible[r] != 0; a row with visible[r] == 0 is neither
 * read nor written in any of the four arrays (a NaN there stays where it is and reaches nothing), so its parameter and
 * its moments keep their bits.  The step count is the caller's: the scalars apply to the rows that are updated.
 *
 * Elements are moved 16 bytes per lane where the table's four pointers are 16-byte aligned, and as single floats
 * otherwise and at the table's end; the result does not depend on which.  Nothing is read or written outside
 * [0, rows * width) of an array.
 *
 * LSR_EINVAL, for any table, empty or not: num_tables out of 0 .. LSR_ADAM_MAX_TABLES; rows out of
 * 0 .. LSR_ADAM_MAX_ROWS; width out of 1 .. LSR_ADAM_MAX_WIDTH; reserved or reserved_f not 0; a beta1, beta2,
 * one_minus_beta1, one_minus_beta2, eps, step_size or inv_sqrt_bc2 that is not finite; a beta outside [0, 1); a
 * one_minus_beta outside [0, 1]; eps < 0; in sparse mode visible_rows < 0 or a
 * table with rows > 0 and rows != visible_rows; more than 2^31 - 1 workgroups (4096 elements each) over all tables.
 * LSR_ENULL: tables NULL with num_tables > 0; a NULL param, grad, exp_avg or exp_avg_sq of a table with rows > 0.
 * LSR_EINVAL is reported before LSR_ENULL.  With num_tables == 0 or every table empty nothing is launched and LSR_OK
 * is returned. */
int lsr_adam_step(const lsr_adam_table *tables, int32_t num_tables, const uint8_t *visible, int64_t visible_rows,
                  lsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_OPTIM_H */
