/* bjx_sylvester_cols.h — companion of bjx.h: one Sylvester layer with its parameters per COLUMN.
 *
 * The amortised Sylvester flow (van den Berg, Hasenclever, Tomczak & Welling, 2018): the planar map widened to a bottleneck of M
 * hidden units, with an encoder that emits (Q, R, R~, b) for every sample.  Per column, with triu(.) the upper triangle, diagonal
 * included:
 *     s = Q' z                       (M)
 *     t = triu(R~) s + b             (M)
 *     a = tanh(t)
 *     p = triu(R) a                  (M)
 *     y = z + Q p
 *     d_m = 1 + (1 - a_m^2) R~_mm R_mm
 *     logabsdetjac = sum_m log|d_m|
 * The strict lower triangles of R and R~ are never read (a NaN there changes nothing).  The log-det is the Jacobian's only when
 * Q'Q = I: that is the caller's job (Q comes out of an orthogonalisation upstream); the entries evaluate the forms above for any Q
 * and the pullback is the pullback of those forms with Q a free parameter.  log|d|, not log d: R_mm R~_mm < -1 is not refused.
 * bjx.h itself is unchanged; the Julia side does not bind these entries yet.
 *
 * Layout: Q[r, m] of column n is at p_q[r + m*dim + n*ld_q], ld_q >= dim*M; R[i, j] at p_r[i + j*M + n*ld_r], ld_r >= M*M, R~ the
 * same with ld_rt; b[m] at p_b[m + n*ld_b], ld_b >= M.  The four ld's are separate, so four slices of ONE network head
 * [dim*M + 2*M*M + M, batch] are passed with no copy.
 *
 * 1 <= M <= BJX_SYLVESTER_COLS_MAX_UNITS, M <= dim and dim <= 1 024 (Float32) / 512 (Float64): BJX_ERR_UNSUPPORTED otherwise.
 * Column strides below the minimum, dim < 1 and batch < 0 are BJX_ERR_SHAPE, null required pointers (batch > 0) and a bad dtype
 * BJX_ERR_ARG; every refusal happens before anything is launched.  No host synchronisation and no allocation beyond the context's
 * scratch.  No atomics: the same call returns the same bits.
 *
 * Not here: the inverse map (M scalar monotone equations solved by back-substitution), a shared-parameter Sylvester
 * layer, a fused log-density pass, the orthogonalisation of Q, columns taller than a lane group holds, the Julia binding. */
#ifndef BJX_SYLVESTER_COLS_H
#define BJX_SYLVESTER_COLS_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_SYLVESTER_COLS_MAX_UNITS 16

/* The layer on in[dim, batch] -> out[dim, batch] (out == in allowed).  ladj_ps, ladj_sum, flags, batch == 0: as
 * bjx_householder_cols (BJX_ACCUMULATE honoured; the summed log-det is a deterministic, fixed-order reduction). */
int bjx_sylvester_cols(bjx_ctx* ctx, bjx_dtype dt, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q,
                       int64_t ld_r, int64_t ld_rt, int64_t ld_b, int M, const void* in, void* out, void* ladj_ps, double* ladj_sum,
                       int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call at in = z.  in_bar: [dim, batch] (in_bar == out_bar allowed).  ladj_bar: T[batch] or NULL (= 0).
 * q_bar dense [dim, M, batch], r_bar and rt_bar dense [M, M, batch] (their strict lower triangles written as exact zeros), b_bar
 * dense [M, batch]: PER-COLUMN cotangents, NOT summed over the batch; any of them may be NULL. */
int bjx_sylvester_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q,
                           int64_t ld_r, int64_t ld_rt, int64_t ld_b, int M, const void* in, const void* out_bar, const void* ladj_bar,
                           void* in_bar, void* q_bar, void* r_bar, void* rt_bar, void* b_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_SYLVESTER_COLS_H */
