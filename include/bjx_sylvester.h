/* bjx_sylvester.h — companion of bjx.h: one Sylvester layer with ONE parameter set (Q, R, R~, b) shared by every column, and its
 * parameter pullback summed over the batch.  The per-column sibling is bjx_sylvester_cols.h.
 *
 * The Sylvester flow (van den Berg, Hasenclever, Tomczak & Welling, 2018) as it is trained outside a VAE and as it sits between
 * coupling layers.  With triu(.) the upper triangle, diagonal included, per column z:
 *     s = Q' z                       (M)
 *     t = triu(R~) s + b             (M)
 *     a = tanh(t)
 *     p = triu(R) a                  (M)
 *     y = z + Q p
 *     d_m = 1 + (1 - a_m^2) R~_mm R_mm
 *     logabsdetjac = sum_m log|d_m|
 * The pullback of (y_bar, l_bar) per column, hp = 1 - a^2:
 *     p_bar = Q' y_bar;  a_bar = triu(R)' p_bar;  t_bar = a_bar*hp - l_bar*2a*hp*diag(R~)*diag(R)/d;  s_bar = triu(R~)' t_bar;
 *     z_bar = y_bar + Q s_bar
 * and the parameter cotangents SUMMED over the batch:
 *     Q_bar  = sum_n y_bar p' + z s_bar'
 *     R_bar  = sum_n triu(p_bar a') + diag(l_bar*hp*diag(R~)/d)
 *     R~_bar = sum_n triu(t_bar s') + diag(l_bar*hp*diag(R)/d)
 *     b_bar  = sum_n t_bar
 * The strict lower triangles of R and R~ are never read (a NaN there changes nothing); those of R_bar and R~_bar are written as exact
 * zeros.  The log-det is the Jacobian's only when Q'Q = I: that is the caller's job; the entries evaluate the forms above for any Q
 * and the pullback is the pullback of those forms with Q a free parameter.  log|d|, not log d: R_mm R~_mm < -1 is not refused.
 * bjx.h itself is unchanged; the Julia side does not bind these entries yet.
 *
 * Layout, all dense: Q[r, m] at q[r + m*dim], R[i, j] at r[i + j*M], R~ the same, b[m] at b[m]; the cotangents use the same layout;
 * in, out, out_bar, in_bar are dense [dim, batch], column-major.
 *
 * 1 <= M <= BJX_SYLVESTER_MAX_UNITS, M <= dim and dim <= 1 024 (Float32) / 512 (Float64): BJX_ERR_UNSUPPORTED otherwise.  The
 * parameter pullback keeps its sums on chip in Float64, one table of dim*M + 2*M*M + M entries per wave of a four-wave block (R, R~
 * and b reach the kernels through uniform loads and take no LDS): BJX_SYLVESTER_LDS_BYTES(dim, M) must not exceed
 * BJX_SYLVESTER_LDS_BUDGET, or bjx_sylvester_vjp_params with parameter cotangents answers BJX_ERR_UNSUPPORTED (dim 64: M <= 16;
 * 128: 13; 256: 7; 512: 3; 1 024: 1).  dim < 1 and batch < 0 are BJX_ERR_SHAPE; a null required pointer (batch > 0), a bad dtype
 * and a mixture of null and non-null parameter cotangents are BJX_ERR_ARG.  Every refusal happens before anything is launched.
 * No host synchronisation and no allocation beyond the context's partials.  No atomics: the same call returns the same bits.
 *
 * Not here: the inverse map (bjx_sylvester_inv.h, for Q'Q = I), the fused parameter pullback of shapes over the LDS rule, a fused log-density pass, the
 * orthogonalisation of Q, columns taller than a lane group holds, the Julia binding. */
#ifndef BJX_SYLVESTER_H
#define BJX_SYLVESTER_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_SYLVESTER_MAX_UNITS 16
#define BJX_SYLVESTER_LDS_BUDGET 65536
/* bytes of LDS one block of the parameter pullback needs: four Float64 tables of dim*M + 2*M*M + M entries (nothing else is staged) */
#define BJX_SYLVESTER_LDS_BYTES(dim, M) ((size_t)32 * ((size_t)(dim) * (size_t)(M) + 2 * (size_t)(M) * (size_t)(M) + (size_t)(M)))

/* The layer on in[dim, batch] -> out[dim, batch] (out == in allowed), one launch.  ladj_ps (T[batch]), ladj_sum (one device double),
 * flags: as bjx_sylvester_cols (BJX_ACCUMULATE honoured; the summed log-det is a fixed-order reduction of per-block partials, one
 * more launch).  batch == 0: nothing is launched (ladj_sum is zeroed without BJX_ACCUMULATE). */
int bjx_sylvester(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M, const void* in,
                  void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call at in = z.  ladj_bar: T[batch] or NULL (= 0).  in_bar: [dim, batch] or NULL (in_bar == out_bar allowed).
 * q_bar T[dim, M], r_bar and rt_bar T[M, M], b_bar T[M]: summed over the batch, given all together or all NULL.  All NULL: the plain
 * input pullback, one launch, no LDS tables, not subject to the LDS rule.  Otherwise one streaming pass over in and out_bar plus one
 * or two folds (at most three launches); in_bar has the same bits either way.  batch == 0: the cotangents are zeroed and nothing is
 * launched. */
int bjx_sylvester_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M,
                             const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* q_bar, void* r_bar,
                             void* rt_bar, void* b_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_SYLVESTER_H */
