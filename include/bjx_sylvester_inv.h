/* bjx_sylvester_inv.h — companion of bjx_sylvester.h: the INVERSE of the shared Sylvester layer and the inverse's input pullback.
 *
 * Served only where the caller declares Q'Q = I and R_mm R~_mm > -1 for every unit (the paper's invertibility condition, the planar
 * flow's w'u^ > -1).  With Q'Q = I the layer y = z + Q triu(R) tanh(triu(R~) Q'z + b) reduces to M scalar monotone equations, solved
 * from the last unit to the first.  U = triu(R), U~ = triu(R~), k_m = R_mm R~_mm; per column y:
 *     s' = Q' y                                              (M)
 *     for m = M-1 ... 0:
 *         c_m   = b_m + sum_{j>m} U~_mj s_j
 *         rho_m = s'_m - sum_{j>m} U_mj a_j
 *         alpha + k_m tanh(alpha + c_m) = R~_mm rho_m        (the planar flow's root solve: three Newton steps from a fixed-point
 *                                                             start and an acceptance test, a bounded safeguarded loop otherwise)
 *         a_m   = tanh(alpha + c_m)
 *         s_m   = rho_m - R_mm a_m                           (no division: R~_mm = 0 and R_mm = 0 need no special case)
 *     z = y - Q (s' - s)
 *     d_m = 1 + (1 - a_m^2) k_m
 *     logabsdetjac = -sum_m log|d_m|                         (of the inverse: minus the layer's own at z)
 * The pullback of (z_bar, l_bar) on (z, logabsdetjac), hp = 1 - a^2:
 *     e = -2 a hp k / d;   eta = Q' z_bar - l_bar U~' e
 *     for m = 0 ... M-1:
 *         sigma_m = sum_{j<m} U_jm pi_j
 *         pi_m    = (eta_m - U~_mm hp_m sigma_m - sum_{i<m} U~_im tau_i) / d_m
 *         tau_m   = hp_m (U_mm pi_m + sigma_m)
 *     y_bar = z_bar - Q U~' (l_bar e + tau)
 * O(M^2) per column, two passes over Q, no M^3 product.  The strict lower triangles of R and R~ are never read.
 *
 * The parameter pullback of the inverse has no entry of its own: by the implicit-function rule it is MINUS the layer's parameter
 * pullback (bjx_sylvester_vjp_params) at z = `pre` with the cotangents (y_bar, l_bar).
 *
 * R_mm R~_mm <= -1 is not refused (no entry reads parameter values on the host): the root solve then returns some root inside the
 * reference's bracket after a bounded number of steps and the values are unspecified.  Where Q'Q differs from I the results are not the
 * inverse of the layer.  log|d|, not log d, as in bjx_sylvester.h.
 *
 * Layouts, limits (1 <= M <= BJX_SYLVESTER_MAX_UNITS, M <= dim, dim <= 1 024 Float32 / 512 Float64) and refusal codes are those of
 * bjx_sylvester.h; there is no LDS rule (no tables are kept).  Every refusal happens before anything is launched.  No host
 * synchronisation, no allocation beyond the context's partials, no atomics: the same call returns the same bits, and the bits depend
 * neither on the form (vector or element) the dispatcher chose nor on the outputs asked for.
 *
 * Not here: the inverse of the per-column layer (bjx_sylvester_cols.h), a fused log-density pass, the orthogonalisation of Q, the
 * Julia binding. */
#ifndef BJX_SYLVESTER_INV_H
#define BJX_SYLVESTER_INV_H

#include "bjx_sylvester.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The inverse on in[dim, batch] = y -> out[dim, batch] = z (out == in allowed), one launch.  ladj_ps (T[batch]), ladj_sum (one device
 * double), flags: as bjx_sylvester (BJX_ACCUMULATE honoured; the summed log-det is a fixed-order reduction of per-block partials, one
 * more launch).  batch == 0: nothing is launched (ladj_sum is zeroed without BJX_ACCUMULATE). */
int bjx_sylvester_inv(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M, const void* in,
                      void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call at in = y, one launch.  out_bar: z_bar [dim, batch].  ladj_bar: T[batch] or NULL (= 0).  in_bar: y_bar
 * [dim, batch] or NULL (in_bar == out_bar allowed).  pre: [dim, batch] or NULL; where given it receives z with the bits of
 * bjx_sylvester_inv (it must not overlap the other buffers).  in_bar has the same bits with and without pre.  batch == 0, or in_bar and
 * pre both NULL: nothing is launched. */
int bjx_sylvester_inv_vjp(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M,
                          const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* pre, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_SYLVESTER_INV_H */
