/* bjx_householder.h — companion of bjx.h: a product of Householder reflections with ONE vector set shared by every column, and its
 * parameter pullback summed over the batch.  The per-column sibling is bjx_householder_cols.h.
 *
 * With V = [v_0 ... v_{L-1}] of shape (dim, L):
 *     t_k = 2 / (v_kᵀ v_k)           (read as 0 where v_kᵀ v_k == 0 exactly: that layer is the identity and its cotangent is 0)
 *     z_0 = x,  z_{k+1} = z_k - t_k (v_kᵀ z_k) v_k,  y = z_L
 * The map is orthogonal: logabsdetjac is exactly 0 in both directions, and the inverse is the same step walked k = L-1 ... 0.  The
 * input pullback of one direction is the map of the other direction applied to the output cotangent (no entry of its own).
 * The parameter pullback, with g the cotangent of a step's output, z_k its input, a_n = v_kᵀ z_{k,n} and c_n = v_kᵀ g_n:
 *     S_k = sum_n (a_n g_n + c_n z_{k,n}),   q_k = sum_n a_n c_n,   v_bar_k = -t_k S_k + t_k^2 q_k v_k,   g <- g - t_k c v_k.
 * A NaN in v is not a zero: it reaches every output.  bjx.h itself is unchanged; the Julia side does not bind these entries yet.
 *
 * Layout: element r of layer k is at v[r + k*dim] (dense); in, out, out_bar, in_bar are dense [dim, batch], column-major.
 *
 * Served: 1 <= n_layers <= 64 and dim <= 1 024 (Float32) / 512 (Float64); BJX_ERR_UNSUPPORTED otherwise.  The parameter pullback
 * keeps its sums on chip in Float64, one table [n_layers][dim + 1] per wave of a four-wave block next to the n_layers values t_k:
 * BJX_HOUSEHOLDER_LDS_BYTES(dim, n_layers) must not exceed BJX_HOUSEHOLDER_LDS_BUDGET, or bjx_householder_vjp_params answers
 * BJX_ERR_UNSUPPORTED (dim 64: 31 layers; dim 512: 3; dim 1 024: 1).  dim < 1 and batch < 0 are BJX_ERR_SHAPE; a null required
 * pointer (batch > 0) and a bad dtype are BJX_ERR_ARG.  Every refusal happens before anything is launched.  No host synchronisation
 * and no allocation beyond the context's scratch.  No atomics: the same call returns the same bits.
 *
 * Not here: a diagonal head or a shift on the shared layer (Scale and Shift are stages of their own), a fused log-density pass,
 * columns taller than a lane group holds, the Julia binding. */
#ifndef BJX_HOUSEHOLDER_H
#define BJX_HOUSEHOLDER_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_HOUSEHOLDER_MAX_LAYERS 64
#define BJX_HOUSEHOLDER_LDS_BUDGET 65536
/* bytes of LDS one block of the parameter pullback needs: four Float64 tables [n_layers][dim + 1] and n_layers values t_k */
#define BJX_HOUSEHOLDER_LDS_BYTES(dim, n_layers) ((size_t)8 * (size_t)(n_layers) * (4 * ((size_t)(dim) + 1) + 1))

/* The map (inverse = 0) or its inverse (inverse = 1) on in[dim, batch] -> out[dim, batch] (out == in allowed), one launch.
 * The log-det is exactly 0: ladj_ps (T[batch]) and ladj_sum (one device double), where not NULL, are written as exact zeros, or
 * left as they are under BJX_ACCUMULATE.  batch == 0: nothing is launched (ladj_sum is zeroed without BJX_ACCUMULATE). */
int bjx_householder(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* v, int n_layers, const void* in, void* out, void* ladj_ps,
                    double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call onto v, summed over the batch, in one streaming pass over in and out_bar plus one or two folds (at
 * most three launches).  in = x (inverse = 0) or y (inverse = 1).  ladj_bar is accepted and ignored.  in_bar: [dim, batch] or NULL
 * (in_bar == out_bar allowed).  v_bar: T[dim, n_layers], required.  batch == 0: v_bar is zeroed and nothing is launched. */
int bjx_householder_vjp_params(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* v, int n_layers, const void* in,
                               const void* out_bar, const void* ladj_bar, void* in_bar, void* v_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_HOUSEHOLDER_H */
