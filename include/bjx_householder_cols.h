/* bjx_householder_cols.h — companion of bjx.h: a product of Householder reflections with one vector set per COLUMN, behind an
 * optional per-column diagonal scale and in front of an optional per-column shift.
 *
 * The amortised Householder flow (Tomczak & Welling, 2016): an encoder emits, for every sample, L reflection vectors v_k and —
 * each optional — a log-scale s and a shift m, and the posterior is N(m, U diag(exp(2s)) Uᵀ) with U = H_{L-1} ... H_0.  Per column:
 *     u = exp(s) .* x            (s absent: u = x)
 *     z_0 = u,  z_{k+1} = z_k - t_k (v_kᵀ z_k) v_k,  t_k = 2 / (v_kᵀ v_k)
 *     y = z_L + m                (m absent: y = z_L)
 *     logabsdetjac = sum(s)      (0 without s)
 * The inverse is x = exp(-s) .* H_0 H_1 ... H_{L-1} (y - m) with the log-det -sum(s): every reflection is its own inverse, so the
 * same step is walked in the other order.  Where v_kᵀv_k == 0 exactly, t_k is read as 0: the layer is the identity and its
 * cotangent is 0 (the sibling of "1/r read as 0 at r = 0" of the radial entries).  A NaN in v is not such a zero: it reaches the
 * output of its column.  bjx.h itself is unchanged; the Julia side does not bind these entries yet.
 *
 * Layout: element r of v of layer k in column n is at p_v[r + k*dim + n*ld_v], ld_v >= dim*n_layers; p_s[r + n*ld_s] and
 * p_m[r + n*ld_m], each ld >= dim.  The three ld's are separate, so three slices of ONE network head [dim*L + 2*dim, batch] are
 * passed with no copy.  p_s or p_m may be NULL: the parameter is absent and its ld is ignored.
 *
 * 1 <= n_layers <= 64 and dim <= 1 024 (Float32) / 512 (Float64): BJX_ERR_UNSUPPORTED otherwise.  Column strides below the
 * minimum, dim < 1 and batch < 0 are BJX_ERR_SHAPE, null required pointers (batch > 0), a cotangent output of an absent parameter
 * and a bad dtype BJX_ERR_ARG; every refusal happens before anything is launched.  No host synchronisation and no allocation
 * beyond the context's scratch.  No atomics: the same call returns the same bits.
 *
 * Not here: n_layers = 0 (a pure amortised diagonal affine), a shared-parameter Householder layer with batch-summed cotangents,
 * a fused log-density pass, columns taller than a lane group holds, the Julia binding. */
#ifndef BJX_HOUSEHOLDER_COLS_H
#define BJX_HOUSEHOLDER_COLS_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_HOUSEHOLDER_COLS_MAX_LAYERS 64

/* The flow (inverse = 0) or its inverse (inverse = 1) on in[dim, batch] -> out[dim, batch] (out == in allowed).
 * ladj_ps, ladj_sum, flags, batch == 0: as bjx_radial_cols (BJX_ACCUMULATE honoured; the summed log-det is a deterministic,
 * fixed-order reduction).  Without p_s the log-det outputs are written as exact zeros (or left as they are under
 * BJX_ACCUMULATE). */
int bjx_householder_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v,
                         int64_t ld_s, int64_t ld_m, int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum,
                         int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call.  in = x (inverse = 0) or y (inverse = 1).  in_bar: [dim, batch] (in_bar == out_bar allowed).
 * ladj_bar: T[batch] or NULL (= 0).  v_bar dense [dim, n_layers, batch], s_bar and m_bar dense [dim, batch]: PER-COLUMN
 * cotangents, NOT summed over the batch; any of them may be NULL; s_bar (m_bar) with p_s (p_m) absent is BJX_ERR_ARG.
 * inverse = 1: they are the cotangents of the inverse map y -> x and its log-det -sum(s), in the same launch. */
int bjx_householder_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v,
                             int64_t ld_s, int64_t ld_m, int n_layers, const void* in, const void* out_bar, const void* ladj_bar,
                             void* in_bar, void* v_bar, void* s_bar, void* m_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_HOUSEHOLDER_COLS_H */
