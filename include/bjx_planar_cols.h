/* bjx_planar_cols.h — companion of bjx.h: a stack of PlanarLayers with one parameter set (w, u, b) per COLUMN.
 *
 * bjx_planar takes ONE (w, u, b) per layer, shared by the batch.  The flow was introduced amortised (Rezende & Mohamed, 2015):
 * an encoder emits a (w, u, b) for every sample and the flow refines that sample's posterior; conditional density estimators
 * use planar layers the same way.  These two entries take the parameters per column, streamed with the data; the scalar work
 * is the one of bjx_planar (get_u_hat, planar_layer.jl:65-70; the forward step :72-110; find_alpha :112-185).  bjx.h itself
 * is unchanged (its prototypes are pinned by the Julia binding's tests); the Julia side does not bind these entries yet.
 *
 * Layout: element r of layer k in column n of w is at p_w[r + k*dim + n*ld_w], ld_w >= dim*n_layers; u the same with ld_u;
 * b of layer k in column n is at p_b[k + n*ld_b], ld_b >= n_layers.  The three ld's are separate, so three slices of ONE
 * network head [2*dim*L + L, batch] are passed with no copy.
 *
 * Layers apply in the order k = 0 ... L-1; the inverse undoes layer L-1 first.  1 <= n_layers <= 64 and
 * dim <= 1 024 (Float32) / 512 (Float64): BJX_ERR_UNSUPPORTED otherwise.  Column strides below the minimum are
 * BJX_ERR_SHAPE, null pointers BJX_ERR_ARG; every refusal happens before anything is launched.  No host synchronisation and
 * no allocation beyond the context's scratch, so a step that uses them can be captured (run it once outside the capture
 * first).  No atomics: the same call returns the same bits. */
#ifndef BJX_PLANAR_COLS_H
#define BJX_PLANAR_COLS_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_PLANAR_COLS_MAX_LAYERS 64

/* The flow (inverse = 0) or its inverse (inverse = 1) on in[dim, batch] -> out[dim, batch] (out == in allowed).
 * ladj_ps, ladj_sum, flags, batch == 0: as bjx_rqs_cols (BJX_ACCUMULATE honoured; the summed log-det is a deterministic,
 * fixed-order reduction). */
int bjx_planar_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w,
                    int64_t ld_u, int64_t ld_b, int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum,
                    int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call.  in = x (inverse = 0) or y (inverse = 1: implicit function theorem at x = f^-1(y), like
 * bjx_planar_vjp).  in_bar: [dim, batch] (in_bar == out_bar allowed).  ladj_bar: T[batch] or NULL (= 0).
 * inverse = 0: w_bar / u_bar dense [dim, n_layers, batch], b_bar dense [n_layers, batch]: PER-COLUMN cotangents of the
 * parameters, NOT summed over the batch; any of them may be NULL.
 * inverse = 1: in_bar only; a non-NULL w_bar / u_bar / b_bar is BJX_ERR_ARG (the parameter pullback of the inverse is the
 * forward one at x with the cotangents (-in_bar, -ladj_bar)). */
int bjx_planar_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w,
                        int64_t ld_u, int64_t ld_b, int n_layers, const void* in, const void* out_bar, const void* ladj_bar,
                        void* in_bar, void* w_bar, void* u_bar, void* b_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_PLANAR_COLS_H */
