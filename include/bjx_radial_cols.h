/* bjx_radial_cols.h — companion of bjx.h: a stack of RadialLayers with one parameter set (α_, β, z₀) per COLUMN.
 *
 * bjx_radial (and the fused runs of bjx_radial_stack.h) take ONE (α_, β, z₀) per layer, shared by the batch.  The radial flow was
 * introduced amortised next to the planar one (Rezende & Mohamed, 2015): an encoder emits (α_, β, z₀) for every sample.  These
 * two entries take the parameters per column, streamed with the data; the scalar work is the one of bjx_radial
 * (radial_layer.jl:43-70; the closed-form inverse compute_r :124-129).  bjx.h itself is unchanged (its prototypes are pinned by
 * the Julia binding's tests); the Julia side does not bind these entries yet.
 *
 * Layout: element r of z₀ of layer k in column n is at p_z0[r + k*dim + n*ld_z], ld_z >= dim*n_layers; the RAW scalars (behind
 * the softplus) of layer k in column n are at p_alpha[k + n*ld_a] and p_beta[k + n*ld_b], ld_a, ld_b >= n_layers.  The three ld's
 * are separate, so three slices of ONE network head [dim*L + 2L, batch] are passed with no copy.
 *
 * Layers apply in the order k = 0 ... L-1; the inverse undoes layer L-1 first.  1 <= n_layers <= 64 and
 * dim <= 1 024 (Float32) / 512 (Float64): BJX_ERR_UNSUPPORTED otherwise.  Column strides below the minimum, dim < 1 and
 * batch < 0 are BJX_ERR_SHAPE, null pointers (batch > 0) and a bad dtype BJX_ERR_ARG; every refusal happens before anything is
 * launched.  No host synchronisation and no allocation beyond the context's scratch, so a step that uses them can be captured
 * (run it once outside the capture first).  No atomics: the same call returns the same bits. */
#ifndef BJX_RADIAL_COLS_H
#define BJX_RADIAL_COLS_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_RADIAL_COLS_MAX_LAYERS 64

/* The flow (inverse = 0) or its inverse (inverse = 1) on in[dim, batch] -> out[dim, batch] (out == in allowed).
 * ladj_ps, ladj_sum, flags, batch == 0: as bjx_planar_cols (BJX_ACCUMULATE honoured; the summed log-det is a deterministic,
 * fixed-order reduction). */
int bjx_radial_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a,
                    int64_t ld_b, int64_t ld_z, int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum,
                    int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call.  in = x (inverse = 0) or y (inverse = 1).  in_bar: [dim, batch] (in_bar == out_bar allowed).
 * ladj_bar: T[batch] or NULL (= 0).  alpha_bar, beta_bar dense [n_layers, batch], z0_bar dense [dim, n_layers, batch]:
 * PER-COLUMN cotangents of the raw parameters, NOT summed over the batch; any of them may be NULL.
 * inverse = 1: they are the cotangents of the inverse map y -> x and its log-det -l(x), in the same launch (the inverse is
 * closed form: the layers are re-applied forwards from the pre-image while the cotangent walks up). */
int bjx_radial_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a,
                        int64_t ld_b, int64_t ld_z, int n_layers, const void* in, const void* out_bar, const void* ladj_bar,
                        void* in_bar, void* alpha_bar, void* beta_bar, void* z0_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_RADIAL_COLS_H */
