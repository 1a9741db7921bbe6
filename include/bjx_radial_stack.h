/* bjx_radial_stack.h — companion of bjx.h: a RUN of RadialLayers l_L ∘ … ∘ l_1 (radial_layer.jl:43-129, composed the way
 * docs/src/flows.md:115 writes a flow) in ONE launch: map, inverse and input pullback.
 *
 * bjx_radial takes one layer, so a composition of L radial layers is L launches and L read-and-write passes over the batch.
 * Here the column stays in registers and the layer loop runs on it: one read and one write whatever L is.  The per-layer
 * arithmetic is the single-layer kernels', in the same operation order (r = ‖z − z₀‖ from the differences, no Gram-matrix
 * shortcut), so a stack of one is bjx_radial's result.
 * bjx.h itself is unchanged (its prototypes are pinned by the Julia binding's tests); the Julia side does not bind these entries.
 *
 * alpha_, beta: device T[n_layers] (the raw parameters behind softplus); z0: device T[dim, n_layers], layer k at z0 + k·dim.
 * Layer 0 is applied first.  inverse = 1 is inverse(l_L ∘ … ∘ l_1): the last layer's inverse first, with the log-det of the
 * inverse map.
 * in, out: [dim, batch] column-major; out may alias in.  ladj_ps (T[batch] or NULL), ladj_sum (device double or NULL) and
 * BJX_ACCUMULATE as in bjx_radial; the sum is a fixed-order reduction of per-block partials (no floating-point atomics: two
 * identical calls give identical bits).  An empty batch launches nothing (ladj_sum is zeroed unless BJX_ACCUMULATE).
 * bjx_radial_stack_vjp: out_bar [dim, batch], ladj_bar T[batch] or NULL (= 0; the same ℓ̄ goes to every layer), in_bar
 * [dim, batch]; in_bar may alias out_bar (not in).  One pass: the primal sweep keeps one or two scalars per layer and column, the
 * reverse sweep rewinds the resident column with them.
 * No host synchronisation, no allocation beyond the context's scratch.
 *
 * Shapes.  dim >= 1, batch >= 0, n_layers >= 1 (BJX_ERR_SHAPE otherwise); Float32 and Float64.  Served: the columns the
 * register kernels of bjx_radial hold — up to 64 lanes x 8 sixteen-byte packs (2 048 rows Float32, 1 024 Float64), G lanes
 * per column; and columns of at most 32 rows that are not whole packs, or Float64, one lane per column.
 * BJX_ERR_UNSUPPORTED, nothing launched: taller columns (bjx_radial's block-per-column kernels are not fused), and stacks
 * whose tables — z0 [dim, n_layers], 2·n_layers scalars, the pullback's per-layer scalars — exceed 64 KiB of LDS per block.
 * The caller then applies the layers one by one. */
#ifndef BJX_RADIAL_STACK_H
#define BJX_RADIAL_STACK_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjx_radial_stack(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                     const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags);
int bjx_radial_stack_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                         const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_RADIAL_STACK_H */
