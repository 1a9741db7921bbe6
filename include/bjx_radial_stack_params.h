/* bjx_radial_stack_params.h — companion of bjx_radial_stack.h: the PARAMETER pullback of a run of RadialLayers l_L ∘ … ∘ l_1
 * (radial_layer.jl:43-129) and of its inverse, in one streaming pass over the batch.
 *
 * bjx_radial_vjp_params takes one layer, so training a composition of L radial layers cost L − 1 bjx_radial launches for the layer
 * inputs and L parameter pullbacks with their reductions (about 2L passes over the batch); the inverse direction — maximum
 * likelihood evaluates the flow backwards on the data — three launches per layer more.  Here ONE pass reads x, ȳ and ℓ̄, writes x̄
 * when asked, and leaves every layer's parameter cotangents; one or two small fold launches follow it (at most three launches
 * whatever L is).
 * bjx.h and bjx_radial_stack.h are unchanged; the Julia side does not bind this entry.
 *
 * Table layout, layer order and `inverse` as in bjx_radial_stack_vjp: alpha_, beta: device T[n_layers] (raw, behind softplus);
 * z0: device T[dim, n_layers], layer k at z0 + k·dim; layer 0 is applied first; inverse = 1 is inverse(l_L ∘ … ∘ l_1).
 * in, out_bar: [dim, batch] column-major; ladj_bar: T[batch] or NULL (= 0; the same ℓ̄ goes to every layer).
 * in_bar: [dim, batch] or NULL (x̄ is not written); it may alias out_bar (not in).  Where written it is bjx_radial_stack_vjp's x̄.
 * alpha_bar, beta_bar: T[n_layers]; z0_bar: T[dim, n_layers], layer k at k·dim — the cotangents of the RAW parameters, summed
 * over the batch with the ℓ̄ term included.  inverse = 1: the implicit-function rule per layer (the forward formulas at the layer's
 * pre-image with the cotangents (−ȳ, −ℓ̄)); Newton's root is not differentiated through.
 *
 * The sums are accumulated in Float64 — on chip per block, one [n_layers, dim + 2] Float64 partial per BLOCK in the context's
 * partials — added in a fixed order and cast to T at the very end: no floating-point atomics anywhere, two identical calls give
 * identical bits.  No host synchronisation, no allocation beyond the context's scratch.  An empty batch writes zeros and launches
 * no kernel.
 *
 * Shapes.  dim >= 1, batch >= 0, n_layers >= 1 (BJX_ERR_SHAPE otherwise); Float32 and Float64.  Served: what bjx_radial_stack_vjp
 * serves whose tables AND Float64 accumulators fit 64 KiB of LDS per block — G lanes per column: 4·n_layers·(dim + 2) doubles on
 * top of the pullback's tables; one lane per column (dim <= 32 that is not a whole pack, or Float64): n_layers·(DMAX + 2) + 65·DMAX
 * doubles, DMAX = 8 / 16 / 32.  BJX_ERR_UNSUPPORTED, nothing launched: taller columns and larger stacks; the caller then takes the
 * layers one by one (bjx_radial_vjp_params). */
#ifndef BJX_RADIAL_STACK_PARAMS_H
#define BJX_RADIAL_STACK_PARAMS_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjx_radial_stack_vjp_params(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                                const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* alpha_bar, void* beta_bar,
                                void* z0_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_RADIAL_STACK_PARAMS_H */
