/* bjx_radial_stack_logpdf.h — companion of bjx_radial_stack_params.h: the LOG-DENSITY of transformed(N(μ, diag σ²), l_L ∘ … ∘ l_1) at y
 * for a run of RadialLayers (radial_layer.jl:43-129; src/transformed_distribution.jl:164-169), with every cotangent a maximum-
 * likelihood step needs, in one streaming pass over y.
 *
 * Evaluating the density and differentiating it took the inverse run three times (logpdf; the pre-image again for the seed; the
 * parameter pullback, which re-runs the sweep) and read or wrote five to six arrays of the batch's size.  Everything is resident
 * after ONE inverse sweep: the column holds x = f⁻¹(y), the base density is one more reduction over it, and the seed of the reverse
 * sweep, x̄ = −c·w/σ with w = (x − μ)/σ, is generated in registers.  Per column
 *     lp = −½‖w‖² − Σ log σ − (d/2)·log 2π + ℓ,   ℓ = logabsdetjac(inverse(l_L ∘ … ∘ l_1), y)
 * and (ȳ, ᾱ_, β̄, z̄₀) is the pullback of with_logabsdet_jacobian(inverse run, ·) at y with the cotangents (x̄, c) — what
 * bjx_radial_stack_vjp_params(inverse = 1) returns for them —, μ̄ = Σ c·w/σ, σ̄ = Σ c·(w² − 1)/σ.
 * bjx.h and the other headers are unchanged; the Julia side does not bind this entry.
 *
 * Table layout and layer order as in bjx_radial_stack_vjp_params with inverse = 1 (the entry is always the inverse run): alpha_,
 * beta: device T[n_layers] (raw, behind softplus); z0: device T[dim, n_layers], layer k at z0 + k·dim; layer 0 is the one the
 * FORWARD run applies first.
 * mu, sigma: device T[dim] or NULL (0 / 1).  y: [dim, batch] column-major.  lp_bar: the cotangent c, T[batch] or NULL (= 1).
 * lp_ps: T[batch] or NULL.  lp_sum: device double, Σ lp over the batch (unweighted), or NULL.
 * y_bar: [dim, batch] or NULL (not written); it aliases nothing.
 * alpha_bar, beta_bar: T[n_layers], z0_bar: T[dim, n_layers] — or all three NULL.  mu_bar, sigma_bar: T[dim] or NULL, each.
 *
 * The rules of bjx_radial_stack_vjp_params hold: Float32 and Float64; sums in Float64 on chip per block, one partial per BLOCK in
 * the context's partials — [n_layers, dim + 2 | Σ lp | μ̄ (dim) | σ̄ (dim)], the last two rows only when mu_bar or sigma_bar is
 * asked for —, one or two fold launches in a fixed order (at most three launches whatever n_layers is; one when nothing summed over
 * the batch is asked for), no floating-point atomics, identical bits from identical calls, no host synchronisation, nothing
 * allocated beyond the context's partials.  An empty batch writes zeros and launches no kernel.
 *
 * Shapes.  dim >= 1, batch >= 0, n_layers >= 1 (BJX_ERR_SHAPE otherwise).  BJX_ERR_UNSUPPORTED, nothing launched: columns taller
 * than the register kernels hold, and stacks whose tables exceed 64 KiB of LDS per block.  LDS per block, DERIVED from the layout
 * (not measured), with s = sizeof(T), P = n_layers·(dim + 2) + 1 (+ 2·dim with the base rows) doubles per table, each term rounded
 * up to 16 bytes:
 *   G lanes per column     2·n_layers·s + n_layers·dim·s + 2·dim·s + (256/G)·UC·2·n_layers·s + 4·P·8
 *                          (the pullback's formula plus the μ | σ rows, 2·dim·s, and 4·(1 + 2·dim)·8 for the wider tables)
 *   one lane per column    (n_layers·(DMAX + 2) + 1 + 2·DMAX + 65·DMAX)·8 + (64·(dim | 1) + n_layers·(DMAX + 4) + 2·DMAX
 *                          + 64·((2·n_layers) | 1))·s, DMAX = 8 / 16 / 32 (one column tile: there is no out_bar tile)
 * Bytes per column, DERIVED: dim·s read (y), + s with lp_bar, + s with lp_ps, + dim·s with y_bar — against 5 to 6 arrays of dim·s
 * for the four calls it replaces. */
#ifndef BJX_RADIAL_STACK_LOGPDF_H
#define BJX_RADIAL_STACK_LOGPDF_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjx_radial_stack_logpdf_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const void* alpha_, const void* beta, const void* z0, int n_layers,
                                       const void* mu, const void* sigma, const void* y, const void* lp_bar, void* lp_ps, double* lp_sum,
                                       void* y_bar, void* alpha_bar, void* beta_bar, void* z0_bar, void* mu_bar, void* sigma_bar,
                                       int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_RADIAL_STACK_LOGPDF_H */
