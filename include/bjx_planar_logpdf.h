/* bjx_planar_logpdf.h — the LOG-DENSITY of transformed(N(μ, diag σ²), l_L ∘ … ∘ l_1) at y for a run of PlanarLayers
 * (planar_layer.jl:12-188; src/transformed_distribution.jl:164-169), with every cotangent a maximum-likelihood step needs, in one
 * streaming pass over y plus the reduction stage of bjx_planar_vjp_params.  Companion of bjx_radial_stack_logpdf.h.
 *
 * Evaluating the density and differentiating it solved the inverse run three times (the pre-image; transform again; the input
 * pullback) and ran a forward pullback at x whose in_bar nobody reads.  Everything is resident after ONE inverse sweep: the column
 * holds x = f⁻¹(y), the base density is one more reduction over it, the seed of the cotangent sweep, x̄ = −c·w/σ with w = (x − μ)/σ,
 * is formed in the registers that held x.  Per column
 *     lp = −½‖w‖² − Σ log σ − (d/2)·log 2π + ℓ,   ℓ = logabsdetjac(inverse(l_L ∘ … ∘ l_1), y) = −Σ_l log1p(c_l (1 − t_l²))
 * and (ȳ, w̄, ū, b̄) is what vjp_params(inverse(run), y, x̄, c) returns — the implicit-function rule of find_alpha, with the chain rule
 * through get_u_hat —, μ̄ = Σ c·w/σ, σ̄ = Σ c·(w² − 1)/σ.
 * With ḡ the inverse-pullback cotangent climbing from x̄ (level 0) to ȳ (level L), the FORWARD parameter pullback at x seeded with
 * (−ȳ, −c) has cotangent −ḡ at every level and its per-layer scalar is exactly the inverse sweep's
 *     s̄_l = q/(1 + c_l q)·(−û_lᵀḡ_l + c·2 c_l t/(1 + c_l q)),  q = 1 − t²,
 * so the sweep leaves the (−s̄, t) tables the reduction stage of bjx_planar_vjp_params consumes; that stage is jointly linear in
 * (out_bar, ladj_bar, s̄), it runs on (x, ȳ, c, −s̄) and its three results are negated by one small launch.
 * bjx.h and the other headers are unchanged; the Julia side does not bind this entry.
 *
 * w, u: device T[dim, n_layers], layer k at w + k·dim (layer-major, as for bjx_planar); b: T[n_layers]; layer 0 is the one the
 * FORWARD run applies first.  mu, sigma: device T[dim] or NULL (0 / 1).  y: [dim, batch] column-major, element-aligned.
 * lp_bar: the cotangent c, T[batch] or NULL (= 1).  lp_ps: T[batch] or NULL.  y_bar: [dim, batch] or NULL; it aliases nothing.
 * w_bar, u_bar: T[dim, n_layers], b_bar: T[n_layers] — all three or all three NULL (BJX_ERR_ARG otherwise).
 * mu_bar, sigma_bar: T[dim] or NULL, each.
 *
 * work: caller-owned device scratch of T, needed only when something summed over the batch is asked for (w_bar / u_bar / b_bar,
 * mu_bar or sigma_bar; BJX_ERR_ARG when it is NULL then); NULL otherwise.  Elements of T, in this order, every term rounded up to a
 * multiple of 4 elements (on a 16-byte aligned work every part is 16-byte aligned, as a y_bar of the caller's usually is: the reduction
 * stage chooses its kernel by alignment, so an aligned y_bar and y_bar == NULL give the same bits):
 *     2·n_layers·batch        the (−s̄, t) tables [batch][n_layers]         — with w_bar / u_bar / b_bar
 *     dim·batch               x = f⁻¹(y)                                    — always (when work is needed)
 *     dim·batch               ȳ                                             — with w_bar / u_bar / b_bar and y_bar == NULL
 *     batch                   c = 1                                         — with w_bar / u_bar / b_bar and lp_bar == NULL
 * bjx_planar_logpdf_work_elems() below is that formula.
 *
 * Rules: Float32 and Float64; no floating-point atomics; sums over the batch in Float64, folded in a fixed order (the layers'
 * cotangents by the reduction stage of bjx_planar_vjp_params; μ̄ and σ̄ from (x − μ) directly — not the expanded Σx² form — by one
 * small kernel over the stored x, one Float64 partial set per block in the context's partials, folded by a second small launch);
 * identical calls give identical bits; no host synchronisation.  An empty batch writes zeros to the summed outputs and launches
 * nothing.  dim >= 1, batch >= 0, n_layers >= 1 (BJX_ERR_SHAPE otherwise).  BJX_ERR_UNSUPPORTED, before anything is launched:
 * columns shorter than two 16-byte packs (8 rows Float32, 4 rows Float64) or taller than 8 192 packs, stacks of more than
 * 32 KiB / (16·sizeof(T)) layers or whose û table exceeds the context's 1 MiB scratch, batches of 2^40 columns or more.
 *
 * Bytes per column, DERIVED from the code (s = sizeof(T)): the pass reads dim·s (y) and writes dim·s (ȳ), + dim·s (x) and
 * 2·n_layers·s (tables) with work; the reduction stage reads x, ȳ and the tables once per group of 8 layers; μ̄ / σ̄ read x once more
 * (dim·s + s). */
#ifndef BJX_PLANAR_LOGPDF_H
#define BJX_PLANAR_LOGPDF_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjx_planar_logpdf_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const void* w, const void* u, const void* b, int n_layers,
                                 const void* mu, const void* sigma, const void* y, const void* lp_bar,
                                 void* lp_ps, void* y_bar,
                                 void* w_bar, void* u_bar, void* b_bar, void* mu_bar, void* sigma_bar,
                                 void* work, int64_t dim, int64_t batch);

/* elements of T the call above needs in `work` (0: work may be NULL) */
static inline int64_t bjx_planar_logpdf_work_elems(int n_layers, int64_t dim, int64_t batch, int want_layers, int want_base, int have_y_bar,
                                                   int have_lp_bar) {
  const int64_t tab = (2 * (int64_t)n_layers * batch + 3) / 4 * 4, col = (dim * batch + 3) / 4 * 4, one = (batch + 3) / 4 * 4;
  if (!want_layers && !want_base) return 0;
  return (want_layers ? tab : 0) + col + ((want_layers && !have_y_bar) ? col : 0) + ((want_layers && !have_lp_bar) ? one : 0);
}

#ifdef __cplusplus
}
#endif

#endif /* BJX_PLANAR_LOGPDF_H */
