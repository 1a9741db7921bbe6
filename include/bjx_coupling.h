/* bjx_coupling.h — companion of bjx.h: Coupling(θ, mask) with a per-sample ELEMENTWISE-CHAIN law.
 *
 * Coupling(θ, mask) (coupling.jl:178-181, 206-259) applies whatever bijector θ(x₂) returns to x₁.  bjx_coupling_affine /
 * bjx_coupling_rqs / bjx_rqs_cols serve Shift, Scale, Shift ∘ Scale and the spline; these two entries serve every law that
 * is a short chain of the elementwise ops of bjx_chain whose parameters come from the conditioner, one set per sample:
 * exp ∘ Shift(t) ∘ Scale(s), inverse(Logit(a, b)) ∘ Shift(t) ∘ Scale(s), LeakyReLU(α) ∘ Shift(t) ∘ Scale(s), ...
 * bjx.h itself is unchanged (its prototypes are pinned by the Julia binding's tests); the Julia side does not bind these
 * entries.
 *
 * The law.  ops[0 .. n_ops-1] in application order, 1 <= n_ops <= BJX_COUPLING_MAX_OPS (the fused limit of the segment
 * kernels, BJX_MAX_SEG_OPS).  ops[k].kind is a bjx_op_kind — BJX_OP_IDENTITY, EXP, LOG, SHIFT, SCALE, SCALE_INV, LOGIT,
 * LOGIT_INV, LEAKY_RELU, SIGNFLIP — or BJX_OP_AFFINE of this header: Shift(p1) ∘ Scale(p0), y = p1 + p0·x with log-det
 * log|p0|, ONE stage (a Scale directly followed by a Shift is what a conditioner almost always emits; as one stage the
 * five-bijector law Shift ∘ Scale ∘ LeakyReLU ∘ Shift ∘ Scale is three stages).  BJX_OP_TRUNCATED / BJX_OP_TRUNCATED_INV are
 * NOT served (their finite/infinite-bound branches are not in the shared link arithmetic): BJX_ERR_UNSUPPORTED, like
 * BJX_OP_STDNORMAL_LOGPDF and n_ops > 4.  Nothing is launched on an error.
 *
 * Where a parameter comes from.  Stage k has the parameter slots 2k (p0: a | a | alpha | scale) and 2k+1 (p1: b of Logit,
 * shift of AFFINE); `params` and `ld_params` are arrays of 2·n_ops entries (either array may be NULL: all-NULL / all-0):
 *     params[i] == NULL                      the host scalar ops[k].p0 / ops[k].p1
 *     params[i] != NULL, ld_params[i] == 0   device T[n1], one value per x₁-row, broadcast over the columns in the kernel
 *     params[i] != NULL, ld_params[i] >= n1  device T[n1, batch], column-major: row r of column n at params[i][r + n·ld]
 *                                            (its own leading dimension: slices of one network head are passed with no copy)
 * 0 < ld < n1 is BJX_ERR_SHAPE.  The fields param_len, v0, v1 of bjx_op are not read by these entries.  The slots of a
 * stage without that parameter (exp, log, SignFlip, identity; p1 of everything but Logit and AFFINE) are ignored.
 *
 * idx1: int32[n1] transformed rows (0-based); rows outside idx1: out = in, in_bar = out_bar (their own dependence on θ
 * stays with the host's AD).  inverse = 1 evaluates the INVERSE law at the same parameters: the stages inverted, last
 * first (coupling.jl:236-250), log-det of the inverse map.  ladj_ps (T[batch]) and ladj_sum (one double, fixed-order
 * deterministic reduction, no floating-point atomics) may each be NULL; BJX_ACCUMULATE adds into both; out may alias in;
 * an empty batch writes 0 to ladj_sum (unless accumulating) and launches nothing.  Float32 and Float64.  No host
 * synchronisation and no allocation beyond the context's scratch. */
#ifndef BJX_COUPLING_H
#define BJX_COUPLING_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_COUPLING_MAX_OPS 4
enum { BJX_OP_AFFINE = 32 }; /* Shift(p1) ∘ Scale(p0) as one stage (this header's entries only) */

int bjx_coupling_chain(bjx_ctx* ctx, bjx_dtype dt, int inverse, const int32_t* idx1, int64_t n1, const bjx_op* ops,
                       int n_ops, const void* const* params, const int64_t* ld_params, const void* in, void* out,
                       void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags);

/* Pullback of the same call, one pass.  in = x (inverse=0) or y (inverse=1: the pre-image x₁ = law⁻¹(y₁) is recomputed
 * and the implicit-function rule applied, as bjx_coupling_affine_vjp does).  out_bar, in_bar: [dim, batch] (in_bar may
 * alias out_bar); ladj_bar: T[batch] or NULL (= 0).
 * params_bar: NULL, or 2·n_ops pointers; params_bar[i] is NULL or receives the PER-COLUMN cotangent of parameter slot i,
 * dense T[n1, batch] (leading dimension n1), NOT summed over the batch.  Only a per-sample parameter (ld_params[i] >= n1)
 * has such a cotangent: a non-NULL params_bar[i] for a host-scalar or per-row slot, or for a slot its stage does not
 * have, is BJX_ERR_ARG — those cotangents are sums over the batch and are not produced here. */
int bjx_coupling_chain_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const int32_t* idx1, int64_t n1, const bjx_op* ops,
                           int n_ops, const void* const* params, const int64_t* ld_params, const void* in,
                           const void* out_bar, const void* ladj_bar, void* in_bar, void* const* params_bar,
                           int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_COUPLING_H */
