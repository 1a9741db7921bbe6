/* bjx_chain_vjp.h — companion of bjx.h: ONE-PASS PARAMETER PULLBACK of an elementwise chain whose parameters are shared by
 * the whole batch (the chains of bjx_chain: a host scalar, a device scalar or one value per row).
 *
 * Training a flow or running ADVI asks, at every step, for the cotangents of the chain's parameters
 *     p̄ = Σ_n [ ȳ_n · ∂y_n/∂p + ℓ̄_n · ∂ logabsdetjac_n/∂p ]                      (summed over the batch, the ℓ̄ term included)
 * next to the input cotangent x̄.  bjx_stacked_vjp_moments serves one head (tail ∘ Shift ∘ Scale) and leaves the arithmetic on its
 * two row moments to the host; bjx_coupling_chain_vjp has the closed forms of every stage parameter but only per column.  This
 * entry is the batch-summed form: one streaming pass over x, ȳ, ℓ̄ (every stage's input stays in registers), Float64 row sums
 * per block, one fixed-order fold launch whose epilogue sums a scalar parameter's rows and casts to T.  No floating-point atomics,
 * no host synchronisation, no allocation beyond the context's scratch; two identical calls give identical bits.
 * bjx.h itself is unchanged (its prototypes are pinned by the Julia binding's tests); the Julia side does not bind these entries.
 *
 * ops[0 .. n_ops-1]: as in bjx_chain — application order; param_len 0 (no parameter), 1 (scalar) or dim (one value per row);
 * v0 / v1 device T[param_len], or NULL for the host scalar p0 / p1 (next to a per-row parameter of a two-parameter stage the
 * other one may be a host scalar: a NULL v1 is p1, a NULL v0 is p0; with param_len == dim > 1 at least one pointer is set).
 * Kinds served: BJX_OP_IDENTITY, EXP, LOG, SHIFT, SCALE, SCALE_INV, LOGIT, LOGIT_INV, LEAKY_RELU, SIGNFLIP.
 * BJX_OP_TRUNCATED / TRUNCATED_INV / STDNORMAL_LOGPDF and n_ops > BJX_CHAIN_VJP_MAX_OPS: BJX_ERR_UNSUPPORTED.  Nothing is launched
 * on an error.
 *
 * x, y_bar: [dim, batch] column-major; ladj_bar: T[batch] or NULL (= 0).
 * x_bar: [dim, batch] or NULL (not wanted); it may alias y_bar.
 * params_bar: NULL, or 2·n_ops pointers.  Slot 2k is p0 of stage k (a of Shift / Scale / Scale⁻¹ / Logit, alpha of LeakyReLU),
 * slot 2k+1 is p1 (b of Logit).  A non-NULL slot receives the cotangent as DEVICE T[len]: len = dim for a per-row parameter
 * (param_len == dim > 1 and a device pointer), 1 for a scalar — host or device — whose cotangent is also summed over the rows.
 * A non-NULL slot for a parameter its stage does not have: BJX_ERR_ARG.
 * The derivative conventions are those of bjx_coupling_chain_vjp (LeakyReLU: the negative branch is x < 0).
 * An empty batch writes zeros to the wanted slots and launches nothing.
 *
 * Shapes.  Every dim >= 1, batch >= 0.  Columns of whole 16-byte packs (dim a multiple of 4 Float32 / 2 Float64 rows, at most
 * 64 packs, 16-byte aligned x / y_bar / x_bar and per-row parameters) take the register layout (G lanes per column, packs along
 * the rows) when the chain is one stage or two one-parameter stages; longer chains, chains of two stages with a Logit, and every
 * other shape take the general kernel (one row per lane, row slabs of 256 for tall columns). */
#ifndef BJX_CHAIN_VJP_H
#define BJX_CHAIN_VJP_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_CHAIN_VJP_MAX_OPS 4 /* the fused limit (= BJX_MAX_SEG_OPS) */

int bjx_chain_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const bjx_op* ops, int n_ops, const void* x, const void* y_bar,
                         const void* ladj_bar, void* x_bar, void* const* params_bar, int64_t dim, int64_t batch);

/* Plans (bjx.h "plans"): the op list and the set of wanted slots validated once; parameters are held BY POINTER (an in-place
 * update of a device parameter is seen by the next run; host scalars are fixed at plan time).  wanted_slots_mask: bit i = slot i
 * of params_bar will be written.  bjx_plan_run_vjp_params: params_bar[i] must be non-NULL for every bit of the mask (NULL
 * params_bar only for an empty mask); entries outside the mask are ignored.  The run issues exactly the launches of the direct
 * entry and gives the same bits.  Destroyed by bjx_plan_destroy. */
enum { BJX_PLAN_CHAIN_VJP_PARAMS = 6 };
int bjx_plan_chain_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const bjx_op* ops, int n_ops, uint32_t wanted_slots_mask, int64_t dim,
                              bjx_plan** plan);
int bjx_plan_run_vjp_params(bjx_plan* plan, const void* x, const void* y_bar, const void* ladj_bar, void* x_bar,
                            void* const* params_bar, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_CHAIN_VJP_H */
