// bjx_radial_stack_params.hip — parameter pullback of a RUN of RadialLayers l_L ∘ … ∘ l_1 and of its inverse, one streaming pass
// (include/bjx_radial_stack_params.h).  The sweeps are radial_stack_vjp_kernel's (bjx_radial_stack.hip): the primal sweep leaves one
// or two scalars per layer and column in LDS, the reverse sweep rewinds the resident column.  At layer k the reverse sweep holds the
// layer's input (δ = z − z₀ₖ, r), the cotangent ḡ of its output, dg = δᵀḡ and, after the update, the cotangent ḡ′ of its input:
//   forward run   z̄₀ₖ += ḡ − ḡ′;  g_β̂ = h·dg + ℓ̄[(d−1)h/a + (h − h²r)/D];  g_α̂ = −h²[β̂·dg + ℓ̄((d−1)β̂/a + (β̂ − 2β̂hr)/D)]
//                 (h = 1/(α̂+r), a = 1 + β̂h, D = a − β̂h²r: radial_param_partial_kernel of bjx_flow.hip)
//   inverse run   the implicit-function rule per layer: the same formulas at the pre-image (δ_pre = gain·δ_in, r = gain·γ) with the
//                 cotangents (−ḡ′, −ℓ̄); δ_preᵀḡ′ = (gain·dg − kl·r²)/(a + c·r²) — the dv/(a + c r²) of rs_coef, no second reduction;
//                 z̄₀ₖ += ḡ − ḡ′ again (the forward input pullback of (−ḡ′, −ℓ̄) is −ḡ).
//   at the end    ᾱ_ = σ(α_)(Σg_α̂ − Σg_β̂),  β̄ = σ(β)·Σg_β̂                                  (the raw parameters behind softplus)
//
// Sums over the batch.  Blocks are persistent: a block walks many column tiles and keeps its sums ON CHIP, in Float64, per layer
// [z̄₀ (dim) | Σg_α̂ | Σg_β̂]:
//   group form  per layer and tile every lane holds ḡ − ḡ′ of its rows (summed over its UC columns); a shuffle butterfly over the
//               column groups of the wave (lanes gl, gl + G, …), then lanes < G add into the wave's PRIVATE LDS table — one writer
//               per entry, the LDS queue of a wave is in order: no atomics.  The four waves' tables are added in a fixed order at
//               the end of the block.
//   walk form   (one wave per block) the 64 lanes' ḡ − ḡ′ go through a [DMAX][65] Float64 LDS tile; lane (row, segment) sums its
//               segment of the row, a butterfly over the segments, lanes < DMAX add into the block's table.
// One [L, dim + 2] Float64 partial per BLOCK (not per tile) goes to the context's partials; one or two fold launches add them in a
// fixed order and cast to T at the very end.  Two identical calls give identical bits.
// The kernels' bodies, the folds and the grid rule live in bjx_radial_stack_common.inc (RS_PARAMS_PASS): bjx_radial_stack_logpdf.hip
// runs the same sweeps with a generated seed.
#include "bjx_internal.h"
#include "bjx_tile.h"
#include "../../include/bjx_radial_stack_params.h"

namespace {
using namespace bjx;
#include "bjx_flow_common.inc"
#define RS_PARAMS_PASS
#include "bjx_radial_stack_common.inc"

template <class T, int V, int R, bool INV>
__global__ __launch_bounds__(256) void radial_stack_params_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                  const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int64_t dim,
                                                                  int64_t batch, int G, int64_t tiles, double* __restrict__ partials) {
  rsp_group_body<T, V, R, INV, false>(alpha_, beta, z0, n_layers, x, gbar, lbar, xbar, dim, batch, G, tiles, partials, RspLogpdf<T>{nullptr, nullptr, nullptr, 0});
}

template <class T, int DMAX, bool INV, int V>
__global__ __launch_bounds__(64) void radial_stack_params_walk_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                       const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int dim, int P,
                                                                       int SP, int64_t batch, double* __restrict__ partials) {
  rsp_walk_body<T, DMAX, INV, V, false>(alpha_, beta, z0, n_layers, x, gbar, lbar, xbar, dim, P, SP, batch, partials, RspLogpdf<T>{nullptr, nullptr, nullptr, 0});
}

// the last fold and the cast (rsp_final_entry) over the [L][dim + 2] table
template <class T>
__global__ __launch_bounds__(256) void rsp_final_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const double* __restrict__ in, int nsets, int n_layers,
                                                        int dim, T* __restrict__ alpha_bar, T* __restrict__ beta_bar, T* __restrict__ z0_bar) {
  const int per = n_layers * (dim + 2);
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  rsp_final_entry<T>(alpha_, beta, in, nsets, per, dim, e, alpha_bar, beta_bar, z0_bar);
}

// ------------------------------------------------------------------ host
#define RSP_SWITCH_R(TT, VV, INVV)                                                                                                                    \
  switch (R) {                                                                                                                                        \
    case 1: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 1, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break;  \
    case 2: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 2, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break;  \
    case 4: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 4, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break;  \
    default: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 8, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break; \
  }

template <class T>
int radial_stack_vjp_params_impl(bjx_ctx* ctx, int inverse, const T* alpha_, const T* beta, const T* z0, int nl, const T* in, const T* out_bar,
                                 const T* ladj_bar, T* in_bar, T* alpha_bar, T* beta_bar, T* z0_bar, int64_t dim, int64_t batch) {
  constexpr int VW = Vec16<T>::N;
  const int ns = inverse ? 2 : 1;
  const bool walk = rs_walk_shape<T>(dim);
  const bool aligned = bjx_aligned16(in) && bjx_aligned16(out_bar) && bjx_aligned16(in_bar);
  int V = 1, G = 1, R = 1, P = 0, SP = 0;
  size_t smem = 0;
  int64_t tiles = 0, cap = 0;
  if (walk) {
    P = (int)(dim | 1);
    SP = (nl * ns) | 1;
    const int DMAX = dim <= 8 ? 8 : (dim <= 16 ? 16 : 32);
    const size_t dbl = (size_t)nl * (DMAX + 2) + (size_t)DMAX * 65;
    smem = (dbl + (dbl & 1)) * sizeof(double) + (2 * ((((size_t)64 * P + 3) / 4) * 4) + (((size_t)nl * (DMAX + 4) + 3) / 4) * 4 + (size_t)64 * SP) * sizeof(T);
    tiles = (batch + 63) / 64;
    cap = (int64_t)ctx->num_cu * 16;
  } else {
    BJX_REQUIRE(ctx, rs_group_cfg<T>(aligned, dim, &V, &G, &R), BJX_ERR_UNSUPPORTED,
                "bjx_radial_stack_vjp_params: columns of %lld rows are not fused (take the layers one by one)", (long long)dim);
    const int uc = R == 1 ? 2 : 1;                                   // StackVjpUC<R>
    const int64_t cpb = (int64_t)(256 / G) * uc;
    smem = rs_round16((size_t)2 * nl * sizeof(T)) + rs_round16((size_t)nl * dim * sizeof(T)) + rs_round16((size_t)cpb * nl * ns * sizeof(T)) +
           (size_t)4 * nl * (dim + 2) * sizeof(double);
    tiles = (batch + cpb - 1) / cpb;
    cap = (int64_t)ctx->num_cu * 4;
  }
  BJX_REQUIRE(ctx, smem <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp_params: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
  const int64_t per64 = (int64_t)nl * (dim + 2);
  BJX_REQUIRE(ctx, per64 < ((int64_t)1 << 24), BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp_params: too many layers");
  const int per = (int)per64;
  if (batch == 0) {
    BJX_HIP(ctx, hipMemsetAsync(z0_bar, 0, (size_t)nl * dim * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(alpha_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(beta_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
    return BJX_OK;
  }
  const int64_t grid = rsp_grid(tiles, cap);
  const int chunks = (int)((grid + RSP_FOLD_CHUNK - 1) / RSP_FOLD_CHUNK);
  { int rc = bjx_ensure_partials(ctx, (size_t)(grid + chunks) * per); if (rc) return rc; }
  double* part = ctx->partials;
  double* part2 = part + (size_t)grid * per;
  {
    BjxProf prof_(ctx);
    if (walk) {
#define RSPW(D_, I_, V_) hipLaunchKernelGGL((radial_stack_params_walk_kernel<T, D_, I_, V_>), dim3((unsigned)grid), dim3(64), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, (int)dim, P, SP, batch, part)
#define RSPW_V(D_, I_) do { if (aligned) RSPW(D_, I_, VW); else RSPW(D_, I_, 1); } while (0)
#define RSPW_D(I_) do { if (dim <= 8) RSPW_V(8, I_); else if (dim <= 16) RSPW_V(16, I_); else RSPW_V(32, I_); } while (0)
      if (inverse) RSPW_D(true); else RSPW_D(false);
#undef RSPW_D
#undef RSPW_V
#undef RSPW
    } else if (V == VW) {
      if (!inverse) { RSP_SWITCH_R(T, VW, false) } else { RSP_SWITCH_R(T, VW, true) }
    } else {
      if (!inverse) { RSP_SWITCH_R(T, 1, false) } else { RSP_SWITCH_R(T, 1, true) }
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  {
    BjxProf prof_(ctx);
    const unsigned eb = (unsigned)((per + 255) / 256);
    if (chunks > 1) {
      hipLaunchKernelGGL(rsp_fold_kernel, dim3(eb, (unsigned)chunks), dim3(256), 0, ctx->stream, part, (int)grid, per, RSP_FOLD_CHUNK, part2);
      hipLaunchKernelGGL(rsp_final_kernel<T>, dim3(eb), dim3(256), 0, ctx->stream, alpha_, beta, part2, chunks, nl, (int)dim, alpha_bar, beta_bar, z0_bar);
    } else {
      hipLaunchKernelGGL(rsp_final_kernel<T>, dim3(eb), dim3(256), 0, ctx->stream, alpha_, beta, part, (int)grid, nl, (int)dim, alpha_bar, beta_bar, z0_bar);
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_radial_stack_vjp_params(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                                        const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* alpha_bar, void* beta_bar,
                                        void* z0_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0 && n_layers >= 1, BJX_ERR_SHAPE, "bjx_radial_stack_vjp_params: bad size");
  BJX_REQUIRE(ctx, alpha_ && beta && z0 && alpha_bar && beta_bar && z0_bar && ((in && out_bar) || batch == 0), BJX_ERR_ARG,
              "bjx_radial_stack_vjp_params: null pointer");
  if (dt == BJX_F32) return radial_stack_vjp_params_impl<float>(ctx, inverse, (const float*)alpha_, (const float*)beta, (const float*)z0, n_layers, (const float*)in, (const float*)out_bar, (const float*)ladj_bar, (float*)in_bar, (float*)alpha_bar, (float*)beta_bar, (float*)z0_bar, dim, batch);
  if (dt == BJX_F64) return radial_stack_vjp_params_impl<double>(ctx, inverse, (const double*)alpha_, (const double*)beta, (const double*)z0, n_layers, (const double*)in, (const double*)out_bar, (const double*)ladj_bar, (double*)in_bar, (double*)alpha_bar, (double*)beta_bar, (double*)z0_bar, dim, batch);
  return bjx_fail(ctx, BJX_ERR_ARG, "bjx_radial_stack_vjp_params: bad dtype %d", (int)dt);
}
