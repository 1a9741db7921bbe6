// bjx_radial_stack_logpdf.hip — log-density of transformed(N(μ, diag σ²), l_L ∘ … ∘ l_1) at y for a run of RadialLayers, with ȳ and
// the cotangents of every layer's parameters and of μ, σ, in one streaming pass over y (include/bjx_radial_stack_logpdf.h).
// The kernels are the inverse-run parameter pullback's (rsp_group_body / rsp_walk_body of bjx_radial_stack_common.inc, LP = true):
//   primal sweep   all L inverse layers — the column ends as x = f⁻¹(y) — with the run's log-det added up per column;
//   at x           w = (x − μ)/σ (μ, σ rows in LDS), one group reduction for ‖w‖², lp = −½‖w‖² − Σ log σ − (d/2) log 2π + ℓ;
//                  the seed ḡ = −c·w/σ goes to the registers the pullback loads out_bar into; μ̄ += −ḡ and σ̄ += −ḡ⊙w − c/σ go to two
//                  more rows of the block's Float64 table by the path z̄₀ takes;
//   reverse sweep  the pullback's, rewinding from x (the pullback skips the last layer's update and rewind, here it is x itself).
// One [L, dim + 2 | Σ lp | μ̄ | σ̄] Float64 partial per block; the folds of the pullback add them in a fixed order.
#include "bjx_internal.h"
#include "bjx_tile.h"
#include "../../include/bjx_radial_stack_logpdf.h"

namespace {
using namespace bjx;
#include "bjx_flow_common.inc"
#define RS_PARAMS_PASS
#include "bjx_radial_stack_common.inc"

template <class T, int V, int R>
__global__ __launch_bounds__(256) void radial_stack_logpdf_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                  const T* __restrict__ y, const T* __restrict__ lp_bar, T* __restrict__ ybar, int64_t dim,
                                                                  int64_t batch, int G, int64_t tiles, double* __restrict__ partials, RspLogpdf<T> q) {
  rsp_group_body<T, V, R, true, true>(alpha_, beta, z0, n_layers, y, nullptr, lp_bar, ybar, dim, batch, G, tiles, partials, q);
}

template <class T, int DMAX, int V>
__global__ __launch_bounds__(64) void radial_stack_logpdf_walk_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                       const T* __restrict__ y, const T* __restrict__ lp_bar, T* __restrict__ ybar, int dim, int P,
                                                                       int SP, int64_t batch, double* __restrict__ partials, RspLogpdf<T> q) {
  rsp_walk_body<T, DMAX, true, V, true>(alpha_, beta, z0, n_layers, y, nullptr, lp_bar, ybar, dim, P, SP, batch, partials, q);
}

// the last fold and the cast: the layers' rows as rsp_final_kernel (when asked for), then Σ lp (kept in Float64), μ̄ and σ̄
template <class T>
__global__ __launch_bounds__(256) void rsl_final_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const double* __restrict__ in, int nsets, int n_layers,
                                                        int dim, int per, T* __restrict__ alpha_bar, T* __restrict__ beta_bar, T* __restrict__ z0_bar,
                                                        double* __restrict__ lp_sum, T* __restrict__ mu_bar, T* __restrict__ sigma_bar) {
  const int tail = n_layers * (dim + 2);
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  if (e < tail) {
    if (z0_bar) rsp_final_entry<T>(alpha_, beta, in, nsets, per, dim, e, alpha_bar, beta_bar, z0_bar);
    return;
  }
  const int k = e - tail - 1;
  T* dst = k < 0 ? nullptr : (k < dim ? (mu_bar ? mu_bar + k : nullptr) : (sigma_bar ? sigma_bar + (k - dim) : nullptr));
  if (k < 0 ? lp_sum == nullptr : dst == nullptr) return;
  double s = 0.0;
  for (int i = 0; i < nsets; ++i) s += in[(size_t)i * per + e];
  if (k < 0) *lp_sum = s;
  else *dst = (T)s;
}

#define RSL_SWITCH_R(TT, VV)                                                                                                                          \
  switch (R) {                                                                                                                                        \
    case 1: hipLaunchKernelGGL((radial_stack_logpdf_kernel<TT, VV, 1>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, y, lp_bar, y_bar, dim, batch, G, tiles, part, q); break;  \
    case 2: hipLaunchKernelGGL((radial_stack_logpdf_kernel<TT, VV, 2>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, y, lp_bar, y_bar, dim, batch, G, tiles, part, q); break;  \
    case 4: hipLaunchKernelGGL((radial_stack_logpdf_kernel<TT, VV, 4>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, y, lp_bar, y_bar, dim, batch, G, tiles, part, q); break;  \
    default: hipLaunchKernelGGL((radial_stack_logpdf_kernel<TT, VV, 8>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, y, lp_bar, y_bar, dim, batch, G, tiles, part, q); break; \
  }

template <class T>
int radial_stack_logpdf_impl(bjx_ctx* ctx, const T* alpha_, const T* beta, const T* z0, int nl, const T* mu, const T* sigma, const T* y, const T* lp_bar, T* lp_ps,
                             double* lp_sum, T* y_bar, T* alpha_bar, T* beta_bar, T* z0_bar, T* mu_bar, T* sigma_bar, int64_t dim, int64_t batch) {
  constexpr int VW = Vec16<T>::N;
  const bool walk = rs_walk_shape<T>(dim);
  const bool aligned = bjx_aligned16(y) && bjx_aligned16(y_bar);
  const bool want_base = mu_bar || sigma_bar;
  int V = 1, G = 1, R = 1, P = 0, SP = 0;
  size_t smem = 0;
  int64_t tiles = 0, cap = 0;
  const int64_t per64 = (int64_t)nl * (dim + 2) + 1 + (want_base ? 2 * dim : 0);
  if (walk) {
    P = (int)(dim | 1);
    SP = (nl * 2) | 1;
    const int DMAX = dim <= 8 ? 8 : (dim <= 16 ? 16 : 32);
    const size_t dbl = (size_t)nl * (DMAX + 2) + 1 + 2 * DMAX + (size_t)DMAX * 65;
    smem = (dbl + (dbl & 1)) * sizeof(double) +
           ((((size_t)64 * P + 3) / 4) * 4 + (((size_t)nl * (DMAX + 4) + 3) / 4) * 4 + (size_t)2 * DMAX + (size_t)64 * SP) * sizeof(T);
    tiles = (batch + 63) / 64;
    cap = (int64_t)ctx->num_cu * 16;
  } else {
    BJX_REQUIRE(ctx, rs_group_cfg<T>(aligned, dim, &V, &G, &R), BJX_ERR_UNSUPPORTED,
                "bjx_radial_stack_logpdf_vjp_params: columns of %lld rows are not fused (take the layers one by one)", (long long)dim);
    const int uc = R == 1 ? 2 : 1;                                   // StackVjpUC<R>
    const int64_t cpb = (int64_t)(256 / G) * uc;
    smem = rs_round16((size_t)2 * nl * sizeof(T)) + rs_round16((size_t)nl * dim * sizeof(T)) + rs_round16((size_t)2 * dim * sizeof(T)) +
           rs_round16((size_t)cpb * nl * 2 * sizeof(T)) + (size_t)4 * per64 * sizeof(double);
    tiles = (batch + cpb - 1) / cpb;
    cap = (int64_t)ctx->num_cu * 4;
  }
  BJX_REQUIRE(ctx, smem <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack_logpdf_vjp_params: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
  BJX_REQUIRE(ctx, per64 < ((int64_t)1 << 24), BJX_ERR_UNSUPPORTED, "bjx_radial_stack_logpdf_vjp_params: too many layers");
  const int per = (int)per64;
  if (batch == 0) {
    if (z0_bar) {
      BJX_HIP(ctx, hipMemsetAsync(z0_bar, 0, (size_t)nl * dim * sizeof(T), ctx->stream));
      BJX_HIP(ctx, hipMemsetAsync(alpha_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
      BJX_HIP(ctx, hipMemsetAsync(beta_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
    }
    if (mu_bar) BJX_HIP(ctx, hipMemsetAsync(mu_bar, 0, (size_t)dim * sizeof(T), ctx->stream));
    if (sigma_bar) BJX_HIP(ctx, hipMemsetAsync(sigma_bar, 0, (size_t)dim * sizeof(T), ctx->stream));
    if (lp_sum) BJX_HIP(ctx, hipMemsetAsync(lp_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  const int64_t grid = rsp_grid(tiles, cap);
  const int chunks = (int)((grid + RSP_FOLD_CHUNK - 1) / RSP_FOLD_CHUNK);
  { int rc = bjx_ensure_partials(ctx, (size_t)(grid + chunks) * per); if (rc) return rc; }
  double* part = ctx->partials;
  double* part2 = part + (size_t)grid * per;
  const RspLogpdf<T> q{mu, sigma, lp_ps, want_base ? 1 : 0};
  {
    BjxProf prof_(ctx);
    if (walk) {
#define RSLW(D_, V_) hipLaunchKernelGGL((radial_stack_logpdf_walk_kernel<T, D_, V_>), dim3((unsigned)grid), dim3(64), smem, ctx->stream, alpha_, beta, z0, nl, y, lp_bar, y_bar, (int)dim, P, SP, batch, part, q)
#define RSLW_V(D_) do { if (aligned) RSLW(D_, VW); else RSLW(D_, 1); } while (0)
      if (dim <= 8) RSLW_V(8); else if (dim <= 16) RSLW_V(16); else RSLW_V(32);
#undef RSLW_V
#undef RSLW
    } else if (V == VW) {
      RSL_SWITCH_R(T, VW)
    } else {
      RSL_SWITCH_R(T, 1)
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  if (!z0_bar && !lp_sum && !want_base) return BJX_OK;              // nothing summed over the batch is asked for: the pass alone
  {
    BjxProf prof_(ctx);
    const unsigned eb = (unsigned)((per + 255) / 256);
    if (chunks > 1) {
      hipLaunchKernelGGL(rsp_fold_kernel, dim3(eb, (unsigned)chunks), dim3(256), 0, ctx->stream, part, (int)grid, per, RSP_FOLD_CHUNK, part2);
      hipLaunchKernelGGL(rsl_final_kernel<T>, dim3(eb), dim3(256), 0, ctx->stream, alpha_, beta, part2, chunks, nl, (int)dim, per, alpha_bar, beta_bar, z0_bar, lp_sum,
                         mu_bar, sigma_bar);
    } else {
      hipLaunchKernelGGL(rsl_final_kernel<T>, dim3(eb), dim3(256), 0, ctx->stream, alpha_, beta, part, (int)grid, nl, (int)dim, per, alpha_bar, beta_bar, z0_bar, lp_sum,
                         mu_bar, sigma_bar);
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_radial_stack_logpdf_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const void* alpha_, const void* beta, const void* z0, int n_layers, const void* mu,
                                               const void* sigma, const void* y, const void* lp_bar, void* lp_ps, double* lp_sum, void* y_bar, void* alpha_bar,
                                               void* beta_bar, void* z0_bar, void* mu_bar, void* sigma_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0 && n_layers >= 1, BJX_ERR_SHAPE, "bjx_radial_stack_logpdf_vjp_params: bad size");
  const int nbar = (alpha_bar != nullptr) + (beta_bar != nullptr) + (z0_bar != nullptr);
  BJX_REQUIRE(ctx, alpha_ && beta && z0 && (y || batch == 0) && (nbar == 0 || nbar == 3), BJX_ERR_ARG,
              "bjx_radial_stack_logpdf_vjp_params: null pointer (alpha_bar, beta_bar, z0_bar: all three or none)");
  if (dt == BJX_F32) return radial_stack_logpdf_impl<float>(ctx, (const float*)alpha_, (const float*)beta, (const float*)z0, n_layers, (const float*)mu, (const float*)sigma, (const float*)y, (const float*)lp_bar, (float*)lp_ps, lp_sum, (float*)y_bar, (float*)alpha_bar, (float*)beta_bar, (float*)z0_bar, (float*)mu_bar, (float*)sigma_bar, dim, batch);
  if (dt == BJX_F64) return radial_stack_logpdf_impl<double>(ctx, (const double*)alpha_, (const double*)beta, (const double*)z0, n_layers, (const double*)mu, (const double*)sigma, (const double*)y, (const double*)lp_bar, (double*)lp_ps, lp_sum, (double*)y_bar, (double*)alpha_bar, (double*)beta_bar, (double*)z0_bar, (double*)mu_bar, (double*)sigma_bar, dim, batch);
  return bjx_fail(ctx, BJX_ERR_ARG, "bjx_radial_stack_logpdf_vjp_params: bad dtype %d", (int)dt);
}
