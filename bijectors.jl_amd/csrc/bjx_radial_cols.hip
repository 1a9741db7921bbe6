// bjx_radial_cols.hip — a stack of RadialLayers with one parameter set (α_, β, z₀) per COLUMN (include/bjx_radial_cols.h): the
// amortised radial flow, whose parameters an encoder emits per sample and which therefore stream with the data.
//
// Mapping (the one of bjx_planar_cols.hip): V = 16 B / sizeof(T) elements per pack, packs = ceil(dim / V); a column gets G lanes
// (G = the power of two >= packs, at most 64) and lane j of the group holds the packs j, j + G, ... (R of them, R = 1, 2 or 4; three
// packs per lane run the R = 4 kernels with a dead pack): 1 024 rows in Float32, 512 in Float64.  A 256-thread block owns
// C = 256/G columns at a time and walks column groups grid-stride over a capped grid.  A lane group never spans two waves, so
// ‖z − z₀‖² of a layer is one butterfly and no kernel has a barrier in its column loop.
//
// Two forms of every kernel: 16-byte vector accesses when dim is a whole number of packs, every base pointer is 16-byte aligned
// and the column stride of z₀ is a multiple of V; the element form otherwise (packs on element-aligned addresses, the last one
// partial, dead rows read as zero: δ = 0 there, so they leave every sum alone).
//
// Per layer α̂ = log1pexp(α_) and log1pexp(β) = α̂ + β̂ are computed per column in registers; the scalars of the step, the log-det,
// the Jacobian J = aI + cδδᵀ and its Sherman–Morrison inverse are the closed forms of bjx_radial_stack_common.inc (rs_scalars,
// rs_logdet, rs_jac, rs_coef; 1/r read as 0 at r = 0).  z₀ is read through the caches, the column stays in registers.
//   Forward pullback: the primal sweep saves r_k per column in a dynamic-LDS table [L][C]; the reverse sweep REWINDS the resident
//   column, z_k = z₀ + (z_{k+1} − z₀)/(1 + β̂h_k), instead of storing L columns, and writes z̄₀ = ȳ_k − z̄_k, β̄ = σ(β)g_β̂,
//   ᾱ_ = σ(α_)(g_α̂ − g_β̂) per column (g_α̂, g_β̂: oracle.radial_param_vjp).  Every lane of a group writes the group's (bit-identical)
//   r_k to the group's slot and reads that slot back: no lane depends on another lane's LDS write.
//   Inverse pullback: the primal sweep (k = L−1 … 0) ends at the pre-image x; the reverse sweep (k = 0 … L−1) holds z_k, so r_k is
//   recomputed from it and no table is needed: ȳ_k = J⁻¹(ḡ − klδ), the parameter cotangents are the forward forms at z_k seeded
//   with (−ȳ_k, −ℓ̄) (z̄₀ = ḡ − ȳ_k), and the column advances by the forward step.  One launch.
// Nothing is summed over columns, so there are no atomics; the summed log-det goes through the per-block partials +
// bjx_launch_finalize (fixed order: run-to-run identical bits).
#include "bjx_internal.h"
#include "../../include/bjx_radial_cols.h"
#include <type_traits>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"
#include "bjx_radial_stack_common.inc"
#include "bjx_cols_lanes.inc"                                      // LanePacks, load_data, load_param, store_data

template <class T> struct RadialColsArgs {
  const T *pa, *pb, *pz;
  int64_t lda, ldb, ldz;
  int64_t dim, batch, groups;
  int L, G;
};

// g_α̂ and g_β̂ of one column from r, δᵀȳ and ℓ̄ (oracle.radial_param_vjp; rsp_terms of the batch-summed pass)
template <class T>
__device__ __forceinline__ void rc_terms(T rr, T alpha, T bh, T dim_m1, T dgx, T lbx, T& ga, T& gb) {
#pragma clang fp contract(off)
  const T h = T(1) / (alpha + rr);
  const T a = T(1) + bh * h;
  const T ia = T(1) / a, iD = T(1) / (a - bh * h * h * rr);
  gb = h * dgx + lbx * (dim_m1 * h * ia + (h - h * h * rr) * iD);
  ga = -h * h * (bh * dgx + lbx * (dim_m1 * bh * ia + (bh - T(2) * bh * h * rr) * iD));
}

// ------------------------------------------------------------------ the map and its inverse
// (x and y may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them)
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void radial_cols_map_kernel(const RadialColsArgs<T> a, const T* x, T* y, T* __restrict__ ladj_ps, int accumulate,
                                                              double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* redd = reinterpret_cast<double*>(smem);
  const int G = a.G, C = (int)blockDim.x / G, L = a.L;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const T dim_m1 = T(dim - 1);
  const LanePacks<V, R> lp(gl, G, (int)dim);
  double acc = 0.0;
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;       // a group past the batch works on the last column and stores nothing
    Pack<T, V> z[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    const T* ac = a.pa + col * a.lda;
    const T* bc = a.pb + col * a.ldb;
    const T* zc = a.pz + col * a.ldz;
    T ladj = T(0);
    for (int li = 0; li < L; ++li) {
      const int k = INV ? L - 1 - li : li;
      Pack<T, V> z0[R];
      load_param<T, V, R, AL>(zc + (int64_t)k * dim, lp, z0);
      const T alpha = d_log1pexp(ac[k]), apb = d_log1pexp(bc[k]);  // radial_layer.jl:44-45: β̂ = −α̂ + log1pexp(β)
      const T bh = -alpha + apb;
      T ss = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) { const T dl = z[r].v[j] - z0[r].v[j]; ss += dl * dl; }
      ss = group_sum_rt(ss, G);
      T gain, fwd_gain, ld;
      rs_scalars<T, INV>(ss, alpha, apb, bh, dim_m1, gain, fwd_gain, ld);
      ladj += ld;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T dl = z[r].v[j] - z0[r].v[j];
          if constexpr (!INV) z[r].v[j] += fwd_gain * dl;
          else z[r].v[j] = z0[r].v[j] + gain * dl;
        }
    }
    if (live) {
      store_data<T, V, R, AL>(y + col * dim, lp, z);
      if (gl == 0) {
        if (ladj_ps) ladj_ps[col] = accumulate ? ladj_ps[col] + ladj : ladj;
        acc += (double)ladj;
      }
    }
  }
  if (partials) block_publish_partial(acc, redd, partials);
}

// ------------------------------------------------------------------ the pullbacks
// x̄ (INV: ȳ) and the per-column (ᾱ_, β̄, z̄₀) of the map or of its inverse (any of the three may be null).
// (gbar and xbar may be the same buffer, as x and y above.)  Contraction is off and the multiply-adds are spelled out, as in the
// run pullbacks: x̄ must not depend on which outputs were asked for or on the form the dispatcher chose.
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void radial_cols_vjp_kernel(const RadialColsArgs<T> a, const T* x, const T* gbar, const T* __restrict__ lbar, T* xbar,
                                                              T* __restrict__ abar, T* __restrict__ bbar, T* __restrict__ zbar) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* tab = reinterpret_cast<T*>(smem);                           // forward only, [L][C]: r_k of the block's columns
  const int G = a.G, C = (int)blockDim.x / G, L = a.L;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const T dim_m1 = T(dim - 1);
  const LanePacks<V, R> lp(gl, G, (int)dim);
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;
    Pack<T, V> z[R], g[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    const T* ac = a.pa + col * a.lda;
    const T* bc = a.pb + col * a.ldb;
    const T* zc = a.pz + col * a.ldz;
    // ---- primal sweep.  Forward: r_k of every layer, the column stops at the INPUT of the last one (its rewind would undo the
    // step).  Inverse: down to the pre-image x.
    for (int li = 0; li < L; ++li) {
      const int k = INV ? L - 1 - li : li;
      Pack<T, V> z0[R];
      load_param<T, V, R, AL>(zc + (int64_t)k * dim, lp, z0);
      const T alpha = d_log1pexp(ac[k]), apb = d_log1pexp(bc[k]);
      const T bh = -alpha + apb;
      T ss = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) { const T dl = z[r].v[j] - z0[r].v[j]; ss = rs_fma(dl, dl, ss); }
      ss = group_sum_rt(ss, G);
      if constexpr (!INV) {
        const T rr = d_sqrt(ss);
        tab[k * C + cl] = rr;
        if (li + 1 < L) {
          const T fwd_gain = bh / (alpha + rr);
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < V; ++j) z[r].v[j] = rs_fma(fwd_gain, z[r].v[j] - z0[r].v[j], z[r].v[j]);
        }
      } else {
        const T gam = d_sqrt(ss);                                // compute_r, radial_layer.jl:124-129
        const T aa = apb - gam;
        const T r0 = (d_sqrt(aa * aa + 4 * alpha * gam) - aa) / 2;
        const T gain = (alpha + r0) / (apb + r0);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) z[r].v[j] = rs_fma(gain, z[r].v[j] - z0[r].v[j], z0[r].v[j]);
      }
    }
    // ---- reverse sweep on the cotangent: the column holds z_k, the input of forward layer k
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    const T lb = lbar ? lbar[col] : T(0);
    for (int li = 0; li < L; ++li) {
      const int k = INV ? li : L - 1 - li;
      Pack<T, V> z0[R];
      load_param<T, V, R, AL>(zc + (int64_t)k * dim, lp, z0);
      const T araw = ac[k], braw = bc[k];
      const T alpha = d_log1pexp(araw), apb = d_log1pexp(braw);
      const T bh = -alpha + apb;
      T rr, dg = T(0);
      if constexpr (!INV) {
        rr = tab[k * C + cl];
        if (li > 0) {                                            // rewind: the column holds the OUTPUT of layer k
          const T back = T(1) / (T(1) + bh * (T(1) / (alpha + rr)));
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < V; ++j) z[r].v[j] = rs_fma(z[r].v[j] - z0[r].v[j], back, z0[r].v[j]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) dg = rs_fma(z[r].v[j] - z0[r].v[j], g[r].v[j], dg);
        dg = group_sum_rt(dg, G);
      } else {
        T ss = T(0);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T dl = z[r].v[j] - z0[r].v[j];
            ss = rs_fma(dl, dl, ss);
            dg = rs_fma(dl, g[r].v[j], dg);
          }
        group_sum2_rt(ss, dg, G);
        rr = d_sqrt(ss);
      }
      T ja, jc, kl, ca, cd;
      rs_jac<T>(rr, alpha, bh, dim_m1, lb, ja, jc, kl);
      rs_coef<T, INV>(ja, jc, kl, rr, T(1), dg, ca, cd);         // INV: Sherman–Morrison at the pre-image itself (gain = 1)
      // the seeds of the parameter forms: forward (δᵀȳ, ℓ̄); inverse (−δᵀȳ_k, −ℓ̄) with δᵀȳ_k = δᵀ(ḡ − klδ)/(a + c r²)
      const T dgx = INV ? -((dg - kl * rr * rr) / (ja + jc * rr * rr)) : dg;
      const T lbx = INV ? -lb : lb;
      T ga, gb;
      rc_terms<T>(rr, alpha, bh, dim_m1, dgx, lbx, ga, gb);
      const T fwd_gain = bh * (T(1) / (alpha + rr));
      const bool step = INV && li + 1 < L;                       // the inverse's column advances by the forward step
      Pack<T, V> zb[R];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T dl = z[r].v[j] - z0[r].v[j];
          const T gn = rs_fma(cd, dl, ca * g[r].v[j]);
          zb[r].v[j] = g[r].v[j] - gn;                           // forward: ȳ_k − z̄_k; inverse: ḡ − ȳ_k
          g[r].v[j] = gn;
          if (step) z[r].v[j] = rs_fma(fwd_gain, dl, z[r].v[j]);
        }
      if (live) {
        if (zbar) store_data<T, V, R, AL>(zbar + (col * L + k) * dim, lp, zb);
        if (gl == 0) {
          if (bbar) bbar[col * L + k] = d_logistic<T>(braw) * gb;
          if (abar) abar[col * L + k] = d_logistic<T>(araw) * (ga - gb);
        }
      }
    }
    if (live) store_data<T, V, R, AL>(xbar + col * dim, lp, g);
  }
}

// ------------------------------------------------------------------ host side
constexpr int kThreads = 256;
constexpr int kBlocksPerCu = 8;

int radial_cols_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a, int64_t ld_b,
                      int64_t ld_z, int n_layers, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, n_layers >= 1 && n_layers <= BJX_RADIAL_COLS_MAX_LAYERS, BJX_ERR_UNSUPPORTED, "%s: %d layers (1 ... %d supported)", name, n_layers,
              BJX_RADIAL_COLS_MAX_LAYERS);
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0, BJX_ERR_SHAPE, "%s: bad size (dim=%lld, batch=%lld)", name, (long long)dim, (long long)batch);
  const int64_t lim = dt == BJX_F32 ? 1024 : 512;
  BJX_REQUIRE(ctx, dim <= lim, BJX_ERR_UNSUPPORTED, "%s: dim %lld above the %lld rows a lane group holds in %s", name, (long long)dim, (long long)lim,
              dt == BJX_F32 ? "Float32" : "Float64");
  BJX_REQUIRE(ctx, ld_a >= n_layers && ld_b >= n_layers && ld_z >= dim * n_layers, BJX_ERR_SHAPE,
              "%s: column strides (%lld, %lld, %lld) below n_layers = %d and dim x n_layers = %lld", name, (long long)ld_a, (long long)ld_b, (long long)ld_z,
              n_layers, (long long)(dim * n_layers));
  BJX_REQUIRE(ctx, batch == 0 || (p_alpha && p_beta && p_z0), BJX_ERR_ARG, "%s: null parameter pointer", name);
  return BJX_OK;
}

// lanes per column, packs per lane
template <class T> void radial_cols_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T>
RadialColsArgs<T> radial_cols_args(const bjx_ctx* ctx, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a, int64_t ld_b, int64_t ld_z, int L,
                                   int64_t dim, int64_t batch, int G, int threads, int* grid) {
  RadialColsArgs<T> a{};
  a.pa = (const T*)p_alpha; a.pb = (const T*)p_beta; a.pz = (const T*)p_z0;
  a.lda = ld_a; a.ldb = ld_b; a.ldz = ld_z;
  a.dim = dim; a.batch = batch; a.L = L; a.G = G;
  const int C = threads / G;
  a.groups = (batch + C - 1) / C;
  const int64_t cap = (int64_t)ctx->num_cu * kBlocksPerCu * (kThreads / threads);
  *grid = (int)(a.groups < cap ? a.groups : cap);
  return a;
}

template <class T> bool radial_cols_vector_form(int64_t dim, int64_t ld_z, std::initializer_list<const void*> ptrs) {
  constexpr int V = Vec16<T>::N;
  if (dim % V || ld_z % V) return false;
  for (const void* p : ptrs)
    if (p && !bjx_aligned16(p)) return false;
  return true;
}

template <class T, int R, bool AL>
void launch_map(bjx_ctx* ctx, const RadialColsArgs<T>& a, int grid, int inverse, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
  constexpr int V = Vec16<T>::N;
  const size_t smem = 8 * sizeof(double);
  if (inverse) hipLaunchKernelGGL((radial_cols_map_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, in, out, ladj_ps, accum, partials);
  else hipLaunchKernelGGL((radial_cols_map_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, in, out, ladj_ps, accum, partials);
}

template <class T>
int radial_cols_impl(bjx_ctx* ctx, int inverse, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a, int64_t ld_b, int64_t ld_z, int L,
                     const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1, grid = 0;
  radial_cols_shape<T>(dim, &G, &R);
  const RadialColsArgs<T> a = radial_cols_args<T>(ctx, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, L, dim, batch, G, kThreads, &grid);
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  const bool al = radial_cols_vector_form<T>(dim, ld_z, {p_z0, in, out});
  {
    BjxProf prof_(ctx);
#define RCM(R_) do { if (al) launch_map<T, R_, true>(ctx, a, grid, inverse, in, out, ladj_ps, accum, partials); \
                     else launch_map<T, R_, false>(ctx, a, grid, inverse, in, out, ladj_ps, accum, partials); } while (0)
    switch (R) {
      case 1: RCM(1); break;
      case 2: RCM(2); break;
      default: RCM(4); break;
    }
#undef RCM
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T, int R, bool AL>
void launch_vjp(bjx_ctx* ctx, const RadialColsArgs<T>& a, int grid, int threads, size_t smem, int inverse, const T* in, const T* gb, const T* lb, T* xb, T* ab,
                T* bb, T* zb) {
  constexpr int V = Vec16<T>::N;
  if (inverse) hipLaunchKernelGGL((radial_cols_vjp_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3((unsigned)threads), smem, ctx->stream, a, in, gb, lb, xb, ab, bb, zb);
  else hipLaunchKernelGGL((radial_cols_vjp_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3((unsigned)threads), smem, ctx->stream, a, in, gb, lb, xb, ab, bb, zb);
}

template <class T>
int radial_cols_vjp_impl(bjx_ctx* ctx, int inverse, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a, int64_t ld_b, int64_t ld_z, int L,
                         const T* in, const T* gb, const T* lb, T* xb, T* ab, T* bb, T* zb, int64_t dim, int64_t batch) {
  if (batch == 0) return BJX_OK;
  int G = 1, R = 1, grid = 0;
  radial_cols_shape<T>(dim, &G, &R);
  // the r table [L][C] of the forward pullback: above 64 KiB with 256 threads (short columns, many layers) the block is one wave;
  // the inverse pullback recomputes r_k from the resident column and has no table
  int threads = kThreads;
  size_t smem = 0;
  if (!inverse) {
    if ((size_t)L * (kThreads / G) * sizeof(T) > 64 * 1024) threads = 64;
    smem = ((size_t)L * (threads / G) * sizeof(T) + 15) & ~(size_t)15;
  }
  const RadialColsArgs<T> a = radial_cols_args<T>(ctx, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, L, dim, batch, G, threads, &grid);
  const bool al = radial_cols_vector_form<T>(dim, ld_z, {p_z0, in, gb, xb, zb});
  {
    BjxProf prof_(ctx);
#define RCV(R_) do { if (al) launch_vjp<T, R_, true>(ctx, a, grid, threads, smem, inverse, in, gb, lb, xb, ab, bb, zb); \
                     else launch_vjp<T, R_, false>(ctx, a, grid, threads, smem, inverse, in, gb, lb, xb, ab, bb, zb); } while (0)
    switch (R) {
      case 1: RCV(1); break;
      case 2: RCV(2); break;
      default: RCV(4); break;
    }
#undef RCV
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_radial_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a, int64_t ld_b,
                            int64_t ld_z, int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = radial_cols_check(ctx, "bjx_radial_cols", dt, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_radial_cols: null pointer");
  if (dt == BJX_F32)
    return radial_cols_impl<float>(ctx, inverse, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, n_layers, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return radial_cols_impl<double>(ctx, inverse, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, n_layers, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_radial_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_alpha, const void* p_beta, const void* p_z0, int64_t ld_a, int64_t ld_b,
                                int64_t ld_z, int n_layers, const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* alpha_bar,
                                void* beta_bar, void* z0_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = radial_cols_check(ctx, "bjx_radial_cols_vjp", dt, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out_bar && in_bar) || batch == 0, BJX_ERR_ARG, "bjx_radial_cols_vjp: null pointer");
  if (dt == BJX_F32)
    return radial_cols_vjp_impl<float>(ctx, inverse, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, n_layers, (const float*)in, (const float*)out_bar,
                                       (const float*)ladj_bar, (float*)in_bar, (float*)alpha_bar, (float*)beta_bar, (float*)z0_bar, dim, batch);
  return radial_cols_vjp_impl<double>(ctx, inverse, p_alpha, p_beta, p_z0, ld_a, ld_b, ld_z, n_layers, (const double*)in, (const double*)out_bar,
                                      (const double*)ladj_bar, (double*)in_bar, (double*)alpha_bar, (double*)beta_bar, (double*)z0_bar, dim, batch);
}
