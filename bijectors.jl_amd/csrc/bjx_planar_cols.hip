// bjx_planar_cols.hip — a stack of PlanarLayers with one parameter set (w, u, b) per COLUMN (include/bjx_planar_cols.h): the
// amortised planar flow, whose parameters an encoder emits per sample and which therefore stream with the data.
//
// Mapping: V = 16 B / sizeof(T) elements per pack, packs = ceil(dim / V); a column gets G lanes (G = the power of two >= packs,
// at most 64) and lane j of the group holds the packs j, j + G, ... (R of them, R = 1, 2 or 4; three packs per lane run the R = 4
// kernels with a dead pack): 1 024 rows in Float32, 512 in Float64.  Every group reads G·16 contiguous bytes of a column.  A
// 256-thread block owns C = 256/G columns at a time and walks column groups grid-stride over a capped grid.  A lane group
// never spans two waves, so the sums of a layer are one butterfly and no kernel has a barrier in its column loop.
//
// Two forms of every kernel: 16-byte vector accesses when dim is a whole number of packs, every base pointer is 16-byte aligned
// and the column strides of w and u are multiples of V; the element form otherwise (load_pack_part / store_pack_part: packs
// on element-aligned addresses, the last one partial, dead rows read as zero and so leave every sum alone).
//
// Per layer the three sums wᵀu, ‖w‖², wᵀz go through one butterfly; κ = (log1pexp(−wᵀu) − 1)/‖w‖² and c = log1pexp(wᵀu) − 1
// are get_u_hat (planar_layer.jl:65-70) in registers, û = u + κw is never stored.  The forward pullback saves t_k per column in
// a dynamic-LDS table [L][C], then walks the layers backwards re-reading w_k, u_k (through the caches) and REWINDS the
// resident column, z_k = z_{k+1} − û_k t_k, instead of storing L columns; the closed forms of the batch-summed parameter pullback
// (bjx_planar_vjp_params) are written per column.  The inverse pullback is the implicit-function rule of bjx_planar_vjp.
// Every lane of a group writes the group's (bit-identical) t_k to the group's slot and reads that slot back: no lane depends
// on another lane's LDS write.  Nothing is summed over columns, so there are no atomics; the summed log-det goes through the
// per-block partials + bjx_launch_finalize (fixed order: run-to-run identical bits).
#include "bjx_internal.h"
#include "../../include/bjx_planar_cols.h"
#include <type_traits>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"

template <class T> struct PlanarColsArgs {
  const T *pw, *pu, *pb;
  int64_t ldw, ldu, ldb;
  int64_t dim, batch, groups;
  int L, G;
};

// three / four values through one butterfly (shares the wave-uniform branches, as group_sum2_rt)
template <class T> __device__ __forceinline__ void group_sum3_rt(T& a, T& b, T& c, int G) {
  a = group_sum_rt(a, G); b = group_sum_rt(b, G); c = group_sum_rt(c, G);
}
template <> __device__ __forceinline__ void group_sum3_rt<float>(float& a, float& b, float& c, int G) {
  if (G >= 2) { a = dpp_xadd<0xB1>(a); b = dpp_xadd<0xB1>(b); c = dpp_xadd<0xB1>(c); }
  if (G >= 4) { a = dpp_xadd<0x4E>(a); b = dpp_xadd<0x4E>(b); c = dpp_xadd<0x4E>(c); }
  if (G >= 8) { a = dpp_xadd<0x141>(a); b = dpp_xadd<0x141>(b); c = dpp_xadd<0x141>(c); }
  if (G >= 16) { a = dpp_xadd<0x140>(a); b = dpp_xadd<0x140>(b); c = dpp_xadd<0x140>(c); }
  if (G >= 32) { a += shfl_xor(a, 16); b += shfl_xor(b, 16); c += shfl_xor(c, 16); }
  if (G >= 64) { a += shfl_xor(a, 32); b += shfl_xor(b, 32); c += shfl_xor(c, 32); }
}
template <class T> __device__ __forceinline__ void group_sum4_rt(T& a, T& b, T& c, T& d, int G) {
  group_sum2_rt(a, b, G);
  group_sum2_rt(c, d, G);
}

#include "bjx_cols_lanes.inc"                                     // LanePacks, load_data, load_param, store_data

// ------------------------------------------------------------------ the map and its inverse
// (x and y may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them)
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void planar_cols_map_kernel(const PlanarColsArgs<T> a, const T* x, T* y, T* __restrict__ ladj_ps, int accumulate,
                                                              double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* redd = reinterpret_cast<double*>(smem);
  const int G = a.G, C = (int)blockDim.x / G, L = a.L;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  double acc = 0.0;
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;       // a group past the batch works on the last column and stores nothing
    Pack<T, V> z[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    const T* wc = a.pw + col * a.ldw;
    const T* uc = a.pu + col * a.ldu;
    const T* bc = a.pb + col * a.ldb;
    T ladj = T(0);
    for (int li = 0; li < L; ++li) {
      const int k = INV ? L - 1 - li : li;
      Pack<T, V> w[R], u[R];
      load_param<T, V, R, AL>(wc + (int64_t)k * dim, lp, w);
      load_param<T, V, R, AL>(uc + (int64_t)k * dim, lp, u);
      const T bk = bc[k];
      T wu = T(0), ww = T(0), wz = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          wu += w[r].v[j] * u[r].v[j];
          ww += w[r].v[j] * w[r].v[j];
          wz += w[r].v[j] * z[r].v[j];
        }
      group_sum3_rt(wu, ww, wz, G);
      const T kap = (d_log1pexp(-wu) - T(1)) / ww;               // planar_layer.jl:65-70: û = u + κ w
      const T c = d_log1pexp(wu) - T(1);                         // wᵀû
      T t, s2;
      if constexpr (!INV) flow_tanh_sech2(wz + bk, t, s2);
      else planar_inv_act<T>(wz, c, bk, t, s2);                  // find_alpha, :112-127
      const T ld = Fast<T>::log1p(c * s2);                       // :107
      ladj += INV ? -ld : ld;
      const T tt = INV ? -t : t;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) z[r].v[j] += (u[r].v[j] + kap * w[r].v[j]) * tt;
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
// INV = false: x̄ and the per-column (w̄, ū, b̄) (any of the three may be null).  INV = true: ȳ of the inverse only.
// (gbar and xbar may be the same buffer, as x and y above)
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void planar_cols_vjp_kernel(const PlanarColsArgs<T> a, const T* x, const T* gbar, const T* __restrict__ lbar, T* xbar,
                                                              T* __restrict__ wbar, T* __restrict__ ubar, T* __restrict__ bbar) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* tab = reinterpret_cast<T*>(smem);                           // [L][C]: t_k of the block's columns
  const int G = a.G, C = (int)blockDim.x / G, L = a.L;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;
    Pack<T, V> z[R], g[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    const T* wc = a.pw + col * a.ldw;
    const T* uc = a.pu + col * a.ldu;
    const T* bc = a.pb + col * a.ldb;
    // ---- primal sweep: t_k of every layer (forward: up to the output; inverse: down to the pre-image)
    for (int li = 0; li < L; ++li) {
      const int k = INV ? L - 1 - li : li;
      Pack<T, V> w[R], u[R];
      load_param<T, V, R, AL>(wc + (int64_t)k * dim, lp, w);
      load_param<T, V, R, AL>(uc + (int64_t)k * dim, lp, u);
      const T bk = bc[k];
      T wu = T(0), ww = T(0), wz = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          wu += w[r].v[j] * u[r].v[j];
          ww += w[r].v[j] * w[r].v[j];
          wz += w[r].v[j] * z[r].v[j];
        }
      group_sum3_rt(wu, ww, wz, G);
      const T kap = (d_log1pexp(-wu) - T(1)) / ww;
      T t;
      if constexpr (!INV) t = flow_tanh(wz + bk);
      else { T s2; planar_inv_act<T>(wz, d_log1pexp(wu) - T(1), bk, t, s2); }
      tab[k * C + cl] = t;
      const T tt = INV ? -t : t;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) z[r].v[j] += (u[r].v[j] + kap * w[r].v[j]) * tt;
    }
    // ---- reverse sweep on the cotangent
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    const T lb = lbar ? lbar[col] : T(0);
    for (int li = 0; li < L; ++li) {
      const int k = INV ? li : L - 1 - li;
      Pack<T, V> w[R], u[R];
      load_param<T, V, R, AL>(wc + (int64_t)k * dim, lp, w);
      load_param<T, V, R, AL>(uc + (int64_t)k * dim, lp, u);
      T wu = T(0), ww = T(0), wg = T(0), ug = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          wu += w[r].v[j] * u[r].v[j];
          ww += w[r].v[j] * w[r].v[j];
          wg += w[r].v[j] * g[r].v[j];
          ug += u[r].v[j] * g[r].v[j];
        }
      group_sum4_rt(wu, ww, wg, ug, G);
      const T kap = (d_log1pexp(-wu) - T(1)) / ww;
      const T c = d_log1pexp(wu) - T(1);
      const T t = tab[k * C + cl];
      const T q = T(1) - t * t;
      const T den = T(1) + c * q;
      const T uhg = ug + kap * wg;                               // ûᵀ z̄
      if constexpr (INV) {
        const T sbar = q / den * (-uhg + lb * T(2) * c * t / den);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) g[r].v[j] += w[r].v[j] * sbar;
      } else {
        const T sbar = uhg * q + lb * c * (T(-2) * t) * q / den;
        const T cb = lb * q / den;                               // c̄
        const T en = d_exp(-d_abs(wu));                          // σ(±a) from one exp
        const T s_hi = T(1) / (T(1) + en), s_lo = en / (T(1) + en);
        const T sig_pos = wu >= T(0) ? s_hi : s_lo, sig_neg = wu >= T(0) ? s_lo : s_hi;
        const T ka = -sig_neg / ww;                              // ∂κ/∂a
        const T wtuhb = wg * t;                                  // wᵀû̄ with û̄ = z̄ t
        const T mix = ka * wtuhb + cb * sig_pos;                 // the weight of w in ū and of u in w̄
        const T cww = T(-2) * kap / ww * wtuhb;
        Pack<T, V> wb[R], ub[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T wv = w[r].v[j], uv = u[r].v[j];
            z[r].v[j] -= (uv + kap * wv) * t;                    // rewind: the input of layer k
            const T uhb = g[r].v[j] * t;
            ub[r].v[j] = uhb + wv * mix;
            wb[r].v[j] = z[r].v[j] * sbar + kap * uhb + mix * uv + cww * wv;
            g[r].v[j] += wv * sbar;
          }
        if (live) {
          const int64_t o = (col * L + k) * dim;
          if (wbar) store_data<T, V, R, AL>(wbar + o, lp, wb);
          if (ubar) store_data<T, V, R, AL>(ubar + o, lp, ub);
          if (bbar && gl == 0) bbar[col * L + k] = sbar;
        }
      }
    }
    if (live) store_data<T, V, R, AL>(xbar + col * dim, lp, g);
  }
}

// ------------------------------------------------------------------ host side
constexpr int kThreads = 256;
constexpr int kBlocksPerCu = 8;

int planar_cols_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w, int64_t ld_u,
                      int64_t ld_b, int n_layers, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, n_layers >= 1 && n_layers <= BJX_PLANAR_COLS_MAX_LAYERS, BJX_ERR_UNSUPPORTED, "%s: %d layers (1 ... %d supported)", name, n_layers,
              BJX_PLANAR_COLS_MAX_LAYERS);
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0, BJX_ERR_SHAPE, "%s: bad size (dim=%lld, batch=%lld)", name, (long long)dim, (long long)batch);
  const int64_t lim = dt == BJX_F32 ? 1024 : 512;
  BJX_REQUIRE(ctx, dim <= lim, BJX_ERR_UNSUPPORTED, "%s: dim %lld above the %lld rows a lane group holds in %s", name, (long long)dim, (long long)lim,
              dt == BJX_F32 ? "Float32" : "Float64");
  BJX_REQUIRE(ctx, ld_w >= dim * n_layers && ld_u >= dim * n_layers && ld_b >= n_layers, BJX_ERR_SHAPE,
              "%s: column strides (%lld, %lld, %lld) below dim x n_layers = %lld and n_layers = %d", name, (long long)ld_w, (long long)ld_u, (long long)ld_b,
              (long long)(dim * n_layers), n_layers);
  BJX_REQUIRE(ctx, batch == 0 || (p_w && p_u && p_b), BJX_ERR_ARG, "%s: null parameter pointer", name);
  return BJX_OK;
}

// lanes per column, packs per lane
template <class T> void planar_cols_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T>
PlanarColsArgs<T> planar_cols_args(const bjx_ctx* ctx, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w, int64_t ld_u, int64_t ld_b, int L,
                                   int64_t dim, int64_t batch, int G, int threads, int* grid) {
  PlanarColsArgs<T> a{};
  a.pw = (const T*)p_w; a.pu = (const T*)p_u; a.pb = (const T*)p_b;
  a.ldw = ld_w; a.ldu = ld_u; a.ldb = ld_b;
  a.dim = dim; a.batch = batch; a.L = L; a.G = G;
  const int C = threads / G;
  a.groups = (batch + C - 1) / C;
  const int64_t cap = (int64_t)ctx->num_cu * kBlocksPerCu * (kThreads / threads);
  *grid = (int)(a.groups < cap ? a.groups : cap);
  return a;
}

template <class T> bool planar_cols_vector_form(int64_t dim, int64_t ld_w, int64_t ld_u, std::initializer_list<const void*> ptrs) {
  constexpr int V = Vec16<T>::N;
  if (dim % V || ld_w % V || ld_u % V) return false;
  for (const void* p : ptrs)
    if (p && !bjx_aligned16(p)) return false;
  return true;
}

template <class T, int R, bool AL>
void launch_map(bjx_ctx* ctx, const PlanarColsArgs<T>& a, int grid, int inverse, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
  constexpr int V = Vec16<T>::N;
  const size_t smem = 8 * sizeof(double);
  if (inverse) hipLaunchKernelGGL((planar_cols_map_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, in, out, ladj_ps, accum, partials);
  else hipLaunchKernelGGL((planar_cols_map_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, in, out, ladj_ps, accum, partials);
}

template <class T>
int planar_cols_impl(bjx_ctx* ctx, int inverse, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w, int64_t ld_u, int64_t ld_b, int L, const T* in,
                     T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1, grid = 0;
  planar_cols_shape<T>(dim, &G, &R);
  const PlanarColsArgs<T> a = planar_cols_args<T>(ctx, p_w, p_u, p_b, ld_w, ld_u, ld_b, L, dim, batch, G, kThreads, &grid);
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  const bool al = planar_cols_vector_form<T>(dim, ld_w, ld_u, {p_w, p_u, in, out});
  {
    BjxProf prof_(ctx);
#define PCM(R_) do { if (al) launch_map<T, R_, true>(ctx, a, grid, inverse, in, out, ladj_ps, accum, partials); \
                     else launch_map<T, R_, false>(ctx, a, grid, inverse, in, out, ladj_ps, accum, partials); } while (0)
    switch (R) {
      case 1: PCM(1); break;
      case 2: PCM(2); break;
      default: PCM(4); break;
    }
#undef PCM
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T, int R, bool AL>
void launch_vjp(bjx_ctx* ctx, const PlanarColsArgs<T>& a, int grid, int threads, size_t smem, int inverse, const T* in, const T* gb, const T* lb, T* xb, T* wb,
                T* ub, T* bb) {
  constexpr int V = Vec16<T>::N;
  if (inverse) hipLaunchKernelGGL((planar_cols_vjp_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3((unsigned)threads), smem, ctx->stream, a, in, gb, lb, xb, wb, ub, bb);
  else hipLaunchKernelGGL((planar_cols_vjp_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3((unsigned)threads), smem, ctx->stream, a, in, gb, lb, xb, wb, ub, bb);
}

template <class T>
int planar_cols_vjp_impl(bjx_ctx* ctx, int inverse, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w, int64_t ld_u, int64_t ld_b, int L,
                         const T* in, const T* gb, const T* lb, T* xb, T* wb, T* ub, T* bb, int64_t dim, int64_t batch) {
  if (batch == 0) return BJX_OK;
  int G = 1, R = 1, grid = 0;
  planar_cols_shape<T>(dim, &G, &R);
  // the t table [L][C]: above 64 KiB with 256 threads (short columns, many layers) the block is one wave
  int threads = kThreads;
  if ((size_t)L * (kThreads / G) * sizeof(T) > 64 * 1024) threads = 64;
  const size_t smem = ((size_t)L * (threads / G) * sizeof(T) + 15) & ~(size_t)15;
  const PlanarColsArgs<T> a = planar_cols_args<T>(ctx, p_w, p_u, p_b, ld_w, ld_u, ld_b, L, dim, batch, G, threads, &grid);
  const bool al = planar_cols_vector_form<T>(dim, ld_w, ld_u, {p_w, p_u, in, gb, xb, wb, ub});
  {
    BjxProf prof_(ctx);
#define PCV(R_) do { if (al) launch_vjp<T, R_, true>(ctx, a, grid, threads, smem, inverse, in, gb, lb, xb, wb, ub, bb); \
                     else launch_vjp<T, R_, false>(ctx, a, grid, threads, smem, inverse, in, gb, lb, xb, wb, ub, bb); } while (0)
    switch (R) {
      case 1: PCV(1); break;
      case 2: PCV(2); break;
      default: PCV(4); break;
    }
#undef PCV
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_planar_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w, int64_t ld_u, int64_t ld_b,
                            int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = planar_cols_check(ctx, "bjx_planar_cols", dt, p_w, p_u, p_b, ld_w, ld_u, ld_b, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_planar_cols: null pointer");
  if (dt == BJX_F32)
    return planar_cols_impl<float>(ctx, inverse, p_w, p_u, p_b, ld_w, ld_u, ld_b, n_layers, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return planar_cols_impl<double>(ctx, inverse, p_w, p_u, p_b, ld_w, ld_u, ld_b, n_layers, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_planar_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_w, const void* p_u, const void* p_b, int64_t ld_w, int64_t ld_u,
                                int64_t ld_b, int n_layers, const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* w_bar, void* u_bar,
                                void* b_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = planar_cols_check(ctx, "bjx_planar_cols_vjp", dt, p_w, p_u, p_b, ld_w, ld_u, ld_b, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, !inverse || (!w_bar && !u_bar && !b_bar), BJX_ERR_ARG,
              "bjx_planar_cols_vjp: the inverse computes in_bar only (parameter cotangents: the forward pullback at the pre-image)");
  BJX_REQUIRE(ctx, (in && out_bar && in_bar) || batch == 0, BJX_ERR_ARG, "bjx_planar_cols_vjp: null pointer");
  if (dt == BJX_F32)
    return planar_cols_vjp_impl<float>(ctx, inverse, p_w, p_u, p_b, ld_w, ld_u, ld_b, n_layers, (const float*)in, (const float*)out_bar, (const float*)ladj_bar,
                                       (float*)in_bar, (float*)w_bar, (float*)u_bar, (float*)b_bar, dim, batch);
  return planar_cols_vjp_impl<double>(ctx, inverse, p_w, p_u, p_b, ld_w, ld_u, ld_b, n_layers, (const double*)in, (const double*)out_bar, (const double*)ladj_bar,
                                      (double*)in_bar, (double*)w_bar, (double*)u_bar, (double*)b_bar, dim, batch);
}
