// bjx_householder_cols.hip — a product of Householder reflections with one vector set per COLUMN, behind an optional per-column
// diagonal scale exp(s) and in front of an optional per-column shift m (include/bjx_householder_cols.h): the amortised Householder
// flow (Tomczak & Welling, 2016), whose parameters an encoder emits per sample and which therefore stream with the data.
//
// Mapping (the one of bjx_radial_cols.hip, unchanged): V = 16 B / sizeof(T) elements per pack, packs = ceil(dim / V); a column gets
// G lanes (G = the power of two >= packs, at most 64) and lane j of the group holds the packs j, j + G, ... (R of them, R = 1, 2 or 4;
// three packs per lane run the R = 4 kernels with a dead pack): 1 024 rows in Float32, 512 in Float64.  A 256-thread block owns
// C = 256/G columns at a time and walks column groups grid-stride over a capped grid.  A lane group never spans two waves, so the
// dot products of a layer are one butterfly and no kernel has a barrier in its column loop.
//
// Two forms of every kernel: 16-byte vector accesses when dim is a whole number of packs, every base pointer is 16-byte aligned
// and every present column stride is a multiple of V; the element form otherwise (packs on element-aligned addresses, the last one
// partial, dead rows read as zero: v = 0 there, so they leave every sum alone).
//
// One step: t = 2/vᵀv (read as 0 where vᵀv == 0 exactly: `s == 0 ? 0 : 2/s`, so a NaN in v stays a NaN), z ← z − t(vᵀz)v.  A reflection
// is its own inverse, so the inverse map is the same step walked k = L−1 … 0, and the reverse sweep of either pullback REWINDS the
// resident column exactly (z_k = H_k z_{k+1}) instead of storing L columns: no table, no LDS beyond the 8 doubles of the partials,
// one launch in either direction.  A reverse step, with the column holding the step's output z⁺ and g the carried cotangent:
//   (s, a′, c) = (vᵀv, vᵀz⁺, vᵀg) in ONE three-value butterfly; a = −a′ (= vᵀz_k); z_k = z⁺ − t a′ v;
//   v̄ = −t (a g + c z_k − t a c v);  g ← g − t c v.
// Forward pullback: the primal sweep runs to z_L, m̄ = ȳ, the reverse sweep k = L−1 … 0 ends with the column at u = exp(s)⊙x and
// g = ū: s̄ = ū⊙u + ℓ̄, x̄ = ū⊙exp(s).  Inverse pullback: the primal sweep gives q = H_0⋯H_{L−1}(y − m) and x = exp(−s)⊙q;
// s̄ = −x⊙x̄ − ℓ̄, the seed is g = exp(−s)⊙x̄, the reverse sweep runs k = 0 … L−1, ȳ = g and m̄ = −g.
// Nothing is summed over columns, so there are no atomics; the summed log-det goes through the per-block partials +
// bjx_launch_finalize (fixed order: run-to-run identical bits).
#include "bjx_internal.h"
#include "../../include/bjx_householder_cols.h"
#include <initializer_list>
#include <type_traits>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"                                     // Pack, load_pack, load_pack_part, store_pack_part
#include "bjx_cols_lanes.inc"                                      // LanePacks, load_data, load_param, store_data

template <class T> struct HouseholderColsArgs {
  const T *pv, *ps, *pm;                                           // ps, pm: null = absent
  int64_t ldv, lds, ldm;
  int64_t dim, batch, groups;
  int L, G;
};

// three values through one butterfly (the sibling of group_sum2_rt: shares the wave-uniform branches)
template <class T> __device__ __forceinline__ void group_sum3_rt(T& a, T& b, T& c, int G) {
  for (int m = G >> 1; m >= 1; m >>= 1) { a += shfl_xor(a, m); b += shfl_xor(b, m); c += shfl_xor(c, m); }
}
template <> __device__ __forceinline__ void group_sum3_rt<float>(float& a, float& b, float& c, int G) {
  if (G >= 2) { a = dpp_xadd<0xB1>(a); b = dpp_xadd<0xB1>(b); c = dpp_xadd<0xB1>(c); }
  if (G >= 4) { a = dpp_xadd<0x4E>(a); b = dpp_xadd<0x4E>(b); c = dpp_xadd<0x4E>(c); }
  if (G >= 8) { a = dpp_xadd<0x141>(a); b = dpp_xadd<0x141>(b); c = dpp_xadd<0x141>(c); }
  if (G >= 16) { a = dpp_xadd<0x140>(a); b = dpp_xadd<0x140>(b); c = dpp_xadd<0x140>(c); }
  if (G >= 32) { a += shfl_xor(a, 16); b += shfl_xor(b, 16); c += shfl_xor(c, 16); }
  if (G >= 64) { a += shfl_xor(a, 32); b += shfl_xor(b, 32); c += shfl_xor(c, 32); }
}

// t = 2/vᵀv, read as 0 at vᵀv == 0 exactly (NOT `s > 0 ? … : 0`: a NaN must stay a NaN)
template <class T> __device__ __forceinline__ T hh_tau(T ss) { return ss == T(0) ? T(0) : T(2) / ss; }

// z ← z − t(vᵀz)v for the layers in the order of the direction (INV: L−1 … 0).  Contraction is off here too: the primal sweep of
// the pullbacks is this one, and the maps are bound by memory, not by the three multiply-adds per element and layer
template <class T, int V, int R, bool AL, bool INV>
__device__ __forceinline__ void hh_sweep(const T* vc, const LanePacks<V, R>& lp, Pack<T, V> (&z)[R], int L, int G, int64_t dim) {
#pragma clang fp contract(off)
  for (int li = 0; li < L; ++li) {
    const int k = INV ? L - 1 - li : li;
    Pack<T, V> v[R];
    load_param<T, V, R, AL>(vc + (int64_t)k * dim, lp, v);
    T ss = T(0), a = T(0);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) { ss += v[r].v[j] * v[r].v[j]; a += v[r].v[j] * z[r].v[j]; }
    group_sum2_rt(ss, a, G);
    const T ta = hh_tau(ss) * a;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) z[r].v[j] -= ta * v[r].v[j];
  }
}

// ------------------------------------------------------------------ the map and its inverse
// (x and y may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them)
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void householder_cols_map_kernel(const HouseholderColsArgs<T> a, const T* x, T* y, T* __restrict__ ladj_ps, int accumulate,
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
    T ladj = T(0);
    if constexpr (!INV) {
      if (a.ps) {
        Pack<T, V> s[R];
        load_param<T, V, R, AL>(a.ps + col * a.lds, lp, s);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) { ladj += s[r].v[j]; z[r].v[j] *= d_exp(s[r].v[j]); }
        ladj = group_sum_rt(ladj, G);
      }
    } else if (a.pm) {
      Pack<T, V> m[R];
      load_param<T, V, R, AL>(a.pm + col * a.ldm, lp, m);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) z[r].v[j] -= m[r].v[j];
    }
    hh_sweep<T, V, R, AL, INV>(a.pv + col * a.ldv, lp, z, L, G, dim);
    if constexpr (!INV) {
      if (a.pm) {
        Pack<T, V> m[R];
        load_param<T, V, R, AL>(a.pm + col * a.ldm, lp, m);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) z[r].v[j] += m[r].v[j];
      }
    } else if (a.ps) {
      Pack<T, V> s[R];
      load_param<T, V, R, AL>(a.ps + col * a.lds, lp, s);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) { ladj -= s[r].v[j]; z[r].v[j] *= d_exp(-s[r].v[j]); }
      ladj = group_sum_rt(ladj, G);
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
// x̄ (INV: ȳ) and the per-column (v̄, s̄, m̄) of the map or of its inverse (any of the three may be null).
// (gbar and xbar may be the same buffer, as x and y above.)  Contraction is off: x̄ must not depend on which outputs were asked
// for or on the form the dispatcher chose.
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void householder_cols_vjp_kernel(const HouseholderColsArgs<T> a, const T* x, const T* gbar, const T* __restrict__ lbar, T* xbar,
                                                                   T* __restrict__ vbar, T* __restrict__ sbar, T* __restrict__ mbar) {
#pragma clang fp contract(off)
  const int G = a.G, C = (int)blockDim.x / G, L = a.L;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;
    const T* vc = a.pv + col * a.ldv;
    const T lb = lbar ? lbar[col] : T(0);
    Pack<T, V> z[R], g[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    // ---- primal sweep.  Forward: u = exp(s)⊙x, then to z_L.  Inverse: y − m, then down to q = H_0⋯H_{L−1}(y − m).
    if constexpr (!INV) {
      if (a.ps) {
        Pack<T, V> s[R];
        load_param<T, V, R, AL>(a.ps + col * a.lds, lp, s);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) z[r].v[j] *= d_exp(s[r].v[j]);
      }
    } else if (a.pm) {
      Pack<T, V> m[R];
      load_param<T, V, R, AL>(a.pm + col * a.ldm, lp, m);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) z[r].v[j] -= m[r].v[j];
    }
    hh_sweep<T, V, R, AL, INV>(vc, lp, z, L, G, dim);
    // ---- the seed of the reverse sweep
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    if constexpr (!INV) {
      if (mbar && live) store_data<T, V, R, AL>(mbar + col * dim, lp, g);          // m̄ = ȳ
    } else if (a.ps) {                                             // x = exp(−s)⊙q: s̄ = −x⊙x̄ − ℓ̄, g = exp(−s)⊙x̄
      Pack<T, V> s[R];
      load_param<T, V, R, AL>(a.ps + col * a.lds, lp, s);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T e = d_exp(-s[r].v[j]);
          s[r].v[j] = -((e * z[r].v[j]) * g[r].v[j]) - lb;
          g[r].v[j] = e * g[r].v[j];
        }
      if (sbar && live) store_data<T, V, R, AL>(sbar + col * dim, lp, s);
    }
    // ---- reverse sweep: the column holds the OUTPUT of layer k and is rewound to its input
    for (int li = 0; li < L; ++li) {
      const int k = INV ? li : L - 1 - li;
      Pack<T, V> v[R];
      load_param<T, V, R, AL>(vc + (int64_t)k * dim, lp, v);
      T ss = T(0), ap = T(0), c = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          ss = ss + v[r].v[j] * v[r].v[j];
          ap = ap + v[r].v[j] * z[r].v[j];
          c = c + v[r].v[j] * g[r].v[j];
        }
      group_sum3_rt(ss, ap, c, G);
      const T t = hh_tau(ss);
      const T aa = -ap;                                            // vᵀz_k
      const T tap = t * ap, tc = t * c, tac = t * aa * c;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T vv = v[r].v[j], gg = g[r].v[j];
          const T zk = z[r].v[j] - tap * vv;
          z[r].v[j] = zk;
          g[r].v[j] = gg - tc * vv;
          v[r].v[j] = -t * (aa * gg + c * zk - tac * vv);          // v̄_k
        }
      if (vbar && live) store_data<T, V, R, AL>(vbar + (col * L + k) * dim, lp, v);
    }
    // ---- the head
    if constexpr (!INV) {
      if (a.ps) {                                                  // the column holds u, g holds ū
        Pack<T, V> s[R];
        load_param<T, V, R, AL>(a.ps + col * a.lds, lp, s);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T e = d_exp(s[r].v[j]);
            s[r].v[j] = g[r].v[j] * z[r].v[j] + lb;
            g[r].v[j] = g[r].v[j] * e;
          }
        if (sbar && live) store_data<T, V, R, AL>(sbar + col * dim, lp, s);
      }
      if (live) store_data<T, V, R, AL>(xbar + col * dim, lp, g);
    } else if (live) {
      store_data<T, V, R, AL>(xbar + col * dim, lp, g);            // ȳ = g
      if (mbar) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) g[r].v[j] = -g[r].v[j];
        store_data<T, V, R, AL>(mbar + col * dim, lp, g);          // m̄ = −g
      }
    }
  }
}

// ------------------------------------------------------------------ host side
constexpr int kThreads = 256;
constexpr int kBlocksPerCu = 8;

int householder_cols_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v, int64_t ld_s,
                           int64_t ld_m, int n_layers, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, n_layers >= 1 && n_layers <= BJX_HOUSEHOLDER_COLS_MAX_LAYERS, BJX_ERR_UNSUPPORTED, "%s: %d layers (1 ... %d supported)", name, n_layers,
              BJX_HOUSEHOLDER_COLS_MAX_LAYERS);
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0, BJX_ERR_SHAPE, "%s: bad size (dim=%lld, batch=%lld)", name, (long long)dim, (long long)batch);
  const int64_t lim = dt == BJX_F32 ? 1024 : 512;
  BJX_REQUIRE(ctx, dim <= lim, BJX_ERR_UNSUPPORTED, "%s: dim %lld above the %lld rows a lane group holds in %s", name, (long long)dim, (long long)lim,
              dt == BJX_F32 ? "Float32" : "Float64");
  BJX_REQUIRE(ctx, ld_v >= dim * n_layers && (!p_s || ld_s >= dim) && (!p_m || ld_m >= dim), BJX_ERR_SHAPE,
              "%s: column strides (%lld, %lld, %lld) below dim x n_layers = %lld and dim = %lld", name, (long long)ld_v, (long long)ld_s, (long long)ld_m,
              (long long)(dim * n_layers), (long long)dim);
  BJX_REQUIRE(ctx, batch == 0 || p_v, BJX_ERR_ARG, "%s: null parameter pointer", name);
  return BJX_OK;
}

// lanes per column, packs per lane
template <class T> void householder_cols_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T>
HouseholderColsArgs<T> householder_cols_args(const bjx_ctx* ctx, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v, int64_t ld_s, int64_t ld_m, int L,
                                             int64_t dim, int64_t batch, int G, int* grid) {
  HouseholderColsArgs<T> a{};
  a.pv = (const T*)p_v; a.ps = (const T*)p_s; a.pm = (const T*)p_m;
  a.ldv = ld_v; a.lds = p_s ? ld_s : 0; a.ldm = p_m ? ld_m : 0;
  a.dim = dim; a.batch = batch; a.L = L; a.G = G;
  const int C = kThreads / G;
  a.groups = (batch + C - 1) / C;
  const int64_t cap = (int64_t)ctx->num_cu * kBlocksPerCu;
  *grid = (int)(a.groups < cap ? a.groups : cap);
  return a;
}

// (the ld of an absent parameter was set to 0 above: it passes)
template <class T> bool householder_cols_vector_form(const HouseholderColsArgs<T>& a, std::initializer_list<const void*> ptrs) {
  constexpr int V = Vec16<T>::N;
  if (a.dim % V || a.ldv % V || a.lds % V || a.ldm % V) return false;
  for (const void* p : ptrs)
    if (p && !bjx_aligned16(p)) return false;
  return true;
}

template <class T, int R, bool AL>
void launch_map(bjx_ctx* ctx, const HouseholderColsArgs<T>& a, int grid, int inverse, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
  constexpr int V = Vec16<T>::N;
  const size_t smem = 8 * sizeof(double);
  if (inverse) hipLaunchKernelGGL((householder_cols_map_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, in, out, ladj_ps, accum, partials);
  else hipLaunchKernelGGL((householder_cols_map_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, in, out, ladj_ps, accum, partials);
}

template <class T>
int householder_cols_impl(bjx_ctx* ctx, int inverse, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v, int64_t ld_s, int64_t ld_m, int L,
                          const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1, grid = 0;
  householder_cols_shape<T>(dim, &G, &R);
  const HouseholderColsArgs<T> a = householder_cols_args<T>(ctx, p_v, p_s, p_m, ld_v, ld_s, ld_m, L, dim, batch, G, &grid);
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  const bool al = householder_cols_vector_form<T>(a, {p_v, p_s, p_m, in, out});
  {
    BjxProf prof_(ctx);
#define HCM(R_) do { if (al) launch_map<T, R_, true>(ctx, a, grid, inverse, in, out, ladj_ps, accum, partials); \
                     else launch_map<T, R_, false>(ctx, a, grid, inverse, in, out, ladj_ps, accum, partials); } while (0)
    switch (R) {
      case 1: HCM(1); break;
      case 2: HCM(2); break;
      default: HCM(4); break;
    }
#undef HCM
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T, int R, bool AL>
void launch_vjp(bjx_ctx* ctx, const HouseholderColsArgs<T>& a, int grid, int inverse, const T* in, const T* gb, const T* lb, T* xb, T* vb, T* sb, T* mb) {
  constexpr int V = Vec16<T>::N;
  if (inverse) hipLaunchKernelGGL((householder_cols_vjp_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a, in, gb, lb, xb, vb, sb, mb);
  else hipLaunchKernelGGL((householder_cols_vjp_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a, in, gb, lb, xb, vb, sb, mb);
}

template <class T>
int householder_cols_vjp_impl(bjx_ctx* ctx, int inverse, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v, int64_t ld_s, int64_t ld_m, int L,
                              const T* in, const T* gb, const T* lb, T* xb, T* vb, T* sb, T* mb, int64_t dim, int64_t batch) {
  if (batch == 0) return BJX_OK;
  int G = 1, R = 1, grid = 0;
  householder_cols_shape<T>(dim, &G, &R);
  const HouseholderColsArgs<T> a = householder_cols_args<T>(ctx, p_v, p_s, p_m, ld_v, ld_s, ld_m, L, dim, batch, G, &grid);
  const bool al = householder_cols_vector_form<T>(a, {p_v, p_s, p_m, in, gb, xb, vb, sb, mb});
  {
    BjxProf prof_(ctx);
#define HCV(R_) do { if (al) launch_vjp<T, R_, true>(ctx, a, grid, inverse, in, gb, lb, xb, vb, sb, mb); \
                     else launch_vjp<T, R_, false>(ctx, a, grid, inverse, in, gb, lb, xb, vb, sb, mb); } while (0)
    switch (R) {
      case 1: HCV(1); break;
      case 2: HCV(2); break;
      default: HCV(4); break;
    }
#undef HCV
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_householder_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v, int64_t ld_s,
                                 int64_t ld_m, int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = householder_cols_check(ctx, "bjx_householder_cols", dt, p_v, p_s, p_m, ld_v, ld_s, ld_m, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_householder_cols: null pointer");
  if (dt == BJX_F32)
    return householder_cols_impl<float>(ctx, inverse, p_v, p_s, p_m, ld_v, ld_s, ld_m, n_layers, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return householder_cols_impl<double>(ctx, inverse, p_v, p_s, p_m, ld_v, ld_s, ld_m, n_layers, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_householder_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* p_v, const void* p_s, const void* p_m, int64_t ld_v, int64_t ld_s,
                                     int64_t ld_m, int n_layers, const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* v_bar,
                                     void* s_bar, void* m_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = householder_cols_check(ctx, "bjx_householder_cols_vjp", dt, p_v, p_s, p_m, ld_v, ld_s, ld_m, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (p_s || !s_bar) && (p_m || !m_bar), BJX_ERR_ARG, "bjx_householder_cols_vjp: a cotangent output of an absent parameter");
  BJX_REQUIRE(ctx, (in && out_bar && in_bar) || batch == 0, BJX_ERR_ARG, "bjx_householder_cols_vjp: null pointer");
  if (dt == BJX_F32)
    return householder_cols_vjp_impl<float>(ctx, inverse, p_v, p_s, p_m, ld_v, ld_s, ld_m, n_layers, (const float*)in, (const float*)out_bar,
                                            (const float*)ladj_bar, (float*)in_bar, (float*)v_bar, (float*)s_bar, (float*)m_bar, dim, batch);
  return householder_cols_vjp_impl<double>(ctx, inverse, p_v, p_s, p_m, ld_v, ld_s, ld_m, n_layers, (const double*)in, (const double*)out_bar,
                                           (const double*)ladj_bar, (double*)in_bar, (double*)v_bar, (double*)s_bar, (double*)m_bar, dim, batch);
}
