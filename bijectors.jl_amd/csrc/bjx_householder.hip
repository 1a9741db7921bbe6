// bjx_householder.hip — a product of Householder reflections y = H_{L−1}⋯H_0 x with ONE vector set V = [v_0 … v_{L−1}] shared by every
// column (include/bjx_householder.h): the trainable orthogonal mixing layer between coupling layers.  The per-column sibling is
// bjx_householder_cols.hip; the lane geometry is the same (bjx_cols_lanes.inc): V = 16 B / sizeof(T) elements per pack, G lanes per
// column (the power of two >= the packs of a column, at most 64), R = 1, 2 or 4 packs per lane, a 256-thread block owns C = 256/G
// columns at a time; the vector form on whole packs and aligned pointers, the element form otherwise (dead rows read v = 0).
//
// t_k = 2/v_kᵀv_k (0 at v_kᵀv_k == 0 exactly) is a function of the parameters alone: every block computes the L of them ONCE, in its
// prologue (wave w takes the layers w, w + 4, …: 64 lanes over the rows, one butterfly), and keeps them in LDS.  A layer is then one
// group reduction per column (vᵀz) where the per-column sibling needs two values (vᵀv, vᵀz).
//
// V is read through the caches (load_param), not staged in LDS: it is at most 256 KiB, every column of every block reads the same
// L·dim elements, and the lane groups of a wave read the SAME addresses, so a layer's read is one L1 line set per wave.  The map
// kernels use no LDS beyond the t table; the pullback keeps its LDS for the Float64 tables below.
//
// Parameter pullback (one streaming pass over x and ȳ): the primal sweep runs to the last state, the reverse sweep rewinds the resident
// column (a reflection is its own inverse: z_k = H_k z_{k+1}; no table of states).  At layer k with the column at the step's OUTPUT z⁺
// and g the cotangent of that output:
//   (a′, c) = (vᵀz⁺, vᵀg) in one two-value butterfly;  a = −a′ (= vᵀz_k);  z_k = z⁺ − t a′ v;
//   S_k += a g + c z_k (dim entries),  q_k += a c;  g ← g − t c v.
// v̄_k = −t_k S_k + t_k² q_k v_k is formed by the last fold.  The sums over the batch stay ON CHIP in Float64: per tile and layer a
// shuffle butterfly over the column groups of a wave (lanes gl, gl + G, …), then the lanes of the wave's first group add into the
// wave's PRIVATE LDS table [L][dim + 1] — one writer per entry, no atomics.  Blocks are persistent; at the end of a block its four
// tables are added in a fixed order into ONE Float64 partial per BLOCK in the context's partials.  One or two fold launches add the
// partials in a fixed order (HH_FOLD_CHUNK block partials per thread of the first fold), form v̄ in Float64 and cast to T: at most three
// launches whatever L is, and the same call returns the same bits.
#include "bjx_internal.h"
#include "../../include/bjx_householder.h"
#include <initializer_list>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"                                     // Pack, load_pack, load_pack_part, store_pack_part
#include "bjx_cols_lanes.inc"                                      // LanePacks, load_data, load_param, store_data

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMapBlocksPerCu = 8;
constexpr int kParamBlocksPerCu = 4;          // the persistent grid of the pullback: at most 4 blocks per CU ...
constexpr int HH_TILES_MIN = 4;               // ... and at least 4 column tiles per block (one [L][dim + 1] partial per block)
constexpr int HH_FOLD_CHUNK = 32;             // block partials one thread of the first fold adds
constexpr size_t HH_LDS_BUDGET = BJX_HOUSEHOLDER_LDS_BUDGET;

// t = 2/vᵀv, read as 0 at vᵀv == 0 exactly (NOT `s > 0 ? … : 0`: a NaN must stay a NaN)
template <class T> __device__ __forceinline__ T hh_tau(T ss) { return ss == T(0) ? T(0) : T(2) / ss; }

// the block's prologue: tau[k] = t_k for every layer, then a barrier (it also publishes whatever the caller zeroed in LDS before)
template <class T> __device__ __forceinline__ void hh_tau_table(const T* __restrict__ v, int L, int64_t dim, T* tau) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = w; k < L; k += kWaves) {
    const T* vk = v + (int64_t)k * dim;
    T ss = T(0);
    for (int64_t r = lane; r < dim; r += 64) { const T e = vk[r]; ss += e * e; }
    for (int m = 32; m >= 1; m >>= 1) ss += shfl_xor(ss, m);
    if (lane == 0) tau[k] = hh_tau(ss);
  }
  __syncthreads();
}

// z ← z − t_k (v_kᵀz) v_k for the layers in the order of the direction (INV: L−1 … 0).  Contraction is off: the primal sweep of the
// pullback is this one, and x̄ of the pullback must be the bits of the other direction's map
template <class T, int V, int R, bool AL, bool INV>
__device__ __forceinline__ void hh_shared_sweep(const T* __restrict__ pv, const T* tau, const LanePacks<V, R>& lp, Pack<T, V> (&z)[R], int L, int G, int64_t dim) {
#pragma clang fp contract(off)
  for (int li = 0; li < L; ++li) {
    const int k = INV ? L - 1 - li : li;
    Pack<T, V> v[R];
    load_param<T, V, R, AL>(pv + (int64_t)k * dim, lp, v);
    T a = T(0);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) a += v[r].v[j] * z[r].v[j];
    a = group_sum_rt(a, G);
    const T ta = tau[k] * a;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) z[r].v[j] -= ta * v[r].v[j];
  }
}

// ------------------------------------------------------------------ the map and its inverse
// (x and y may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them.)
// The log-det is exactly 0: ladj_ps and ladj_sum are written as zeros here, in the same launch (the host passes null under
// BJX_ACCUMULATE: adding 0 leaves them as they are).
template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void householder_map_kernel(const T* __restrict__ pv, int L, int G, const T* x, T* y, T* __restrict__ ladj_ps,
                                                              double* __restrict__ ladj_sum, int64_t dim, int64_t batch, int64_t groups) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* tau = reinterpret_cast<T*>(smem);
  hh_tau_table<T>(pv, L, dim, tau);
  const int C = kThreads / G;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  if (ladj_sum && blockIdx.x == 0 && threadIdx.x == 0) *ladj_sum = 0.0;
  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const bool live = grp * C + cl < batch;
    const int64_t col = live ? grp * C + cl : batch - 1;           // a group past the batch works on the last column and stores nothing
    Pack<T, V> z[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    hh_shared_sweep<T, V, R, AL, INV>(pv, tau, lp, z, L, G, dim);
    if (live) {
      store_data<T, V, R, AL>(y + col * dim, lp, z);
      if (ladj_ps && gl == 0) ladj_ps[col] = T(0);
    }
  }
}

// ------------------------------------------------------------------ the parameter pullback
// sum over the column groups of a wave (lanes gl, gl + G, …): afterwards the lanes of the first group hold the wave's sum
__device__ __forceinline__ double hh_groups_sum(double s, int G) {
  for (int m = G; m < 64; m <<= 1) s += shfl_xor(s, m);
  return s;
}

template <class T, int V, int R, bool AL, bool INV>
__global__ __launch_bounds__(256) void householder_params_kernel(const T* __restrict__ pv, int L, int G, const T* __restrict__ x, const T* gbar, T* xbar, int64_t dim,
                                                                 int64_t batch, int64_t tiles, double* __restrict__ partials) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int per = L * ((int)dim + 1);
  double* tab = reinterpret_cast<double*>(smem);                   // [kWaves][L][dim + 1]
  T* tau = reinterpret_cast<T*>(tab + (size_t)kWaves * per);       // [L]
  for (int e = threadIdx.x; e < kWaves * per; e += kThreads) tab[e] = 0.0;
  hh_tau_table<T>(pv, L, dim, tau);
  const int C = kThreads / G;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int lane = threadIdx.x & 63;
  double* mine = tab + (size_t)(threadIdx.x >> 6) * per;           // this wave's table
  const LanePacks<V, R> lp(gl, G, (int)dim);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const bool live = tile * C + cl < batch;
    const int64_t col = live ? tile * C + cl : batch - 1;
    Pack<T, V> z[R], g[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    hh_shared_sweep<T, V, R, AL, INV>(pv, tau, lp, z, L, G, dim);
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    // ---- reverse sweep: the column holds the OUTPUT of layer k and is rewound to its input
    for (int li = 0; li < L; ++li) {
      const int k = INV ? li : L - 1 - li;
      Pack<T, V> v[R];
      load_param<T, V, R, AL>(pv + (int64_t)k * dim, lp, v);
      T ap = T(0), c = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          ap = ap + v[r].v[j] * z[r].v[j];
          c = c + v[r].v[j] * g[r].v[j];
        }
      group_sum2_rt(ap, c, G);
      const T t = tau[k];
      const T aa = -ap;                                            // vᵀz_k
      const T tap = t * ap, tc = t * c;
      double* row = mine + (size_t)k * (dim + 1);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T vv = v[r].v[j], gg = g[r].v[j];
          const T zk = z[r].v[j] - tap * vv;
          z[r].v[j] = zk;
          g[r].v[j] = gg - tc * vv;
          double s = live ? (double)aa * (double)gg + (double)c * (double)zk : 0.0;   // a dead column adds nothing (a select: its NaN would)
          s = hh_groups_sum(s, G);
          if (lane < G && j < lp.nrow[r]) row[lp.off[r] + j] += s;
        }
      double q = (live && gl == 0) ? (double)aa * (double)c : 0.0;
      q = hh_groups_sum(q, G);
      if (lane == 0) row[dim] += q;
    }
    if (xbar && live) store_data<T, V, R, AL>(xbar + col * dim, lp, g);
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * per;
  for (int e = threadIdx.x; e < per; e += kThreads) out[e] = ((tab[e] + tab[(size_t)per + e]) + tab[(size_t)2 * per + e]) + tab[(size_t)3 * per + e];
}

// first fold (only when there are more block partials than one chunk): out[chunk][e] = Σ of the chunk's block partials, in order
__global__ __launch_bounds__(256) void householder_fold_kernel(const double* __restrict__ in, int nsets, int per, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const int k0 = blockIdx.y * HH_FOLD_CHUNK;
  const int k1 = k0 + HH_FOLD_CHUNK < nsets ? k0 + HH_FOLD_CHUNK : nsets;
  double a = 0.0;
  for (int k = k0; k < k1; ++k) a += in[(size_t)k * per + e];
  out[(size_t)blockIdx.y * per + e] = a;
}

// last fold and the cast: block k forms v̄_k = −t S + t² q v in Float64 (t from v_k in Float64, fixed-order tree)
template <class T>
__global__ __launch_bounds__(256) void householder_final_kernel(const T* __restrict__ pv, const double* __restrict__ in, int nsets, int per, int dim, T* __restrict__ v_bar) {
  __shared__ double red[256];
  const int k = blockIdx.x;
  const T* vk = pv + (size_t)k * dim;
  double ss = 0.0;
  for (int r = threadIdx.x; r < dim; r += 256) { const double e = (double)vk[r]; ss += e * e; }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  ss = red[0];
  const double t = ss == 0.0 ? 0.0 : 2.0 / ss;
  const double* base = in + (size_t)k * (dim + 1);
  double q = 0.0;
  for (int s = 0; s < nsets; ++s) q += base[(size_t)s * per + dim];
  for (int r = threadIdx.x; r < dim; r += 256) {
    double S = 0.0;
    for (int s = 0; s < nsets; ++s) S += base[(size_t)s * per + r];
    v_bar[(size_t)k * dim + r] = (T)(-t * S + t * t * q * (double)vk[r]);
  }
}

// ------------------------------------------------------------------ host side
int householder_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* v, int n_layers, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, n_layers >= 1 && n_layers <= BJX_HOUSEHOLDER_MAX_LAYERS, BJX_ERR_UNSUPPORTED, "%s: %d layers (1 ... %d supported)", name, n_layers,
              BJX_HOUSEHOLDER_MAX_LAYERS);
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0, BJX_ERR_SHAPE, "%s: bad size (dim=%lld, batch=%lld)", name, (long long)dim, (long long)batch);
  const int64_t lim = dt == BJX_F32 ? 1024 : 512;
  BJX_REQUIRE(ctx, dim <= lim, BJX_ERR_UNSUPPORTED, "%s: dim %lld above the %lld rows a lane group holds in %s", name, (long long)dim, (long long)lim,
              dt == BJX_F32 ? "Float32" : "Float64");
  BJX_REQUIRE(ctx, batch == 0 || v, BJX_ERR_ARG, "%s: null parameter pointer", name);
  return BJX_OK;
}

// lanes per column, packs per lane (householder_cols_shape of the sibling)
template <class T> void householder_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T> bool householder_vector_form(int64_t dim, std::initializer_list<const void*> ptrs) {
  if (dim % Vec16<T>::N) return false;
  for (const void* p : ptrs)
    if (p && !bjx_aligned16(p)) return false;
  return true;
}

template <class T, int R, bool AL>
void launch_map(bjx_ctx* ctx, int grid, int inverse, const T* v, int L, int G, const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, int64_t groups) {
  constexpr int V = Vec16<T>::N;
  const size_t smem = (size_t)L * sizeof(T);
  if (inverse) hipLaunchKernelGGL((householder_map_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, v, L, G, in, out, ladj_ps, ladj_sum, dim, batch, groups);
  else hipLaunchKernelGGL((householder_map_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, v, L, G, in, out, ladj_ps, ladj_sum, dim, batch, groups);
}

template <class T>
int householder_impl(bjx_ctx* ctx, int inverse, const T* v, int L, const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (flags & BJX_ACCUMULATE) { ladj_ps = nullptr; ladj_sum = nullptr; }       // + 0: left as they are
  if (batch == 0) {
    if (ladj_sum) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1;
  householder_shape<T>(dim, &G, &R);
  const int C = kThreads / G;
  const int64_t groups = (batch + C - 1) / C;
  const int64_t cap = (int64_t)ctx->num_cu * kMapBlocksPerCu;
  const int grid = (int)(groups < cap ? groups : cap);
  const bool al = householder_vector_form<T>(dim, {v, in, out});
  {
    BjxProf prof_(ctx);
#define HHM(R_) do { if (al) launch_map<T, R_, true>(ctx, grid, inverse, v, L, G, in, out, ladj_ps, ladj_sum, dim, batch, groups); \
                     else launch_map<T, R_, false>(ctx, grid, inverse, v, L, G, in, out, ladj_ps, ladj_sum, dim, batch, groups); } while (0)
    switch (R) {
      case 1: HHM(1); break;
      case 2: HHM(2); break;
      default: HHM(4); break;
    }
#undef HHM
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}

template <class T, int R, bool AL>
void launch_params(bjx_ctx* ctx, int grid, size_t smem, int inverse, const T* v, int L, int G, const T* in, const T* gb, T* xb, int64_t dim, int64_t batch, int64_t tiles,
                   double* part) {
  constexpr int V = Vec16<T>::N;
  if (inverse) hipLaunchKernelGGL((householder_params_kernel<T, V, R, AL, true>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, v, L, G, in, gb, xb, dim, batch, tiles, part);
  else hipLaunchKernelGGL((householder_params_kernel<T, V, R, AL, false>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, v, L, G, in, gb, xb, dim, batch, tiles, part);
}

template <class T>
int householder_vjp_params_impl(bjx_ctx* ctx, int inverse, const T* v, int L, const T* in, const T* gb, T* xb, T* vb, int64_t dim, int64_t batch) {
  const size_t smem = BJX_HOUSEHOLDER_LDS_BYTES(dim, L);
  BJX_REQUIRE(ctx, smem <= HH_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_householder_vjp_params: the Float64 tables of %d layers of %lld rows (%zu bytes) exceed the LDS budget of %zu bytes",
              L, (long long)dim, smem, HH_LDS_BUDGET);
  if (batch == 0) {
    BJX_HIP(ctx, hipMemsetAsync(vb, 0, (size_t)L * dim * sizeof(T), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1;
  householder_shape<T>(dim, &G, &R);
  const int C = kThreads / G;
  const int64_t tiles = (batch + C - 1) / C;
  const int64_t cap = (int64_t)ctx->num_cu * kParamBlocksPerCu;
  int64_t grid64 = (tiles + HH_TILES_MIN - 1) / HH_TILES_MIN;
  if (grid64 > cap) grid64 = cap;
  if (grid64 < 1) grid64 = 1;
  const int grid = (int)grid64;
  const int per = L * ((int)dim + 1);
  const int chunks = (grid + HH_FOLD_CHUNK - 1) / HH_FOLD_CHUNK;
  { int rc = bjx_ensure_partials(ctx, (size_t)(grid + chunks) * per); if (rc) return rc; }
  double* part = ctx->partials;
  double* part2 = part + (size_t)grid * per;
  const bool al = householder_vector_form<T>(dim, {v, in, gb, xb});
  {
    BjxProf prof_(ctx);
#define HHP(R_) do { if (al) launch_params<T, R_, true>(ctx, grid, smem, inverse, v, L, G, in, gb, xb, dim, batch, tiles, part); \
                     else launch_params<T, R_, false>(ctx, grid, smem, inverse, v, L, G, in, gb, xb, dim, batch, tiles, part); } while (0)
    switch (R) {
      case 1: HHP(1); break;
      case 2: HHP(2); break;
      default: HHP(4); break;
    }
#undef HHP
  }
  BJX_CHECK_LAUNCH(ctx);
  if (chunks > 1) {
    hipLaunchKernelGGL(householder_fold_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)chunks), dim3(256), 0, ctx->stream, part, grid, per, part2);
    hipLaunchKernelGGL(householder_final_kernel<T>, dim3((unsigned)L), dim3(256), 0, ctx->stream, v, part2, chunks, per, (int)dim, vb);
  } else {
    hipLaunchKernelGGL(householder_final_kernel<T>, dim3((unsigned)L), dim3(256), 0, ctx->stream, v, part, grid, per, (int)dim, vb);
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_householder(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* v, int n_layers, const void* in, void* out, void* ladj_ps, double* ladj_sum,
                            int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = householder_check(ctx, "bjx_householder", dt, v, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_householder: null pointer");
  if (dt == BJX_F32)
    return householder_impl<float>(ctx, inverse, (const float*)v, n_layers, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return householder_impl<double>(ctx, inverse, (const double*)v, n_layers, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_householder_vjp_params(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* v, int n_layers, const void* in, const void* out_bar,
                                       const void* ladj_bar, void* in_bar, void* v_bar, int64_t dim, int64_t batch) {
  (void)ladj_bar;                                                  // the log-det is the constant 0: its cotangent contributes nothing
  if (!ctx) return BJX_ERR_ARG;
  int rc = householder_check(ctx, "bjx_householder_vjp_params", dt, v, n_layers, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, v_bar && ((in && out_bar) || batch == 0), BJX_ERR_ARG, "bjx_householder_vjp_params: null pointer");
  if (dt == BJX_F32)
    return householder_vjp_params_impl<float>(ctx, inverse, (const float*)v, n_layers, (const float*)in, (const float*)out_bar, (float*)in_bar, (float*)v_bar, dim, batch);
  return householder_vjp_params_impl<double>(ctx, inverse, (const double*)v, n_layers, (const double*)in, (const double*)out_bar, (double*)in_bar, (double*)v_bar, dim, batch);
}
