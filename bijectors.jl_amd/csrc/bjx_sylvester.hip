// bjx_sylvester.hip — one Sylvester layer z' = z + Q R tanh(R̃ Qᵀz + b) with ONE parameter set (Q, R, R̃, b) shared by every column
// (include/bjx_sylvester.h): the Sylvester flow as it is trained outside a VAE and as it sits between coupling layers.  The per-column
// sibling is bjx_sylvester_cols.hip; the lane geometry is the same (bjx_cols_lanes.inc): V = 16 B / sizeof(T) elements per pack, G lanes
// per column (the power of two >= the packs of a column, at most 64), R = 1, 2 or 4 packs per lane, a 256-thread block owns C = 256/G
// columns at a time; the vector form on whole packs and aligned pointers, the element form otherwise.  Contraction is off in every
// kernel: the bits depend neither on the form the dispatcher chose nor on the outputs asked for.
//
// Parameters.  R, R̃ and b are the same for every lane of every wave: they are read at wave-uniform addresses through the constant
// address space inside the unrolled M-sized algebra, one triangle column at a time (syl_fresh), so they arrive through uniform (scalar)
// loads and the scalar cache and are operands of the vector arithmetic, not per-lane registers held across the column loop as in the
// sibling (where every column has its own).  Q is read through the caches (load_param), not staged in LDS: it is at most 64 KiB, every column of every block reads the
// same dim·M elements and the lane groups of a wave read the SAME addresses.  Where MP·R <= 8 packs a lane's share of Q is loaded ONCE
// per block, before the column loop, and stays in registers; otherwise both passes of every column read it through the caches (behind
// syl_fresh_q(), which keeps the compiler from hoisting those loop-invariant loads into registers).
// The M-vectors of a column (s, a, p, and p̄, t̄, s̄ in the pullback) live in registers with the compile-time bound MP = M padded to
// 1, 2, 4, 8, 16: every loop over units is unrolled to MP and guarded by the wave-uniform `m < M`, so a padded unit reads nothing.
//
// A column (the forms of bjx_sylvester_cols.hip): the data stays in registers; one pass over the M columns of Q forms s = Qᵀz (the
// pullback: s and p̄ = Qᵀȳ through one butterfly); the M-sized algebra follows, replicated on every lane of the group; a second pass
// forms y = z + Qp (the pullback: z̄ = ȳ + Q s̄).  The input pullback and the parameter pullback run the SAME device function for a
// column, so z̄ has the same bits whether or not the parameter cotangents are asked for.
//
// Parameter pullback (the scheme of householder_params_kernel: one streaming pass over z and ȳ).  The grid is persistent: at most
// SYL_BLOCKS_PER_CU = 4 blocks per CU, at least SYL_TILES_MIN = 4 column tiles per block.  A column's summands — Q̄: ȳpᵀ + z s̄ᵀ;
// R̄: triu(p̄aᵀ) + its diagonal term; R̃̄: triu(t̄sᵀ) + its diagonal term; b̄: t̄ — are formed in Float64 from the column's T values, a dead
// column's replaced by 0 through a select (its NaN would leak), and summed over the column groups of the wave by a shuffle butterfly
// (lanes gl, gl + G, …); one writer per entry (the lanes of the wave's first group for Q̄, lane 0 for the M² + M others) adds the
// result into the wave's PRIVATE Float64 LDS table of P = dim·M + 2M² + M entries: no atomics.  At the end of a block its four
// tables are added in a fixed order into ONE partial per block in the context's partials.  Above SYL_FOLD_CHUNK = 32 partials a first
// fold adds chunks of 32 in order; the last fold adds what is left in order, casts to T and writes the strict lower triangles of R̄
// and R̃̄ as zeros: at most three launches, and the same call returns the same bits.
#include "bjx_internal.h"
#include "../../include/bjx_sylvester.h"
#include <initializer_list>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"                                     // Pack, load_pack, load_pack_part, store_pack_part
#include "bjx_cols_lanes.inc"                                      // LanePacks, load_data, load_param, store_data

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMapBlocksPerCu = 8;
constexpr int SYL_BLOCKS_PER_CU = 4;          // the persistent grid of the parameter pullback: at most 4 blocks per CU ...
constexpr int SYL_TILES_MIN = 4;              // ... and at least 4 column tiles per block (one partial of P doubles per block)
constexpr int SYL_FOLD_CHUNK = 32;            // block partials one thread of the first fold adds
constexpr size_t SYL_LDS_BUDGET = BJX_SYLVESTER_LDS_BUDGET;

// R, R̃ and b are read through the CONSTANT address space (nothing writes them while a kernel runs): a load at a wave-uniform address
// there is a scalar load whatever else the kernel stores.  syl_fresh() hands a walk over a triangle a pointer the compiler cannot
// trace back to the kernel argument, so the loads of that walk are not hoisted out of the column loop or shared between walks (left
// alone the compiler did exactly that: all M² + M values loaded once per block, held in SGPRs and spilled to vector registers).
#define SYL_CONST(T) const T __attribute__((address_space(4)))
template <class T> __device__ __forceinline__ SYL_CONST(T)* syl_fresh(SYL_CONST(T)* p) {
  asm volatile("" : "+s"(p));
  return p;
}
// the same for Q where a lane does not keep its share (MP·R > 8 packs): one fresh pointer per pass, or the loop-invariant loads of all
// M columns are hoisted out of the column loop and held in vector registers
template <class T> __device__ __forceinline__ const T* syl_fresh_q(const T* p) {
  asm volatile("" : "+s"(p));
  return p;
}
template <class T> struct SylvesterArgs {
  const T* pq;
  SYL_CONST(T) *pr, *prt, *pb;
  int64_t dim, batch, groups;
  int M, G;
};
#define SYL_PARAM_ARGS const T* __restrict__ pq_, const T* __restrict__ pr_, const T* __restrict__ prt_, const T* __restrict__ pb_
#define SYL_GATHER(a0) SylvesterArgs<T> a = a0; a.pq = pq_; a.pr = (SYL_CONST(T)*)pr_; a.prt = (SYL_CONST(T)*)prt_; a.pb = (SYL_CONST(T)*)pb_

// packs of Q a lane keeps for the whole block (MP·R of them), else one scratch column per pass
template <int MP, int R> struct KeepQ { static constexpr bool value = MP * R <= 8; static constexpr int cols = value ? MP : 1; };

template <class T> __device__ __forceinline__ T syl_abs(T x) { return x < T(0) ? -x : x; }          // a NaN stays a NaN

// a lane's share of Q, once per block (KEEP only)
template <class T, int V, int R, bool AL, int MP>
__device__ __forceinline__ void syl_keep_q(const T* __restrict__ pq, int M, int64_t dim, const LanePacks<V, R>& lp, Pack<T, V> (&qk)[KeepQ<MP, R>::cols][R]) {
  if constexpr (KeepQ<MP, R>::value) {
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) load_param<T, V, R, AL>(pq + (int64_t)m * dim, lp, qk[m]);
      else {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) qk[m][r].v[j] = T(0);
      }
    }
  }
}

// ------------------------------------------------------------------ the map
// (z and y may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them)
template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_map_kernel(const SylvesterArgs<T> a0, SYL_PARAM_ARGS, const T* x, T* y, T* __restrict__ ladj_ps, int accumulate,
                                                            double* __restrict__ partials) {
#pragma clang fp contract(off)
  SYL_GATHER(a0);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* redd = reinterpret_cast<double*>(smem);
  constexpr bool KEEP = KeepQ<MP, R>::value;
  const int G = a.G, C = kThreads / G, M = a.M;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  Pack<T, V> qk[KeepQ<MP, R>::cols][R];
  syl_keep_q<T, V, R, AL, MP>(a.pq, M, dim, lp, qk);
  double acc = 0.0;
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;       // a group past the batch works on the last column and stores nothing
    Pack<T, V> z[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    // ---- first pass over Q: s = Qᵀz
    T s[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      s[m] = T(0);
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) s[m] += q[r].v[j] * z[r].v[j];
        s[m] = group_sum_rt(s[m], G);
      }
    }
    // ---- the M-sized algebra: t = triu(R̃)s + b, a = tanh t, p = triu(R)a, ladj = Σ log|1 + (1 − a²) R̃_mm R_mm|
    T t[MP], p[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) { t[m] = T(0); p[m] = T(0); }
    T ladj = T(0);
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
        SYL_CONST(T)* rtj = syl_fresh<T>(a.prt) + j * M;
#pragma unroll
        for (int i = 0; i < MP; ++i)
          if (i <= j) t[i] += rtj[i] * s[j];
      }
    }
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
        SYL_CONST(T)* rj = syl_fresh<T>(a.pr) + j * M;
        const T aj = d_tanh(t[j] + syl_fresh<T>(a.pb)[j]);
        T rjj = T(0);
#pragma unroll
        for (int i = 0; i < MP; ++i) {
          if (i > j) continue;
          const T r = rj[i];
          p[i] += r * aj;
          if (i == j) rjj = r;
        }
        const T d = T(1) + (T(1) - aj * aj) * syl_fresh<T>(a.prt)[j + j * M] * rjj;
        ladj += d_log(syl_abs(d));
      }
    }
    // ---- second pass over Q: y = z + Qp
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) z[r].v[j] += q[r].v[j] * p[m];
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

// ------------------------------------------------------------------ one column of the pullback, up to the second pass over Q
// the M-vectors a column's pullback leaves behind: the input pullback needs p̄-free s̄ only, the parameter pullback all of them
template <class T, int MP> struct SylUnits {
  T s[MP], pb[MP], a[MP], p[MP], tb[MP], sb[MP], er[MP], ert[MP];   // er, ert: the diagonal terms of R̄ and R̃̄
};

template <class T, int V, int R, bool AL, int MP>
__device__ __forceinline__ void syl_column_units(const SylvesterArgs<T>& a, const LanePacks<V, R>& lp, Pack<T, V> (&qk)[KeepQ<MP, R>::cols][R],
                                                 const Pack<T, V> (&z)[R], const Pack<T, V> (&g)[R], T lb, SylUnits<T, MP>& u) {
#pragma clang fp contract(off)
  constexpr bool KEEP = KeepQ<MP, R>::value;
  const int M = a.M, G = a.G;
  // ---- first pass over Q: s = Qᵀz and p̄ = Qᵀȳ through one butterfly
#pragma unroll
  for (int m = 0; m < MP; ++m) {
    u.s[m] = T(0); u.pb[m] = T(0);
    if (m < M) {
      Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
      if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * a.dim, lp, q);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) { u.s[m] += q[r].v[j] * z[r].v[j]; u.pb[m] += q[r].v[j] * g[r].v[j]; }
      group_sum2_rt(u.s[m], u.pb[m], G);
    }
  }
  // ---- R̃, first walk: t = triu(R̃)s
  T t[MP];
#pragma unroll
  for (int m = 0; m < MP; ++m) { t[m] = T(0); u.p[m] = T(0); u.tb[m] = T(0); u.sb[m] = T(0); u.er[m] = T(0); u.ert[m] = T(0); u.a[m] = T(0); }
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    if (j < M) {
      SYL_CONST(T)* rtj = syl_fresh<T>(a.prt) + j * M;
#pragma unroll
      for (int i = 0; i < MP; ++i)
        if (i <= j) t[i] += rtj[i] * u.s[j];
    }
  }
#pragma unroll
  for (int j = 0; j < MP; ++j)
    if (j < M) u.a[j] = d_tanh(t[j] + syl_fresh<T>(a.pb)[j]);
  // ---- R, one walk: p = triu(R)a, ā = Rᵀp̄; column j completes ā_j, so t̄_j and the diagonal terms
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    if (j < M) {
      const T aj = u.a[j], hp = T(1) - aj * aj;
      T ab = T(0), rjj = T(0);
      SYL_CONST(T)* rj = syl_fresh<T>(a.pr) + j * M;
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        if (i > j) continue;
        const T r = rj[i];
        u.p[i] += r * aj;
        ab += r * u.pb[i];
        if (i == j) rjj = r;
      }
      const T rtjj = syl_fresh<T>(a.prt)[j + j * M];
      const T d = T(1) + hp * rtjj * rjj;
      u.er[j] = lb * (hp * rtjj / d);
      u.ert[j] = lb * (hp * rjj / d);
      u.tb[j] = ab * hp + lb * (T(-2) * aj * hp * rtjj * rjj / d);
    }
  }
  // ---- R̃, second walk: s̄ = R̃ᵀt̄
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    if (j < M) {
      SYL_CONST(T)* rtj = syl_fresh<T>(a.prt) + j * M;
#pragma unroll
      for (int i = 0; i < MP; ++i)
        if (i <= j) u.sb[j] += rtj[i] * u.tb[i];
    }
  }
}

// ------------------------------------------------------------------ the input pullback alone
// (gbar and xbar may be the same buffer, as x and y above)
template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_vjp_kernel(const SylvesterArgs<T> a0, SYL_PARAM_ARGS, const T* x, const T* gbar, const T* __restrict__ lbar, T* xbar) {
#pragma clang fp contract(off)
  SYL_GATHER(a0);
  constexpr bool KEEP = KeepQ<MP, R>::value;
  const int G = a.G, C = kThreads / G, M = a.M;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  Pack<T, V> qk[KeepQ<MP, R>::cols][R];
  syl_keep_q<T, V, R, AL, MP>(a.pq, M, dim, lp, qk);
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;
    const T lb = lbar ? lbar[col] : T(0);
    Pack<T, V> z[R], g[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    SylUnits<T, MP> u;
    syl_column_units<T, V, R, AL, MP>(a, lp, qk, z, g, lb, u);
    // ---- second pass over Q: z̄ = ȳ + Q s̄
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
        const T sm = u.sb[m];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) g[r].v[j] += q[r].v[j] * sm;
      }
    }
    if (live) store_data<T, V, R, AL>(xbar + col * dim, lp, g);
  }
}

// ------------------------------------------------------------------ the parameter pullback
// sum over the column groups of a wave (lanes gl, gl + G, …): afterwards every lane holds the sum of the lanes with its gl
__device__ __forceinline__ double syl_groups_sum(double s, int G) {
  for (int m = G; m < 64; m <<= 1) s += shfl_xor(s, m);
  return s;
}

template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_params_kernel(const SylvesterArgs<T> a0, SYL_PARAM_ARGS, const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar,
                                                               int64_t tiles, double* __restrict__ partials) {
#pragma clang fp contract(off)
  SYL_GATHER(a0);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool KEEP = KeepQ<MP, R>::value;
  const int G = a.G, C = kThreads / G, M = a.M;
  const int64_t dim = a.dim;
  const int P = (int)dim * M + 2 * M * M + M;
  double* tab = reinterpret_cast<double*>(smem);                   // [kWaves][P]: Q̄ [M][dim], R̄ [M][M], R̃̄ [M][M], b̄ [M]
  for (int e = threadIdx.x; e < kWaves * P; e += kThreads) tab[e] = 0.0;
  __syncthreads();
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int lane = threadIdx.x & 63;
  double* mine = tab + (size_t)(threadIdx.x >> 6) * P;             // this wave's table
  double* mine_r = mine + (size_t)dim * M;
  double* mine_rt = mine_r + M * M;
  double* mine_b = mine_rt + M * M;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  Pack<T, V> qk[KeepQ<MP, R>::cols][R];
  syl_keep_q<T, V, R, AL, MP>(a.pq, M, dim, lp, qk);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const bool live = tile * C + cl < a.batch;
    const int64_t col = live ? tile * C + cl : a.batch - 1;
    const T lb = lbar ? lbar[col] : T(0);
    Pack<T, V> z[R], g[R], xb[R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    SylUnits<T, MP> u;
    syl_column_units<T, V, R, AL, MP>(a, lp, qk, z, g, lb, u);
    // ---- the M² + M summands (identical on every lane of a group): R̄, R̃̄, b̄; a dead column adds nothing (a select: its NaN would)
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
#pragma unroll
        for (int i = 0; i < MP; ++i) {
          if (i > j) continue;
          double vr = (double)u.pb[i] * (double)u.a[j];
          double vt = (double)u.tb[i] * (double)u.s[j];
          if (i == j) { vr += (double)u.er[j]; vt += (double)u.ert[j]; }
          vr = syl_groups_sum(live ? vr : 0.0, G);
          vt = syl_groups_sum(live ? vt : 0.0, G);
          if (lane == 0) { mine_r[i + j * M] += vr; mine_rt[i + j * M] += vt; }
        }
        const double vb = syl_groups_sum(live ? (double)u.tb[j] : 0.0, G);
        if (lane == 0) mine_b[j] += vb;
      }
    }
    // ---- second pass over Q: z̄ = ȳ + Q s̄ (carried in xb: Q̄ needs ȳ itself) and the summands of Q̄ = ȳpᵀ + z s̄ᵀ
#pragma unroll
    for (int r = 0; r < R; ++r) xb[r] = g[r];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
        const T pm = u.p[m], sm = u.sb[m];
        double* row = mine + (size_t)m * dim;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            xb[r].v[j] += q[r].v[j] * sm;
            double v = live ? (double)g[r].v[j] * (double)pm + (double)z[r].v[j] * (double)sm : 0.0;
            v = syl_groups_sum(v, G);
            if (lane < G && j < lp.nrow[r]) row[lp.off[r] + j] += v;
          }
      }
    }
    if (xbar && live) store_data<T, V, R, AL>(xbar + col * dim, lp, xb);
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * P;
  for (int e = threadIdx.x; e < P; e += kThreads) out[e] = ((tab[e] + tab[(size_t)P + e]) + tab[(size_t)2 * P + e]) + tab[(size_t)3 * P + e];
}

// first fold (only when there are more block partials than one chunk): out[chunk][e] = Σ of the chunk's block partials, in order
__global__ __launch_bounds__(256) void sylvester_fold_kernel(const double* __restrict__ in, int nsets, int per, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const int k0 = blockIdx.y * SYL_FOLD_CHUNK;
  const int k1 = k0 + SYL_FOLD_CHUNK < nsets ? k0 + SYL_FOLD_CHUNK : nsets;
  double a = 0.0;
  for (int k = k0; k < k1; ++k) a += in[(size_t)k * per + e];
  out[(size_t)blockIdx.y * per + e] = a;
}

// last fold and the cast; the strict lower triangles of R̄ and R̃̄ are written as zeros
template <class T>
__global__ __launch_bounds__(256) void sylvester_final_kernel(const double* __restrict__ in, int nsets, int per, int dim, int M, T* __restrict__ q_bar,
                                                              T* __restrict__ r_bar, T* __restrict__ rt_bar, T* __restrict__ b_bar) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  double a = 0.0;
  for (int k = 0; k < nsets; ++k) a += in[(size_t)k * per + e];
  const int nq = dim * M, mm = M * M;
  if (e < nq) { q_bar[e] = (T)a; return; }
  int f = e - nq;
  if (f < 2 * mm) {
    T* o = f < mm ? r_bar : rt_bar;
    f = f < mm ? f : f - mm;
    o[f] = (f % M) > (f / M) ? T(0) : (T)a;
    return;
  }
  b_bar[f - 2 * mm] = (T)a;
}

// ------------------------------------------------------------------ host side
int sylvester_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* q, const void* r, const void* rt, const void* b, int M, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, M >= 1 && M <= BJX_SYLVESTER_MAX_UNITS, BJX_ERR_UNSUPPORTED, "%s: %d hidden units (1 ... %d supported)", name, M, BJX_SYLVESTER_MAX_UNITS);
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0, BJX_ERR_SHAPE, "%s: bad size (dim=%lld, batch=%lld)", name, (long long)dim, (long long)batch);
  BJX_REQUIRE(ctx, M <= dim, BJX_ERR_UNSUPPORTED, "%s: %d hidden units above dim %lld", name, M, (long long)dim);
  const int64_t lim = dt == BJX_F32 ? 1024 : 512;
  BJX_REQUIRE(ctx, dim <= lim, BJX_ERR_UNSUPPORTED, "%s: dim %lld above the %lld rows a lane group holds in %s", name, (long long)dim, (long long)lim,
              dt == BJX_F32 ? "Float32" : "Float64");
  BJX_REQUIRE(ctx, batch == 0 || (q && r && rt && b), BJX_ERR_ARG, "%s: null parameter pointer", name);
  return BJX_OK;
}

// lanes per column, packs per lane (sylvester_cols_shape of the sibling)
template <class T> void sylvester_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T> SylvesterArgs<T> sylvester_args(const void* q, const void* r, const void* rt, const void* b, int M, int64_t dim, int64_t batch, int G) {
  SylvesterArgs<T> a{};
  a.pq = (const T*)q; a.pr = nullptr; a.prt = nullptr; a.pb = nullptr;      // R, R̃, b travel as kernel arguments of their own
  a.dim = dim; a.batch = batch; a.M = M; a.G = G;
  const int C = kThreads / G;
  a.groups = (batch + C - 1) / C;
  return a;
}

// only the [dim]-shaped arrays take vector accesses: R, R̃, b go element by element in either form
template <class T> bool sylvester_vector_form(int64_t dim, std::initializer_list<const void*> ptrs) {
  if (dim % Vec16<T>::N) return false;
  for (const void* p : ptrs)
    if (p && !bjx_aligned16(p)) return false;
  return true;
}

inline int sylvester_pad(int M) { return M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16))); }

template <class T, int R, bool AL, int MP>
void launch_map(bjx_ctx* ctx, const SylvesterArgs<T>& a, const T* pr, const T* prt, const T* pb, int grid, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
  constexpr int V = Vec16<T>::N;
  hipLaunchKernelGGL((sylvester_map_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), 8 * sizeof(double), ctx->stream, a, a.pq, pr, prt, pb, in, out, ladj_ps, accum, partials);
}
template <class T, int R, bool AL, int MP>
void launch_vjp(bjx_ctx* ctx, const SylvesterArgs<T>& a, const T* pr, const T* prt, const T* pb, int grid, const T* in, const T* gb, const T* lb, T* xb) {
  constexpr int V = Vec16<T>::N;
  hipLaunchKernelGGL((sylvester_vjp_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a, a.pq, pr, prt, pb, in, gb, lb, xb);
}
// the parameter pullback never runs at (R, MP) pairs the LDS rule refuses outright: R packs per lane mean dim > 64·V·R/2 rows, MP padded
// units mean M > MP/2, and the smallest table of that pair must fit the budget (Float32 R = 4: MP <= 4; R = 2 and Float64 R = 4: MP <= 8)
template <class T, int R, int MP> constexpr bool syl_params_served() {
  constexpr size_t dim = R == 1 ? 1 : (size_t)64 * Vec16<T>::N * (R / 2) + 1;
  constexpr size_t M = MP == 1 ? 1 : MP / 2 + 1;
  return BJX_SYLVESTER_LDS_BYTES(dim < M ? M : dim, M) <= SYL_LDS_BUDGET;
}

template <class T, int R, bool AL, int MP>
void launch_params(bjx_ctx* ctx, const SylvesterArgs<T>& a, const T* pr, const T* prt, const T* pb, int grid, size_t smem, const T* in, const T* gb, const T* lb, T* xb, int64_t tiles, double* part) {
  constexpr int V = Vec16<T>::N;
  if constexpr (syl_params_served<T, R, MP>())
    hipLaunchKernelGGL((sylvester_params_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), smem, ctx->stream, a, a.pq, pr, prt, pb, in, gb, lb, xb, tiles, part);
}

// (R, AL, MP) -> the instantiation
#define SYL_MP(R_, AL_, CALL) do { switch (mp) { \
      case 1: CALL(R_, AL_, 1); break; case 2: CALL(R_, AL_, 2); break; case 4: CALL(R_, AL_, 4); break; \
      case 8: CALL(R_, AL_, 8); break; default: CALL(R_, AL_, 16); break; } } while (0)
#define SYL_DISPATCH(CALL) do { \
    if (al) { switch (R) { case 1: SYL_MP(1, true, CALL); break; case 2: SYL_MP(2, true, CALL); break; default: SYL_MP(4, true, CALL); break; } } \
    else { switch (R) { case 1: SYL_MP(1, false, CALL); break; case 2: SYL_MP(2, false, CALL); break; default: SYL_MP(4, false, CALL); break; } } } while (0)

template <class T>
int sylvester_impl(bjx_ctx* ctx, const void* q, const void* r, const void* rt, const void* b, int M, const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim,
                   int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1;
  sylvester_shape<T>(dim, &G, &R);
  const SylvesterArgs<T> a = sylvester_args<T>(q, r, rt, b, M, dim, batch, G);
  const int64_t cap = (int64_t)ctx->num_cu * kMapBlocksPerCu;
  const int grid = (int)(a.groups < cap ? a.groups : cap);
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  const bool al = sylvester_vector_form<T>(dim, {q, in, out});
  const int mp = sylvester_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_MAP(R_, AL_, MP_) launch_map<T, R_, AL_, MP_>(ctx, a, (const T*)r, (const T*)rt, (const T*)b, grid, in, out, ladj_ps, accum, partials)
    SYL_DISPATCH(SYL_MAP);
#undef SYL_MAP
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T>
int sylvester_vjp_impl(bjx_ctx* ctx, const void* q, const void* r, const void* rt, const void* b, int M, const T* in, const T* gb, const T* lb, T* xb, int64_t dim,
                       int64_t batch) {
  if (batch == 0 || !xb) return BJX_OK;
  int G = 1, R = 1;
  sylvester_shape<T>(dim, &G, &R);
  const SylvesterArgs<T> a = sylvester_args<T>(q, r, rt, b, M, dim, batch, G);
  const int64_t cap = (int64_t)ctx->num_cu * kMapBlocksPerCu;
  const int grid = (int)(a.groups < cap ? a.groups : cap);
  const bool al = sylvester_vector_form<T>(dim, {q, in, gb, xb});
  const int mp = sylvester_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_VJP(R_, AL_, MP_) launch_vjp<T, R_, AL_, MP_>(ctx, a, (const T*)r, (const T*)rt, (const T*)b, grid, in, gb, lb, xb)
    SYL_DISPATCH(SYL_VJP);
#undef SYL_VJP
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}

template <class T>
int sylvester_params_impl(bjx_ctx* ctx, const void* q, const void* r, const void* rt, const void* b, int M, const T* in, const T* gb, const T* lb, T* xb, T* qb, T* rb,
                          T* rtb, T* bb, int64_t dim, int64_t batch) {
  const size_t smem = BJX_SYLVESTER_LDS_BYTES(dim, M);
  BJX_REQUIRE(ctx, smem <= SYL_LDS_BUDGET, BJX_ERR_UNSUPPORTED,
              "bjx_sylvester_vjp_params: the Float64 tables of %d hidden units on %lld rows (%zu bytes) exceed the LDS budget of %zu bytes", M, (long long)dim, smem,
              SYL_LDS_BUDGET);
  if (batch == 0) {
    BJX_HIP(ctx, hipMemsetAsync(qb, 0, (size_t)dim * M * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(rb, 0, (size_t)M * M * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(rtb, 0, (size_t)M * M * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(bb, 0, (size_t)M * sizeof(T), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1;
  sylvester_shape<T>(dim, &G, &R);
  const SylvesterArgs<T> a = sylvester_args<T>(q, r, rt, b, M, dim, batch, G);
  const int64_t tiles = a.groups;
  const int64_t cap = (int64_t)ctx->num_cu * SYL_BLOCKS_PER_CU;
  int64_t grid64 = (tiles + SYL_TILES_MIN - 1) / SYL_TILES_MIN;
  if (grid64 > cap) grid64 = cap;
  if (grid64 < 1) grid64 = 1;
  const int grid = (int)grid64;
  const int per = (int)dim * M + 2 * M * M + M;
  const int chunks = (grid + SYL_FOLD_CHUNK - 1) / SYL_FOLD_CHUNK;
  { int rc = bjx_ensure_partials(ctx, (size_t)(grid + chunks) * per); if (rc) return rc; }
  double* part = ctx->partials;
  double* part2 = part + (size_t)grid * per;
  const bool al = sylvester_vector_form<T>(dim, {q, in, gb, xb});
  const int mp = sylvester_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_PAR(R_, AL_, MP_) launch_params<T, R_, AL_, MP_>(ctx, a, (const T*)r, (const T*)rt, (const T*)b, grid, smem, in, gb, lb, xb, tiles, part)
    SYL_DISPATCH(SYL_PAR);
#undef SYL_PAR
  }
  BJX_CHECK_LAUNCH(ctx);
  const unsigned fb = (unsigned)((per + 255) / 256);
  if (chunks > 1) {
    hipLaunchKernelGGL(sylvester_fold_kernel, dim3(fb, (unsigned)chunks), dim3(256), 0, ctx->stream, part, grid, per, part2);
    hipLaunchKernelGGL(sylvester_final_kernel<T>, dim3(fb), dim3(256), 0, ctx->stream, part2, chunks, per, (int)dim, M, qb, rb, rtb, bb);
  } else {
    hipLaunchKernelGGL(sylvester_final_kernel<T>, dim3(fb), dim3(256), 0, ctx->stream, part, grid, per, (int)dim, M, qb, rb, rtb, bb);
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
#undef SYL_DISPATCH
#undef SYL_MP
#undef SYL_GATHER
#undef SYL_CONST
#undef SYL_PARAM_ARGS
}  // namespace

BJX_API int bjx_sylvester(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M, const void* in, void* out,
                          void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = sylvester_check(ctx, "bjx_sylvester", dt, q, r, r_tilde, b, M, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_sylvester: null pointer");
  if (dt == BJX_F32) return sylvester_impl<float>(ctx, q, r, r_tilde, b, M, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return sylvester_impl<double>(ctx, q, r, r_tilde, b, M, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_sylvester_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M, const void* in,
                                     const void* out_bar, const void* ladj_bar, void* in_bar, void* q_bar, void* r_bar, void* rt_bar, void* b_bar, int64_t dim,
                                     int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = sylvester_check(ctx, "bjx_sylvester_vjp_params", dt, q, r, r_tilde, b, M, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out_bar) || batch == 0, BJX_ERR_ARG, "bjx_sylvester_vjp_params: null pointer");
  const int given = (q_bar != nullptr) + (r_bar != nullptr) + (rt_bar != nullptr) + (b_bar != nullptr);
  BJX_REQUIRE(ctx, given == 0 || given == 4, BJX_ERR_ARG, "bjx_sylvester_vjp_params: q_bar, r_bar, rt_bar, b_bar are given all together or all NULL (%d of 4 given)", given);
  if (given == 0) {
    if (dt == BJX_F32)
      return sylvester_vjp_impl<float>(ctx, q, r, r_tilde, b, M, (const float*)in, (const float*)out_bar, (const float*)ladj_bar, (float*)in_bar, dim, batch);
    return sylvester_vjp_impl<double>(ctx, q, r, r_tilde, b, M, (const double*)in, (const double*)out_bar, (const double*)ladj_bar, (double*)in_bar, dim, batch);
  }
  if (dt == BJX_F32)
    return sylvester_params_impl<float>(ctx, q, r, r_tilde, b, M, (const float*)in, (const float*)out_bar, (const float*)ladj_bar, (float*)in_bar, (float*)q_bar,
                                        (float*)r_bar, (float*)rt_bar, (float*)b_bar, dim, batch);
  return sylvester_params_impl<double>(ctx, q, r, r_tilde, b, M, (const double*)in, (const double*)out_bar, (const double*)ladj_bar, (double*)in_bar, (double*)q_bar,
                                       (double*)r_bar, (double*)rt_bar, (double*)b_bar, dim, batch);
}
