// bjx_sylvester_cols.hip — one Sylvester layer with its parameters per COLUMN (include/bjx_sylvester_cols.h): the amortised Sylvester
// flow (van den Berg et al., 2018), z' = z + Q R tanh(R̃ Qᵀz + b) with M hidden units, whose (Q, R, R̃, b) an encoder emits per sample
// and which therefore stream with the data.
//
// Mapping (the one of bjx_householder_cols.hip, unchanged): V = 16 B / sizeof(T) elements per pack, packs = ceil(dim / V); a column
// gets G lanes (G = the power of two >= packs, at most 64) and lane j of the group holds the packs j, j + G, ... (R of them, R = 1, 2 or
// 4; three packs per lane run the R = 4 kernels with a dead pack): 1 024 rows in Float32, 512 in Float64.  A 256-thread block owns
// C = 256/G columns at a time and walks column groups grid-stride over a capped grid.  A lane group never spans two waves, so the M
// dot products of a column are one butterfly and no kernel has a barrier in its column loop.
//
// Two forms of every kernel: 16-byte vector accesses when dim is a whole number of packs, every [dim]-shaped base pointer is 16-byte
// aligned and the column stride of Q is a multiple of V; the element form otherwise.  R, R̃, b and their cotangents are read and
// written element by element in either form (M² + M values that every lane of the group asks for at the same address).
//
// A column: the data stays in registers; ONE pass over the M columns of Q forms s = Qᵀz (the pullback: s and p̄ = Qᵀȳ, 2M values
// through one butterfly); the M-sized algebra follows, REPLICATED on every lane of the group (the lanes of a group run in lock step,
// so splitting M² multiply-adds over them saves no issue slot unless the results are gathered again by M more cross-lane moves, and
// at G = 1 there is nobody to split with); a second pass over Q forms y = z + Qp (the pullback: z̄ = ȳ + Q s̄ and Q̄ = ȳpᵀ + z s̄ᵀ).
// The second pass takes Q from registers where MP·R <= 8 packs were kept from the first, through the caches otherwise.
// The M-vectors live in registers with the compile-time bound MP = M padded to 1, 2, 4, 8, 16: every loop over units is unrolled to
// MP and guarded by the wave-uniform `m < M`, so a padded unit reads nothing and costs a scalar branch.
//
// The pullback, with hp = 1 − a², d = 1 + hp·diag(R̃)·diag(R):   ā = Rᵀp̄,   t̄ = ā⊙hp − ℓ̄·2a⊙hp⊙diag(R̃)⊙diag(R)/d,   s̄ = R̃ᵀt̄,
//   R̄ = triu(p̄aᵀ) + diag(ℓ̄·hp⊙diag(R̃)/d),   R̃̄ = triu(t̄sᵀ) + diag(ℓ̄·hp⊙diag(R)/d),   b̄ = t̄;  the strict lower triangles of R̄, R̃̄ are
// written as exact zeros.  The triangles are walked column by column: R̃ once for t (its diagonal kept), R once for p, ā and R̄
// together (column j of R completes ā_j, hence t̄_j), R̃ a second time for s̄ and R̃̄.  Lane 0 of the group stores the M-sized outputs.
// Contraction is off in both kernels: the values must not depend on the form the dispatcher chose or on the outputs asked for.
// Nothing is summed over columns, so there are no atomics; the summed log-det goes through the per-block partials +
// bjx_launch_finalize (fixed order: run-to-run identical bits).
#include "bjx_internal.h"
#include "../../include/bjx_sylvester_cols.h"
#include <initializer_list>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"                                     // Pack, load_pack, load_pack_part, store_pack_part
#include "bjx_cols_lanes.inc"                                      // LanePacks, load_data, load_param, store_data

template <class T> struct SylvesterColsArgs {
  const T *pq, *pr, *prt, *pb;
  int64_t ldq, ldr, ldrt, ldb;
  int64_t dim, batch, groups;
  int M, G;
};

// packs of Q a lane keeps from the first pass for the second (MP·R of them), else one scratch column
template <int MP, int R> struct KeepQ { static constexpr bool value = MP * R <= 8; static constexpr int cols = value ? MP : 1; };

template <class T> __device__ __forceinline__ T syl_abs(T x) { return x < T(0) ? -x : x; }          // a NaN stays a NaN

// ------------------------------------------------------------------ the map
// (z and y may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them)
template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_cols_map_kernel(const SylvesterColsArgs<T> a, const T* x, T* y, T* __restrict__ ladj_ps, int accumulate,
                                                                 double* __restrict__ partials) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* redd = reinterpret_cast<double*>(smem);
  constexpr bool KEEP = KeepQ<MP, R>::value;
  const int G = a.G, C = (int)blockDim.x / G, M = a.M;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  double acc = 0.0;
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;       // a group past the batch works on the last column and stores nothing
    const T* qc = a.pq + col * a.ldq;
    const T* rc = a.pr + col * a.ldr;
    const T* rtc = a.prt + col * a.ldrt;
    const T* bc = a.pb + col * a.ldb;
    Pack<T, V> z[R], qk[KeepQ<MP, R>::cols][R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    // ---- first pass over Q: s = Qᵀz
    T s[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      s[m] = T(0);
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        load_param<T, V, R, AL>(qc + (int64_t)m * dim, lp, q);
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
#pragma unroll
        for (int i = 0; i < MP; ++i)
          if (i <= j) t[i] += rtc[i + j * M] * s[j];
      }
    }
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
        const T aj = d_tanh(t[j] + bc[j]);
        T rjj = T(0);
#pragma unroll
        for (int i = 0; i < MP; ++i) {
          if (i > j) continue;
          const T r = rc[i + j * M];
          p[i] += r * aj;
          if (i == j) rjj = r;
        }
        const T d = T(1) + (T(1) - aj * aj) * rtc[j + j * M] * rjj;
        ladj += d_log(syl_abs(d));
      }
    }
    // ---- second pass over Q: y = z + Qp
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(qc + (int64_t)m * dim, lp, q);
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

// ------------------------------------------------------------------ the pullback
// z̄ and the per-column (Q̄, R̄, R̃̄, b̄) (any of the four may be null).  (gbar and xbar may be the same buffer, as x and y above.)
template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_cols_vjp_kernel(const SylvesterColsArgs<T> a, const T* x, const T* gbar, const T* __restrict__ lbar, T* xbar,
                                                                 T* __restrict__ qbar, T* __restrict__ rbar, T* __restrict__ rtbar, T* __restrict__ bbar) {
#pragma clang fp contract(off)
  constexpr bool KEEP = KeepQ<MP, R>::value;
  const int G = a.G, C = (int)blockDim.x / G, M = a.M;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int64_t dim = a.dim;
  const LanePacks<V, R> lp(gl, G, (int)dim);
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const bool live = grp * C + cl < a.batch;
    const int64_t col = live ? grp * C + cl : a.batch - 1;
    const bool lead = live && gl == 0;                             // the lane that stores the M-sized outputs of its column
    const T* qc = a.pq + col * a.ldq;
    const T* rc = a.pr + col * a.ldr;
    const T* rtc = a.prt + col * a.ldrt;
    const T* bc = a.pb + col * a.ldb;
    const T lb = lbar ? lbar[col] : T(0);
    Pack<T, V> z[R], g[R], qk[KeepQ<MP, R>::cols][R];
    load_data<T, V, R, AL>(x + col * dim, lp, z);
    load_data<T, V, R, AL>(gbar + col * dim, lp, g);
    // ---- first pass over Q: s = Qᵀz and p̄ = Qᵀȳ through one butterfly
    T s[MP], pb[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      s[m] = T(0); pb[m] = T(0);
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        load_param<T, V, R, AL>(qc + (int64_t)m * dim, lp, q);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) { s[m] += q[r].v[j] * z[r].v[j]; pb[m] += q[r].v[j] * g[r].v[j]; }
        group_sum2_rt(s[m], pb[m], G);
      }
    }
    // ---- R̃, first walk: t = triu(R̃)s; its diagonal is kept (e[] holds diag(R̃) until column j of R is done, ℓ̄·hp·R_jj/d after)
    T t[MP], p[MP], e[MP], sb[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) { t[m] = T(0); p[m] = T(0); e[m] = T(0); sb[m] = T(0); }
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
#pragma unroll
        for (int i = 0; i < MP; ++i) {
          if (i > j) continue;
          const T rt = rtc[i + j * M];
          t[i] += rt * s[j];
          if (i == j) e[j] = rt;
        }
      }
    }
    // ---- R, one walk: a = tanh(t + b), p = triu(R)a, ā = Rᵀp̄, R̄; column j completes ā_j, so t̄_j (kept in t[j]: every t was
    //      read when a was formed)
    T av[MP];
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      av[j] = T(0);
      if (j < M) av[j] = d_tanh(t[j] + bc[j]);
    }
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
        const T aj = av[j], hp = T(1) - aj * aj;
        T ab = T(0), rjj = T(0);
#pragma unroll
        for (int i = 0; i < MP; ++i) {
          if (i > j) continue;
          const T r = rc[i + j * M];
          p[i] += r * aj;
          ab += r * pb[i];
          if (i == j) rjj = r;
        }
        const T rtjj = e[j];
        const T d = T(1) + hp * rtjj * rjj;
        const T er = lb * (hp * rtjj / d);                         // the diagonal term of R̄
        e[j] = lb * (hp * rjj / d);                                // … and of R̃̄
        t[j] = ab * hp + lb * (T(-2) * aj * hp * rtjj * rjj / d);  // t̄_j
        if (rbar && lead) {
          T* o = rbar + col * (int64_t)M * M + (int64_t)j * M;
#pragma unroll
          for (int i = 0; i < MP; ++i) {
            if (i < j) o[i] = pb[i] * aj;
            else if (i == j) o[i] = pb[i] * aj + er;
            else if (i < M) o[i] = T(0);
          }
        }
      }
    }
    // ---- R̃, second walk: s̄ = R̃ᵀt̄ and R̃̄; b̄ = t̄
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < M) {
#pragma unroll
        for (int i = 0; i < MP; ++i)
          if (i <= j) sb[j] += rtc[i + j * M] * t[i];
        if (rtbar && lead) {
          T* o = rtbar + col * (int64_t)M * M + (int64_t)j * M;
#pragma unroll
          for (int i = 0; i < MP; ++i) {
            if (i < j) o[i] = t[i] * s[j];
            else if (i == j) o[i] = t[i] * s[j] + e[j];
            else if (i < M) o[i] = T(0);
          }
        }
        if (bbar && lead) bbar[col * (int64_t)M + j] = t[j];
      }
    }
    // ---- second pass over Q: Q̄ = ȳpᵀ + z s̄ᵀ, z̄ = ȳ + Q s̄ (the sum is carried in xb: Q̄ needs ȳ itself)
    Pack<T, V> xb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) xb[r] = g[r];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(qc + (int64_t)m * dim, lp, q);
        const T pm = p[m], sm = sb[m];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            xb[r].v[j] += q[r].v[j] * sm;
            q[r].v[j] = g[r].v[j] * pm + z[r].v[j] * sm;
          }
        if (qbar && live) store_data<T, V, R, AL>(qbar + (col * M + m) * dim, lp, q);
      }
    }
    if (live) store_data<T, V, R, AL>(xbar + col * dim, lp, xb);
  }
}

// ------------------------------------------------------------------ host side
constexpr int kThreads = 256;
constexpr int kBlocksPerCu = 8;

int sylvester_cols_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q,
                         int64_t ld_r, int64_t ld_rt, int64_t ld_b, int M, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, M >= 1 && M <= BJX_SYLVESTER_COLS_MAX_UNITS, BJX_ERR_UNSUPPORTED, "%s: %d hidden units (1 ... %d supported)", name, M,
              BJX_SYLVESTER_COLS_MAX_UNITS);
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0, BJX_ERR_SHAPE, "%s: bad size (dim=%lld, batch=%lld)", name, (long long)dim, (long long)batch);
  BJX_REQUIRE(ctx, M <= dim, BJX_ERR_UNSUPPORTED, "%s: %d hidden units above dim %lld", name, M, (long long)dim);
  const int64_t lim = dt == BJX_F32 ? 1024 : 512;
  BJX_REQUIRE(ctx, dim <= lim, BJX_ERR_UNSUPPORTED, "%s: dim %lld above the %lld rows a lane group holds in %s", name, (long long)dim, (long long)lim,
              dt == BJX_F32 ? "Float32" : "Float64");
  BJX_REQUIRE(ctx, ld_q >= dim * M && ld_r >= (int64_t)M * M && ld_rt >= (int64_t)M * M && ld_b >= M, BJX_ERR_SHAPE,
              "%s: column strides (%lld, %lld, %lld, %lld) below dim x M = %lld, M x M = %lld and M = %d", name, (long long)ld_q, (long long)ld_r,
              (long long)ld_rt, (long long)ld_b, (long long)(dim * M), (long long)M * M, M);
  BJX_REQUIRE(ctx, batch == 0 || (p_q && p_r && p_rt && p_b), BJX_ERR_ARG, "%s: null parameter pointer", name);
  return BJX_OK;
}

// lanes per column, packs per lane (householder_cols_shape of the sibling)
template <class T> void sylvester_cols_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T>
SylvesterColsArgs<T> sylvester_cols_args(const bjx_ctx* ctx, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q, int64_t ld_r,
                                         int64_t ld_rt, int64_t ld_b, int M, int64_t dim, int64_t batch, int G, int* grid) {
  SylvesterColsArgs<T> a{};
  a.pq = (const T*)p_q; a.pr = (const T*)p_r; a.prt = (const T*)p_rt; a.pb = (const T*)p_b;
  a.ldq = ld_q; a.ldr = ld_r; a.ldrt = ld_rt; a.ldb = ld_b;
  a.dim = dim; a.batch = batch; a.M = M; a.G = G;
  const int C = kThreads / G;
  a.groups = (batch + C - 1) / C;
  const int64_t cap = (int64_t)ctx->num_cu * kBlocksPerCu;
  *grid = (int)(a.groups < cap ? a.groups : cap);
  return a;
}

// only the [dim]-shaped arrays take vector accesses: R, R̃, b and their cotangents go element by element in either form
template <class T> bool sylvester_cols_vector_form(const SylvesterColsArgs<T>& a, std::initializer_list<const void*> ptrs) {
  constexpr int V = Vec16<T>::N;
  if (a.dim % V || a.ldq % V) return false;
  for (const void* p : ptrs)
    if (p && !bjx_aligned16(p)) return false;
  return true;
}

inline int sylvester_cols_pad(int M) { return M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16))); }

template <class T, int R, bool AL, int MP>
void launch_map(bjx_ctx* ctx, const SylvesterColsArgs<T>& a, int grid, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
  constexpr int V = Vec16<T>::N;
  hipLaunchKernelGGL((sylvester_cols_map_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), 8 * sizeof(double), ctx->stream, a, in, out, ladj_ps, accum,
                     partials);
}
template <class T, int R, bool AL, int MP>
void launch_vjp(bjx_ctx* ctx, const SylvesterColsArgs<T>& a, int grid, const T* in, const T* gb, const T* lb, T* xb, T* qb, T* rb, T* rtb, T* bb) {
  constexpr int V = Vec16<T>::N;
  hipLaunchKernelGGL((sylvester_cols_vjp_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a, in, gb, lb, xb, qb, rb, rtb, bb);
}

// (R, AL, MP) -> the instantiation; F is launch_map or launch_vjp behind a generic lambda
#define SYL_MP(R_, AL_, CALL) do { switch (mp) { \
      case 1: CALL(R_, AL_, 1); break; case 2: CALL(R_, AL_, 2); break; case 4: CALL(R_, AL_, 4); break; \
      case 8: CALL(R_, AL_, 8); break; default: CALL(R_, AL_, 16); break; } } while (0)
#define SYL_DISPATCH(CALL) do { \
    if (al) { switch (R) { case 1: SYL_MP(1, true, CALL); break; case 2: SYL_MP(2, true, CALL); break; default: SYL_MP(4, true, CALL); break; } } \
    else { switch (R) { case 1: SYL_MP(1, false, CALL); break; case 2: SYL_MP(2, false, CALL); break; default: SYL_MP(4, false, CALL); break; } } } while (0)

template <class T>
int sylvester_cols_impl(bjx_ctx* ctx, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q, int64_t ld_r, int64_t ld_rt, int64_t ld_b,
                        int M, const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1, grid = 0;
  sylvester_cols_shape<T>(dim, &G, &R);
  const SylvesterColsArgs<T> a = sylvester_cols_args<T>(ctx, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, dim, batch, G, &grid);
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  const bool al = sylvester_cols_vector_form<T>(a, {p_q, in, out});
  const int mp = sylvester_cols_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_MAP(R_, AL_, MP_) launch_map<T, R_, AL_, MP_>(ctx, a, grid, in, out, ladj_ps, accum, partials)
    SYL_DISPATCH(SYL_MAP);
#undef SYL_MAP
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T>
int sylvester_cols_vjp_impl(bjx_ctx* ctx, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q, int64_t ld_r, int64_t ld_rt,
                            int64_t ld_b, int M, const T* in, const T* gb, const T* lb, T* xb, T* qb, T* rb, T* rtb, T* bb, int64_t dim, int64_t batch) {
  if (batch == 0) return BJX_OK;
  int G = 1, R = 1, grid = 0;
  sylvester_cols_shape<T>(dim, &G, &R);
  const SylvesterColsArgs<T> a = sylvester_cols_args<T>(ctx, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, dim, batch, G, &grid);
  const bool al = sylvester_cols_vector_form<T>(a, {p_q, in, gb, xb, qb});
  const int mp = sylvester_cols_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_VJP(R_, AL_, MP_) launch_vjp<T, R_, AL_, MP_>(ctx, a, grid, in, gb, lb, xb, qb, rb, rtb, bb)
    SYL_DISPATCH(SYL_VJP);
#undef SYL_VJP
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
#undef SYL_DISPATCH
#undef SYL_MP
}  // namespace

BJX_API int bjx_sylvester_cols(bjx_ctx* ctx, bjx_dtype dt, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q, int64_t ld_r,
                               int64_t ld_rt, int64_t ld_b, int M, const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch,
                               uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = sylvester_cols_check(ctx, "bjx_sylvester_cols", dt, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_sylvester_cols: null pointer");
  if (dt == BJX_F32)
    return sylvester_cols_impl<float>(ctx, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return sylvester_cols_impl<double>(ctx, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_sylvester_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, const void* p_q, const void* p_r, const void* p_rt, const void* p_b, int64_t ld_q, int64_t ld_r,
                                   int64_t ld_rt, int64_t ld_b, int M, const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* q_bar,
                                   void* r_bar, void* rt_bar, void* b_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = sylvester_cols_check(ctx, "bjx_sylvester_cols_vjp", dt, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out_bar && in_bar) || batch == 0, BJX_ERR_ARG, "bjx_sylvester_cols_vjp: null pointer");
  if (dt == BJX_F32)
    return sylvester_cols_vjp_impl<float>(ctx, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, (const float*)in, (const float*)out_bar, (const float*)ladj_bar,
                                          (float*)in_bar, (float*)q_bar, (float*)r_bar, (float*)rt_bar, (float*)b_bar, dim, batch);
  return sylvester_cols_vjp_impl<double>(ctx, p_q, p_r, p_rt, p_b, ld_q, ld_r, ld_rt, ld_b, M, (const double*)in, (const double*)out_bar, (const double*)ladj_bar,
                                         (double*)in_bar, (double*)q_bar, (double*)r_bar, (double*)rt_bar, (double*)b_bar, dim, batch);
}
