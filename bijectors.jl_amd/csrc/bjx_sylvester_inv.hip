// bjx_sylvester_inv.hip — the INVERSE of the shared Sylvester layer and the inverse's input pullback (include/bjx_sylvester_inv.h), for a
// layer whose caller declares QᵀQ = I and R_mm·R̃_mm > −1.  The forward sibling is bjx_sylvester.hip; the lane geometry, the parameter
// paths and the dispatcher are its own, repeated here so that file and the bits of its entries stay as they are: V = 16 B / sizeof(T)
// elements per pack, G lanes per column, R = 1, 2 or 4 packs per lane, a 256-thread block owns C = 256/G columns at a time, the vector
// form on whole packs and aligned pointers and the element form otherwise; R, R̃ and b through uniform loads behind an opaque pointer
// copy (syl_fresh), Q through the caches or, where MP·R <= 8 packs, once per block into registers; the M-vectors of a column in
// registers with the compile-time bound MP = M padded to 1, 2, 4, 8, 16 and every loop over units unrolled and guarded by the
// wave-uniform `m < M`.  Contraction is off in every kernel: the bits depend neither on the form nor on the outputs asked for.
//
// A column: the data stays in registers; one pass over the M columns of Q forms s′ = Qᵀy (the pullback: s′ and η₀ = Qᵀz̄ through one
// butterfly, which adds each of the two exactly as the single one does); the M-sized algebra follows, replicated on every lane of the
// group; a second pass forms z = y − Q(s′ − s) (the pullback: ȳ = z̄ − Qv, and z where `pre` is asked for).
//
// The primal sweep (syl_inv_units, the SAME device function in both kernels) walks the units from the last to the first.  Unit j has
// all of c_j = b_j + Σ_{i>j} Ũ_ji s_i and ρ_j = s′_j − Σ_{i>j} U_ji a_i when its turn comes: it solves α + k_j tanh(α + c_j) = R̃_jj ρ_j
// with the planar flow's root solve (planar_inv_act: straight-line Newton steps and an acceptance test; a lane that fails it takes the
// bounded safeguarded loop, the only data-dependent loop here), sets s_j = ρ_j − R_jj a_j and then adds its share to the c_i and ρ_i of
// the units i < j — a walk down COLUMN j of both triangles, contiguous like the forward's, instead of a walk along row i when unit i's
// turn comes; the sums are the same.  The M solves are a dependent chain.
//
// The pullback sweep (syl_inv_pull) walks the units from the first to the last, one walk down column m of both triangles per unit:
// ue = Σ_{i<=m} Ũ_im e_i, σ = Σ_{i<m} U_im π_i, st = Σ_{i<m} Ũ_im τ_i; π_m = (η₀_m − ℓ̄·ue − Ũ_mm hp_m σ − st)/d_m; τ_m = hp_m(U_mm π_m + σ);
// v_m = ℓ̄·ue + st + Ũ_mm τ_m, the m-th entry of Ũᵀ(ℓ̄e + τ).
#include "bjx_internal.h"
#include "../../include/bjx_sylvester_inv.h"
#include <initializer_list>

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"                                     // Pack, load_pack, load_pack_part, store_pack_part, planar_inv_act
#include "bjx_cols_lanes.inc"                                      // LanePacks, load_data, load_param, store_data

constexpr int kThreads = 256;
constexpr int kMapBlocksPerCu = 8;

// R, R̃, b through the constant address space behind an opaque pointer copy, Q behind one where a lane does not keep its share: the
// devices of bjx_sylvester.hip (DESIGN.md §7 says what the compiler does without them)
#define SYL_CONST(T) const T __attribute__((address_space(4)))
template <class T> __device__ __forceinline__ SYL_CONST(T)* syl_fresh(SYL_CONST(T)* p) {
  asm volatile("" : "+s"(p));
  return p;
}
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

template <int MP, int R> struct KeepQ { static constexpr bool value = MP * R <= 8; static constexpr int cols = value ? MP : 1; };

template <class T> __device__ __forceinline__ T syl_abs(T x) { return x < T(0) ? -x : x; }          // a NaN stays a NaN

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

// ------------------------------------------------------------------ the primal sweep: s′ -> s, a and the inverse's log-det
// the M-vectors a column's inverse leaves behind: w = s′ − s is what the second pass over Q takes off y
template <class T, int MP> struct SylInvUnits {
  T sp[MP], s[MP], a[MP];
  T ladj;
};

template <class T, int MP>
__device__ __forceinline__ void syl_inv_units(const SylvesterArgs<T>& a, SylInvUnits<T, MP>& u) {
#pragma clang fp contract(off)
  const int M = a.M;
  T c[MP], rho[MP];
#pragma unroll
  for (int m = 0; m < MP; ++m) { c[m] = T(0); rho[m] = u.sp[m]; u.s[m] = T(0); u.a[m] = T(0); }
  T ladj = T(0);
#pragma unroll
  for (int j = MP - 1; j >= 0; --j) {
    if (j < M) {
      SYL_CONST(T)* rtj = syl_fresh<T>(a.prt) + j * M;
      SYL_CONST(T)* rj = syl_fresh<T>(a.pr) + j * M;
      const T rtjj = rtj[j], rjj = rj[j];
      const T k = rjj * rtjj;
      T aj, s2;
      planar_inv_act<T>(rtjj * rho[j], k, c[j] + syl_fresh<T>(a.pb)[j], aj, s2);
      const T sj = rho[j] - rjj * aj;
      u.a[j] = aj;
      u.s[j] = sj;
      const T d = T(1) + (T(1) - aj * aj) * k;
      ladj -= d_log(syl_abs(d));
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        if (i >= j) continue;
        c[i] += rtj[i] * sj;
        rho[i] -= rj[i] * aj;
      }
    }
  }
  u.ladj = ladj;
}

// ------------------------------------------------------------------ the map
// (y and z may be the same buffer: a lane reads its packs of a column before it writes them, and no other lane touches them)
template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_inv_kernel(const SylvesterArgs<T> a0, SYL_PARAM_ARGS, const T* x, T* out, T* __restrict__ ladj_ps, int accumulate,
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
    Pack<T, V> y[R];
    load_data<T, V, R, AL>(x + col * dim, lp, y);
    // ---- first pass over Q: s′ = Qᵀy
    SylInvUnits<T, MP> u;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      u.sp[m] = T(0);
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) u.sp[m] += q[r].v[j] * y[r].v[j];
        u.sp[m] = group_sum_rt(u.sp[m], G);
      }
    }
    syl_inv_units<T, MP>(a, u);
    // ---- second pass over Q: z = y − Q(s′ − s)
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
        const T wm = u.sp[m] - u.s[m];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) y[r].v[j] -= q[r].v[j] * wm;
      }
    }
    if (live) {
      store_data<T, V, R, AL>(out + col * dim, lp, y);
      if (gl == 0) {
        if (ladj_ps) ladj_ps[col] = accumulate ? ladj_ps[col] + u.ladj : u.ladj;
        acc += (double)u.ladj;
      }
    }
  }
  if (partials) block_publish_partial(acc, redd, partials);
}

// ------------------------------------------------------------------ the pullback sweep: η₀ = Qᵀz̄, ℓ̄ and the primal's a -> v = Ũᵀ(ℓ̄e + τ)
template <class T, int MP>
__device__ __forceinline__ void syl_inv_pull(const SylvesterArgs<T>& a, const SylInvUnits<T, MP>& u, const T (&eta)[MP], T lb, T (&v)[MP]) {
#pragma clang fp contract(off)
  const int M = a.M;
  T e[MP], pi[MP], tau[MP];
#pragma unroll
  for (int m = 0; m < MP; ++m) { e[m] = T(0); pi[m] = T(0); tau[m] = T(0); v[m] = T(0); }
#pragma unroll
  for (int m = 0; m < MP; ++m) {
    if (m < M) {
      SYL_CONST(T)* rtm = syl_fresh<T>(a.prt) + m * M;
      SYL_CONST(T)* rm = syl_fresh<T>(a.pr) + m * M;
      const T rtmm = rtm[m], rmm = rm[m];
      const T k = rmm * rtmm;
      const T am = u.a[m], hp = T(1) - am * am;
      const T d = T(1) + hp * k;
      e[m] = T(-2) * am * hp * k / d;
      T ue = rtmm * e[m], sg = T(0), st = T(0);
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        if (i >= m) continue;
        const T rt = rtm[i];
        ue += rt * e[i];
        st += rt * tau[i];
        sg += rm[i] * pi[i];
      }
      const T lue = lb * ue;
      pi[m] = (((eta[m] - lue) - rtmm * hp * sg) - st) / d;
      tau[m] = hp * (rmm * pi[m] + sg);
      v[m] = (lue + st) + rtmm * tau[m];
    }
  }
}

// ------------------------------------------------------------------ the input pullback (and z where `pre` is asked for)
// (zbar and ybar may be the same buffer, as x and out above)
template <class T, int V, int R, bool AL, int MP>
__global__ __launch_bounds__(256) void sylvester_inv_vjp_kernel(const SylvesterArgs<T> a0, SYL_PARAM_ARGS, const T* __restrict__ x, const T* zbar, const T* __restrict__ lbar,
                                                                T* ybar, T* __restrict__ pre) {
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
    Pack<T, V> y[R], g[R];
    load_data<T, V, R, AL>(x + col * dim, lp, y);
    load_data<T, V, R, AL>(zbar + col * dim, lp, g);
    // ---- first pass over Q: s′ = Qᵀy and η₀ = Qᵀz̄ through one butterfly
    SylInvUnits<T, MP> u;
    T eta[MP], v[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      u.sp[m] = T(0); eta[m] = T(0);
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) { u.sp[m] += q[r].v[j] * y[r].v[j]; eta[m] += q[r].v[j] * g[r].v[j]; }
        group_sum2_rt(u.sp[m], eta[m], G);
      }
    }
    syl_inv_units<T, MP>(a, u);
    syl_inv_pull<T, MP>(a, u, eta, lb, v);
    // ---- second pass over Q: ȳ = z̄ − Qv, and z = y − Q(s′ − s) as the map forms it
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      if (m < M) {
        Pack<T, V>(&q)[R] = qk[KEEP ? m : 0];
        if constexpr (!KEEP) load_param<T, V, R, AL>(syl_fresh_q(a.pq) + (int64_t)m * dim, lp, q);
        const T vm = v[m], wm = u.sp[m] - u.s[m];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) g[r].v[j] -= q[r].v[j] * vm;
        if (pre) {
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < V; ++j) y[r].v[j] -= q[r].v[j] * wm;
        }
      }
    }
    if (live) {
      if (ybar) store_data<T, V, R, AL>(ybar + col * dim, lp, g);
      if (pre) store_data<T, V, R, AL>(pre + col * dim, lp, y);
    }
  }
}

// ------------------------------------------------------------------ host side (the checks, shapes and dispatcher of bjx_sylvester.hip)
int sylvester_inv_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const void* q, const void* r, const void* rt, const void* b, int M, int64_t dim, int64_t batch) {
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

template <class T> void sylvester_shape(int64_t dim, int* G, int* R) {
  const int64_t packs = (dim + Vec16<T>::N - 1) / Vec16<T>::N;
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t per = (packs + g - 1) / g;
  *G = g;
  *R = per <= 1 ? 1 : (per <= 2 ? 2 : 4);
}

template <class T> SylvesterArgs<T> sylvester_args(const void* q, int M, int64_t dim, int64_t batch, int G) {
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
void launch_inv(bjx_ctx* ctx, const SylvesterArgs<T>& a, const T* pr, const T* prt, const T* pb, int grid, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
  constexpr int V = Vec16<T>::N;
  hipLaunchKernelGGL((sylvester_inv_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), 8 * sizeof(double), ctx->stream, a, a.pq, pr, prt, pb, in, out, ladj_ps, accum, partials);
}
template <class T, int R, bool AL, int MP>
void launch_inv_vjp(bjx_ctx* ctx, const SylvesterArgs<T>& a, const T* pr, const T* prt, const T* pb, int grid, const T* in, const T* zb, const T* lb, T* yb, T* pre) {
  constexpr int V = Vec16<T>::N;
  hipLaunchKernelGGL((sylvester_inv_vjp_kernel<T, V, R, AL, MP>), dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a, a.pq, pr, prt, pb, in, zb, lb, yb, pre);
}

// (R, AL, MP) -> the instantiation
#define SYL_MP(R_, AL_, CALL) do { switch (mp) { \
      case 1: CALL(R_, AL_, 1); break; case 2: CALL(R_, AL_, 2); break; case 4: CALL(R_, AL_, 4); break; \
      case 8: CALL(R_, AL_, 8); break; default: CALL(R_, AL_, 16); break; } } while (0)
#define SYL_DISPATCH(CALL) do { \
    if (al) { switch (R) { case 1: SYL_MP(1, true, CALL); break; case 2: SYL_MP(2, true, CALL); break; default: SYL_MP(4, true, CALL); break; } } \
    else { switch (R) { case 1: SYL_MP(1, false, CALL); break; case 2: SYL_MP(2, false, CALL); break; default: SYL_MP(4, false, CALL); break; } } } while (0)

template <class T>
int sylvester_inv_impl(bjx_ctx* ctx, const void* q, const void* r, const void* rt, const void* b, int M, const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim,
                       int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int G = 1, R = 1;
  sylvester_shape<T>(dim, &G, &R);
  const SylvesterArgs<T> a = sylvester_args<T>(q, M, dim, batch, G);
  const int64_t cap = (int64_t)ctx->num_cu * kMapBlocksPerCu;
  const int grid = (int)(a.groups < cap ? a.groups : cap);
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  const bool al = sylvester_vector_form<T>(dim, {q, in, out});
  const int mp = sylvester_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_INV(R_, AL_, MP_) launch_inv<T, R_, AL_, MP_>(ctx, a, (const T*)r, (const T*)rt, (const T*)b, grid, in, out, ladj_ps, accum, partials)
    SYL_DISPATCH(SYL_INV);
#undef SYL_INV
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T>
int sylvester_inv_vjp_impl(bjx_ctx* ctx, const void* q, const void* r, const void* rt, const void* b, int M, const T* in, const T* zb, const T* lb, T* yb, T* pre,
                           int64_t dim, int64_t batch) {
  if (batch == 0 || (!yb && !pre)) return BJX_OK;
  int G = 1, R = 1;
  sylvester_shape<T>(dim, &G, &R);
  const SylvesterArgs<T> a = sylvester_args<T>(q, M, dim, batch, G);
  const int64_t cap = (int64_t)ctx->num_cu * kMapBlocksPerCu;
  const int grid = (int)(a.groups < cap ? a.groups : cap);
  const bool al = sylvester_vector_form<T>(dim, {q, in, zb, yb, pre});
  const int mp = sylvester_pad(M);
  {
    BjxProf prof_(ctx);
#define SYL_INV_VJP(R_, AL_, MP_) launch_inv_vjp<T, R_, AL_, MP_>(ctx, a, (const T*)r, (const T*)rt, (const T*)b, grid, in, zb, lb, yb, pre)
    SYL_DISPATCH(SYL_INV_VJP);
#undef SYL_INV_VJP
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

BJX_API int bjx_sylvester_inv(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M, const void* in, void* out,
                              void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = sylvester_inv_check(ctx, "bjx_sylvester_inv", dt, q, r, r_tilde, b, M, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || batch == 0, BJX_ERR_ARG, "bjx_sylvester_inv: null pointer");
  if (dt == BJX_F32) return sylvester_inv_impl<float>(ctx, q, r, r_tilde, b, M, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return sylvester_inv_impl<double>(ctx, q, r, r_tilde, b, M, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_sylvester_inv_vjp(bjx_ctx* ctx, bjx_dtype dt, const void* q, const void* r, const void* r_tilde, const void* b, int M, const void* in,
                                  const void* out_bar, const void* ladj_bar, void* in_bar, void* pre, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = sylvester_inv_check(ctx, "bjx_sylvester_inv_vjp", dt, q, r, r_tilde, b, M, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out_bar) || batch == 0, BJX_ERR_ARG, "bjx_sylvester_inv_vjp: null pointer");
  if (dt == BJX_F32)
    return sylvester_inv_vjp_impl<float>(ctx, q, r, r_tilde, b, M, (const float*)in, (const float*)out_bar, (const float*)ladj_bar, (float*)in_bar, (float*)pre, dim, batch);
  return sylvester_inv_vjp_impl<double>(ctx, q, r, r_tilde, b, M, (const double*)in, (const double*)out_bar, (const double*)ladj_bar, (double*)in_bar, (double*)pre, dim,
                                        batch);
}
