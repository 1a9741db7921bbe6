// bjx_coupling_chain.hip — Coupling(θ, mask) whose law is a short chain of elementwise bijectors with per-sample parameters
// (include/bjx_coupling.h): coupling.jl:178-181, 206-259 with b = θ(x₂) any composition of exp / log / Shift / Scale / Logit /
// LeakyReLU / SignFlip stages, the parameters of every stage a host scalar, one value per x₁-row, or one value per x₁-row AND column.
//
// Forward / inverse: a functor of the column-group skeleton (bjx_stream.h), the mapping of the affine coupling (CouplingAffineF):
// G lanes per column, 16-byte packs along the rows, four columns in flight per lane group, the row map in LDS.  The law sits in
// the functor (kernel arguments: the stage kinds and parameter sources are wave-uniform, the stage `switch` is a scalar branch);
// the parameter packs of a data pack are fetched together with it — one 16-byte load per per-sample array when the pack's rows are
// consecutive, aligned positions of x₁ (a row-range mask), V gathers otherwise (scattered masks, odd heights).  The inverse is the
// same kernel on the inverted stage list (last stage first: coupling.jl:236-250), built on the host.  Per-column log-det: the
// skeleton's butterfly over the column's lanes; summed log-det: the context's partials and finalize (fixed order, no atomics).
//
// Pullback: one pass, the mapping of coupling_affine_vjp_kernel.  Per x₁ element the law runs forward keeping every stage's input
// (at most 4 values) and its closed-form partials, then walks back: x̄ and the cotangent of every requested per-sample parameter
// come out of the same registers.  Inverse direction: the pre-image is recomputed and the implicit rule applied —
//   x = X(y, θ), ℓ = −L(x, θ):   ȳ = (x̄ − ℓ̄ L_x) / y_x =: r,   θ̄ = −r y_θ − ℓ̄ L_θ   (the forward law's walk with (−r, −ℓ̄)).
#include "bjx_stream.h"
#include "../../include/bjx_coupling.h"

namespace {
using namespace bjx;

#include "bjx_chain_stage.h"      // the stage kinds CK_* and stage_partials

// parameter j of a stage: p[j] == null -> the scalar s[j]; else p[j][r + col*ld[j]] (ld 0: one value per row for every column)
template <class T> struct CStage {
  int kind, ikind;          // the stage, and its inverse (pullback of the inverse direction: the pre-image)
  const T* p[2];
  int64_t ld[2];
  T s[2];
};
template <class T, int NOPS> struct CLaw { CStage<T> st[NOPS]; };

// one stage on the V elements of a pack: value and log-det terms (the arithmetic of apply_kind in bjx_chain.hip; Scale's log|a| is
// a term of every element here, its parameter being per-sample).  The `switch` is OUTSIDE the element loop, as in apply_kind: one
// scalar branch chain per stage and pack, not per element.
#define BJX_CC_FORJ _Pragma("unroll") for (int j = 0; j < V; ++j)
template <class T, int V> __device__ __forceinline__ void stage_fwd_pack(const int kind, T (&v)[V], const T* a, const T* b, T (&l)[V]) {
  using F = Fast<T>;
  switch (kind) {
    case CK_EXP: BJX_CC_FORJ { l[j] += v[j]; v[j] = F::exp(v[j]); } break;                                   // exp_log.jl:5-6
    case CK_LOG: BJX_CC_FORJ { const T t = F::log(v[j]); l[j] -= t; v[j] = t; } break;                       // exp_log.jl:8-9
    case CK_SHIFT: BJX_CC_FORJ v[j] = a[j] + v[j]; break;                                                    // shift.jl:14
    case CK_SHIFT_INV: BJX_CC_FORJ v[j] = v[j] - a[j]; break;                                                // shift.jl:12: Shift(-a)
    case CK_SCALE: BJX_CC_FORJ { l[j] += F::log(d_abs(a[j])); v[j] = a[j] * v[j]; } break;                   // scale.jl:13,26-32
    case CK_SCALE_INV: BJX_CC_FORJ { l[j] -= F::log(d_abs(a[j])); v[j] = F::rcp(a[j]) * v[j]; } break;       // scale.jl:15-16
    case CK_LOGIT:                                                                                          // logit.jl:15,24-30
      BJX_CC_FORJ {
        const T xa = v[j] - a[j], xb = b[j] - v[j];
        l[j] -= F::log(xa * xb * F::rcp(b[j] - a[j]));
        v[j] = F::log(xa * F::rcp(xb));                     // logit((x-a)/(b-a)) = log((x-a)/(b-x)): ±Inf at the bounds
      }
      break;
    case CK_LOGIT_INV:                                                                                      // logit.jl:19-21; interface.jl:276-281
      BJX_CC_FORJ {
        const T w = b[j] - a[j];
        const T x = w * f_logistic(v[j]) + a[j];
        l[j] += F::log((x - a[j]) * (b[j] - x) * F::rcp(w));
        v[j] = x;
      }
      break;
    case CK_LEAKY: BJX_CC_FORJ { const T J = v[j] < T(0) ? a[j] : T(1); l[j] += F::log(d_abs(J)); v[j] = J * v[j]; } break;              // leaky_relu.jl:25-29
    case CK_LEAKY_INV: BJX_CC_FORJ { const T J = v[j] < T(0) ? F::rcp(a[j]) : T(1); l[j] += F::log(d_abs(J)); v[j] = J * v[j]; } break;  // leaky_relu.jl:16
    case CK_FLIP: BJX_CC_FORJ v[j] = -v[j]; break;                                                           // ordered.jl:3
    case CK_AFFINE: BJX_CC_FORJ { l[j] += F::log(d_abs(a[j])); v[j] = b[j] + a[j] * v[j]; } break;           // Shift(b) ∘ Scale(a)
    case CK_AFFINE_INV: BJX_CC_FORJ { l[j] -= F::log(d_abs(a[j])); v[j] = F::rcp(a[j]) * (v[j] - b[j]); } break;   // inverse(Scale) ∘ inverse(Shift)
    default: break;
  }
}
template <class T> __device__ __forceinline__ void stage_fwd(const int kind, T& v, const T a, const T b, T& l) {
  T vv[1] = {v}, aa[1] = {a}, bb[1] = {b}, ll[1] = {l};
  stage_fwd_pack<T, 1>(kind, vv, aa, bb, ll);
  v = vv[0]; l = ll[0];
}

template <class T, int NOPS> struct CouplingChainF {
  static constexpr bool kLoadInput = true;
  static constexpr bool kMasked = true;           // fetch() takes any first row; apply_masked drops the log-det terms of rows outside the mask
  const int32_t* map;       // row -> position in idx1, or -1
  CLaw<T, NOPS> law;        // application order of THIS call (already inverted for inverse = 1)
  int map_in_lds;
  int64_t dim;
  double per_sample_const;
  const double* per_sample_dev;
  int walk_smem_offset = 0;
  // the parameters of one data pack, slot 2k + j = parameter j of stage k (a fixed slot per parameter: every register index is a
  // compile-time constant; a scalar source is broadcast into its slot)
  template <int V> struct AuxV { Pack<T, V> q[2 * NOPS]; uint32_t on; };
  using Aux = AuxV<Vec16<T>::N>;
  __device__ void stage(char* smem) const {
    if (!map_in_lds) return;
    int32_t* m = reinterpret_cast<int32_t*>(smem);
    for (int64_t i = threadIdx.x; i < dim; i += blockDim.x) m[i] = map[i];
    __syncthreads();
  }
  template <int V> __device__ Aux fetch(const char* smem, int64_t row, int64_t col) const {
    if (map_in_lds) return fetch_from<V>(reinterpret_cast<const int32_t*>(smem), row, col);   // two calls: each keeps its address space
    return fetch_from<V>(map, row, col);
  }
  template <int V> __device__ __forceinline__ Aux fetch_from(const int32_t* m, int64_t row, int64_t col) const {
    static_assert(V <= Vec16<T>::N, "pack wider than Aux");
    Aux a;
    a.on = 0;
    int32_t mi[V];
    bool run = V > 1;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      mi[j] = m[row + j];
      if (mi[j] >= 0) a.on |= 1u << j;
      run = run && mi[j] == mi[0] + j;
    }
    run = run && mi[0] >= 0 && (mi[0] % V) == 0;
#pragma unroll
    for (int i = 0; i < 2 * NOPS; ++i) {
      const T* p = law.st[i >> 1].p[i & 1];
      const int64_t ld = law.st[i >> 1].ld[i & 1];
      const T sc = law.st[i >> 1].s[i & 1];
#pragma unroll
      for (int j = 0; j < V; ++j) a.q[i].v[j] = sc;
      if (p && a.on) {                                      // (p: wave-uniform)
        const T* pc = p + col * ld;
        if (run && (ld % V) == 0 && bjx_aligned16_dev(p)) {
          Pack<T, V> t;
          if (ld) t = load_pack<T, V, true>(pc + mi[0]); else t = load_pack<T, V, false>(pc + mi[0]);   // per-row vectors are re-read by every column
#pragma unroll
          for (int j = 0; j < V; ++j) a.q[i].v[j] = t.v[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (mi[j] >= 0) a.q[i].v[j] = pc[mi[j]];
        }
      }
    }
    return a;
  }
  template <int V> __device__ T apply(const char* sm, Pack<T, V>& p, const Aux& a, const T* xc, int64_t row, int64_t col) const {
    return apply_masked<V>(sm, p, a, xc, row, col, ~0u);
  }
  template <int V> __device__ T apply_masked(const char*, Pack<T, V>& p, const Aux& a, const T*, int64_t, int64_t, uint32_t mask) const {
    T l = T(0);
    if (a.on) {
      T v[V], lj[V];
#pragma unroll
      for (int j = 0; j < V; ++j) { v[j] = p.v[j]; lj[j] = T(0); }
#pragma unroll
      for (int k = 0; k < NOPS; ++k) {
        stage_fwd_pack<T, V>(law.st[k].kind, v, a.q[2 * k].v, a.q[2 * k + 1].v, lj);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool on = (a.on >> j) & (mask >> j) & 1u;      // rows outside x₁ keep their value whatever the stages made of it
        if (on) { p.v[j] = v[j]; l += lj[j]; }
      }
    }
    return l;
  }
};

// ------------------------------------------------------------------ pullback
template <class T, int NOPS> struct CBars { T* p[NOPS][2]; };

// one x₁ element: -> x̄ (forward) / ȳ (inverse); writes the requested parameter cotangents at [r + col*n1]
template <class T, int NOPS, bool INV>
__device__ __forceinline__ T elem_vjp(const CLaw<T, NOPS>& law, const CBars<T, NOPS>& bars, int64_t col, int32_t r, int64_t n1, T in, T g, T lb) {
  T a[NOPS], b[NOPS];
#pragma unroll
  for (int k = 0; k < NOPS; ++k) {
    const CStage<T>& s = law.st[k];
    a[k] = s.p[0] ? s.p[0][col * s.ld[0] + r] : s.s[0];
    b[k] = s.p[1] ? s.p[1][col * s.ld[1] + r] : s.s[1];
  }
  T v = in;
  if (INV) {                                                // the pre-image x = law⁻¹(y)
    T dummy = T(0);
#pragma unroll
    for (int k = NOPS - 1; k >= 0; --k) stage_fwd<T>(law.st[k].ikind, v, a[k], b[k], dummy);
  }
  StageD<T> d[NOPS];
#pragma unroll
  for (int k = 0; k < NOPS; ++k) d[k] = stage_partials<T>(law.st[k].kind, v, a[k], b[k]);
  T gg = g, ll = lb, res = T(0);
  if (INV) {
    T A = T(1), Bq = T(0);                                  // x̄ = A ȳ + Bq ℓ̄ of the forward law: A = y_x, Bq = L_x
#pragma unroll
    for (int k = NOPS - 1; k >= 0; --k) { Bq = Bq * d[k].dy + d[k].dl; A = A * d[k].dy; }
    res = (g - lb * Bq) / A;
    gg = -res;
    ll = -lb;
  }
#pragma unroll
  for (int k = NOPS - 1; k >= 0; --k) {
    if (bars.p[k][0]) bars.p[k][0][col * n1 + r] = gg * d[k].ya + ll * d[k].la;
    if (bars.p[k][1]) bars.p[k][1][col * n1 + r] = gg * d[k].yb + ll * d[k].lb;
    gg = gg * d[k].dy + ll * d[k].dl;
  }
  return INV ? res : gg;
}

// G lanes per column, 4 columns in flight, the row map in LDS (coupling_affine_vjp_kernel)
template <class T, int V, int NOPS, bool INV>
__global__ __launch_bounds__(256) void coupling_chain_vjp_kernel(const int32_t* __restrict__ map, const CLaw<T, NOPS> law, const CBars<T, NOPS> bars,
                                                                 const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int64_t n1,
                                                                 int64_t dim, int64_t batch, int G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* m = reinterpret_cast<int32_t*>(smem);
  for (int64_t i = threadIdx.x; i < dim; i += blockDim.x) m[i] = map[i];
  __syncthreads();
  const int gl = threadIdx.x & (G - 1);
  const int cols_per_block = 256 / G;
  const int64_t nvc = dim / V;
  constexpr int UC = 4;
  const int64_t col0 = (int64_t)blockIdx.x * cols_per_block * UC + threadIdx.x / G;
  for (int64_t pv = gl; pv < nvc; pv += G) {
    const int64_t row = pv * V;
    Pack<T, V> px[UC], pg[UC];
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      const int64_t col = col0 + (int64_t)u * cols_per_block;
      if (col < batch) { px[u] = load_pack<T, V, true>(x + col * dim + row); pg[u] = load_pack<T, V, true>(gbar + col * dim + row); }
    }
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      const int64_t col = col0 + (int64_t)u * cols_per_block;
      if (col >= batch) continue;
      const T lb = lbar ? lbar[col] : T(0);
      Pack<T, V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int32_t mi = m[row + j];
        T out = pg[u].v[j];                                   // rows outside x₁ pass ȳ through
        if (mi >= 0) out = elem_vjp<T, NOPS, INV>(law, bars, col, mi, n1, px[u].v[j], pg[u].v[j], lb);
        o.v[j] = out;
      }
      store_pack<T, V, true>(xbar + col * dim + row, o);
    }
  }
}

// ------------------------------------------------------------------ host side
// rowmap as build_rowmap in bjx_elem.hip (-1 = copy-through row); an index outside [0, dim) is skipped, never written through
__global__ void chain_rowmap_kernel(const int32_t* idx1, int64_t n1, int64_t dim, int32_t* map) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n1) {
    const int32_t r = idx1[i];
    if (r >= 0 && r < dim) map[r] = (int32_t)i;
  }
}

int chain_rowmap(bjx_ctx* ctx, const char* name, const int32_t* idx1, int64_t n1, int64_t dim, int32_t** map_out) {
  BJX_REQUIRE(ctx, (size_t)dim * sizeof(int32_t) + 16 <= BJX_SCRATCH_BYTES, BJX_ERR_UNSUPPORTED, "%s: dim %lld too large for the context scratch", name, (long long)dim);
  int32_t* map = static_cast<int32_t*>(ctx->scratch);
  BJX_HIP(ctx, hipMemsetAsync(map, 0xFF, (size_t)dim * sizeof(int32_t), ctx->stream));
  if (n1 > 0) {
    hipLaunchKernelGGL(chain_rowmap_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, ctx->stream, idx1, n1, dim, map);
    BJX_CHECK_LAUNCH(ctx);
  }
  *map_out = map;
  return BJX_OK;
}

struct KindInfo { int ck, ick, np; };       // kernel kind, its inverse, number of parameters (-1: not served, -2: unknown)
KindInfo kind_info(int kind) {
  switch (kind) {
    case BJX_OP_IDENTITY: return {CK_ID, CK_ID, 0};
    case BJX_OP_EXP: return {CK_EXP, CK_LOG, 0};
    case BJX_OP_LOG: return {CK_LOG, CK_EXP, 0};
    case BJX_OP_SHIFT: return {CK_SHIFT, CK_SHIFT_INV, 1};
    case BJX_OP_SCALE: return {CK_SCALE, CK_SCALE_INV, 1};
    case BJX_OP_SCALE_INV: return {CK_SCALE_INV, CK_SCALE, 1};
    case BJX_OP_LOGIT: return {CK_LOGIT, CK_LOGIT_INV, 2};
    case BJX_OP_LOGIT_INV: return {CK_LOGIT_INV, CK_LOGIT, 2};
    case BJX_OP_LEAKY_RELU: return {CK_LEAKY, CK_LEAKY_INV, 1};
    case BJX_OP_SIGNFLIP: return {CK_FLIP, CK_FLIP, 0};
    case BJX_OP_AFFINE: return {CK_AFFINE, CK_AFFINE_INV, 2};
    case BJX_OP_TRUNCATED: case BJX_OP_TRUNCATED_INV: case BJX_OP_STDNORMAL_LOGPDF: return {0, 0, -1};
    default: return {0, 0, -2};
  }
}

// the law as the kernels take it (4 slots, stages beyond n are CK_ID), validated; `bars` (may be null) checked against the sources
template <class T>
int law_build(bjx_ctx* ctx, const char* name, const bjx_op* ops, int n_ops, const void* const* params, const int64_t* ld_params, void* const* params_bar,
              int64_t n1, CLaw<T, BJX_COUPLING_MAX_OPS>* law, CBars<T, BJX_COUPLING_MAX_OPS>* bars) {
  BJX_REQUIRE(ctx, ops && n_ops >= 1, BJX_ERR_ARG, "%s: empty op list", name);
  BJX_REQUIRE(ctx, n_ops <= BJX_COUPLING_MAX_OPS, BJX_ERR_UNSUPPORTED, "%s: %d stages (at most %d are fused)", name, n_ops, BJX_COUPLING_MAX_OPS);
  for (int k = 0; k < BJX_COUPLING_MAX_OPS; ++k) {
    CStage<T>& s = law->st[k];
    s.kind = s.ikind = CK_ID;
    s.p[0] = s.p[1] = nullptr;
    s.ld[0] = s.ld[1] = 0;
    s.s[0] = s.s[1] = T(0);
    if (bars) bars->p[k][0] = bars->p[k][1] = nullptr;
    if (k >= n_ops) continue;
    const KindInfo ki = kind_info(ops[k].kind);
    BJX_REQUIRE(ctx, ki.np != -2, BJX_ERR_ARG, "%s: op %d has unknown kind %d", name, k, (int)ops[k].kind);
    BJX_REQUIRE(ctx, ki.np != -1, BJX_ERR_UNSUPPORTED, "%s: op %d (kind %d) is not served as a coupling law (identity, exp, log, Shift, Scale, Scale^-1, Logit, Logit^-1, LeakyReLU, SignFlip, affine)",
                name, k, (int)ops[k].kind);
    s.kind = ki.ck;
    s.ikind = ki.ick;
    for (int j = 0; j < 2; ++j) {
      const int i = 2 * k + j;
      const void* p = params ? params[i] : nullptr;
      const int64_t ld = ld_params ? ld_params[i] : 0;
      void* pb = params_bar ? params_bar[i] : nullptr;
      if (j >= ki.np) {
        BJX_REQUIRE(ctx, !pb, BJX_ERR_ARG, "%s: params_bar[%d] set, but op %d has no such parameter", name, i, k);
        continue;
      }
      s.s[j] = (T)(j == 0 ? ops[k].p0 : ops[k].p1);
      if (p) {
        BJX_REQUIRE(ctx, ld == 0 || ld >= n1, BJX_ERR_SHAPE, "%s: ld_params[%d] = %lld (0 for a per-row vector, >= n1 = %lld for a per-sample array)", name, i, (long long)ld, (long long)n1);
        s.p[j] = static_cast<const T*>(p);
        s.ld[j] = ld;
      }
      BJX_REQUIRE(ctx, !pb || (p && ld >= n1 && ld > 0), BJX_ERR_ARG, "%s: params_bar[%d] set, but parameter %d is not per-sample (scalar and per-row parameters get no cotangent here)", name, i, i);
      if (bars) bars->p[k][j] = static_cast<T*>(pb);
    }
  }
  return BJX_OK;
}

int chain_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const int32_t* idx1, int64_t n1, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, dim >= 0 && batch >= 0 && n1 >= 0 && n1 <= dim, BJX_ERR_SHAPE, "%s: bad size (n1=%lld, dim=%lld, batch=%lld)", name, (long long)n1, (long long)dim, (long long)batch);
  BJX_REQUIRE(ctx, idx1 || n1 == 0, BJX_ERR_ARG, "%s: null idx1", name);
  return BJX_OK;
}

template <class T, int NOPS>
int chain_launch(bjx_ctx* ctx, const int32_t* map, const CLaw<T, BJX_COUPLING_MAX_OPS>& full, int inverse, int n_ops, const T* in, T* out, T* ladj_ps,
                 double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  CouplingChainF<T, NOPS> f{};
  f.map = map;
  for (int k = 0; k < NOPS; ++k) {
    f.law.st[k] = full.st[inverse ? n_ops - 1 - k : k];
    if (inverse) f.law.st[k].kind = f.law.st[k].ikind;
  }
  f.map_in_lds = dim <= 12 * 1024 ? 1 : 0;
  f.dim = dim;
  f.per_sample_const = 0.0;
  f.per_sample_dev = nullptr;
  const size_t fsm = f.map_in_lds ? (size_t)dim * sizeof(int32_t) + 16 : 0;
  return launch_colgroup<T>(ctx, f, fsm, in, out, ladj_ps, ladj_sum, dim, batch, flags & BJX_ACCUMULATE, 0.0);
}

template <class T>
int chain_impl(bjx_ctx* ctx, int inverse, const int32_t* idx1, int64_t n1, const bjx_op* ops, int n_ops, const void* const* params, const int64_t* ld_params,
               const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  CLaw<T, BJX_COUPLING_MAX_OPS> law;
  int rc = law_build<T>(ctx, "bjx_coupling_chain", ops, n_ops, params, ld_params, nullptr, n1, &law, nullptr);
  if (rc) return rc;
  if (dim * batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  int32_t* map = nullptr;
  rc = chain_rowmap(ctx, "bjx_coupling_chain", idx1, n1, dim, &map);
  if (rc) return rc;
  switch (n_ops) {
    case 1: return chain_launch<T, 1>(ctx, map, law, inverse, n_ops, in, out, ladj_ps, ladj_sum, dim, batch, flags);
    case 2: return chain_launch<T, 2>(ctx, map, law, inverse, n_ops, in, out, ladj_ps, ladj_sum, dim, batch, flags);
    case 3: return chain_launch<T, 3>(ctx, map, law, inverse, n_ops, in, out, ladj_ps, ladj_sum, dim, batch, flags);
    default: return chain_launch<T, 4>(ctx, map, law, inverse, n_ops, in, out, ladj_ps, ladj_sum, dim, batch, flags);
  }
}

template <class T, int NOPS>
void chain_vjp_launch(bjx_ctx* ctx, const int32_t* map, const CLaw<T, BJX_COUPLING_MAX_OPS>& full, const CBars<T, BJX_COUPLING_MAX_OPS>& fbars, int inverse,
                      bool v_ok, int64_t grid, size_t smem, const T* in, const T* gb, const T* lb, T* xb, int64_t n1, int64_t dim, int64_t batch, int G) {
  CLaw<T, NOPS> law;
  CBars<T, NOPS> bars;
  for (int k = 0; k < NOPS; ++k) { law.st[k] = full.st[k]; bars.p[k][0] = fbars.p[k][0]; bars.p[k][1] = fbars.p[k][1]; }
  constexpr int VW = Vec16<T>::N;
#define CCV(V_, I_) hipLaunchKernelGGL((coupling_chain_vjp_kernel<T, V_, NOPS, I_>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, map, law, bars, in, gb, lb, xb, n1, dim, batch, G)
  if (v_ok) { if (inverse) CCV(VW, true); else CCV(VW, false); }
  else { if (inverse) CCV(1, true); else CCV(1, false); }
#undef CCV
}

template <class T>
int chain_vjp_impl(bjx_ctx* ctx, int inverse, const int32_t* idx1, int64_t n1, const bjx_op* ops, int n_ops, const void* const* params,
                   const int64_t* ld_params, const T* in, const T* out_bar, const T* ladj_bar, T* in_bar, void* const* params_bar, int64_t dim, int64_t batch) {
  CLaw<T, BJX_COUPLING_MAX_OPS> law;
  CBars<T, BJX_COUPLING_MAX_OPS> bars;
  int rc = law_build<T>(ctx, "bjx_coupling_chain_vjp", ops, n_ops, params, ld_params, params_bar, n1, &law, &bars);
  if (rc) return rc;
  if (dim * batch == 0) return BJX_OK;
  const size_t smem = (size_t)dim * sizeof(int32_t);
  BJX_REQUIRE(ctx, smem <= 60 * 1024, BJX_ERR_UNSUPPORTED, "bjx_coupling_chain_vjp: dim %lld too large for the LDS row map", (long long)dim);
  int32_t* map = nullptr;
  rc = chain_rowmap(ctx, "bjx_coupling_chain_vjp", idx1, n1, dim, &map);
  if (rc) return rc;
  constexpr int VW = Vec16<T>::N;
  const bool v_ok = bjx_aligned16(in) && bjx_aligned16(out_bar) && bjx_aligned16(in_bar) && dim % VW == 0;
  const int64_t packs = dim / (v_ok ? VW : 1);             // heights that are not whole packs: one element per lane
  int G = 1;
  while (G < 64 && G < packs) G <<= 1;
  const int64_t cpb = (int64_t)(256 / G) * 4;
  const int64_t grid = (batch + cpb - 1) / cpb;
  BJX_REQUIRE(ctx, grid < (int64_t)1 << 31, BJX_ERR_UNSUPPORTED, "bjx_coupling_chain_vjp: batch too large for one launch");
  {
    BjxProf prof_(ctx);
    switch (n_ops) {
      case 1: chain_vjp_launch<T, 1>(ctx, map, law, bars, inverse, v_ok, grid, smem, in, out_bar, ladj_bar, in_bar, n1, dim, batch, G); break;
      case 2: chain_vjp_launch<T, 2>(ctx, map, law, bars, inverse, v_ok, grid, smem, in, out_bar, ladj_bar, in_bar, n1, dim, batch, G); break;
      case 3: chain_vjp_launch<T, 3>(ctx, map, law, bars, inverse, v_ok, grid, smem, in, out_bar, ladj_bar, in_bar, n1, dim, batch, G); break;
      default: chain_vjp_launch<T, 4>(ctx, map, law, bars, inverse, v_ok, grid, smem, in, out_bar, ladj_bar, in_bar, n1, dim, batch, G); break;
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_coupling_chain(bjx_ctx* ctx, bjx_dtype dt, int inverse, const int32_t* idx1, int64_t n1, const bjx_op* ops, int n_ops,
                               const void* const* params, const int64_t* ld_params, const void* in, void* out, void* ladj_ps, double* ladj_sum,
                               int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = chain_check(ctx, "bjx_coupling_chain", dt, idx1, n1, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || dim * batch == 0, BJX_ERR_ARG, "bjx_coupling_chain: null pointer");
  if (dt == BJX_F32)
    return chain_impl<float>(ctx, inverse, idx1, n1, ops, n_ops, params, ld_params, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return chain_impl<double>(ctx, inverse, idx1, n1, ops, n_ops, params, ld_params, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_coupling_chain_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const int32_t* idx1, int64_t n1, const bjx_op* ops, int n_ops,
                                   const void* const* params, const int64_t* ld_params, const void* in, const void* out_bar, const void* ladj_bar,
                                   void* in_bar, void* const* params_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = chain_check(ctx, "bjx_coupling_chain_vjp", dt, idx1, n1, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out_bar && in_bar) || dim * batch == 0, BJX_ERR_ARG, "bjx_coupling_chain_vjp: null pointer");
  if (dt == BJX_F32)
    return chain_vjp_impl<float>(ctx, inverse, idx1, n1, ops, n_ops, params, ld_params, (const float*)in, (const float*)out_bar, (const float*)ladj_bar,
                                 (float*)in_bar, params_bar, dim, batch);
  return chain_vjp_impl<double>(ctx, inverse, idx1, n1, ops, n_ops, params, ld_params, (const double*)in, (const double*)out_bar, (const double*)ladj_bar,
                                (double*)in_bar, params_bar, dim, batch);
}
