// bjx_chain_vjp.hip — one-pass parameter pullback of an elementwise chain with batch-shared parameters (include/bjx_chain_vjp.h):
//     p̄ = Σ_n [ ȳ_n ∂y_n/∂p + ℓ̄_n ∂ladj_n/∂p ]   for every wanted parameter slot of the chain, next to x̄.
//
// Main pass (one launch).  Per element the chain runs forward keeping every stage's closed-form partials (stage_partials of
// bjx_chain_stage.h: the arithmetic of bjx_coupling_chain_vjp), then walks back: x̄ and the summand ȳ-part + ℓ̄-part of every wanted
// slot come out of the same registers.  The ℓ̄ term rides in the summand, so the fold needs no parameter reads and one formula
// serves the kinds whose log-det derivative depends on x (LeakyReLU, Logit) and those where it does not (Scale).
//   REG  columns of whole aligned 16-byte packs, at most 64 packs: G lanes per column (one pack per lane: the lane's rows and hence
//        its parameters never change), the next column's packs in flight, a block walks a CONTIGUOUS run of columns.  Per-lane Float64
//        accumulators [pack element][slot]; then the reduction skeleton of bjx_stacked_vjp_moments: a shuffle butterfly over the
//        column groups of a wave, the four waves through LDS in a fixed order, one Float64 partial per (block, slot, row).
//   GEN  every other shape: one row per lane (RW = the next power of two >= dim lanes per column, 256 / RW columns side by side;
//        columns taller than 256 rows: row slabs of 256 on blockIdx.x), scalar loads, the column lanes of a block through LDS.
// Fold (one launch, one block per wanted slot): per row the blocks' partials in a fixed order (1024 / RW strided chains, then
// their sum in index order); epilogue: a per-row parameter gets T(row sum), a scalar the sum over the rows in index order.
// Grid sizes depend on the shape only: two identical calls give identical bits.
#include <algorithm>

#include "bjx_internal.h"
#include "../../include/bjx_chain_vjp.h"

namespace {
using namespace bjx;
#include "bjx_chain_stage.h"

constexpr int CV_MAX = BJX_CHAIN_VJP_MAX_OPS;
constexpr int64_t CV_PART_DOUBLES = (int64_t)1 << 21;   // cap of the partials of one call (16 MiB)
constexpr int CV_GRID_MAX = 2048;

// parameter j of a stage: p[j] == null -> the host scalar s[j]; else p[j][row * stride[j]] (stride 0: a device scalar)
template <class T> struct VStage {
  int kind;
  const T* p[2];
  int stride[2];
  T s[2];
};
template <class T, int NOPS> struct VLaw {
  VStage<T> st[NOPS];
  uint32_t want;            // bit i: slot i is accumulated
  int pos[2 * NOPS];        // compact index of slot i among the wanted ones
  int nw;
};

// Accumulators of one row: [k] = slot 2k (p0 of stage k), and with HASB (the chain has a two-parameter stage: Logit, Logit^-1)
// [NOPS + k] = slot 2k+1.  Chains without such a stage carry neither the second parameter nor its accumulators (half the registers).
template <int NOPS, bool HASB> constexpr int cv_nacc() { return HASB ? 2 * NOPS : NOPS; }
template <int NOPS> __host__ __device__ constexpr int cv_acc_of(int slot) { return (slot & 1) ? NOPS + (slot >> 1) : (slot >> 1); }

// one element: -> x̄; adds the summand of every wanted slot to its accumulator
template <class T, int NOPS, bool HASB>
__device__ __forceinline__ T elem_vjp(const VLaw<T, NOPS>& law, const T (&a)[NOPS], const T (&b)[NOPS], T x, T g, T lb, double (&acc)[cv_nacc<NOPS, HASB>()]) {
  StageD<T> d[NOPS];
  T v = x;
#pragma unroll
  for (int k = 0; k < NOPS; ++k) d[k] = stage_partials<T>(law.st[k].kind, v, a[k], b[k]);
  T gg = g;
#pragma unroll
  for (int k = NOPS - 1; k >= 0; --k) {
    if ((law.want >> (2 * k)) & 1u) acc[k] += (double)(gg * d[k].ya + lb * d[k].la);                  // (want: wave-uniform)
    if constexpr (HASB) {
      if ((law.want >> (2 * k + 1)) & 1u) acc[NOPS + k] += (double)(gg * d[k].yb + lb * d[k].lb);
    }
    gg = gg * d[k].dy + lb * d[k].dl;
  }
  return gg;
}

template <class T, int V, int NOPS, bool HASB>
__global__ __launch_bounds__(256) void chain_vjp_reg_kernel(const VLaw<T, NOPS> law, const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar,
                                                            T* xbar, int64_t dim, int64_t batch, int G, int64_t cols_per_block,
                                                            double* __restrict__ part, int64_t per) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* mp = reinterpret_cast<double*>(smem);            // [4 waves][dim]
  const int gl = threadIdx.x & (G - 1);
  const int cpb = 256 / G;
  const int64_t nvc = dim / V;
  const bool lane_ok = gl < nvc;
  const int64_t row = (int64_t)gl * V;
  // the lane's rows are fixed: its parameters are loaded once
  T a[V][NOPS], b[V][NOPS];
#pragma unroll
  for (int k = 0; k < NOPS; ++k) {
    const VStage<T>& s = law.st[k];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      a[j][k] = (s.p[0] && lane_ok) ? s.p[0][(row + j) * s.stride[0]] : s.s[0];
      b[j][k] = (HASB && s.p[1] && lane_ok) ? s.p[1][(row + j) * s.stride[1]] : s.s[1];
    }
  }
  constexpr int NACC = cv_nacc<NOPS, HASB>();
  double acc[V][NACC];
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[j][i] = 0.0;
  // the block's contiguous run of columns, cpb at a time; the next column's packs are in flight while this one is worked on
  const int64_t cb0 = (int64_t)blockIdx.x * cols_per_block;
  const int64_t cb1 = cb0 + cols_per_block < batch ? cb0 + cols_per_block : batch;
  int64_t col = cb0 + threadIdx.x / G;
  Pack<T, V> px, pg;
  T lb = T(0);
  bool have = lane_ok && col < cb1;
  if (have) {
    px = load_pack<T, V, true>(x + col * dim + row);
    pg = load_pack<T, V, true>(gbar + col * dim + row);
    if (lbar) lb = lbar[col];
  }
#pragma unroll 1
  for (int64_t c = cb0; c < cb1; c += cpb) {                   // (block-uniform trip count)
    const int64_t ncol = col + cpb;
    const bool have_n = lane_ok && ncol < cb1;
    Pack<T, V> nx, ng;
    T nlb = T(0);
    if (have_n) {
      nx = load_pack<T, V, true>(x + ncol * dim + row);
      ng = load_pack<T, V, true>(gbar + ncol * dim + row);
      if (lbar) nlb = lbar[ncol];
    }
    if (have) {
      Pack<T, V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = elem_vjp<T, NOPS, HASB>(law, a[j], b[j], px.v[j], pg.v[j], lb, acc[j]);
      if (xbar) store_pack<T, V, true>(xbar + col * dim + row, o);
    }
    px = nx; pg = ng; lb = nlb; have = have_n; col = ncol;
  }
  // the column groups of a wave (lanes gl, gl + G, ...: a fixed butterfly), then the four waves through LDS in index order
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 2 * NOPS; ++i) {
    if (!HASB && (i & 1)) continue;
    if (!((law.want >> i) & 1u)) continue;                   // (block-uniform)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double v = acc[j][cv_acc_of<NOPS>(i)];
      for (int m = G; m < 64; m <<= 1) v += shfl_xor(v, m);
      if ((threadIdx.x & 63) < G && lane_ok) mp[(int64_t)wv * dim + row + j] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < dim; e += 256)
      part[(int64_t)blockIdx.x * per + (int64_t)law.pos[i] * dim + e] = ((mp[e] + mp[dim + e]) + mp[2 * dim + e]) + mp[3 * dim + e];
    __syncthreads();
  }
}

template <class T, int NOPS, bool HASB>
__global__ __launch_bounds__(256) void chain_vjp_gen_kernel(const VLaw<T, NOPS> law, const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar,
                                                            T* xbar, int64_t dim, int64_t batch, int RW, int64_t cols_per_block,
                                                            double* __restrict__ part, int64_t per) {
  __shared__ double red[256];
  const int r_in = threadIdx.x & (RW - 1), q = threadIdx.x / RW, P = 256 / RW;
  const int64_t row = (int64_t)blockIdx.x * RW + r_in;
  const bool row_ok = row < dim;
  T a[NOPS], b[NOPS];
#pragma unroll
  for (int k = 0; k < NOPS; ++k) {
    const VStage<T>& s = law.st[k];
    a[k] = (s.p[0] && row_ok) ? s.p[0][row * s.stride[0]] : s.s[0];
    b[k] = (HASB && s.p[1] && row_ok) ? s.p[1][row * s.stride[1]] : s.s[1];
  }
  constexpr int NACC = cv_nacc<NOPS, HASB>();
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  const int64_t c0 = (int64_t)blockIdx.y * cols_per_block;
  const int64_t c1 = c0 + cols_per_block < batch ? c0 + cols_per_block : batch;
  if (row_ok) {
#pragma unroll 1
    for (int64_t c = c0 + q; c < c1; c += P) {
      const T xv = x[c * dim + row], gv = gbar[c * dim + row];
      const T lb = lbar ? lbar[c] : T(0);
      const T r = elem_vjp<T, NOPS, HASB>(law, a, b, xv, gv, lb, acc);
      if (xbar) xbar[c * dim + row] = r;
    }
  }
#pragma unroll
  for (int i = 0; i < 2 * NOPS; ++i) {
    if (!HASB && (i & 1)) continue;
    if (!((law.want >> i) & 1u)) continue;                   // (block-uniform)
    red[threadIdx.x] = acc[cv_acc_of<NOPS>(i)];
    __syncthreads();
    if (q == 0 && row_ok) {
      double s = 0.0;
      for (int qq = 0; qq < P; ++qq) s += red[qq * RW + r_in];
      part[(int64_t)blockIdx.y * per + (int64_t)law.pos[i] * dim + row] = s;
    }
    __syncthreads();
  }
}

// one block per wanted slot: Σ over the nb blocks' partials per row (fixed order), then the epilogue
template <class T> struct VOut {
  T* out[2 * CV_MAX];
  int vec[2 * CV_MAX];      // 1: T[dim], one value per row; 0: T[1], summed over the rows
};
template <class T>
__global__ __launch_bounds__(1024) void chain_vjp_fold_kernel(const double* __restrict__ part, int nb, int64_t per, int64_t dim, int RW, const VOut<T> o) {
  __shared__ double red[1024];
  const int k = blockIdx.x;
  const int t = threadIdx.x, r_in = t & (RW - 1), q = t / RW, P = 1024 / RW;
  const double* base = part + (int64_t)k * dim;
  double tot = 0.0;                                          // scalar parameter: this thread's rows (threads q == 0)
  for (int64_t row0 = 0; row0 < dim; row0 += RW) {
    const int64_t row = row0 + r_in;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (row < dim) {
      int b = q;
      for (; b + 3 * P < nb; b += 4 * P) {
        a0 += base[(int64_t)b * per + row];
        a1 += base[(int64_t)(b + P) * per + row];
        a2 += base[(int64_t)(b + 2 * P) * per + row];
        a3 += base[(int64_t)(b + 3 * P) * per + row];
      }
      for (; b < nb; b += P) a0 += base[(int64_t)b * per + row];
    }
    red[t] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (q == 0 && row < dim) {
      double s = 0.0;
      for (int qq = 0; qq < P; ++qq) s += red[qq * RW + r_in];
      if (o.vec[k]) o.out[k][row] = (T)s;
      else tot += s;
    }
    __syncthreads();
  }
  if (!o.vec[k]) {
    red[t] = q == 0 ? tot : 0.0;
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int i = 0; i < RW; ++i) s += red[i];
      o.out[k][0] = (T)s;
    }
  }
}

// ------------------------------------------------------------------ host side
struct KindInfo { int ck, np; };       // kernel kind, number of parameters (-1: not served, -2: unknown)
KindInfo kind_info(int kind) {
  switch (kind) {
    case BJX_OP_IDENTITY: return {CK_ID, 0};
    case BJX_OP_EXP: return {CK_EXP, 0};
    case BJX_OP_LOG: return {CK_LOG, 0};
    case BJX_OP_SHIFT: return {CK_SHIFT, 1};
    case BJX_OP_SCALE: return {CK_SCALE, 1};
    case BJX_OP_SCALE_INV: return {CK_SCALE_INV, 1};
    case BJX_OP_LOGIT: return {CK_LOGIT, 2};
    case BJX_OP_LOGIT_INV: return {CK_LOGIT_INV, 2};
    case BJX_OP_LEAKY_RELU: return {CK_LEAKY, 1};
    case BJX_OP_SIGNFLIP: return {CK_FLIP, 0};
    case BJX_OP_TRUNCATED: case BJX_OP_TRUNCATED_INV: case BJX_OP_STDNORMAL_LOGPDF: return {0, -1};
    default: return {0, -2};
  }
}

int pow2_ceil(int64_t n, int cap) {
  int r = 1;
  while (r < cap && r < n) r <<= 1;
  return r;
}

template <class T, int NOPS, bool HASB>
int launch_main(bjx_ctx* ctx, const VLaw<T, CV_MAX>& full, const T* x, const T* gb, const T* lb, T* xb, int64_t dim, int64_t batch, bool reg,
                int64_t per, int* nb_out) {
  VLaw<T, NOPS> law;
  for (int k = 0; k < NOPS; ++k) law.st[k] = full.st[k];
  for (int i = 0; i < 2 * NOPS; ++i) law.pos[i] = full.pos[i];
  law.want = full.want;
  law.nw = full.nw;
  const int64_t gcap = std::max<int64_t>(1, std::min<int64_t>(CV_GRID_MAX, CV_PART_DOUBLES / std::max<int64_t>(per, 1)));
  constexpr int VW = Vec16<T>::N;
  // Register budget (compiler's resource report, no scratch anywhere): the pack form keeps V rows' accumulators, parameters and
  // stage partials per lane — 83 / 114 VGPRs for one stage, 160 for two one-parameter stages (5 / 4 / 3 waves per SIMD), but
  // 206 ... 256 (2 or 1 waves) from three stages or two with a Logit; the one-row-per-lane form stays at 30 ... 102 (Float32) /
  // 64 ... 174 (Float64).  So the pack form serves the chains it holds at >= 3 waves per SIMD and the longer ones go one row per lane.
  constexpr bool kRegFits = NOPS == 1 || (NOPS == 2 && !HASB);
  if constexpr (kRegFits) {
   if (reg) {
    const int G = pow2_ceil(dim / VW, 64);
    const int64_t cpt = (int64_t)(256 / G) * 4;                // granule of a block's run: four steps of the column loop, so that the prefetch has a next column to overlap
    const int64_t tiles = (batch + cpt - 1) / cpt;
    const int64_t cpb = (tiles + gcap - 1) / gcap * cpt;
    const int64_t grid = (batch + cpb - 1) / cpb;
    { int rc = bjx_ensure_partials(ctx, (size_t)(grid * per)); if (rc) return rc; }
    const size_t smem = (size_t)4 * dim * sizeof(double);
    {
      BjxProf prof_(ctx);
      hipLaunchKernelGGL((chain_vjp_reg_kernel<T, VW, NOPS, HASB>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, law, x, gb, lb, xb, dim, batch, G, cpb,
                         ctx->partials, per);
    }
    BJX_CHECK_LAUNCH(ctx);
    *nb_out = (int)grid;
    return BJX_OK;
   }
  }
  const int RW = pow2_ceil(dim, 256);
  const int64_t slabs = (dim + RW - 1) / RW;
  const int P = 256 / RW;
  int64_t cpb = (batch + gcap - 1) / gcap;                     // columns per block, a multiple of P
  cpb = (cpb + P - 1) / P * P;
  const int64_t grid = (batch + cpb - 1) / cpb;
  { int rc = bjx_ensure_partials(ctx, (size_t)(grid * per)); if (rc) return rc; }
  {
    BjxProf prof_(ctx);
    hipLaunchKernelGGL((chain_vjp_gen_kernel<T, NOPS, HASB>), dim3((unsigned)slabs, (unsigned)grid), dim3(256), 0, ctx->stream, law, x, gb, lb, xb, dim, batch, RW, cpb,
                       ctx->partials, per);
  }
  BJX_CHECK_LAUNCH(ctx);
  *nb_out = (int)grid;
  return BJX_OK;
}

template <class T>
int run_impl(bjx_ctx* ctx, const bjx_op* ops, int n_ops, uint32_t mask, const T* x, const T* gb, const T* lb, T* xb, void* const* params_bar, int64_t dim,
             int64_t batch) {
  VLaw<T, CV_MAX> law;
  VOut<T> out{};
  law.want = mask;
  law.nw = 0;
  bool rows_aligned = true, hasb = false;
  for (int k = 0; k < CV_MAX; ++k) {
    VStage<T>& s = law.st[k];
    s.kind = CK_ID;
    s.p[0] = s.p[1] = nullptr;
    s.stride[0] = s.stride[1] = 0;
    s.s[0] = s.s[1] = T(0);
    law.pos[2 * k] = law.pos[2 * k + 1] = 0;
    if (k >= n_ops) continue;
    const KindInfo ki = kind_info(ops[k].kind);
    s.kind = ki.ck;
    if (ki.np == 2) hasb = true;
    for (int j = 0; j < ki.np; ++j) {
      const void* v = j == 0 ? ops[k].v0 : ops[k].v1;
      s.s[j] = (T)(j == 0 ? ops[k].p0 : ops[k].p1);
      const bool per_row = v && ops[k].param_len > 1;
      if (v) {
        s.p[j] = static_cast<const T*>(v);
        s.stride[j] = per_row ? 1 : 0;
        if (per_row && !bjx_aligned16(v)) rows_aligned = false;
      }
      const int i = 2 * k + j;
      if ((mask >> i) & 1u) {
        law.pos[i] = law.nw;
        out.out[law.nw] = static_cast<T*>(params_bar[i]);
        out.vec[law.nw] = per_row ? 1 : 0;
        ++law.nw;
      }
    }
  }
  if (batch == 0) {                                            // zeros (a fill, no launch)
    for (int k = 0; k < law.nw; ++k) BJX_HIP(ctx, hipMemsetAsync(out.out[k], 0, (size_t)(out.vec[k] ? dim : 1) * sizeof(T), ctx->stream));
    return BJX_OK;
  }
  constexpr int VW = Vec16<T>::N;
  const bool reg = dim % VW == 0 && dim / VW <= 64 && bjx_aligned16(x) && bjx_aligned16(gb) && (!xb || bjx_aligned16(xb)) && rows_aligned;
  const int64_t per = (int64_t)std::max(law.nw, 1) * dim;
  int nb = 0, rc;
#define CV_MAIN(N_) (hasb ? launch_main<T, N_, true>(ctx, law, x, gb, lb, xb, dim, batch, reg, per, &nb) : launch_main<T, N_, false>(ctx, law, x, gb, lb, xb, dim, batch, reg, per, &nb))
  switch (n_ops) {
    case 1: rc = CV_MAIN(1); break;
    case 2: rc = CV_MAIN(2); break;
    case 3: rc = CV_MAIN(3); break;
    default: rc = CV_MAIN(4); break;
  }
#undef CV_MAIN
  if (rc || law.nw == 0) return rc;
  {
    BjxProf prof_(ctx);
    hipLaunchKernelGGL(chain_vjp_fold_kernel<T>, dim3((unsigned)law.nw), dim3(1024), 0, ctx->stream, ctx->partials, nb, per, dim, pow2_ceil(dim, 1024), out);
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

// validation shared by the direct entry and the plan (launches nothing)
int bjx_chain_vjp_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, const bjx_op* ops, int n_ops, uint32_t mask, int64_t dim) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, dim >= 1 && dim < ((int64_t)1 << 31), BJX_ERR_SHAPE, "%s: bad number of rows %lld", name, (long long)dim);
  BJX_REQUIRE(ctx, ops && n_ops >= 1, BJX_ERR_ARG, "%s: empty op list", name);
  BJX_REQUIRE(ctx, n_ops <= CV_MAX, BJX_ERR_UNSUPPORTED, "%s: %d stages (at most %d are fused)", name, n_ops, CV_MAX);
  BJX_REQUIRE(ctx, (mask >> (2 * n_ops)) == 0, BJX_ERR_ARG, "%s: a wanted slot beyond the %d slots of %d stages", name, 2 * n_ops, n_ops);
  for (int k = 0; k < n_ops; ++k) {
    const KindInfo ki = kind_info(ops[k].kind);
    BJX_REQUIRE(ctx, ki.np != -2, BJX_ERR_ARG, "%s: op %d has unknown kind %d", name, k, (int)ops[k].kind);
    BJX_REQUIRE(ctx, ki.np != -1, BJX_ERR_UNSUPPORTED, "%s: op %d (kind %d) is not served (identity, exp, log, Shift, Scale, Scale^-1, Logit, Logit^-1, LeakyReLU, SignFlip)",
                name, k, (int)ops[k].kind);
    BJX_REQUIRE(ctx, ops[k].param_len == 0 || ops[k].param_len == 1 || ops[k].param_len == dim, BJX_ERR_SHAPE, "%s: op %d has a parameter of length %d for %lld rows",
                name, k, (int)ops[k].param_len, (long long)dim);
    BJX_REQUIRE(ctx, ops[k].param_len <= 1 || ki.np == 0 || ops[k].v0 || (ki.np == 2 && ops[k].v1), BJX_ERR_ARG,
                "%s: op %d has per-row parameters but no device pointer", name, k);
    for (int j = ki.np; j < 2; ++j)
      BJX_REQUIRE(ctx, !((mask >> (2 * k + j)) & 1u), BJX_ERR_ARG, "%s: params_bar[%d] wanted, but op %d has no such parameter", name, 2 * k + j, k);
  }
  return BJX_OK;
}

int bjx_chain_vjp_run(bjx_ctx* ctx, bjx_dtype dt, const bjx_op* ops, int n_ops, uint32_t mask, const void* x, const void* y_bar, const void* ladj_bar,
                      void* x_bar, void* const* params_bar, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, batch >= 0, BJX_ERR_SHAPE, "bjx_chain_vjp_params: negative batch");
  BJX_REQUIRE(ctx, (x && y_bar) || batch == 0, BJX_ERR_ARG, "bjx_chain_vjp_params: null pointer");
  BJX_REQUIRE(ctx, x_bar != x || batch == 0 || !x_bar, BJX_ERR_ARG, "bjx_chain_vjp_params: x_bar may not alias x");
  if (dt == BJX_F32)
    return run_impl<float>(ctx, ops, n_ops, mask, (const float*)x, (const float*)y_bar, (const float*)ladj_bar, (float*)x_bar, params_bar, dim, batch);
  return run_impl<double>(ctx, ops, n_ops, mask, (const double*)x, (const double*)y_bar, (const double*)ladj_bar, (double*)x_bar, params_bar, dim, batch);
}

BJX_API int bjx_chain_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const bjx_op* ops, int n_ops, const void* x, const void* y_bar, const void* ladj_bar, void* x_bar,
                                 void* const* params_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  uint32_t mask = 0;
  if (params_bar && ops && n_ops >= 1 && n_ops <= CV_MAX)
    for (int i = 0; i < 2 * n_ops; ++i)
      if (params_bar[i]) mask |= 1u << i;
  const int rc = bjx_chain_vjp_check(ctx, "bjx_chain_vjp_params", dt, ops, n_ops, mask, dim);
  if (rc) return rc;
  return bjx_chain_vjp_run(ctx, dt, ops, n_ops, mask, x, y_bar, ladj_bar, x_bar, params_bar, dim, batch);
}
