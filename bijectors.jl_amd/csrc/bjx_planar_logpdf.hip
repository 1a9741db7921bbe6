// bjx_planar_logpdf.hip — log-density of transformed(N(μ, diag σ²), l_L ∘ … ∘ l_1) at y for a run of PlanarLayers, with ȳ and the
// cotangents of every layer's parameters and of μ, σ (include/bjx_planar_logpdf.h).
//   the pass       planar_logpdf_cols_kernel, the sibling of planar_vjp_cols_kernel<…, INV = true> (bjx_flow_cols.hip: a block owns C
//                  columns at a time, the columns in registers) and, for Float32 whole packs with 16 < dim <= 128 on aligned bases,
//                  planar_logpdf_reg_kernel, the sibling of planar_vjp_reg_kernel<G, NL, true, false> (bjx_flow_vjp_reg.hip).
//                  Primal sweep: all L inverse layers — the column ends as x = f⁻¹(y), the templates skip the last update; at x:
//                  w = (x − μ)/σ, one more reduction for ‖w‖², ℓ from the saved t's, lp; x goes to the work buffer and the seed −c·w/σ
//                  into the registers that held it; cotangent sweep: the template's, and every layer's (−s̄, t) goes to the work tables.
//   layers         the reduction stage of bjx_planar_vjp_params (bjx::planar_param_reduce_launch, bjx_flow.hip) on (x, ȳ, c, −s̄),
//                  then planar_logpdf_negate_kernel on its three results (the stage is jointly linear in (ȳ, c, s̄)).
//   μ̄, σ̄          planar_logpdf_base_kernel over the stored x (Float64 from (x − μ) directly, one partial set per block) and
//                  planar_logpdf_base_fold_kernel (fixed order).
#include "bjx_internal.h"
#include <type_traits>
#include "../../include/bjx_planar_logpdf.h"

namespace {
using namespace bjx;

#include "bjx_flow_common.inc"
#include "bjx_flow_cols.inc"
#include "bjx_flow_reg.inc"

template <class T> struct PlanarLogpdf {
  const T *mu, *sigma, *lp_bar;      // NULL: 0 / 1 / 1
  T *lp_ps, *xs, *s_tab, *t_tab, *ones;
};

template <class T, int V, int R, int C, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu((R <= 4 && sizeof(T) == 4) ? 4 : 1, 8))) void planar_logpdf_cols_kernel(const PlanarArgs<T> A, const T* __restrict__ y, T* __restrict__ ybar, int64_t dim,
                                                                int64_t batch, const PlanarLogpdf<T> Q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NWV = NT / 64;
  constexpr bool PF = R <= 4;                          // as planar_vjp_cols_kernel: parameter rows requested ahead of the barrier
  T* red = reinterpret_cast<T*>(smem);                 // [2][NWV][C]
  T* tsave = red + 2 * NWV * C;                        // [C][n_layers], then Σ log σ + (d/2) log 2π
  const int nl = A.n_layers;
  const int64_t nvc = (dim + V - 1) / V;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cme = lane & (C - 1);
  int nrow[R];
  int64_t off[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t v = threadIdx.x + (int64_t)r * NT;
    off[r] = v * V;
    nrow[r] = v < nvc ? (int)(dim - v * V < V ? dim - v * V : V) : 0;
  }
  int par = 0;
  auto reduce = [&](const T (&s)[C]) -> T {
    const T v = wave_sum_scatter<T, C>(s, lane);
    T* rp = red + par * NWV * C;
    if ((lane & (64 / C - 1)) == 0) rp[wv * C + lane / (64 / C)] = v;
    __syncthreads();
    T a = T(0);
#pragma unroll
    for (int q = 0; q < NWV; ++q) a += rp[q * C + cme];
    par ^= 1;
    return a;
  };
  auto load_row = [&](const T* row, Pack<T, V> (&p)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (nrow[r] > 0) p[r] = load_pack_part<T, V>(row + off[r], nrow[r]);
      else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[r].v[j] = T(0);
      }
    }
  };
  auto load_par = [&](const T* row, Pack<T, V> (&p)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (nrow[r] > 0) p[r] = load_pack_part_cached<T, V>(row + off[r], nrow[r]);
      else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[r].v[j] = T(0);
      }
    }
  };
  // Σ log σ + (d/2) log 2π, once per block: every thread its rows in Float64, one block reduction
  // (kept in the LDS slot behind tsave, not in a register across the sweeps)
  T lpconst = (T)dim * T(0.91893853320467274178);
  if (Q.sigma) {
    double ls = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r)
      for (int j = 0; j < nrow[r]; ++j) ls += log((double)Q.sigma[off[r] + j]);
    T s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = (T)ls;
    lpconst += reduce(s);
  }
  if (threadIdx.x == 0) tsave[C * nl] = lpconst;
  const int64_t tiles = (batch + C - 1) / C;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t col0 = tile * C;
    Pack<T, V> z[C][R];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int64_t col = col0 + c < batch ? col0 + c : batch - 1;
      load_row(y + col * dim, z[c]);
    }
    const bool me_ok = col0 + cme < batch;
    // ---- primal sweep: the inverse of every layer, the last one first; the column ends as x
    Pack<T, V> pw[R], pu[R], pnx[R];
    if (PF) load_par(A.w + (int64_t)(nl - 1) * dim, pw);
    for (int li = 0; li < nl; ++li) {
      const int l = nl - 1 - li;
      const bool more = li + 1 < nl;
      if constexpr (PF) load_par(A.u_hat + (int64_t)l * dim, pu);
      else load_par(A.w + (int64_t)l * dim, pw);
      T s[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        s[c] = T(0);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) s[c] += pw[r].v[j] * z[c][r].v[j];
      }
      if constexpr (PF) { if (more) load_par(A.w + (int64_t)(l - 1) * dim, pnx); }
      const T sme = reduce(s);
      T tme, s2;
      planar_inv_act<T>(sme, A.wtu_hat[l], A.b[l], tme, s2);
      if (threadIdx.x < C) tsave[threadIdx.x * nl + l] = tme;
      if constexpr (!PF) load_par(A.u_hat + (int64_t)l * dim, pu);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T a = -lane_bcast(tme, c);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) z[c][r].v[j] += pu[r].v[j] * a;
      }
      if constexpr (PF) {
        if (more) {
#pragma unroll
          for (int r = 0; r < R; ++r) pw[r] = pnx[r];
        }
      }
    }
    // ---- at x: store it, w = (x − μ)/σ, lp, and the seed x̄ = −c·w/σ into the same registers
    if (Q.xs) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (col0 + c < batch) {
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (nrow[r] > 0) store_pack_part<T, V>(Q.xs + (col0 + c) * dim + off[r], z[c][r], nrow[r]);
        }
      }
    }
    if (Q.mu) load_par(Q.mu, pw);
    if (Q.sigma) load_par(Q.sigma, pu);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (!Q.mu) pw[r].v[j] = T(0);
        pu[r].v[j] = j < nrow[r] ? (Q.sigma ? T(1) / pu[r].v[j] : T(1)) : T(0);       // 1/σ; rows that do not exist: 0
      }
    const T lbme = me_ok ? (Q.lp_bar ? Q.lp_bar[col0 + cme] : T(1)) : T(0);
    {
      T q[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        q[c] = T(0);
        const T cc = lane_bcast(lbme, c);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T wv_ = (z[c][r].v[j] - pw[r].v[j]) * pu[r].v[j];
            q[c] += wv_ * wv_;
            z[c][r].v[j] = -(cc * wv_) * pu[r].v[j];
          }
      }
      const T qme = reduce(q);
      if (threadIdx.x < C && me_ok) {                  // (thread c < C wrote the t's of column c itself: no barrier needed to read them)
        if (Q.lp_ps) {
          T ld = T(0);                                   // ℓ of the inverse run from the saved t's: −Σ log1p(c_l·sech²), planar_layer.jl:107
          for (int l = 0; l < nl; ++l) { const T t = tsave[cme * nl + l]; ld += Fast<T>::log1p(A.wtu_hat[l] * (T(1) - t * t)); }
          Q.lp_ps[col0 + cme] = T(-0.5) * qme - tsave[C * nl] - ld;
        }
        if (Q.ones) Q.ones[col0 + cme] = T(1);
      }
    }
    __syncthreads();                                   // tsave complete
    // ---- cotangent sweep of the inverse run: level 0 (x̄) up to level L (ȳ)
    if (PF) load_par(A.u_hat, pu);
    for (int li = 0; li < nl; ++li) {
      const int l = li;
      const bool more = li + 1 < nl;
      if constexpr (PF) load_par(A.w + (int64_t)l * dim, pw);
      else load_par(A.u_hat + (int64_t)l * dim, pu);
      T d[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        d[c] = T(0);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) d[c] += pu[r].v[j] * z[c][r].v[j];
      }
      if constexpr (PF) { if (more) load_par(A.u_hat + (int64_t)(l + 1) * dim, pnx); }
      const T dme = reduce(d);
      const T cw = A.wtu_hat[l];
      const T t = tsave[cme * nl + l];
      const T q = T(1) - t * t;
      const T den = T(1) + cw * q;
      const T sbme = q / den * (-dme + lbme * T(2) * cw * t / den);
      if (Q.s_tab && threadIdx.x < C && me_ok) { Q.s_tab[(col0 + cme) * nl + l] = -sbme; Q.t_tab[(col0 + cme) * nl + l] = t; }
      if constexpr (!PF) load_par(A.w + (int64_t)l * dim, pw);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T sb = lane_bcast(sbme, c);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < V; ++j) z[c][r].v[j] += pw[r].v[j] * sb;
      }
      if constexpr (PF) {
        if (more) {
#pragma unroll
          for (int r = 0; r < R; ++r) pu[r] = pnx[r];
        }
      }
    }
    if (ybar) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (col0 + c < batch) {
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (nrow[r] > 0) store_pack_part<T, V>(ybar + (col0 + c) * dim + off[r], z[c][r], nrow[r]);
        }
      }
    }
    __syncthreads();                                   // tsave is rewritten by the next tile
  }
}

// ------------------------------------------------------------------ the same pass on the one-wave register tile (Float32)
// The sibling of planar_vjp_reg_kernel<G, NL, true, false> (bjx_flow_vjp_reg.hip): a wave holds a 64-column tile, lane (gl, cg) the rows
// 4gl … 4gl+3 of the columns r·(64/G) + cg, and runs the layers' recurrence with lane = column on the tables of planar_prep_reg_kernel.
// Whole 16-byte packs, 16 < dim <= 128.  The primal sweep updates the tile after the LAST group too (the column ends as x); at x the
// G per-column partial sums of ‖w‖² a lane holds are summed over the group's lanes by halving exchanges (lane gl ends with column
// gl·(64/G) + cg) and handed to lane = column through the LDS, as the cotangent c comes the other way.
template <int C> __device__ __forceinline__ float group_scatter_sum(const float (&s)[C], int gl) {
  if constexpr (C == 1) return s[0];
  else {
    constexpr int H = C / 2;
    const bool hi = gl & H;
    float a[H];
#pragma unroll
    for (int i = 0; i < H; ++i) a[i] = (hi ? s[H + i] : s[i]) + shfl_xor(hi ? s[i] : s[H + i], H);
    return group_scatter_sum<H>(a, gl);
  }
}

template <int G, int NL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void planar_logpdf_reg_kernel(const PlanarRegArgs A, const float* __restrict__ y, float* __restrict__ ybar, int dim,
                                                                                                        int64_t batch, int nl, const PlanarLogpdf<float> Q) {
  constexpr int COLS = 64;
  constexpr int CPS = 64 / G;
  constexpr int NS = (COLS * G) / 64;
  static_assert(NS == G, "a lane holds G columns");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* st = reinterpret_cast<float*>(smem) + (size_t)wave * COLS * NL;
  float* tsave = reinterpret_cast<float*>(smem) + (size_t)4 * COLS * NL + (size_t)wave * COLS * A.nl_pad;   // [column][layer]
  const int gl = lane & (G - 1);
  const int cg = lane / G;
  const int64_t col0 = ((int64_t)blockIdx.x * 4 + wave) * COLS;
  const bool row_ok = 4 * gl < dim;
  const int64_t left = batch - col0;
  const int nvalid = left >= COLS ? COLS : (left > 0 ? (int)left : 0);
  const int64_t step_elems = (int64_t)CPS * dim;
  const int64_t tile_off = (col0 + cg) * dim + 4 * gl;
  bjx_f4 z[NS];
  {
    const float* px = y + tile_off;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      if (row_ok && r * CPS + cg < nvalid) z[r] = __builtin_nontemporal_load(reinterpret_cast<const bjx_f4*>(px));
      else z[r] = bjx_f4{0.f, 0.f, 0.f, 0.f};
      px += step_elems;
    }
  }
  auto store_tile = [&](float* base) {
    float* py = base + tile_off;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      if (row_ok && r * CPS + cg < nvalid) __builtin_nontemporal_store(z[r], reinterpret_cast<bjx_f4*>(py));
      py += step_elems;
    }
  };
  const int ngroups = A.nl_pad / NL;
  // ---- primal sweep: the inverse of every layer, the LAST group first; the tile ends as x
  for (int gi = 0; gi < ngroups; ++gi) {
    const int l0 = (ngroups - 1 - gi) * NL;
    reg_dots<G, NL, NS>(A.w, l0, dim, z, st, lane, gl, cg, row_ok);
    __builtin_amdgcn_wave_barrier();
    {
      float s[NL], t[NL];
#pragma unroll
      for (int k = 0; k < NL; ++k) { s[k] = st[lane * NL + k]; t[k] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < NL; ++kk) {
        const int k = NL - 1 - kk;
        const float* Gk = A.G + (int64_t)(l0 + k) * A.nl_pad + l0;
        float a = s[k];
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          if (j > k) a += Gk[j] * t[j];                               // t holds -tanh
        }
        float th, ld;
        find_alpha_act(a, A.wtu_hat[l0 + k], A.b[l0 + k], th, ld);
        t[k] = -th;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < NL; ++k) { st[lane * NL + k] = t[k]; tsave[lane * A.nl_pad + l0 + k] = -t[k]; }
    }
    __builtin_amdgcn_wave_barrier();
    reg_update<G, NL, NS>(A.u_hat, l0, dim, z, st, gl, cg, row_ok);   // after the last group too: the templates reload the tile instead
    __builtin_amdgcn_wave_barrier();
  }
  // ---- at x: store it, w = (x − μ)/σ, lp, and the seed x̄ = −c·w/σ into the same registers
  if (Q.xs) store_tile(Q.xs);
  const float lb = lane < nvalid ? (Q.lp_bar ? Q.lp_bar[col0 + lane] : 1.0f) : 0.f;
  {
    bjx_f4 m4 = bjx_f4{0.f, 0.f, 0.f, 0.f}, rs4 = m4;
    float lsum = 0.f;
    if (row_ok) {
      if (Q.mu) m4 = *reinterpret_cast<const bjx_f4*>(Q.mu + 4 * gl);
      rs4 = bjx_f4{1.f, 1.f, 1.f, 1.f};
      if (Q.sigma) {
        const bjx_f4 s4 = *reinterpret_cast<const bjx_f4*>(Q.sigma + 4 * gl);
        rs4 = rs4 / s4;
        lsum = (logf(s4.x) + logf(s4.y)) + (logf(s4.z) + logf(s4.w));
      }
    }
#pragma unroll
    for (int h = G / 2; h >= 1; h >>= 1) lsum += shfl_xor(lsum, h);   // Σ log σ over the rows: every group of G lanes holds all of them
    st[lane] = lb;
    __builtin_amdgcn_wave_barrier();
    float q[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      const float cc = st[r * CPS + cg];
      const bjx_f4 w4 = (z[r] - m4) * rs4;
      q[r] = (w4.x * w4.x + w4.y * w4.y) + (w4.z * w4.z + w4.w * w4.w);
      z[r] = -(w4 * cc) * rs4;
    }
    const float qs = group_scatter_sum<NS>(q, gl);                    // lane gl: the column gl·CPS + cg
    __builtin_amdgcn_wave_barrier();
    st[gl * CPS + cg] = qs;
    __builtin_amdgcn_wave_barrier();
    if (lane < nvalid) {
      if (Q.lp_ps) {
        float ld = 0.f;                                              // ℓ of the inverse run from the saved t's (planar_layer.jl:107); padding layers left out
        for (int l = 0; l < nl; ++l) { const float t = tsave[lane * A.nl_pad + l]; ld += Fast<float>::log1p(A.wtu_hat[l] * (1.0f - t * t)); }
        Q.lp_ps[col0 + lane] = -0.5f * st[lane] - (lsum + (float)dim * 0.91893853320467274178f) - ld;
      }
      if (Q.ones) Q.ones[col0 + lane] = 1.0f;
    }
    __builtin_amdgcn_wave_barrier();
  }
  // ---- cotangent sweep of the inverse run: level 0 (x̄) up to level L (ȳ)
  for (int gi = 0; gi < ngroups; ++gi) {
    const int l0 = gi * NL;
    reg_dots<G, NL, NS>(A.u_hat, l0, dim, z, st, lane, gl, cg, row_ok);
    __builtin_amdgcn_wave_barrier();
    {
      float g[NL], sb[NL];
#pragma unroll
      for (int k = 0; k < NL; ++k) { g[k] = st[lane * NL + k]; sb[k] = 0.f; }
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        float tb = g[k];
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          if (j < k) tb += A.G[(int64_t)(l0 + j) * A.nl_pad + l0 + k] * sb[j];   // û_kᵀ w_j
        }
        const float t = tsave[lane * A.nl_pad + l0 + k], c = A.wtu_hat[l0 + k];
        const float q = 1.0f - t * t;
        const float rden = Fast<float>::rcp(1.0f + c * q);
        sb[k] = q * rden * (-tb + lb * 2.0f * c * t * rden);        // find_alpha rule: dα/d(wᵀy) = 1/(1 + c q)
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < NL; ++k) st[lane * NL + k] = sb[k];
      if (Q.s_tab && lane < nvalid) {                      // (−s̄, t) of every layer, [batch][n_layers]: input of the reduction stage
#pragma unroll
        for (int k = 0; k < NL; ++k)
          if (l0 + k < nl) { Q.s_tab[(col0 + lane) * nl + l0 + k] = -sb[k]; Q.t_tab[(col0 + lane) * nl + l0 + k] = tsave[lane * A.nl_pad + l0 + k]; }
      }
    }
    __builtin_amdgcn_wave_barrier();
    reg_update<G, NL, NS>(A.w, l0, dim, z, st, gl, cg, row_ok);
    __builtin_amdgcn_wave_barrier();
  }
  if (ybar) store_tile(ybar);
}

// μ̄ = Σ c·w/σ, σ̄ = Σ c·(w² − 1)/σ over the stored x, w = (x − μ)/σ in Float64.  A block owns TR rows (thread t: row t % TR) and
// walks the columns blockIdx.y·CG + t / TR, + gridDim.y·CG, …; the CG column groups are added in a fixed order through the LDS and
// the block writes ONE partial set [2][dim] slice.
template <class T>
__global__ __launch_bounds__(256) void planar_logpdf_base_kernel(const T* __restrict__ x, const T* __restrict__ mu, const T* __restrict__ sigma, const T* __restrict__ c,
                                                                 int64_t dim, int64_t batch, int TR, double* __restrict__ partial) {
  __shared__ double red[2][256];
  const int CG = 256 / TR;
  const int rl = threadIdx.x % TR, cg = threadIdx.x / TR;
  const int64_t row = (int64_t)blockIdx.x * TR + rl;
  double am = 0.0, as = 0.0;
  if (row < dim) {
    const double m = mu ? (double)mu[row] : 0.0;
    const double rs = sigma ? 1.0 / (double)sigma[row] : 1.0;
    for (int64_t n = (int64_t)blockIdx.y * CG + cg; n < batch; n += (int64_t)gridDim.y * CG) {
      const double cn = c ? (double)c[n] : 1.0;
      const double wv = ((double)x[n * dim + row] - m) * rs;
      am += cn * wv * rs;
      as += cn * (wv * wv - 1.0) * rs;
    }
  }
  red[0][threadIdx.x] = am;
  red[1][threadIdx.x] = as;
  __syncthreads();
  if (cg == 0 && row < dim) {
    double a = 0.0, b = 0.0;
    for (int g = 0; g < CG; ++g) { a += red[0][g * TR + rl]; b += red[1][g * TR + rl]; }
    partial[((size_t)blockIdx.y * 2) * dim + row] = a;
    partial[((size_t)blockIdx.y * 2 + 1) * dim + row] = b;
  }
}

template <class T>
__global__ __launch_bounds__(256) void planar_logpdf_base_fold_kernel(const double* __restrict__ partial, int nsets, int64_t dim, T* __restrict__ mu_bar, T* __restrict__ sigma_bar) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * dim) return;
  T* dst = e < dim ? (mu_bar ? mu_bar + e : nullptr) : (sigma_bar ? sigma_bar + (e - dim) : nullptr);
  if (!dst) return;
  double s = 0.0;
  for (int i = 0; i < nsets; ++i) s += partial[(size_t)i * 2 * dim + e];
  *dst = (T)s;
}

template <class T>
__global__ __launch_bounds__(256) void planar_logpdf_negate_kernel(T* __restrict__ w_bar, T* __restrict__ u_bar, T* __restrict__ b_bar, int64_t n_tab, int nl) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_tab) { w_bar[e] = -w_bar[e]; u_bar[e] = -u_bar[e]; }
  if (e < nl) b_bar[e] = -b_bar[e];
}

template <class T>
int planar_logpdf_impl(bjx_ctx* ctx, const T* w, const T* u, const T* b, int nl, const T* mu, const T* sigma, const T* y, const T* lp_bar, T* lp_ps, T* y_bar,
                       T* w_bar, T* u_bar, T* b_bar, T* mu_bar, T* sigma_bar, T* work, int64_t dim, int64_t batch) {
  constexpr int VW = Vec16<T>::N;
  constexpr bool is_f64 = std::is_same<T, double>::value;
  const bool want_layers = w_bar != nullptr, want_base = mu_bar || sigma_bar;
  // ---- what the pass serves, decided before anything is launched (the geometry of planar_vjp_cols_launch)
  const int64_t packs = (dim + VW - 1) / VW;
  const size_t tab_bytes = (((size_t)nl * dim + nl) * sizeof(T) + 255) / 256 * 256;
  BJX_REQUIRE(ctx, dim >= 2 * VW && packs <= 256 * 32, BJX_ERR_UNSUPPORTED, "bjx_planar_logpdf_vjp_params: columns of %lld rows are not fused", (long long)dim);
  BJX_REQUIRE(ctx, (size_t)nl * 16 * sizeof(T) <= 32 * 1024 && tab_bytes <= BJX_SCRATCH_BYTES, BJX_ERR_UNSUPPORTED,
              "bjx_planar_logpdf_vjp_params: %d layers of %lld rows are not fused", nl, (long long)dim);
  BJX_REQUIRE(ctx, batch < ((int64_t)1 << 40), BJX_ERR_UNSUPPORTED, "bjx_planar_logpdf_vjp_params: batch too large");
  if (batch == 0) {
    if (want_layers) {
      BJX_HIP(ctx, hipMemsetAsync(w_bar, 0, (size_t)nl * dim * sizeof(T), ctx->stream));
      BJX_HIP(ctx, hipMemsetAsync(u_bar, 0, (size_t)nl * dim * sizeof(T), ctx->stream));
      BJX_HIP(ctx, hipMemsetAsync(b_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
    }
    if (mu_bar) BJX_HIP(ctx, hipMemsetAsync(mu_bar, 0, (size_t)dim * sizeof(T), ctx->stream));
    if (sigma_bar) BJX_HIP(ctx, hipMemsetAsync(sigma_bar, 0, (size_t)dim * sizeof(T), ctx->stream));
    return BJX_OK;
  }
  // ---- the work buffer (include/bjx_planar_logpdf.h)
  T *s_tab = nullptr, *t_tab = nullptr, *xs = nullptr, *ones = nullptr, *yb = y_bar;
  if (want_layers || want_base) {
    T* p = work;
    auto up4 = [](size_t n) { return (n + 3) / 4 * 4; };
    if (want_layers) { s_tab = p; t_tab = p + (size_t)nl * batch; p += up4((size_t)2 * nl * batch); }
    xs = p; p += up4((size_t)dim * batch);
    if (want_layers && !y_bar) { yb = p; p += up4((size_t)dim * batch); }
    if (want_layers && !lp_bar) ones = p;
  }
  T* u_hat = static_cast<T*>(ctx->scratch);
  T* wtu = u_hat + (size_t)nl * dim;
  { int rc = planar_prep_launch<T>(ctx, w, u, nl, dim, u_hat, wtu); if (rc) return rc; }
  bool on_reg = false;
  if constexpr (!is_f64) {
    // the one-wave register tile: whole packs on 16-byte aligned bases, 16 < dim <= 128, through planar_prep_reg_kernel's tables
    const int NL = nl >= 8 ? 8 : (nl > 2 ? 4 : nl);
    const int nl_pad = (nl + NL - 1) / NL * NL;
    const size_t off0 = ((size_t)nl * dim + nl + 3) / 4 * 4;
    const size_t need_reg = (off0 + (size_t)2 * nl_pad * dim + (size_t)nl_pad * nl_pad + 2 * (size_t)nl_pad) * sizeof(float);
    const size_t smem = (size_t)4 * 64 * (NL + nl_pad) * sizeof(float);
    const int64_t grid = (batch + 4 * 64 - 1) / (4 * 64);
    on_reg = dim % 4 == 0 && dim > 16 && dim <= 128 && bjx_aligned16(y) && bjx_aligned16(yb) && bjx_aligned16(xs) && bjx_aligned16(mu) && bjx_aligned16(sigma) &&
             need_reg <= BJX_SCRATCH_BYTES && smem <= 64 * 1024 && grid < ((int64_t)1 << 31);
    if (on_reg) {
      float* wp = u_hat + off0;
      float* up = wp + (size_t)nl_pad * dim;
      float* Gp = up + (size_t)nl_pad * dim;
      float* cp = Gp + (size_t)nl_pad * nl_pad;
      float* bp = cp + nl_pad;
      hipLaunchKernelGGL(planar_prep_reg_kernel<float>, dim3(nl_pad * nl_pad), dim3(256), 0, ctx->stream, w, (const float*)u_hat, (const float*)wtu, b, dim, nl, nl_pad, wp, up, Gp, cp, bp, dim, 0);
      BJX_CHECK_LAUNCH(ctx);
      const PlanarRegArgs RA{wp, up, Gp, cp, bp, nl_pad, nl, (int)dim, 0, 0};
      const PlanarLogpdf<float> Q{mu, sigma, lp_bar, lp_ps, xs, s_tab, t_tab, ones};
      const int G = dim > 64 ? 32 : (dim > 32 ? 16 : 8);
      BjxProf prof_(ctx);
#define PLR(G_, NL_) hipLaunchKernelGGL((planar_logpdf_reg_kernel<G_, NL_>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, RA, y, yb, (int)dim, batch, nl, Q)
#define PLR_NL(G_) switch (NL) { case 1: PLR(G_, 1); break; case 2: PLR(G_, 2); break; case 4: PLR(G_, 4); break; default: PLR(G_, 8); break; }
      switch (G) { case 8: PLR_NL(8) break; case 16: PLR_NL(16) break; default: PLR_NL(32) break; }
#undef PLR_NL
#undef PLR
    }
  }
  if (!on_reg) {
    // threads per block x packs per thread: the smallest NT·R that covers the column (NT = 64 … 256 in waves, R a power of two)
    int NTc = 256, Rc = 32;
    for (int r = 32; r >= 1; r >>= 1)
      for (int nt = 256; nt >= (r == 1 ? 64 : (r <= 4 ? 192 : 256)); nt -= 64)
        if ((int64_t)nt * r >= packs && nt * r <= NTc * Rc) { NTc = nt; Rc = r; }
    const int Cc = Rc == 1 ? (is_f64 ? 16 : 8) : (Rc >= 16 ? 1 : 16 / Rc);
    const int64_t tiles = (batch + Cc - 1) / Cc;
    const int64_t capc = (int64_t)ctx->num_cu * (2048 / NTc);
    const int gridc = (int)(tiles < capc ? tiles : capc);
    PlanarArgs<T> Ac{w, u_hat, wtu, b, nl, 0};
    const PlanarLogpdf<T> Q{mu, sigma, lp_bar, lp_ps, xs, s_tab, t_tab, ones};
    const size_t smem_c = ((size_t)2 * (NTc / 64) * Cc + (size_t)Cc * nl + 1) * sizeof(T);
    BjxProf prof_(ctx);
#define PLC(R_, C_, NT_) hipLaunchKernelGGL((planar_logpdf_cols_kernel<T, VW, R_, C_, NT_>), dim3(gridc), dim3(NT_), smem_c, ctx->stream, Ac, y, yb, dim, batch, Q)
    if constexpr (is_f64) {
      if (Rc == 1) { switch (NTc) { case 64: PLC(1, 16, 64); break; case 128: PLC(1, 16, 128); break; case 192: PLC(1, 16, 192); break; default: PLC(1, 16, 256); break; } }
    }
    if (is_f64 && Rc == 1) {}
    else if (NTc == 64) PLC(1, 8, 64);
    else if (NTc == 128) PLC(1, 8, 128);
    else if (NTc == 192) { switch (Rc) { case 1: PLC(1, 8, 192); break; case 2: PLC(2, 8, 192); break; default: PLC(4, 4, 192); break; } }
    else switch (Rc) { case 1: PLC(1, 8, 256); break; case 2: PLC(2, 8, 256); break; case 4: PLC(4, 4, 256); break; case 8: PLC(8, 2, 256); break; case 16: PLC(16, 1, 256); break; default: PLC(32, 1, 256); break; }
#undef PLC
  }
  BJX_CHECK_LAUNCH(ctx);
  if (want_base) {
    int TR = 256;
    while (TR / 2 >= dim && TR > 4) TR /= 2;
    const int CG = 256 / TR;
    const int64_t chunks = (dim + TR - 1) / TR;
    int64_t S = ((int64_t)ctx->num_cu * 4 + chunks - 1) / chunks;
    const int64_t s_cols = (batch + (int64_t)CG * 64 - 1) / ((int64_t)CG * 64);      // at least 64 columns per thread's walk
    if (S > s_cols) S = s_cols;
    if (S > 256) S = 256;
    if (S < 1) S = 1;
    { int rc = bjx_ensure_partials(ctx, (size_t)S * 2 * dim); if (rc) return rc; }
    hipLaunchKernelGGL(planar_logpdf_base_kernel<T>, dim3((unsigned)chunks, (unsigned)S), dim3(256), 0, ctx->stream, (const T*)xs, mu, sigma, lp_bar, dim, batch, TR, ctx->partials);
    hipLaunchKernelGGL(planar_logpdf_base_fold_kernel<T>, dim3((unsigned)((2 * dim + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)ctx->partials, (int)S, dim, mu_bar, sigma_bar);
    BJX_CHECK_LAUNCH(ctx);
  }
  if (want_layers) {
    const int rc = planar_param_reduce_launch<T>(ctx, w, u, nl, xs, yb, lp_bar ? lp_bar : ones, s_tab, t_tab, u_hat, wtu, w_bar, u_bar, b_bar, dim, batch);
    if (rc) return rc;
    const int64_t n_tab = (int64_t)nl * dim;
    hipLaunchKernelGGL(planar_logpdf_negate_kernel<T>, dim3((unsigned)((n_tab + 255) / 256)), dim3(256), 0, ctx->stream, w_bar, u_bar, b_bar, n_tab, nl);
    BJX_CHECK_LAUNCH(ctx);
  }
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_planar_logpdf_vjp_params(bjx_ctx* ctx, bjx_dtype dt, const void* w, const void* u, const void* b, int n_layers, const void* mu, const void* sigma,
                                         const void* y, const void* lp_bar, void* lp_ps, void* y_bar, void* w_bar, void* u_bar, void* b_bar, void* mu_bar,
                                         void* sigma_bar, void* work, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0 && n_layers >= 1, BJX_ERR_SHAPE, "bjx_planar_logpdf_vjp_params: bad size");
  const int nbar = (w_bar != nullptr) + (u_bar != nullptr) + (b_bar != nullptr);
  BJX_REQUIRE(ctx, w && u && b && (y || batch == 0) && (nbar == 0 || nbar == 3), BJX_ERR_ARG,
              "bjx_planar_logpdf_vjp_params: null pointer (w_bar, u_bar, b_bar: all three or none)");
  BJX_REQUIRE(ctx, work || batch == 0 || !(nbar || mu_bar || sigma_bar), BJX_ERR_ARG, "bjx_planar_logpdf_vjp_params: work is needed for the summed outputs");
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "bjx_planar_logpdf_vjp_params: bad dtype %d", (int)dt);
  if (dt == BJX_F32) return planar_logpdf_impl<float>(ctx, (const float*)w, (const float*)u, (const float*)b, n_layers, (const float*)mu, (const float*)sigma, (const float*)y, (const float*)lp_bar, (float*)lp_ps, (float*)y_bar, (float*)w_bar, (float*)u_bar, (float*)b_bar, (float*)mu_bar, (float*)sigma_bar, (float*)work, dim, batch);
  return planar_logpdf_impl<double>(ctx, (const double*)w, (const double*)u, (const double*)b, n_layers, (const double*)mu, (const double*)sigma, (const double*)y, (const double*)lp_bar, (double*)lp_ps, (double*)y_bar, (double*)w_bar, (double*)u_bar, (double*)b_bar, (double*)mu_bar, (double*)sigma_bar, (double*)work, dim, batch);
}
