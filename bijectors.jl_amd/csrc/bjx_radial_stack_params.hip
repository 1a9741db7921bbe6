// bjx_radial_stack_params.hip — parameter pullback of a RUN of RadialLayers l_L ∘ … ∘ l_1 and of its inverse, one streaming pass
// (include/bjx_radial_stack_params.h).  The sweeps are radial_stack_vjp_kernel's (bjx_radial_stack.hip): the primal sweep leaves one
// or two scalars per layer and column in LDS, the reverse sweep rewinds the resident column.  At layer k the reverse sweep holds the
// layer's input (δ = z − z₀ₖ, r), the cotangent ḡ of its output, dg = δᵀḡ and, after the update, the cotangent ḡ′ of its input:
//   forward run   z̄₀ₖ += ḡ − ḡ′;  g_β̂ = h·dg + ℓ̄[(d−1)h/a + (h − h²r)/D];  g_α̂ = −h²[β̂·dg + ℓ̄((d−1)β̂/a + (β̂ − 2β̂hr)/D)]
//                 (h = 1/(α̂+r), a = 1 + β̂h, D = a − β̂h²r: radial_param_partial_kernel of bjx_flow.hip)
//   inverse run   the implicit-function rule per layer: the same formulas at the pre-image (δ_pre = gain·δ_in, r = gain·γ) with the
//                 cotangents (−ḡ′, −ℓ̄); δ_preᵀḡ′ = (gain·dg − kl·r²)/(a + c·r²) — the dv/(a + c r²) of rs_coef, no second reduction;
//                 z̄₀ₖ += ḡ − ḡ′ again (the forward input pullback of (−ḡ′, −ℓ̄) is −ḡ).
//   at the end    ᾱ_ = σ(α_)(Σg_α̂ − Σg_β̂),  β̄ = σ(β)·Σg_β̂                                  (the raw parameters behind softplus)
//
// Sums over the batch.  Blocks are persistent: a block walks many column tiles and keeps its sums ON CHIP, in Float64, per layer
// [z̄₀ (dim) | Σg_α̂ | Σg_β̂]:
//   group form  per layer and tile every lane holds ḡ − ḡ′ of its rows (summed over its UC columns); a shuffle butterfly over the
//               column groups of the wave (lanes gl, gl + G, …), then lanes < G add into the wave's PRIVATE LDS table — one writer
//               per entry, the LDS queue of a wave is in order: no atomics.  The four waves' tables are added in a fixed order at
//               the end of the block.
//   walk form   (one wave per block) the 64 lanes' ḡ − ḡ′ go through a [DMAX][65] Float64 LDS tile; lane (row, segment) sums its
//               segment of the row, a butterfly over the segments, lanes < DMAX add into the block's table.
// One [L, dim + 2] Float64 partial per BLOCK (not per tile) goes to the context's partials; one or two fold launches add them in a
// fixed order and cast to T at the very end.  Two identical calls give identical bits.
#include "bjx_internal.h"
#include "bjx_tile.h"
#include "../../include/bjx_radial_stack_params.h"

namespace {
using namespace bjx;
#include "bjx_flow_common.inc"
#include "bjx_radial_stack_common.inc"

constexpr int RSP_TILES_MIN = 4;        // a block walks at least this many tiles before the grid grows (table staging and the block's partial are per block)
constexpr int RSP_FOLD_CHUNK = 32;      // block partials one thread of the first fold adds

// g_α̂ and g_β̂ of one column from r, the dot product dgx and ℓ̄ (forward: δᵀḡ, ℓ̄; inverse: −δ_preᵀḡ′, −ℓ̄)
template <class T>
__device__ __forceinline__ void rsp_terms(T rr, T alpha, T bh, T dim_m1, T dgx, T lbx, T& ga, T& gb) {
  const T h = T(1) / (alpha + rr);
  const T a = T(1) + bh * h;
  const T ia = T(1) / a, iD = T(1) / (a - bh * h * h * rr);
  gb = h * dgx + lbx * (dim_m1 * h * ia + (h - h * h * rr) * iD);
  ga = -h * h * (bh * dgx + lbx * (dim_m1 * bh * ia + (bh - T(2) * bh * h * rr) * iD));
}
// the dot product and ℓ̄ rsp_terms takes, from what the reverse sweep holds
template <class T, bool INV>
__device__ __forceinline__ void rsp_dot(T a, T c, T kl, T rr, T gain, T dg, T lb, T& dgx, T& lbx) {
  if (!INV) { dgx = dg; lbx = lb; }
  else { dgx = -((gain * dg - kl * rr * rr) / (a + c * rr * rr)); lbx = -lb; }
}

// ------------------------------------------------------------------ group form
// LDS: [sc][tab][stash: (256/G)·UC column slots x L·NS of T][acc: 4 waves x L x (dim + 2) of double]
template <class T, int V, int R, bool INV>
__global__ __launch_bounds__(256) void radial_stack_params_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                  const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int64_t dim,
                                                                  int64_t batch, int G, int64_t tiles, double* __restrict__ partials) {
#pragma clang fp contract(off)
  constexpr int UC = StackVjpUC<R>::value;
  constexpr int NS = INV ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cols_per_block = blockDim.x / G;
  const int AW = (int)dim + 2;
  T* sc = reinterpret_cast<T*>(smem);
  const size_t tab_off = rs_round16((size_t)2 * n_layers * sizeof(T));
  T* tab = reinterpret_cast<T*>(smem + tab_off);
  const size_t stash_off = tab_off + rs_round16((size_t)n_layers * dim * sizeof(T));
  T* stash = reinterpret_cast<T*>(smem + stash_off);
  double* acc = reinterpret_cast<double*>(smem + stash_off + rs_round16((size_t)cols_per_block * UC * n_layers * NS * sizeof(T)));
  rs_stage_tables<T>(alpha_, beta, z0, n_layers, dim, sc, tab);
  for (int i = threadIdx.x; i < 4 * n_layers * AW; i += blockDim.x) acc[i] = 0.0;
  __syncthreads();

  const int gl = threadIdx.x & (G - 1);
  const int wl = threadIdx.x & 63;
  double* wacc = acc + (size_t)(threadIdx.x >> 6) * n_layers * AW;          // this wave's table
  const int64_t nvc = (dim + V - 1) / V;
  const T dim_m1 = T(dim - 1);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t col_first = tile * cols_per_block * UC + threadIdx.x / G;
    Pack<T, V> zz[UC][R], gg[UC][R];
    T lb[UC];
    bool ok[UC];
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      const int64_t col_raw = col_first + (int64_t)u * cols_per_block;
      ok[u] = col_raw < batch;
      const int64_t col = ok[u] ? col_raw : batch - 1;           // lanes past the batch run on the last column, their sums are dropped
      lb[u] = lbar ? lbar[col] : T(0);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
        if (v < nvc) {
          const int nrow = (int)(dim - v * V < V ? dim - v * V : V);
          zz[u][r] = load_pack_part<T, V>(x + col * dim + v * V, nrow); gg[u][r] = load_pack_part<T, V>(gbar + col * dim + v * V, nrow);
        }
      }
    }
    // ---- primal sweep (radial_stack_vjp_kernel)
    for (int li = 0; li < n_layers; ++li) {
      const int l = INV ? n_layers - 1 - li : li;
      const T alpha = sc[2 * l], apb = sc[2 * l + 1];
      const T bh = -alpha + apb;
      const T* Z0 = tab + (size_t)l * dim;
      T z0r[R][V];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
#pragma unroll
        for (int j = 0; j < V; ++j) z0r[r][j] = v * V + j < dim ? Z0[v * V + j] : T(0);
      }
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        T ss = T(0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t v = gl + (int64_t)r * G;
          if (v < nvc) {
#pragma unroll
            for (int j = 0; j < V; ++j) { const T dlt = zz[u][r].v[j] - z0r[r][j]; ss = rs_fma(dlt, dlt, ss); }
          }
        }
        ss = group_sum_rt(ss, G);
        T* st = stash + ((size_t)(threadIdx.x / G + u * cols_per_block) * n_layers + l) * NS;
        T gain = T(1), fwd_gain = T(0);
        if (!INV) {
          const T rr = d_sqrt(ss);
          if (gl == 0) st[0] = rr;
          fwd_gain = bh / (alpha + rr);
        } else {
          const T gam = d_sqrt(ss);              // compute_r, radial_layer.jl:124-129
          const T aa = apb - gam;
          const T r0 = (d_sqrt(aa * aa + 4 * alpha * gam) - aa) / 2;
          gain = (alpha + r0) / (apb + r0);
          if (gl == 0) { st[0] = gain; st[1] = gam; }
        }
        if (li + 1 < n_layers) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t v = gl + (int64_t)r * G;
            if (v < nvc) {
#pragma unroll
              for (int j = 0; j < V; ++j) {
                const T dlt = zz[u][r].v[j] - z0r[r][j];
                if (!INV) zz[u][r].v[j] = rs_fma(fwd_gain, dlt, zz[u][r].v[j]);
                else zz[u][r].v[j] = rs_fma(gain, dlt, z0r[r][j]);
              }
            }
          }
        }
      }
    }
    tile_sync();        // the stash is written and read inside one wave (G <= 64): the LDS queue is in order, only the compiler is pinned
    // ---- reverse sweep, with the parameter sums
    for (int li = n_layers - 1; li >= 0; --li) {
      const int l = INV ? n_layers - 1 - li : li;
      const T alpha = sc[2 * l], apb = sc[2 * l + 1];
      const T bh = -alpha + apb;
      const T* Z0 = tab + (size_t)l * dim;
      T z0r[R][V];
      double dz[R][V];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
#pragma unroll
        for (int j = 0; j < V; ++j) { z0r[r][j] = v * V + j < dim ? Z0[v * V + j] : T(0); dz[r][j] = 0.0; }
      }
      double sga = 0.0, sgb = 0.0;
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        const T* st = stash + ((size_t)(threadIdx.x / G + u * cols_per_block) * n_layers + l) * NS;
        T rr, gain = T(1);
        if (!INV) rr = st[0];
        else { gain = st[0]; rr = gain * st[1]; }
        T a, c, kl;
        rs_jac<T>(rr, alpha, bh, dim_m1, lb[u], a, c, kl);
        if (li + 1 < n_layers) {                 // rewind: the column holds this layer's OUTPUT (in the direction the run applies it)
          const T back = !INV ? T(1) / a : T(1) / gain;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t v = gl + (int64_t)r * G;
            if (v < nvc) {
#pragma unroll
              for (int j = 0; j < V; ++j) zz[u][r].v[j] = rs_fma(zz[u][r].v[j] - z0r[r][j], back, z0r[r][j]);
            }
          }
        }
        T dg = T(0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t v = gl + (int64_t)r * G;
          if (v < nvc) {
#pragma unroll
            for (int j = 0; j < V; ++j) dg = rs_fma(zz[u][r].v[j] - z0r[r][j], gg[u][r].v[j], dg);
          }
        }
        dg = group_sum_rt(dg, G);
        T ca, cd;
        rs_coef<T, INV>(a, c, kl, rr, gain, dg, ca, cd);
        T dgx, lbx, ga, gb;
        rsp_dot<T, INV>(a, c, kl, rr, gain, dg, lb[u], dgx, lbx);
        rsp_terms<T>(rr, alpha, bh, dim_m1, dgx, lbx, ga, gb);
        if (ok[u]) { sga += (double)ga; sgb += (double)gb; }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t v = gl + (int64_t)r * G;
          if (v < nvc) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const T gn = rs_fma(cd, zz[u][r].v[j] - z0r[r][j], ca * gg[u][r].v[j]);
              if (ok[u]) dz[r][j] += (double)gg[u][r].v[j] - (double)gn;
              gg[u][r].v[j] = gn;
            }
          }
        }
      }
      // the column groups of the wave: a fixed butterfly over lanes gl, gl + G, …; then one writer per entry of the wave's table
      double* wl_acc = wacc + (size_t)l * AW;
      for (int m = G; m < 64; m <<= 1) { sga += shfl_xor(sga, m); sgb += shfl_xor(sgb, m); }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          double s = dz[r][j];
          for (int m = G; m < 64; m <<= 1) s += shfl_xor(s, m);
          if (wl < G && v * V + j < dim) wl_acc[v * V + j] += s;
        }
      }
      if (wl == 0) { wl_acc[dim] += sga; wl_acc[dim + 1] += sgb; }
    }
    if (xbar) {
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        const int64_t col = col_first + (int64_t)u * cols_per_block;
        if (col < batch) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t v = gl + (int64_t)r * G;
            if (v < nvc) store_pack_part<T, V>(xbar + col * dim + v * V, gg[u][r], (int)(dim - v * V < V ? dim - v * V : V));
          }
        }
      }
    }
    tile_sync();        // the next tile's primal sweep overwrites the stash this one has read
  }
  __syncthreads();
  const int per = n_layers * AW;
  double* mine = partials + (size_t)blockIdx.x * per;
  for (int e = threadIdx.x; e < per; e += blockDim.x) mine[e] = (acc[e] + acc[per + e]) + (acc[2 * per + e] + acc[3 * per + e]);
}

// ------------------------------------------------------------------ walk form: ONE LANE per column (dim <= 32)
// LDS: [acc: L x (DMAX + 2) of double][red: DMAX x 65 of double][tx][tg][tab][stash] — tiles, table and stash as radial_stack_vjp_walk_kernel
template <class T, int DMAX, bool INV, int V>
__global__ __launch_bounds__(64) void radial_stack_params_walk_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                       const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int dim, int P,
                                                                       int SP, int64_t batch, double* __restrict__ partials) {
#pragma clang fp contract(off)
  constexpr int LW = DMAX + 4;
  constexpr int AW = DMAX + 2;
  constexpr int RP = 65;                         // odd pitch of the reduction tile: lane (row, segment) reads bank pair (lane + i) mod 32
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* acc = reinterpret_cast<double*>(smem);
  double* red = acc + (size_t)n_layers * AW;
  T* tx = reinterpret_cast<T*>(red + (size_t)DMAX * RP + ((n_layers * AW + DMAX * RP) & 1));      // 16-byte aligned
  const size_t tile_e = (((size_t)64 * P + 3) / 4) * 4;
  T* tg = tx + tile_e;
  T* tab = tg + tile_e;
  T* stash = tab + (((size_t)n_layers * LW + 3) / 4) * 4;
  const int lane = threadIdx.x;
  rs_walk_tables<T, DMAX>(alpha_, beta, z0, n_layers, dim, tab, lane);
  for (int i = lane; i < n_layers * AW; i += 64) acc[i] = 0.0;
  tile_sync();
  const T dim_m1 = T(dim - 1);
  T* st = stash + (size_t)lane * SP;
  const int rrow = lane & (DMAX - 1), rseg = lane / DMAX;       // this lane's row and segment in the reduction
  for (int64_t c0 = (int64_t)blockIdx.x * 64; c0 < batch; c0 += (int64_t)gridDim.x * 64) {
    const int ncols = (int)((batch - c0) < 64 ? (batch - c0) : 64);
    const bool live = lane < ncols;
    tile_stage_in<T, V>(tx, x + c0 * dim, dim, P, ncols, lane);
    tile_stage_in<T, V>(tg, gbar + c0 * dim, dim, P, ncols, lane);
    tile_sync();
    T* mx = tx + lane * P;
    const T* mg = tg + lane * P;
    T z[DMAX], g[DMAX];
#pragma unroll
    for (int r = 0; r < DMAX; ++r) {
      z[r] = (r < dim && live) ? mx[r] : T(0);
      g[r] = (r < dim && live) ? mg[r] : T(0);
    }
    const T lb = (lbar && live) ? lbar[c0 + lane] : T(0);
    // ---- primal sweep (radial_stack_vjp_walk_kernel)
    for (int li = 0; li < n_layers; ++li) {
      const int l = INV ? n_layers - 1 - li : li;
      const T* tl = tab + l * LW;
      const T alpha = tl[DMAX], apb = tl[DMAX + 1];
      const T bh = -alpha + apb;
      T z0v[DMAX], dz[DMAX];
      T ss = T(0);
#pragma unroll
      for (int r = 0; r < DMAX; ++r) { z0v[r] = tl[r]; dz[r] = z[r] - z0v[r]; ss = rs_fma(dz[r], dz[r], ss); }
      T gain = T(1), fwd_gain = T(0);
      if (!INV) {
        const T rr = d_sqrt(ss);
        st[l] = rr;
        fwd_gain = bh / (alpha + rr);
      } else {
        const T gam = d_sqrt(ss);              // compute_r, radial_layer.jl:124-129
        const T aa = apb - gam;
        const T r0 = (d_sqrt(aa * aa + 4 * alpha * gam) - aa) / 2;
        gain = (alpha + r0) / (apb + r0);
        st[2 * l] = gain; st[2 * l + 1] = gam;
      }
      if (li + 1 < n_layers) {
#pragma unroll
        for (int r = 0; r < DMAX; ++r) {
          if (!INV) z[r] = rs_fma(fwd_gain, dz[r], z[r]);
          else z[r] = rs_fma(gain, dz[r], z0v[r]);
        }
      }
    }
    tile_sync();
    // ---- reverse sweep, with the parameter sums
    for (int li = n_layers - 1; li >= 0; --li) {
      const int l = INV ? n_layers - 1 - li : li;
      const T* tl = tab + l * LW;
      const T alpha = tl[DMAX], apb = tl[DMAX + 1];
      const T bh = -alpha + apb;
      T rr, gain = T(1);
      if (!INV) rr = st[l];
      else { gain = st[2 * l]; rr = gain * st[2 * l + 1]; }
      T a, c, kl;
      rs_jac<T>(rr, alpha, bh, dim_m1, lb, a, c, kl);
      T z0v[DMAX];
#pragma unroll
      for (int r = 0; r < DMAX; ++r) z0v[r] = tl[r];
      if (li + 1 < n_layers) {
        const T back = !INV ? T(1) / a : T(1) / gain;
#pragma unroll
        for (int r = 0; r < DMAX; ++r) z[r] = rs_fma(z[r] - z0v[r], back, z0v[r]);
      }
      T dg = T(0);
#pragma unroll
      for (int r = 0; r < DMAX; ++r) dg = rs_fma(z[r] - z0v[r], g[r], dg);
      T ca, cd;
      rs_coef<T, INV>(a, c, kl, rr, gain, dg, ca, cd);
      T dgx, lbx, ga, gb;
      rsp_dot<T, INV>(a, c, kl, rr, gain, dg, lb, dgx, lbx);
      rsp_terms<T>(rr, alpha, bh, dim_m1, dgx, lbx, ga, gb);
#pragma unroll
      for (int r = 0; r < DMAX; ++r) {
        const T gn = rs_fma(cd, z[r] - z0v[r], ca * g[r]);
        red[r * RP + lane] = (live && r < dim) ? (double)g[r] - (double)gn : 0.0;
        g[r] = gn;
      }
      double sga = group_sum<64>(live ? (double)ga : 0.0), sgb = group_sum<64>(live ? (double)gb : 0.0);
      tile_sync();
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < DMAX; ++i) s += red[rrow * RP + rseg * DMAX + i];
#pragma unroll
      for (int m = DMAX; m < 64; m <<= 1) s += shfl_xor(s, m);
      double* la = acc + (size_t)l * AW;
      if (lane < DMAX) la[lane] += s;
      if (lane == 0) { la[DMAX] += sga; la[DMAX + 1] += sgb; }
      tile_sync();
    }
    if (xbar) {
#pragma unroll
      for (int r = 0; r < DMAX; ++r) if (r < dim) mx[r] = g[r];
      tile_sync();
      tile_stage_out<T, V>(tx, xbar + c0 * dim, dim, P, ncols, lane);
    }
    tile_sync();
  }
  const int aw = dim + 2;
  double* mine = partials + (size_t)blockIdx.x * n_layers * aw;
  for (int e = lane; e < n_layers * aw; e += 64) {
    const int l = e / aw, q = e - l * aw;
    mine[e] = acc[l * AW + (q < dim ? q : DMAX + (q - dim))];
  }
}

// ------------------------------------------------------------------ folds: fixed order, coalesced over the entries
// out[c][e] = Σ_{k in chunk c} in[k][e], four accumulators (flow_sets_reduce_kernel of bjx_flow.hip); grid (entries / 256, chunks)
__global__ __launch_bounds__(256) void rsp_fold_kernel(const double* __restrict__ in, int nsets, int per, int chunk, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const int k0 = blockIdx.y * chunk;
  const int k1 = k0 + chunk < nsets ? k0 + chunk : nsets;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int k = k0;
  for (; k + 4 <= k1; k += 4) {
    a0 += in[(size_t)k * per + e]; a1 += in[(size_t)(k + 1) * per + e]; a2 += in[(size_t)(k + 2) * per + e]; a3 += in[(size_t)(k + 3) * per + e];
  }
  for (; k < k1; ++k) a0 += in[(size_t)k * per + e];
  out[(size_t)blockIdx.y * per + e] = (a0 + a1) + (a2 + a3);
}
// the last fold and the cast: entry (l, q) of [L][dim + 2] — q < dim: z̄₀; q = dim: Σg_α̂ (with q + 1: Σg_β̂) -> ᾱ_, β̄
template <class T>
__global__ __launch_bounds__(256) void rsp_final_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const double* __restrict__ in, int nsets, int n_layers,
                                                        int dim, T* __restrict__ alpha_bar, T* __restrict__ beta_bar, T* __restrict__ z0_bar) {
  const int aw = dim + 2, per = n_layers * aw;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const int l = e / aw, q = e - l * aw;
  if (q > dim) return;
  double s = 0.0, s2 = 0.0;
  for (int k = 0; k < nsets; ++k) s += in[(size_t)k * per + e];
  if (q < dim) { z0_bar[(size_t)l * dim + q] = (T)s; return; }
  for (int k = 0; k < nsets; ++k) s2 += in[(size_t)k * per + e + 1];
  const double sa = 1.0 / (1.0 + exp(-(double)alpha_[l])), sb = 1.0 / (1.0 + exp(-(double)beta[l]));
  alpha_bar[l] = (T)(sa * (s - s2));
  beta_bar[l] = (T)(sb * s2);
}

// ------------------------------------------------------------------ host
#define RSP_SWITCH_R(TT, VV, INVV)                                                                                                                    \
  switch (R) {                                                                                                                                        \
    case 1: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 1, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break;  \
    case 2: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 2, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break;  \
    case 4: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 4, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break;  \
    default: hipLaunchKernelGGL((radial_stack_params_kernel<TT, VV, 8, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G, tiles, part); break; \
  }

// blocks of the streaming pass: every block walks at least RSP_TILES_MIN tiles, at most `cap` blocks
inline int64_t rsp_grid(int64_t tiles, int64_t cap) {
  int64_t g = (tiles + RSP_TILES_MIN - 1) / RSP_TILES_MIN;
  if (g > cap) g = cap;
  return g < 1 ? 1 : g;
}

template <class T>
int radial_stack_vjp_params_impl(bjx_ctx* ctx, int inverse, const T* alpha_, const T* beta, const T* z0, int nl, const T* in, const T* out_bar,
                                 const T* ladj_bar, T* in_bar, T* alpha_bar, T* beta_bar, T* z0_bar, int64_t dim, int64_t batch) {
  constexpr int VW = Vec16<T>::N;
  const int ns = inverse ? 2 : 1;
  const bool walk = rs_walk_shape<T>(dim);
  const bool aligned = bjx_aligned16(in) && bjx_aligned16(out_bar) && bjx_aligned16(in_bar);
  int V = 1, G = 1, R = 1, P = 0, SP = 0;
  size_t smem = 0;
  int64_t tiles = 0, cap = 0;
  if (walk) {
    P = (int)(dim | 1);
    SP = (nl * ns) | 1;
    const int DMAX = dim <= 8 ? 8 : (dim <= 16 ? 16 : 32);
    const size_t dbl = (size_t)nl * (DMAX + 2) + (size_t)DMAX * 65;
    smem = (dbl + (dbl & 1)) * sizeof(double) + (2 * ((((size_t)64 * P + 3) / 4) * 4) + (((size_t)nl * (DMAX + 4) + 3) / 4) * 4 + (size_t)64 * SP) * sizeof(T);
    tiles = (batch + 63) / 64;
    cap = (int64_t)ctx->num_cu * 16;
  } else {
    BJX_REQUIRE(ctx, rs_group_cfg<T>(aligned, dim, &V, &G, &R), BJX_ERR_UNSUPPORTED,
                "bjx_radial_stack_vjp_params: columns of %lld rows are not fused (take the layers one by one)", (long long)dim);
    const int uc = R == 1 ? 2 : 1;                                   // StackVjpUC<R>
    const int64_t cpb = (int64_t)(256 / G) * uc;
    smem = rs_round16((size_t)2 * nl * sizeof(T)) + rs_round16((size_t)nl * dim * sizeof(T)) + rs_round16((size_t)cpb * nl * ns * sizeof(T)) +
           (size_t)4 * nl * (dim + 2) * sizeof(double);
    tiles = (batch + cpb - 1) / cpb;
    cap = (int64_t)ctx->num_cu * 4;
  }
  BJX_REQUIRE(ctx, smem <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp_params: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
  const int64_t per64 = (int64_t)nl * (dim + 2);
  BJX_REQUIRE(ctx, per64 < ((int64_t)1 << 24), BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp_params: too many layers");
  const int per = (int)per64;
  if (batch == 0) {
    BJX_HIP(ctx, hipMemsetAsync(z0_bar, 0, (size_t)nl * dim * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(alpha_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
    BJX_HIP(ctx, hipMemsetAsync(beta_bar, 0, (size_t)nl * sizeof(T), ctx->stream));
    return BJX_OK;
  }
  const int64_t grid = rsp_grid(tiles, cap);
  const int chunks = (int)((grid + RSP_FOLD_CHUNK - 1) / RSP_FOLD_CHUNK);
  { int rc = bjx_ensure_partials(ctx, (size_t)(grid + chunks) * per); if (rc) return rc; }
  double* part = ctx->partials;
  double* part2 = part + (size_t)grid * per;
  {
    BjxProf prof_(ctx);
    if (walk) {
#define RSPW(D_, I_, V_) hipLaunchKernelGGL((radial_stack_params_walk_kernel<T, D_, I_, V_>), dim3((unsigned)grid), dim3(64), smem, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, (int)dim, P, SP, batch, part)
#define RSPW_V(D_, I_) do { if (aligned) RSPW(D_, I_, VW); else RSPW(D_, I_, 1); } while (0)
#define RSPW_D(I_) do { if (dim <= 8) RSPW_V(8, I_); else if (dim <= 16) RSPW_V(16, I_); else RSPW_V(32, I_); } while (0)
      if (inverse) RSPW_D(true); else RSPW_D(false);
#undef RSPW_D
#undef RSPW_V
#undef RSPW
    } else if (V == VW) {
      if (!inverse) { RSP_SWITCH_R(T, VW, false) } else { RSP_SWITCH_R(T, VW, true) }
    } else {
      if (!inverse) { RSP_SWITCH_R(T, 1, false) } else { RSP_SWITCH_R(T, 1, true) }
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  {
    BjxProf prof_(ctx);
    const unsigned eb = (unsigned)((per + 255) / 256);
    if (chunks > 1) {
      hipLaunchKernelGGL(rsp_fold_kernel, dim3(eb, (unsigned)chunks), dim3(256), 0, ctx->stream, part, (int)grid, per, RSP_FOLD_CHUNK, part2);
      hipLaunchKernelGGL(rsp_final_kernel<T>, dim3(eb), dim3(256), 0, ctx->stream, alpha_, beta, part2, chunks, nl, (int)dim, alpha_bar, beta_bar, z0_bar);
    } else {
      hipLaunchKernelGGL(rsp_final_kernel<T>, dim3(eb), dim3(256), 0, ctx->stream, alpha_, beta, part, (int)grid, nl, (int)dim, alpha_bar, beta_bar, z0_bar);
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_radial_stack_vjp_params(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                                        const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* alpha_bar, void* beta_bar,
                                        void* z0_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0 && n_layers >= 1, BJX_ERR_SHAPE, "bjx_radial_stack_vjp_params: bad size");
  BJX_REQUIRE(ctx, alpha_ && beta && z0 && alpha_bar && beta_bar && z0_bar && ((in && out_bar) || batch == 0), BJX_ERR_ARG,
              "bjx_radial_stack_vjp_params: null pointer");
  if (dt == BJX_F32) return radial_stack_vjp_params_impl<float>(ctx, inverse, (const float*)alpha_, (const float*)beta, (const float*)z0, n_layers, (const float*)in, (const float*)out_bar, (const float*)ladj_bar, (float*)in_bar, (float*)alpha_bar, (float*)beta_bar, (float*)z0_bar, dim, batch);
  if (dt == BJX_F64) return radial_stack_vjp_params_impl<double>(ctx, inverse, (const double*)alpha_, (const double*)beta, (const double*)z0, n_layers, (const double*)in, (const double*)out_bar, (const double*)ladj_bar, (double*)in_bar, (double*)alpha_bar, (double*)beta_bar, (double*)z0_bar, dim, batch);
  return bjx_fail(ctx, BJX_ERR_ARG, "bjx_radial_stack_vjp_params: bad dtype %d", (int)dt);
}
