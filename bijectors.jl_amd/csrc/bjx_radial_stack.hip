// bjx_radial_stack.hip — a RUN of RadialLayers l_L ∘ … ∘ l_1 in one launch (include/bjx_radial_stack.h): map, inverse, input pullback.
//   RadialLayer  radial_layer.jl:43-72 (forward), :88-129 (inverse); a flow is a composition (composed.jl:4-25, docs/src/flows.md:115)
//
// bjx_radial (bjx_flow.hip) takes one layer: L layers are L launches and L read-and-write passes over the batch.  A radial layer
// needs one reduction along the column (r = ‖z − z₀‖), a handful of scalars, and an update of the same column — the single-layer
// kernels already keep the column in registers between the reduction and the update, so a stack repeats that loop L times on the
// resident column.  The per-layer arithmetic below is the single-layer kernels' (radial_kernel / radial_walk_kernel /
// radial_vjp_kernel), operation for operation: r comes from the differences (no Gram-matrix shortcut — it would compute r² by
// cancellation), and a stack of one gives bjx_radial's result.
//
// Two register-resident forms, the two radial_impl dispatches to:
//   group form  G lanes own a column, R packs per lane (16-byte packs, or V = 1), one group reduction per layer; UC columns per
//               group in flight, the layer loop OUTSIDE the column loop (the z₀ row of a layer is read from LDS once for the UC
//               columns, whose reductions are independent instruction streams)
//   walk form   one lane per column (dim <= 32 that is not a whole pack, or Float64): 64 columns through a [64][P odd] LDS tile,
//               no cross-lane traffic
// Columns taller than 64 lanes x 8 packs (the radial_tall_kernel shapes) are not fused: BJX_ERR_UNSUPPORTED, nothing launched.
// The tables — softplus of the 2·L raw scalars, evaluated ONCE per block, and z₀ [dim, L] — live in LDS.
#include "bjx_internal.h"
#include "bjx_tile.h"
#include "../../include/bjx_radial_stack.h"

namespace {
using namespace bjx;
#include "bjx_flow_common.inc"

#include "bjx_radial_stack_common.inc"      // rs_scalars, rs_jac, rs_coef, the table staging and the geometry: shared with bjx_radial_stack_params.hip

// ------------------------------------------------------------------ group form: map and inverse
// LDS: [red: 32 bytes][sc: 2·L of T, padded to 16 bytes][tab: z₀, L·dim of T]
template <class T, int V, int R, bool INV>
__global__ __launch_bounds__(256) void radial_stack_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                           const T* x, T* y, T* ladj_ps, int64_t dim, int64_t batch, int G, int accumulate, double* partials) {
  constexpr int UC = StackUC<R>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);
  T* sc = reinterpret_cast<T*>(smem + 32);
  T* tab = reinterpret_cast<T*>(smem + 32 + rs_round16((size_t)2 * n_layers * sizeof(T)));
  rs_stage_tables<T>(alpha_, beta, z0, n_layers, dim, sc, tab);
  __syncthreads();

  const int gl = threadIdx.x & (G - 1);
  const int cols_per_block = blockDim.x / G;
  const int64_t nvc = (dim + V - 1) / V;         // the last pack may be partial (element-aligned packs, load_pack_part: dead rows read as 0 and stay 0)
  const T dim_m1 = T(dim - 1);
  // non-persistent grid: UC columns per G-lane group, all loaded before the first layer.  Lanes of a group past the batch keep
  // running (on column batch-1, results discarded) so the group shuffles stay convergent.
  const int64_t col_first = (int64_t)blockIdx.x * cols_per_block * UC + threadIdx.x / G;
  Pack<T, V> zz[UC][R];
#pragma unroll
  for (int u = 0; u < UC; ++u) {
    const int64_t col_raw = col_first + (int64_t)u * cols_per_block;
    const int64_t col = col_raw < batch ? col_raw : batch - 1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t v = gl + (int64_t)r * G;
      if (v < nvc) zz[u][r] = load_pack_part<T, V>(x + col * dim + v * V, (int)(dim - v * V < V ? dim - v * V : V));
    }
  }
  T ladj[UC];
#pragma unroll
  for (int u = 0; u < UC; ++u) ladj[u] = T(0);
  for (int li = 0; li < n_layers; ++li) {
    const int l = INV ? n_layers - 1 - li : li;      // the inverse of the run applies the last layer's inverse first
    const T alpha = sc[2 * l], apb = sc[2 * l + 1];
    const T beta_hat = -alpha + apb;                 // :45
    const T* Z0 = tab + (size_t)l * dim;
    T z0r[R][V];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t v = gl + (int64_t)r * G;
#pragma unroll
      for (int j = 0; j < V; ++j) z0r[r][j] = v * V + j < dim ? Z0[v * V + j] : T(0);
    }
    T ss[UC];
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      T s = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
        if (v < nvc) {
#pragma unroll
          for (int j = 0; j < V; ++j) { const T dlt = zz[u][r].v[j] - z0r[r][j]; s += dlt * dlt; }
        }
      }
      ss[u] = s;
    }
#pragma unroll
    for (int u = 0; u < UC; ++u) ss[u] = group_sum_rt(ss[u], G);
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      T gain, fwd_gain, ld;
      rs_scalars<T, INV>(ss[u], alpha, apb, beta_hat, dim_m1, gain, fwd_gain, ld);
      ladj[u] += ld;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
        if (v < nvc) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T dlt = zz[u][r].v[j] - z0r[r][j];
            if (!INV) zz[u][r].v[j] = zz[u][r].v[j] + fwd_gain * dlt;           // :52
            else zz[u][r].v[j] = z0r[r][j] + gain * dlt;                       // :101
          }
        }
      }
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < UC; ++u) {
    const int64_t col = col_first + (int64_t)u * cols_per_block;
    if (col < batch) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
        if (v < nvc) store_pack_part<T, V>(y + col * dim + v * V, zz[u][r], (int)(dim - v * V < V ? dim - v * V : V));
      }
      if (gl == 0) {
        if (ladj_ps) ladj_ps[col] = accumulate ? ladj_ps[col] + ladj[u] : ladj[u];
        acc += (double)ladj[u];
      }
    }
  }
  if (partials) block_publish_partial(acc, red, partials);
}

// ------------------------------------------------------------------ group form: input pullback, one pass
// Reads x and ȳ, writes x̄.  Forward run: the primal sweep applies layers 1 … L-1 to the resident column and leaves r_k of every
// layer in LDS (one scalar per layer and column); the reverse sweep pulls ȳ back from layer L down and REWINDS the column with
// a_k = 1 + β̂h(r_k) > 0 (β̂ >= -α):  z_k − z₀ₖ = a_k δ_k  =>  z_{k-1} = z₀ₖ + (z_k − z₀ₖ)/a_k — no layer input is stored.  The last
// layer's update and its rewind cancel and are skipped, so a stack of one is radial_vjp_kernel's arithmetic.
// Inverse run, mirror image: primal sweep from layer L down keeps (γ_k, ‖y_k − z₀ₖ‖); the pullback goes from layer 1 up and
// re-advances the column with 1/γ_k.  Two group reductions per layer and column (‖δ‖² in the primal sweep, δᵀḡ in the reverse one).
// LDS: [sc][tab][stash: (256/G)·UC column slots x L·NS of T], written by lane 0 of the group, read by the group (same wave)
template <class T, int V, int R, bool INV>
__global__ __launch_bounds__(256) void radial_stack_vjp_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                               const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int64_t dim,
                                                               int64_t batch, int G) {
#pragma clang fp contract(off)
  constexpr int UC = StackVjpUC<R>::value;
  constexpr int NS = INV ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sc = reinterpret_cast<T*>(smem);
  const size_t tab_off = rs_round16((size_t)2 * n_layers * sizeof(T));
  T* tab = reinterpret_cast<T*>(smem + tab_off);
  T* stash = reinterpret_cast<T*>(smem + tab_off + rs_round16((size_t)n_layers * dim * sizeof(T)));
  rs_stage_tables<T>(alpha_, beta, z0, n_layers, dim, sc, tab);
  __syncthreads();

  const int gl = threadIdx.x & (G - 1);
  const int cols_per_block = blockDim.x / G;
  const int64_t nvc = (dim + V - 1) / V;
  const T dim_m1 = T(dim - 1);
  const int64_t col_first = (int64_t)blockIdx.x * cols_per_block * UC + threadIdx.x / G;
  Pack<T, V> zz[UC][R], gg[UC][R];
  T lb[UC];
#pragma unroll
  for (int u = 0; u < UC; ++u) {
    const int64_t col_raw = col_first + (int64_t)u * cols_per_block;
    const int64_t col = col_raw < batch ? col_raw : batch - 1;
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
  // ---- primal sweep
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
      if (li + 1 < n_layers) {                 // the last layer of the sweep is not applied: the reverse sweep starts at its input
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
  // ---- reverse sweep
  for (int li = n_layers - 1; li >= 0; --li) {
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
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
        if (v < nvc) {
#pragma unroll
          for (int j = 0; j < V; ++j) gg[u][r].v[j] = rs_fma(cd, zz[u][r].v[j] - z0r[r][j], ca * gg[u][r].v[j]);
        }
      }
    }
  }
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

// ------------------------------------------------------------------ walk form: ONE LANE per column (dim <= 32), map and inverse
// The mapping of radial_walk_kernel (bjx_flow.hip): a wave takes 64 consecutive columns through a [64][P odd] LDS tile (DX > 0:
// columns of exactly DX <= 7 rows are read and written by their lane directly), lane t keeps column t in registers and runs the
// whole stack on it; nothing crosses lanes.  The layer table is wave-uniform: [z₀ padded with zeros to DMAX | α | α + β̂ | pad]
// (rs_walk_tables).
template <class T, int DMAX, bool INV, int V, int DX = 0>
__global__ __launch_bounds__(64) void radial_stack_walk_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                const T* x, T* y, T* ladj_ps, int dim, int P, int64_t batch, int accumulate, double* partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double red[1];
  constexpr int LW = DMAX + 4;
  T* tile = reinterpret_cast<T*>(smem);
  T* tab = tile + (((size_t)64 * P + 3) / 4) * 4;
  const int lane = threadIdx.x;
  rs_walk_tables<T, DMAX>(alpha_, beta, z0, n_layers, dim, tab, lane);
  tile_sync();
  const T dim_m1 = T(dim - 1);
  double acc = 0.0;
  for (int64_t c0 = (int64_t)blockIdx.x * 64; c0 < batch; c0 += (int64_t)gridDim.x * 64) {
    const int ncols = (int)((batch - c0) < 64 ? (batch - c0) : 64);
    T* mine = tile + lane * P;
    T z[DMAX];
    if constexpr (DX > 0) {
      TinyCol<T, DX> t{};
      if (lane < ncols) t = *reinterpret_cast<const TinyCol<T, DX>*>(x + (c0 + lane) * DX);
#pragma unroll
      for (int r = 0; r < DMAX; ++r) z[r] = r < DX ? t.v[r < DX ? r : 0] : T(0);
    } else {
      tile_stage_in<T, V>(tile, x + c0 * dim, dim, P, ncols, lane);
      tile_sync();
#pragma unroll
      for (int r = 0; r < DMAX; ++r) z[r] = r < dim ? mine[r] : T(0);
    }
    T ladj = T(0);
    for (int li = 0; li < n_layers; ++li) {
      const int l = INV ? n_layers - 1 - li : li;
      const T* tl = tab + l * LW;
      const T alpha = tl[DMAX], apb = tl[DMAX + 1];
      const T beta_hat = -alpha + apb;                                  // :45
      T z0v[DMAX], dz[DMAX];
      T ss = T(0);
#pragma unroll
      for (int r = 0; r < DMAX; ++r) { z0v[r] = tl[r]; dz[r] = z[r] - z0v[r]; ss += dz[r] * dz[r]; }     // padded rows: 0 − 0
      T gain, fwd_gain, ld;
      rs_scalars<T, INV>(ss, alpha, apb, beta_hat, dim_m1, gain, fwd_gain, ld);
      ladj += ld;
#pragma unroll
      for (int r = 0; r < DMAX; ++r) {
        if (!INV) z[r] = z[r] + fwd_gain * dz[r];                       // :52
        else z[r] = z0v[r] + gain * dz[r];                              // :101
      }
    }
    if constexpr (DX > 0) {
      if (lane < ncols) {
        TinyCol<T, DX> t;
#pragma unroll
        for (int r = 0; r < DX; ++r) t.v[r] = z[r];
        *reinterpret_cast<TinyCol<T, DX>*>(y + (c0 + lane) * DX) = t;
      }
    } else {
#pragma unroll
      for (int r = 0; r < DMAX; ++r) if (r < dim) mine[r] = z[r];
      tile_sync();
      tile_stage_out<T, V>(tile, y + c0 * dim, dim, P, ncols, lane);
      tile_sync();
    }
    if (lane < ncols) {
      if (ladj_ps) ladj_ps[c0 + lane] = accumulate ? ladj_ps[c0 + lane] + ladj : ladj;
      acc += (double)ladj;
    }
  }
  if (partials) block_publish_partial(acc, red, partials);
}

// ------------------------------------------------------------------ walk form: input pullback, one pass
// x and ȳ through two odd-pitch tiles (x̄ leaves through the first); the per-layer scalars of the primal sweep go to the lane's strip
// of LDS ([64][SP odd]); sweeps as in radial_stack_vjp_kernel.
template <class T, int DMAX, bool INV, int V>
__global__ __launch_bounds__(64) void radial_stack_vjp_walk_kernel(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                                                    const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int dim, int P, int SP,
                                                                    int64_t batch) {
#pragma clang fp contract(off)
  constexpr int NS = INV ? 2 : 1;
  constexpr int LW = DMAX + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* tx = reinterpret_cast<T*>(smem);
  const size_t tile_e = (((size_t)64 * P + 3) / 4) * 4;
  T* tg = tx + tile_e;
  T* tab = tg + tile_e;
  T* stash = tab + (((size_t)n_layers * LW + 3) / 4) * 4;
  const int lane = threadIdx.x;
  rs_walk_tables<T, DMAX>(alpha_, beta, z0, n_layers, dim, tab, lane);
  tile_sync();
  const T dim_m1 = T(dim - 1);
  T* st = stash + (size_t)lane * SP;
  for (int64_t c0 = (int64_t)blockIdx.x * 64; c0 < batch; c0 += (int64_t)gridDim.x * 64) {
    const int ncols = (int)((batch - c0) < 64 ? (batch - c0) : 64);
    tile_stage_in<T, V>(tx, x + c0 * dim, dim, P, ncols, lane);
    tile_stage_in<T, V>(tg, gbar + c0 * dim, dim, P, ncols, lane);
    tile_sync();
    T* mx = tx + lane * P;
    const T* mg = tg + lane * P;
    T z[DMAX], g[DMAX];
#pragma unroll
    for (int r = 0; r < DMAX; ++r) {
      z[r] = (r < dim && lane < ncols) ? mx[r] : T(0);
      g[r] = (r < dim && lane < ncols) ? mg[r] : T(0);
    }
    const T lb = (lbar && lane < ncols) ? lbar[c0 + lane] : T(0);
    // ---- primal sweep
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
    // ---- reverse sweep
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
#pragma unroll
      for (int r = 0; r < DMAX; ++r) g[r] = rs_fma(cd, z[r] - z0v[r], ca * g[r]);
    }
#pragma unroll
    for (int r = 0; r < DMAX; ++r) if (r < dim) mx[r] = g[r];
    tile_sync();
    tile_stage_out<T, V>(tx, xbar + c0 * dim, dim, P, ncols, lane);
    tile_sync();
  }
}

// ------------------------------------------------------------------ host
#define RS_SWITCH_R(KERNEL, TT, VV, INVV, ...)                                                                            \
  switch (R) {                                                                                                            \
    case 1: hipLaunchKernelGGL((KERNEL<TT, VV, 1, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, __VA_ARGS__); break;  \
    case 2: hipLaunchKernelGGL((KERNEL<TT, VV, 2, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, __VA_ARGS__); break;  \
    case 4: hipLaunchKernelGGL((KERNEL<TT, VV, 4, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, __VA_ARGS__); break;  \
    default: hipLaunchKernelGGL((KERNEL<TT, VV, 8, INVV>), dim3((unsigned)grid), dim3(256), smem, ctx->stream, __VA_ARGS__); break; \
  }

template <class T>
int radial_stack_impl(bjx_ctx* ctx, int inverse, const T* alpha_, const T* beta, const T* z0, int nl, const T* in, T* out, T* ladj_ps,
                      double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  constexpr int VW = Vec16<T>::N;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  if (rs_walk_shape<T>(dim)) {
    const bool direct = dim <= 7;                                    // short columns: no tile (DX = dim)
    const int P = direct ? 0 : (int)(dim | 1);
    const int DMAX = dim <= 4 ? 4 : (dim <= 8 ? 8 : (dim <= 16 ? 16 : 32));
    const size_t smem_w = ((((size_t)64 * P + 3) / 4) * 4 + (size_t)nl * (DMAX + 4)) * sizeof(T);
    BJX_REQUIRE(ctx, smem_w <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
    const int64_t tiles = (batch + 63) / 64;
    const int64_t cap = (int64_t)ctx->num_cu * 32;
    const int grid_w = (int)(tiles < cap ? tiles : cap);
    if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid_w); if (rc) return rc; }
    double* partials_w = ladj_sum ? ctx->partials : nullptr;
    const bool vec = bjx_aligned16(in) && bjx_aligned16(out);
    {
      BjxProf prof_(ctx);
#define RSW(D_, I_, V_) hipLaunchKernelGGL((radial_stack_walk_kernel<T, D_, I_, V_>), dim3(grid_w), dim3(64), smem_w, ctx->stream, alpha_, beta, z0, nl, in, out, ladj_ps, (int)dim, P, batch, accum, partials_w)
#define RSW_V(D_, I_) do { if (vec) RSW(D_, I_, VW); else RSW(D_, I_, 1); } while (0)
#define RSW_D(I_) do { if (dim <= 8) RSW_V(8, I_); else if (dim <= 16) RSW_V(16, I_); else RSW_V(32, I_); } while (0)
#define RSWX(D_, X_) do { if (inverse) hipLaunchKernelGGL((radial_stack_walk_kernel<T, D_, true, 1, X_>), dim3(grid_w), dim3(64), smem_w, ctx->stream, alpha_, beta, z0, nl, in, out, ladj_ps, (int)dim, P, batch, accum, partials_w); \
                           else hipLaunchKernelGGL((radial_stack_walk_kernel<T, D_, false, 1, X_>), dim3(grid_w), dim3(64), smem_w, ctx->stream, alpha_, beta, z0, nl, in, out, ladj_ps, (int)dim, P, batch, accum, partials_w); } while (0)
      if (direct) {
        switch ((int)dim) {
          case 1: RSWX(4, 1); break;
          case 2: RSWX(4, 2); break;
          case 3: RSWX(4, 3); break;
          case 4: RSWX(4, 4); break;
          case 5: RSWX(8, 5); break;
          case 6: RSWX(8, 6); break;
          default: RSWX(8, 7); break;
        }
      }
      else if (inverse) RSW_D(true); else RSW_D(false);
#undef RSWX
#undef RSW_D
#undef RSW_V
#undef RSW
    }
    BJX_CHECK_LAUNCH(ctx);
    if (ladj_sum) return bjx_launch_finalize(ctx, grid_w, ladj_sum, 0.0, 0, 0.0, flags);
    return BJX_OK;
  }
  int V, G, R;
  BJX_REQUIRE(ctx, rs_group_cfg<T>(bjx_aligned16(in) && bjx_aligned16(out), dim, &V, &G, &R), BJX_ERR_UNSUPPORTED,
              "bjx_radial_stack: columns of %lld rows are not fused (apply the layers one by one)", (long long)dim);
  const size_t smem = 32 + rs_round16((size_t)2 * nl * sizeof(T)) + (size_t)nl * dim * sizeof(T);
  BJX_REQUIRE(ctx, smem <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
  const int uc = R == 1 ? 4 : (R == 2 ? 2 : 1);                      // StackUC<R>
  const int64_t cpb = (int64_t)(256 / G) * uc;
  const int64_t grid = (batch + cpb - 1) / cpb;
  BJX_REQUIRE(ctx, grid < ((int64_t)1 << 31), BJX_ERR_UNSUPPORTED, "bjx_radial_stack: batch too large for one launch");
  if (ladj_sum) { int rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  {
    BjxProf prof_(ctx);
    if (V == VW) {
      if (!inverse) { RS_SWITCH_R(radial_stack_kernel, T, VW, false, alpha_, beta, z0, nl, in, out, ladj_ps, dim, batch, G, accum, partials) }
      else { RS_SWITCH_R(radial_stack_kernel, T, VW, true, alpha_, beta, z0, nl, in, out, ladj_ps, dim, batch, G, accum, partials) }
    } else {
      if (!inverse) { RS_SWITCH_R(radial_stack_kernel, T, 1, false, alpha_, beta, z0, nl, in, out, ladj_ps, dim, batch, G, accum, partials) }
      else { RS_SWITCH_R(radial_stack_kernel, T, 1, true, alpha_, beta, z0, nl, in, out, ladj_ps, dim, batch, G, accum, partials) }
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, (int)grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T>
int radial_stack_vjp_impl(bjx_ctx* ctx, int inverse, const T* alpha_, const T* beta, const T* z0, int nl, const T* in, const T* out_bar,
                          const T* ladj_bar, T* in_bar, int64_t dim, int64_t batch) {
  if (batch == 0) return BJX_OK;
  constexpr int VW = Vec16<T>::N;
  const int ns = inverse ? 2 : 1;
  if (rs_walk_shape<T>(dim)) {
    const int P = (int)(dim | 1);
    const int SP = (nl * ns) | 1;
    const int DMAX = dim <= 8 ? 8 : (dim <= 16 ? 16 : 32);
    const size_t smem_w = (2 * ((((size_t)64 * P + 3) / 4) * 4) + (((size_t)nl * (DMAX + 4) + 3) / 4) * 4 + (size_t)64 * SP) * sizeof(T);
    BJX_REQUIRE(ctx, smem_w <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
    const int64_t tiles = (batch + 63) / 64;
    const int64_t cap = (int64_t)ctx->num_cu * 32;
    const int grid_w = (int)(tiles < cap ? tiles : cap);
    const bool vec = bjx_aligned16(in) && bjx_aligned16(out_bar) && bjx_aligned16(in_bar);
    {
      BjxProf prof_(ctx);
#define RSVW(D_, I_, V_) hipLaunchKernelGGL((radial_stack_vjp_walk_kernel<T, D_, I_, V_>), dim3(grid_w), dim3(64), smem_w, ctx->stream, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, (int)dim, P, SP, batch)
#define RSVW_V(D_, I_) do { if (vec) RSVW(D_, I_, VW); else RSVW(D_, I_, 1); } while (0)
#define RSVW_D(I_) do { if (dim <= 8) RSVW_V(8, I_); else if (dim <= 16) RSVW_V(16, I_); else RSVW_V(32, I_); } while (0)
      if (inverse) RSVW_D(true); else RSVW_D(false);
#undef RSVW_D
#undef RSVW_V
#undef RSVW
    }
    BJX_CHECK_LAUNCH(ctx);
    return BJX_OK;
  }
  int V, G, R;
  BJX_REQUIRE(ctx, rs_group_cfg<T>(bjx_aligned16(in) && bjx_aligned16(out_bar) && bjx_aligned16(in_bar), dim, &V, &G, &R), BJX_ERR_UNSUPPORTED,
              "bjx_radial_stack_vjp: columns of %lld rows are not fused (apply the layers one by one)", (long long)dim);
  const int uc = R == 1 ? 2 : 1;                                     // StackVjpUC<R>
  const int64_t cpb = (int64_t)(256 / G) * uc;
  const size_t smem = rs_round16((size_t)2 * nl * sizeof(T)) + rs_round16((size_t)nl * dim * sizeof(T)) + (size_t)cpb * nl * ns * sizeof(T);
  BJX_REQUIRE(ctx, smem <= RS_LDS_BUDGET, BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp: %d layers of %lld rows exceed the LDS budget", nl, (long long)dim);
  const int64_t grid = (batch + cpb - 1) / cpb;
  BJX_REQUIRE(ctx, grid < ((int64_t)1 << 31), BJX_ERR_UNSUPPORTED, "bjx_radial_stack_vjp: batch too large for one launch");
  {
    BjxProf prof_(ctx);
    if (V == VW) {
      if (!inverse) { RS_SWITCH_R(radial_stack_vjp_kernel, T, VW, false, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G) }
      else { RS_SWITCH_R(radial_stack_vjp_kernel, T, VW, true, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G) }
    } else {
      if (!inverse) { RS_SWITCH_R(radial_stack_vjp_kernel, T, 1, false, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G) }
      else { RS_SWITCH_R(radial_stack_vjp_kernel, T, 1, true, alpha_, beta, z0, nl, in, out_bar, ladj_bar, in_bar, dim, batch, G) }
    }
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_radial_stack(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                             const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0 && n_layers >= 1, BJX_ERR_SHAPE, "bjx_radial_stack: bad size");
  BJX_REQUIRE(ctx, alpha_ && beta && z0 && ((in && out) || batch == 0), BJX_ERR_ARG, "bjx_radial_stack: null pointer");
  if (dt == BJX_F32) return radial_stack_impl<float>(ctx, inverse, (const float*)alpha_, (const float*)beta, (const float*)z0, n_layers, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  if (dt == BJX_F64) return radial_stack_impl<double>(ctx, inverse, (const double*)alpha_, (const double*)beta, (const double*)z0, n_layers, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
  return bjx_fail(ctx, BJX_ERR_ARG, "bjx_radial_stack: bad dtype %d", (int)dt);
}

BJX_API int bjx_radial_stack_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, const void* alpha_, const void* beta, const void* z0, int n_layers,
                                 const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  BJX_REQUIRE(ctx, dim >= 1 && batch >= 0 && n_layers >= 1, BJX_ERR_SHAPE, "bjx_radial_stack_vjp: bad size");
  BJX_REQUIRE(ctx, alpha_ && beta && z0 && ((in && out_bar && in_bar) || batch == 0), BJX_ERR_ARG, "bjx_radial_stack_vjp: null pointer");
  if (dt == BJX_F32) return radial_stack_vjp_impl<float>(ctx, inverse, (const float*)alpha_, (const float*)beta, (const float*)z0, n_layers, (const float*)in, (const float*)out_bar, (const float*)ladj_bar, (float*)in_bar, dim, batch);
  if (dt == BJX_F64) return radial_stack_vjp_impl<double>(ctx, inverse, (const double*)alpha_, (const double*)beta, (const double*)z0, n_layers, (const double*)in, (const double*)out_bar, (const double*)ladj_bar, (double*)in_bar, dim, batch);
  return bjx_fail(ctx, BJX_ERR_ARG, "bjx_radial_stack_vjp: bad dtype %d", (int)dt);
}
