// bjx_radial_stack_common.inc — device and host helpers shared by bjx_radial_stack.hip, bjx_radial_stack_params.hip and
// bjx_radial_stack_logpdf.hip; included INSIDE each file's anonymous namespace (after `using namespace bjx;` and bjx_flow_common.inc),
// so every translation unit has its own internal copies.  The second half (RS_PARAMS_PASS) holds the bodies of the streaming
// parameter pass, which only the last two files compile.

constexpr size_t RS_LDS_BUDGET = 64 * 1024;      // per block: tables + (pullback) per-layer scalars; beyond it the entry refuses
constexpr int RS_R_MAX = 8;                      // packs per lane of the group form (FLOW_R_MAX of bjx_flow.hip)

template <int R> struct StackUC { static constexpr int value = R == 1 ? 4 : (R == 2 ? 2 : 1); };      // RadialUC of bjx_flow.hip
template <int R> struct StackVjpUC { static constexpr int value = R == 1 ? 2 : 1; };                  // UC of radial_vjp_kernel

__host__ __device__ inline size_t rs_round16(size_t b) { return (b + 15) / 16 * 16; }

// logabsdetjac of the forward layer at r = ‖z − z₀‖ (radial_layer.jl:68-70)
template <class T>
__device__ __forceinline__ T rs_logdet(T r_fwd, T alpha, T beta_hat, T dim_m1) {
  const T h_ = T(1) / (alpha + r_fwd);
  return dim_m1 * d_log(T(1) + beta_hat * h_) + d_log(T(1) + beta_hat * h_ + beta_hat * (-(h_ * h_)) * r_fwd);
}

// One layer's scalars from ss = ‖in − z₀‖² (radial_kernel, same operation order): out = z₀ + gain·δ, or in + fwd_gain·δ
template <class T, bool INV>
__device__ __forceinline__ void rs_scalars(T ss, T alpha, T apb, T beta_hat, T dim_m1, T& gain, T& fwd_gain, T& ld) {
  T r_fwd;                                          // ‖z − z₀‖ at the forward layer's input: the log-det is evaluated there
  if (!INV) {
    r_fwd = d_sqrt(ss);
    gain = T(1) + beta_hat / (alpha + r_fwd);       // z + β̂/(α+r)(z−z0) = z0 + (1+β̂h)(z−z0)
  } else {
    const T gam = d_sqrt(ss);                       // compute_r :124-129
    const T a = apb - gam;
    const T rr = (d_sqrt(a * a + 4 * alpha * gam) - a) / 2;
    gain = (alpha + rr) / (apb + rr);               // γ :96-101
    r_fwd = gain * gam;
  }
  ld = rs_logdet<T>(r_fwd, alpha, beta_hat, dim_m1);
  if (INV) ld = -ld;
  fwd_gain = beta_hat / (alpha + r_fwd);
}

// The pullback kernels of both files (the input pullback and the parameter pullback, whose x̄ must be the input pullback's BIT FOR BIT)
// switch floating-point contraction OFF in their bodies and in rs_jac / rs_coef, and spell the multiply-adds of the column loops as
// rs_fma: which products the compiler fuses, and how the vectoriser pairs the scalar closed forms with the column arithmetic, otherwise
// depends on the code around them, and the two kernels rounded differently in the last bits.
__device__ __forceinline__ float rs_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double rs_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// The closed forms of radial_vjp_kernel at r = rr: J = a I + c δδᵀ, kl = ℓ̄ ℓ'(r)/r
template <class T>
__device__ __forceinline__ void rs_jac(T rr, T alpha, T bh, T dim_m1, T lb, T& a, T& c, T& kl) {
#pragma clang fp contract(off)
  const T h = T(1) / (alpha + rr);
  a = T(1) + bh * h;
  const T rinv = rr > T(0) ? T(1) / rr : T(0);
  c = -bh * h * h * rinv;
  const T lr = dim_m1 * (-bh * h * h) / a + (T(-2) * bh * h * h + T(2) * bh * h * h * h * rr) / (T(1) + bh * h - bh * h * h * rr);
  kl = lb * lr * rinv;                              // coefficient of δ from the log-det term
}
// out = ca · ḡ + cd · δ_in (δ_in = input − z₀ of the layer in the direction it is applied; dg = δ_inᵀḡ)
template <class T, bool INV>
__device__ __forceinline__ void rs_coef(T a, T c, T kl, T rr, T gain, T dg, T& ca, T& cd) {
#pragma clang fp contract(off)
  if (!INV) { ca = a; cd = c * dg + kl; }
  else {
    // v = ḡ - kl δ;  δᵀv = gain·dg - kl r²;  out = v/a - c (δᵀv) δ / (a (a + c r²))     (Sherman–Morrison at the pre-image)
    const T dv = gain * dg - kl * rr * rr;
    ca = T(1) / a;
    cd = gain * (-kl / a - c * dv / (a * (a + c * rr * rr)));
  }
}

// softplus of the raw scalars, once per block: sc[2l] = α_l, sc[2l+1] = α_l + β̂_l; the z₀ table as it is
template <class T>
__device__ __forceinline__ void rs_stage_tables(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers, int64_t dim,
                                                T* sc, T* tab) {
  const int ne = n_layers * (int)dim;
  for (int i = threadIdx.x; i < ne; i += blockDim.x) tab[i] = z0[i];
  for (int i = threadIdx.x; i < n_layers; i += blockDim.x) { sc[2 * i] = d_log1pexp(alpha_[i]); sc[2 * i + 1] = d_log1pexp(beta[i]); }   // :44-45
}

// The layer table of the lane-per-column form, wave-uniform: [z₀ padded with zeros to DMAX | α | α + β̂ | pad] per layer
template <class T, int DMAX>
__device__ __forceinline__ void rs_walk_tables(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers, int dim, T* tab, int lane) {
  constexpr int LW = DMAX + 4;
  for (int i = lane; i < n_layers * LW; i += 64) {
    const int l = i / LW, q = i - l * LW;
    T v = T(0);
    if (q < DMAX) { if (q < dim) v = z0[l * dim + q]; }
    else if (q == DMAX) v = d_log1pexp(alpha_[l]);          // :44
    else if (q == DMAX + 1) v = d_log1pexp(beta[l]);        // α + β̂
    tab[i] = v;
  }
}

// the lanes-per-column geometry of flow_cfg (bjx_flow.hip) with partial last packs allowed; false: the column is taller than the
// register kernels hold
template <class T> bool rs_group_cfg(bool aligned, int64_t dim, int* V, int* G, int* R) {
  constexpr int VW = Vec16<T>::N;
  const bool v_ok = aligned && dim % VW == 0;
  int v = v_ok ? VW : 1;
  int64_t packs = dim / v;
  if (!v_ok && dim >= 32) { v = VW; packs = (dim + VW - 1) / VW; }     // odd heights / element-aligned bases: 16-byte packs all the same
  int g = 1;
  while (g < 64 && g < packs) g <<= 1;
  const int64_t need = (packs + g - 1) / g;
  int r = 1;
  while (r < need) r <<= 1;
  if (r > RS_R_MAX) return false;
  *V = v; *G = g; *R = r;
  return true;
}
// the shapes radial_walk_kernel serves
template <class T> bool rs_walk_shape(int64_t dim) { return dim <= 32 && (dim % Vec16<T>::N != 0 || sizeof(T) == 8); }

// ====================================================================================================================================
// The parameter pass — the streaming kernels' bodies, the folds and the grid rule shared by bjx_radial_stack_params.hip (the pullback of
// a run and of its inverse) and bjx_radial_stack_logpdf.hip (log-density of a flow with a normal base and all its cotangents, LP = true).
// Only those two files define RS_PARAMS_PASS before including this one (bjx_tile.h must be included first).
#ifdef RS_PARAMS_PASS

constexpr int RSP_TILES_MIN = 4;        // a block walks at least this many tiles before the grid grows (table staging and the block's partial are per block)
constexpr int RSP_FOLD_CHUNK = 32;      // block partials one thread of the first fold adds
constexpr double RS_HALF_LOG_2PI = 0.91893853320467274178;

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

// What the log-density pass (LP) adds to the pullback's arguments: the base N(μ, diag σ²) — device T[dim] or NULL (0 / 1) —, the
// per-column log-density (T[batch] or NULL) and whether the block's table carries the rows of μ̄ and σ̄.  The block's partial is then
// [n_layers x (dim + 2) | Σ lp | μ̄ (dim) | σ̄ (dim)], the last two only with want_base.
template <class T> struct RspLogpdf { const T* mu; const T* sigma; T* lp_ps; int want_base; };

// Σ log σ + (d/2)·log 2π in Float64, the same in every lane of the wave (a fixed butterfly; `sg`: dim entries, lanes stride over them)
template <class T>
__device__ __forceinline__ double rsp_base_const(const T* sg, bool has_sigma, int dim, int lane) {
  double s = 0.0;
  if (has_sigma) for (int i = lane; i < dim; i += 64) s += log((double)sg[i]);
  return group_sum<64>(s) + RS_HALF_LOG_2PI * (double)dim;
}

// ------------------------------------------------------------------ group form
// LDS: [sc][tab][LP: μ | σ, 2·dim of T][stash: (256/G)·UC column slots x L·NS of T][acc: 4 waves x `per` of double]
// LP (INV only): `x` is y, nothing is read at `gbar`; lbar is the cotangent c of the log-density (NULL = 1).  The primal sweep applies
// EVERY layer (the column ends as x = f⁻¹(y)) and adds up the inverse run's log-det; the seed ḡ = −c·w/σ, w = (x − μ)/σ, is generated
// in the registers the pullback loads out_bar into; the reverse sweep then rewinds from x.
template <class T, int V, int R, bool INV, bool LP>
__device__ __forceinline__ void rsp_group_body(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                               const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int64_t dim, int64_t batch, int G,
                                               int64_t tiles, double* __restrict__ partials, const RspLogpdf<T>& q) {
#pragma clang fp contract(off)
  static_assert(!LP || INV, "the log-density pass is the inverse run");
  constexpr int UC = StackVjpUC<R>::value;
  constexpr int NS = INV ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cols_per_block = blockDim.x / G;
  const int AW = (int)dim + 2;
  const int tail = n_layers * AW;                                            // first entry past the layers' rows
  const int per = tail + (LP ? 1 + (q.want_base ? 2 * (int)dim : 0) : 0);
  T* sc = reinterpret_cast<T*>(smem);
  const size_t tab_off = rs_round16((size_t)2 * n_layers * sizeof(T));
  T* tab = reinterpret_cast<T*>(smem + tab_off);
  const size_t base_off = tab_off + rs_round16((size_t)n_layers * dim * sizeof(T));
  T* bmu = reinterpret_cast<T*>(smem + base_off);
  T* bsg = bmu + dim;
  const size_t stash_off = base_off + (LP ? rs_round16((size_t)2 * dim * sizeof(T)) : 0);
  T* stash = reinterpret_cast<T*>(smem + stash_off);
  double* acc = reinterpret_cast<double*>(smem + stash_off + rs_round16((size_t)cols_per_block * UC * n_layers * NS * sizeof(T)));
  rs_stage_tables<T>(alpha_, beta, z0, n_layers, dim, sc, tab);
  if constexpr (LP) {
    for (int i = threadIdx.x; i < (int)dim; i += blockDim.x) { bmu[i] = q.mu ? q.mu[i] : T(0); bsg[i] = q.sigma ? q.sigma[i] : T(1); }
  }
  for (int i = threadIdx.x; i < 4 * per; i += blockDim.x) acc[i] = 0.0;
  __syncthreads();

  const int gl = threadIdx.x & (G - 1);
  const int wl = threadIdx.x & 63;
  double* wacc = acc + (size_t)(threadIdx.x >> 6) * per;                     // this wave's table
  const int64_t nvc = (dim + V - 1) / V;
  const T dim_m1 = T(dim - 1);
  T cst = T(0);
  if constexpr (LP) cst = (T)rsp_base_const<T>(bsg, q.sigma != nullptr, (int)dim, wl);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t col_first = tile * cols_per_block * UC + threadIdx.x / G;
    Pack<T, V> zz[UC][R], gg[UC][R];
    T lb[UC], ldet[UC];
    bool ok[UC];
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      const int64_t col_raw = col_first + (int64_t)u * cols_per_block;
      ok[u] = col_raw < batch;
      const int64_t col = ok[u] ? col_raw : batch - 1;           // lanes past the batch run on the last column, their sums are dropped
      lb[u] = lbar ? lbar[col] : T(LP ? 1 : 0);
      ldet[u] = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t v = gl + (int64_t)r * G;
        if (v < nvc) {
          const int nrow = (int)(dim - v * V < V ? dim - v * V : V);
          zz[u][r] = load_pack_part<T, V>(x + col * dim + v * V, nrow);
          if constexpr (!LP) gg[u][r] = load_pack_part<T, V>(gbar + col * dim + v * V, nrow);
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
          if constexpr (LP) ldet[u] -= rs_logdet<T>(gain * gam, alpha, bh, dim_m1);
        }
        if (LP || li + 1 < n_layers) {           // the pullback skips the last update (its rewind would undo it); here it is x itself
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
    if constexpr (LP) {
      // ---- the base density at x, and the seed of the reverse sweep: w = (x − μ)/σ, lp = −½‖w‖² − cst + ℓ, ḡ = −c·w/σ
      double slp = 0.0;
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        T ss = T(0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t v = gl + (int64_t)r * G;
          if (v < nvc) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const bool in = v * V + j < dim;
              const T w = in ? (zz[u][r].v[j] - bmu[v * V + j]) / bsg[v * V + j] : T(0);
              ss = rs_fma(w, w, ss);
              gg[u][r].v[j] = in ? -lb[u] * w / bsg[v * V + j] : T(0);
            }
          }
        }
        ss = group_sum_rt(ss, G);
        const T lp = T(-0.5) * ss - cst + ldet[u];
        const int64_t col = col_first + (int64_t)u * cols_per_block;
        if (ok[u]) {
          slp += (double)lp;
          if (gl == 0 && q.lp_ps) q.lp_ps[col] = lp;
        }
      }
      for (int m = G; m < 64; m <<= 1) slp += shfl_xor(slp, m);
      if (wl == 0) wacc[tail] += slp;
      if (q.want_base) {
        // μ̄ += −ḡ, then σ̄ += −ḡ⊙w − c/σ: the path z̄₀ takes below (one row set at a time: the registers of one `dz`)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t v = gl + (int64_t)r * G;
#pragma unroll
            for (int j = 0; j < V; ++j) {
              double s = 0.0;
              const bool in = v < nvc && v * V + j < dim;
              if (in) {
                const T sg = bsg[v * V + j];
#pragma unroll
                for (int u = 0; u < UC; ++u) {
                  if (!ok[u]) continue;
                  const T g = gg[u][r].v[j];
                  if (pass == 0) s += -(double)g;
                  else { const T w = (zz[u][r].v[j] - bmu[v * V + j]) / sg; s += (double)(-g * w - lb[u] / sg); }
                }
              }
              for (int m = G; m < 64; m <<= 1) s += shfl_xor(s, m);
              if (wl < G && in) wacc[tail + 1 + pass * (int)dim + v * V + j] += s;
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
        if (LP || li + 1 < n_layers) {           // rewind: the column holds this layer's OUTPUT (in the direction the run applies it)
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
  double* mine = partials + (size_t)blockIdx.x * per;
  for (int e = threadIdx.x; e < per; e += blockDim.x) mine[e] = (acc[e] + acc[per + e]) + (acc[2 * per + e] + acc[3 * per + e]);
}

// ------------------------------------------------------------------ walk form: ONE LANE per column (dim <= 32)
// Σ over the 64 lanes of one row each, through the [DMAX][65] Float64 tile `red` the lanes have filled: lane (row, segment) sums its
// segment of the row, a butterfly over the segments; lanes < DMAX hold their row's sum
template <int DMAX>
__device__ __forceinline__ double rsp_walk_rowsum(const double* red, int rrow, int rseg) {
  constexpr int RP = 65;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < DMAX; ++i) s += red[rrow * RP + rseg * DMAX + i];
#pragma unroll
  for (int m = DMAX; m < 64; m <<= 1) s += shfl_xor(s, m);
  return s;
}

// LDS: [acc: L x (DMAX + 2) of double (LP: + Σ lp | μ̄ | σ̄, 1 + 2·DMAX)][red: DMAX x 65 of double][tx][tg (not LP)][tab][LP: μ | σ,
// 2·DMAX of T][stash] — tiles, table and stash as radial_stack_vjp_walk_kernel.  LP as in rsp_group_body.
template <class T, int DMAX, bool INV, int V, bool LP>
__device__ __forceinline__ void rsp_walk_body(const T* __restrict__ alpha_, const T* __restrict__ beta, const T* __restrict__ z0, int n_layers,
                                              const T* __restrict__ x, const T* gbar, const T* __restrict__ lbar, T* xbar, int dim, int P, int SP,
                                              int64_t batch, double* __restrict__ partials, const RspLogpdf<T>& q) {
#pragma clang fp contract(off)
  static_assert(!LP || INV, "the log-density pass is the inverse run");
  constexpr int LW = DMAX + 4;
  constexpr int AW = DMAX + 2;
  constexpr int RP = 65;                         // odd pitch of the reduction tile: lane (row, segment) reads bank pair (lane + i) mod 32
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tail = n_layers * AW;
  const int nacc = tail + (LP ? 1 + 2 * DMAX : 0);
  double* acc = reinterpret_cast<double*>(smem);
  double* red = acc + (size_t)nacc;
  T* tx = reinterpret_cast<T*>(red + (size_t)DMAX * RP + ((nacc + DMAX * RP) & 1));      // 16-byte aligned
  const size_t tile_e = (((size_t)64 * P + 3) / 4) * 4;
  T* tg = tx + tile_e;
  T* tab = tg + (LP ? 0 : tile_e);
  T* bmu = tab + (((size_t)n_layers * LW + 3) / 4) * 4;
  T* bsg = bmu + DMAX;
  T* stash = bmu + (LP ? 2 * DMAX : 0);
  const int lane = threadIdx.x;
  rs_walk_tables<T, DMAX>(alpha_, beta, z0, n_layers, dim, tab, lane);
  if constexpr (LP) {
    if (lane < DMAX) { bmu[lane] = (q.mu && lane < dim) ? q.mu[lane] : T(0); bsg[lane] = (q.sigma && lane < dim) ? q.sigma[lane] : T(1); }
  }
  for (int i = lane; i < nacc; i += 64) acc[i] = 0.0;
  tile_sync();
  const T dim_m1 = T(dim - 1);
  T* st = stash + (size_t)lane * SP;
  const int rrow = lane & (DMAX - 1), rseg = lane / DMAX;       // this lane's row and segment in the reduction
  T cst = T(0);
  if constexpr (LP) cst = (T)rsp_base_const<T>(bsg, q.sigma != nullptr, dim, lane);
  for (int64_t c0 = (int64_t)blockIdx.x * 64; c0 < batch; c0 += (int64_t)gridDim.x * 64) {
    const int ncols = (int)((batch - c0) < 64 ? (batch - c0) : 64);
    const bool live = lane < ncols;
    tile_stage_in<T, V>(tx, x + c0 * dim, dim, P, ncols, lane);
    if constexpr (!LP) tile_stage_in<T, V>(tg, gbar + c0 * dim, dim, P, ncols, lane);
    tile_sync();
    T* mx = tx + lane * P;
    const T* mg = tg + lane * P;
    T z[DMAX], g[DMAX];
#pragma unroll
    for (int r = 0; r < DMAX; ++r) {
      z[r] = (r < dim && live) ? mx[r] : T(0);
      if constexpr (!LP) g[r] = (r < dim && live) ? mg[r] : T(0);
    }
    const T lb = (lbar && live) ? lbar[c0 + lane] : T(LP && live ? 1 : 0);
    T ldet = T(0);
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
        if constexpr (LP) ldet -= rs_logdet<T>(gain * gam, alpha, bh, dim_m1);
      }
      if (LP || li + 1 < n_layers) {
#pragma unroll
        for (int r = 0; r < DMAX; ++r) {
          if (!INV) z[r] = rs_fma(fwd_gain, dz[r], z[r]);
          else z[r] = rs_fma(gain, dz[r], z0v[r]);
        }
      }
    }
    if constexpr (LP) {
      // ---- the base density at x and the seed ḡ = −c·w/σ; rows past dim hold z = z₀ = 0, μ = 0, σ = 1: w = 0 there
      T ss = T(0);
#pragma unroll
      for (int r = 0; r < DMAX; ++r) {
        const T w = (z[r] - bmu[r]) / bsg[r];
        ss = rs_fma(w, w, ss);
        g[r] = -lb * w / bsg[r];
      }
      const T lp = T(-0.5) * ss - cst + ldet;
      if (live && q.lp_ps) q.lp_ps[c0 + lane] = lp;
      const double slp = group_sum<64>(live ? (double)lp : 0.0);
      if (lane == 0) acc[tail] += slp;
      if (q.want_base) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
          for (int r = 0; r < DMAX; ++r) {
            const T w = (z[r] - bmu[r]) / bsg[r];
            const T t = pass == 0 ? -g[r] : -g[r] * w - lb / bsg[r];
            red[r * RP + lane] = (live && r < dim) ? (double)t : 0.0;
          }
          tile_sync();
          const double s = rsp_walk_rowsum<DMAX>(red, rrow, rseg);
          if (lane < DMAX) acc[tail + 1 + pass * DMAX + lane] += s;
          tile_sync();
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
      if (LP || li + 1 < n_layers) {
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
      const double s = rsp_walk_rowsum<DMAX>(red, rrow, rseg);
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
  const int ltail = n_layers * aw;
  const int per = ltail + (LP ? 1 + (q.want_base ? 2 * dim : 0) : 0);
  double* mine = partials + (size_t)blockIdx.x * per;
  for (int e = lane; e < ltail; e += 64) {
    const int l = e / aw, k = e - l * aw;
    mine[e] = acc[l * AW + (k < dim ? k : DMAX + (k - dim))];
  }
  if constexpr (LP) {
    for (int e = lane; e < per - ltail; e += 64) {          // Σ lp, then μ̄ and σ̄ without the padding rows
      const int k = e - 1;
      mine[ltail + e] = e == 0 ? acc[tail] : acc[tail + 1 + (k < dim ? k : DMAX + (k - dim))];
    }
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
// the last fold and the cast of entry e = (l, k) of the layers' rows [L][dim + 2] in sets of `per` doubles — k < dim: z̄₀; k = dim:
// Σg_α̂ (with k + 1: Σg_β̂) -> ᾱ_, β̄
template <class T>
__device__ __forceinline__ void rsp_final_entry(const T* __restrict__ alpha_, const T* __restrict__ beta, const double* __restrict__ in, int nsets, int per, int dim,
                                                int e, T* __restrict__ alpha_bar, T* __restrict__ beta_bar, T* __restrict__ z0_bar) {
  const int aw = dim + 2;
  const int l = e / aw, k = e - l * aw;
  if (k > dim) return;
  double s = 0.0, s2 = 0.0;
  for (int i = 0; i < nsets; ++i) s += in[(size_t)i * per + e];
  if (k < dim) { z0_bar[(size_t)l * dim + k] = (T)s; return; }
  for (int i = 0; i < nsets; ++i) s2 += in[(size_t)i * per + e + 1];
  const double sa = 1.0 / (1.0 + exp(-(double)alpha_[l])), sb = 1.0 / (1.0 + exp(-(double)beta[l]));
  alpha_bar[l] = (T)(sa * (s - s2));
  beta_bar[l] = (T)(sb * s2);
}

// blocks of the streaming pass: every block walks at least RSP_TILES_MIN tiles, at most `cap` blocks
inline int64_t rsp_grid(int64_t tiles, int64_t cap) {
  int64_t g = (tiles + RSP_TILES_MIN - 1) / RSP_TILES_MIN;
  if (g > cap) g = cap;
  return g < 1 ? 1 : g;
}

#endif  // RS_PARAMS_PASS
