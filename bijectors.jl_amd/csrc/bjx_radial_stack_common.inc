// bjx_radial_stack_common.inc — device and host helpers shared by bjx_radial_stack.hip and bjx_radial_stack_params.hip; included
// INSIDE each file's anonymous namespace (after `using namespace bjx;` and bjx_flow_common.inc), so every translation unit has its
// own internal copies.

constexpr size_t RS_LDS_BUDGET = 64 * 1024;      // per block: tables + (pullback) per-layer scalars; beyond it the entry refuses
constexpr int RS_R_MAX = 8;                      // packs per lane of the group form (FLOW_R_MAX of bjx_flow.hip)

template <int R> struct StackUC { static constexpr int value = R == 1 ? 4 : (R == 2 ? 2 : 1); };      // RadialUC of bjx_flow.hip
template <int R> struct StackVjpUC { static constexpr int value = R == 1 ? 2 : 1; };                  // UC of radial_vjp_kernel

__host__ __device__ inline size_t rs_round16(size_t b) { return (b + 15) / 16 * 16; }

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
  const T h_ = T(1) / (alpha + r_fwd);
  ld = dim_m1 * d_log(T(1) + beta_hat * h_) + d_log(T(1) + beta_hat * h_ + beta_hat * (-(h_ * h_)) * r_fwd);   // :68-70
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
