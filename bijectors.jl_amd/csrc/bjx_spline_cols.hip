// bjx_spline_cols.hip — RationalQuadraticSpline with one parameter set per COLUMN (include/bjx_cols.h): the spline law of
// Coupling(θ, mask) when θ(x₂) returns per-sample knots (neural spline flows), and the plain per-column spline.
//
// Mapping: a column gets G lanes (G = the power of two >= n1, at most 64); a 256-thread block owns C = 256/G columns at a time
// and walks column groups grid-stride.  Lane (column n, x₁-row r) reads its parameters p[r + j*n1 + n*ld], j = 0..m-1: for every j
// the lanes of a column read n1 consecutive values, and the m slices of a column are one contiguous span when ld = n1*m.
// Parameters are loaded straight into registers (all loads of a lane in flight together); the knots of the common bin counts
// (K = 4, 8, 16) stay in registers with every index known at compile time, other K run a kernel that streams the parameters.
//
// Bin search: the bin is the number of knots below the input, accumulated by a branch-free scan over the knots.  On a
// non-decreasing knot vector (the B constructor always gives one; a valid spline has one) this is exactly
// Base.searchsortedfirst(knots, x) - 1 as `ssf` in bjx_elem.hip computes it: the same `<` comparisons, the same bin at ties.
// The raw form (B constructor, rational_quadratic_spline.jl:109-123) builds the knots in the order of operations of
// rqs_params_kernel (max-subtracted softmax, sequential cumsum, 2B·c − B, log1pexp) so fused and two-step agree to rounding.
// The inverse's log-det is the forward log-det at x = f⁻¹(y) with its own search (interface.jl:276-281), as rqs_elem does.
//
// Per-column log-det: a fixed butterfly over the G lanes of a column; the summed log-det goes through the library's per-block
// partials + bjx_launch_finalize (fixed order: run-to-run identical bits).  The pullback writes x̄ and the per-column parameter
// cotangents in one pass (nothing is summed over columns: no atomics).
#include "bjx_internal.h"
#include "../../include/bjx_cols.h"

namespace {
using namespace bjx;

template <class T> struct ColsArgs {
  const int32_t* idx1;   // [n1] rows of x₁ or null (every row)
  const int32_t* map;    // [dim] row -> position in idx1 or -1 (context scratch), null without idx1
  const T *pw, *ph, *pd;
  int64_t ldw, ldh, ldd;
  int64_t n1, dim, batch, groups;
  int K, G;
  T B;
};

// ------------------------------------------------------------------ knot sources
// get(i, w, h, d) for i = 0, 1, ..., K IN THAT ORDER (the streaming raw source keeps its cumsum); lastw / lasth = knot K.
// Knot arrays in registers (KC > 0: every index a compile-time constant after unrolling).
template <class T, int KC> struct RegKnots {
  T w[KC + 1], h[KC + 1], d[KC + 1];
  __device__ __forceinline__ void get(int i, T& a, T& b, T& c) const { a = w[i]; b = h[i]; c = d[i]; }
  __device__ __forceinline__ T lastw() const { return w[KC]; }
  __device__ __forceinline__ T lasth() const { return h[KC]; }
};

template <class T, int KC> __device__ __forceinline__ void load_knots(RegKnots<T, KC>& k, const T* w, const T* h, const T* d, int64_t st) {
#pragma unroll
  for (int i = 0; i <= KC; ++i) { k.w[i] = w[i * st]; k.h[i] = h[i * st]; k.d[i] = d[i * st]; }
}
// rqs_params_kernel, one element: the same operations in the same order
template <class T, int KC>
__device__ __forceinline__ void raw_knots(RegKnots<T, KC>& k, const T* rw, const T* rh, const T* rd, int64_t st, T B) {
  T r[KC];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const T* src = pass == 0 ? rw : rh;
#pragma unroll
    for (int j = 0; j < KC; ++j) r[j] = src[j * st];
    T mx = r[0];
#pragma unroll
    for (int j = 1; j < KC; ++j) mx = d_max(mx, r[j]);
    T s = T(0);
#pragma unroll
    for (int j = 0; j < KC; ++j) s += d_exp(r[j] - mx);
    T c = T(0);
    T* o = pass == 0 ? k.w : k.h;
    o[0] = (2 * B) * c - B;
#pragma unroll
    for (int j = 0; j < KC; ++j) { c += d_exp(r[j] - mx) / s; o[j + 1] = (2 * B) * c - B; }
  }
  k.d[0] = T(1);
#pragma unroll
  for (int j = 0; j < KC - 1; ++j) k.d[j + 1] = d_log1pexp(rd[j * st]);
  k.d[KC] = T(1);
}

// runtime K, knot form: read from global memory
template <class T> struct GlobKnots {
  const T *w, *h, *d;
  int64_t st;
  int K;
  __device__ __forceinline__ void get(int i, T& a, T& b, T& c) const { a = w[i * st]; b = h[i * st]; c = d[i * st]; }
  __device__ __forceinline__ T lastw() const { return w[K * st]; }
  __device__ __forceinline__ T lasth() const { return h[K * st]; }
};
// runtime K, raw form: the B constructor streamed (max and Σexp first, then the cumsum as the knots are visited)
template <class T> struct RawStream {
  const T *rw, *rh, *rd;
  int64_t st;
  int K;
  T B, mw, sw, mh, sh, lw, lh;
  mutable T cw, ch;
  __device__ void init() {
    mw = rw[0]; mh = rh[0];
    for (int j = 1; j < K; ++j) { mw = d_max(mw, rw[j * st]); mh = d_max(mh, rh[j * st]); }
    sw = T(0); sh = T(0);
    for (int j = 0; j < K; ++j) { sw += d_exp(rw[j * st] - mw); sh += d_exp(rh[j * st] - mh); }
    T a, b, c;
    for (int i = 0; i <= K; ++i) get(i, a, b, c);
    lw = a; lh = b;
  }
  __device__ __forceinline__ void get(int i, T& a, T& b, T& c) const {
    if (i == 0) { cw = T(0); ch = T(0); }
    else { cw += d_exp(rw[(i - 1) * st] - mw) / sw; ch += d_exp(rh[(i - 1) * st] - mh) / sh; }
    a = (2 * B) * cw - B;
    b = (2 * B) * ch - B;
    c = (i == 0 || i == K) ? T(1) : d_log1pexp(rd[(i - 1) * st]);
  }
  __device__ __forceinline__ T lastw() const { return lw; }
  __device__ __forceinline__ T lasth() const { return lh; }
};

// ------------------------------------------------------------------ bin scan and the scalar maps
template <class T> struct Bin { T wlo, wup, hlo, hup, dlo, dup; int k; };   // k = upper knot index = searchsortedfirst - 1

template <class T, int KC, bool ONH, class S>
__device__ __forceinline__ Bin<T> scan_bin(const S& src, int Krt, T v, T wK, T hK) {
  const int K = KC ? KC : Krt;
  Bin<T> b;
  T pw, ph, pd;
  src.get(0, pw, ph, pd);
  b.wlo = -wK; b.hlo = -hK; b.dlo = T(1);                 // k = 0: the lower knot is -knot K, its derivative 1
  b.wup = pw; b.hup = ph; b.dup = pd; b.k = 0;
#pragma unroll
  for (int i = 1; i <= K; ++i) {
    T wi, hi, di;
    src.get(i, wi, hi, di);
    if (i == K) di = T(1);                                  // the derivative at the last knot is 1 (not read)
    const bool c = (ONH ? ph : pw) < v;                     // knot i-1 below v
    b.wlo = c ? pw : b.wlo; b.hlo = c ? ph : b.hlo; b.dlo = c ? pd : b.dlo;
    b.wup = c ? wi : b.wup; b.hup = c ? hi : b.hup; b.dup = c ? di : b.dup;
    b.k = c ? i : b.k;
    pw = wi; ph = hi; pd = di;
  }
  return b;
}

// rational_quadratic_spline.jl:317-357 (the expressions of rqs_forward_dev)
template <class T, int KC, class S>
__device__ __forceinline__ void fwd_elem(const S& src, int K, T wK, T hK, T x, T& y, T& lj) {
  if ((x <= -wK) || (x >= wK)) { y = x; lj = T(0) * x; return; }
  const Bin<T> b = scan_bin<T, KC, false>(src, K, x, wK, hK);
  T w = b.wup - b.wlo;
  T dy = b.hup - b.hlo;
  T s = dy / w;
  T xi = (x - b.wlo) / w;
  T om = T(1) - xi;
  T den = s + (b.dup + b.dlo - 2 * s) * xi * om;
  T num_jl = s * s * (b.dup * (xi * xi) + 2 * s * xi * om + b.dlo * (om * om));
  lj = d_log(num_jl) - 2 * d_log(den);
  T num_y = dy * (s * (xi * xi) + b.dlo * xi * om);
  y = b.hlo + num_y / den;
}
// rational_quadratic_spline.jl:183-220 (rqs_inverse_dev)
template <class T, int KC, class S>
__device__ __forceinline__ T inv_elem(const S& src, int K, T wK, T hK, T y) {
  if ((y <= -hK) || (y >= hK)) return y;
  const Bin<T> b = scan_bin<T, KC, true>(src, K, y, wK, hK);
  T w = b.wup - b.wlo;
  T dy = b.hup - b.hlo;
  T s = dy / w;
  T ds = b.dup + b.dlo - 2 * s;
  T a1 = dy * (s - b.dlo) + (y - b.hlo) * ds;
  T a2 = dy * b.dlo - (y - b.hlo) * ds;
  T a3 = -s * (y - b.hlo);
  T num = -2 * a3;
  T den = a2 + d_sqrt(a2 * a2 - 4 * a1 * a3);
  T xi = num / den;
  return xi * w + b.wlo;
}
template <class T, int KC, bool INV, class S>
__device__ __forceinline__ T spline_elem(const S& src, int K, T& v) {
  const T wK = src.lastw(), hK = src.lasth();
  T y, lj;
  if (!INV) { fwd_elem<T, KC>(src, K, wK, hK, v, y, lj); v = y; return lj; }
  const T x = inv_elem<T, KC>(src, K, wK, hK, v);
  fwd_elem<T, KC>(src, K, wK, hK, x, y, lj);
  v = x;
  return -lj;
}

// ------------------------------------------------------------------ forward / inverse kernel
// KC: compile-time bin count (0 = runtime K); FORM: BJX_COLS_KNOTS / BJX_COLS_RAW.
template <class T, int KC, int FORM, bool INV>
__global__ __launch_bounds__(256) void rqs_cols_kernel(const ColsArgs<T> a, const T* x, T* y, T* __restrict__ ladj_ps, int accumulate,
                                                        double* __restrict__ partials) {
  __shared__ double red[4];
  const int G = a.G, C = 256 / G;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  double acc = 0.0;
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const int64_t col = grp * C + cl;
    T l = T(0);
    if (col < a.batch) {
      for (int64_t r = gl; r < a.n1; r += G) {
        const int64_t row = a.idx1 ? (int64_t)a.idx1[r] : r;
        if (row < 0 || row >= a.dim) continue;               // a bad index list is not a licence to write elsewhere
        T v = x[col * a.dim + row];
        const T* pw = a.pw + r + col * a.ldw;
        const T* ph = a.ph + r + col * a.ldh;
        const T* pd = a.pd ? a.pd + r + col * a.ldd : nullptr;
        if constexpr (KC > 0) {
          RegKnots<T, KC> kn;
          if constexpr (FORM == BJX_COLS_RAW) raw_knots<T, KC>(kn, pw, ph, pd, a.n1, a.B);
          else load_knots<T, KC>(kn, pw, ph, pd, a.n1);
          l += spline_elem<T, KC, INV>(kn, KC, v);
        } else if constexpr (FORM == BJX_COLS_RAW) {
          RawStream<T> kn{pw, ph, pd, a.n1, a.K, a.B};
          kn.init();
          l += spline_elem<T, 0, INV>(kn, a.K, v);
        } else {
          GlobKnots<T> kn{pw, ph, pd, a.n1, a.K};
          l += spline_elem<T, 0, INV>(kn, a.K, v);
        }
        y[col * a.dim + row] = v;
      }
    }
    l = group_sum_rt<T>(l, G);                                // every lane of the wave takes part (idle lanes add 0)
    if (gl == 0 && col < a.batch) {
      if (ladj_ps) ladj_ps[col] = accumulate ? ladj_ps[col] + l : l;
      acc += (double)l;
    }
    if (a.map && x != y) {                                    // rows outside x₁ copy through (coupling.jl:125)
      const int span = C * (int)a.dim;
      for (int q = threadIdx.x; q < span; q += 256) {
        const int c = q / (int)a.dim, row = q - c * (int)a.dim;
        const int64_t cc = grp * C + c;
        if (cc < a.batch && a.map[row] < 0) y[cc * a.dim + row] = x[cc * a.dim + row];
      }
    }
  }
  if (partials) block_publish_partial(acc, red, partials);
}

// ------------------------------------------------------------------ pullback kernel
// Closed-form partials of rational_quadratic_spline.jl:128-164 (value) and :266-297 (logjac), as bjx_rqs_vjp_knots /
// oracle.rqs_vjp_knots, for ONE element; the knot cotangents stay per column.  The raw form continues through the B
// constructor as rqs_params_vjp_kernel does (p̄_i = 2B Σ_{j>i} c̄_j, raw̄_i = p_i (p̄_i − Σ p_m p̄_m), raw̄_d_j = d̄_{j+1} σ(raw_d_j)).
template <class T> struct ElemVjp { T xbar, gw_lo, gw_up, gh_lo, gh_up, gd_lo, gd_up; int klo, kup, on; };

template <class T, int KC, bool INV, class S>
__device__ __forceinline__ ElemVjp<T> vjp_elem(const S& src, int K, T vin, T g, T lb) {
  const T wK = src.lastw(), hK = src.lasth();
  ElemVjp<T> e;
  e.on = 0; e.klo = -1; e.kup = -1;
  e.gw_lo = e.gw_up = e.gh_lo = e.gh_up = e.gd_lo = e.gd_up = T(0);
  const T xv = INV ? inv_elem<T, KC>(src, K, wK, hK, vin) : vin;
  if (!((-wK < xv) && (xv < wK))) { e.xbar = g; return e; }    // identity outside the knots
  const Bin<T> b = scan_bin<T, KC, false>(src, K, xv, wK, hK);
  const T wd = b.wup - b.wlo, dy = b.hup - b.hlo;
  const T s = dy / wd;
  const T dk = b.dlo, dk1 = b.dup;
  const T xi = (xv - b.wlo) / wd;
  const T p = xi * (1 - xi);
  const T om = 1 - 2 * xi;
  const T ds = dk1 + dk - 2 * s;
  const T den = s + ds * p;
  const T M = dk1 * xi * xi + 2 * s * p + dk * (1 - xi) * (1 - xi);
  const T Nn = s * xi * xi + dk * p;
  const T l_xi = (2 * dk1 * xi + 2 * s * om - 2 * dk * (1 - xi)) / M - 2 * ds * om / den;
  const T J = s * s * M / (den * den);
  const T dl = l_xi / wd;
  T gg = g, lbb = lb;
  if (INV) {
    e.xbar = (g - lb * dl) / J;
    gg = -e.xbar;
    lbb = -lb;
  } else {
    e.xbar = g * J + lb * dl;
  }
  const T den2 = den * den;
  const T y_xi = dy * ((2 * s * xi + dk * om) * den - Nn * ds * om) / den2;
  const T y_s = dy * (xi * xi * den - Nn * (1 - 2 * p)) / den2;
  const T y_dh = Nn / den;
  const T y_dk = dy * p * (den - Nn) / den2;
  const T y_dk1 = -dy * Nn * p / den2;
  const T l_s = 2 / s + 2 * p / M - 2 * (1 - 2 * p) / den;
  const T l_dk = (1 - xi) * (1 - xi) / M - 2 * p / den;
  const T l_dk1 = xi * xi / M - 2 * p / den;
  const T Gxi = gg * y_xi + lbb * l_xi, Gs = gg * y_s + lbb * l_s, Gdh = gg * y_dh;
  const T gw_k = (Gxi * (xi - 1) + Gs * s) / wd, gw_k1 = -(Gxi * xi + Gs * s) / wd;
  const T gh_k = gg - Gdh - Gs / wd, gh_k1 = Gdh + Gs / wd;
  e.on = 1;
  e.kup = b.k;
  if (b.k == 0) {                      // lower knot = -knot K
    e.klo = K; e.gw_lo = -gw_k; e.gh_lo = -gh_k; e.gd_lo = T(0);
  } else {
    e.klo = b.k - 1; e.gw_lo = gw_k; e.gh_lo = gh_k; e.gd_lo = gg * y_dk + lbb * l_dk;
  }
  e.gw_up = gw_k1; e.gh_up = gh_k1;
  e.gd_up = (b.k != K) ? gg * y_dk1 + lbb * l_dk1 : T(0);
  return e;
}

// knot index i's cotangent out of the two non-zero entries (the sum in index order of a dense accumulation: exact)
template <class T> __device__ __forceinline__ T pick2(int i, int ka, T va, int kb, T vb) { return (i == ka ? va : T(0)) + (i == kb ? vb : T(0)); }

// raw̄ of one softmax/cumsum head (K raw values at r[j*st]) from the knot cotangents (klo, vlo), (kup, vup): the loops of
// rqs_params_vjp_kernel, descending, on the sparse c̄
template <class T, int KC>
__device__ __forceinline__ void raw_head_vjp(const T* r, int64_t st, int Krt, T B, int klo, T vlo, int kup, T vup, T* out, int64_t ost) {
  const int K = KC ? KC : Krt;
  T mx = r[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = d_max(mx, r[k * st]);
  T s = T(0);
#pragma unroll
  for (int k = 0; k < K; ++k) s += d_exp(r[k * st] - mx);
  T tail = T(0), dot = T(0);
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    tail += pick2<T>(k + 1, klo, vlo, kup, vup);
    dot += (d_exp(r[k * st] - mx) / s) * ((2 * B) * tail);
  }
  tail = T(0);
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    tail += pick2<T>(k + 1, klo, vlo, kup, vup);
    out[k * ost] = (d_exp(r[k * st] - mx) / s) * ((2 * B) * tail - dot);
  }
}

template <class T, int KC, int FORM, bool INV>
__global__ __launch_bounds__(256) void rqs_cols_vjp_kernel(const ColsArgs<T> a, const T* __restrict__ x, const T* __restrict__ gbar,
                                                            const T* __restrict__ lbar, T* __restrict__ xbar, T* __restrict__ wbar,
                                                            T* __restrict__ hbar, T* __restrict__ dbar) {
  const int G = a.G, C = 256 / G;
  const int gl = threadIdx.x & (G - 1), cl = threadIdx.x / G;
  const int K = KC ? KC : a.K;
  const int mw = FORM == BJX_COLS_RAW ? K : K + 1, md = FORM == BJX_COLS_RAW ? K - 1 : K + 1;
  const int64_t ow = (int64_t)a.n1 * mw, od = (int64_t)a.n1 * md;     // dense [n1, m, batch] outputs
  for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
    const int64_t col = grp * C + cl;
    if (col < a.batch) {
      const T lb = lbar ? lbar[col] : T(0);
      for (int64_t r = gl; r < a.n1; r += G) {
        const int64_t row = a.idx1 ? (int64_t)a.idx1[r] : r;
        if (row < 0 || row >= a.dim) continue;
        const T v = x[col * a.dim + row], g = gbar[col * a.dim + row];
        const T* pw = a.pw + r + col * a.ldw;
        const T* ph = a.ph + r + col * a.ldh;
        const T* pd = a.pd ? a.pd + r + col * a.ldd : nullptr;
        ElemVjp<T> e;
        if constexpr (KC > 0) {
          RegKnots<T, KC> kn;
          if constexpr (FORM == BJX_COLS_RAW) raw_knots<T, KC>(kn, pw, ph, pd, a.n1, a.B);
          else load_knots<T, KC>(kn, pw, ph, pd, a.n1);
          e = vjp_elem<T, KC, INV>(kn, KC, v, g, lb);
        } else if constexpr (FORM == BJX_COLS_RAW) {
          RawStream<T> kn{pw, ph, pd, a.n1, a.K, a.B};
          kn.init();
          e = vjp_elem<T, 0, INV>(kn, a.K, v, g, lb);
        } else {
          GlobKnots<T> kn{pw, ph, pd, a.n1, a.K};
          e = vjp_elem<T, 0, INV>(kn, a.K, v, g, lb);
        }
        xbar[col * a.dim + row] = e.xbar;
        T* wo = wbar ? wbar + r + col * ow : nullptr;
        T* ho = hbar ? hbar + r + col * ow : nullptr;
        T* dout = dbar ? dbar + r + col * od : nullptr;
        if constexpr (FORM == BJX_COLS_KNOTS) {
#pragma unroll
          for (int i = 0; i <= K; ++i) {
            if (wo) wo[i * a.n1] = pick2<T>(i, e.klo, e.gw_lo, e.kup, e.gw_up);
            if (ho) ho[i * a.n1] = pick2<T>(i, e.klo, e.gh_lo, e.kup, e.gh_up);
            if (dout) dout[i * a.n1] = pick2<T>(i, e.klo, e.gd_lo, e.kup, e.gd_up);
          }
        } else {
          if (wo) raw_head_vjp<T, KC>(pw, a.n1, K, a.B, e.klo, e.gw_lo, e.kup, e.gw_up, wo, a.n1);
          if (ho) raw_head_vjp<T, KC>(ph, a.n1, K, a.B, e.klo, e.gh_lo, e.kup, e.gh_up, ho, a.n1);
          if (dout) {
#pragma unroll
            for (int j = 0; j < K - 1; ++j)      // d_{j+1} = log1pexp(raw_d_j): d̄_{j+1} σ(raw_d_j)
              dout[j * a.n1] = pick2<T>(j + 1, e.klo, e.gd_lo, e.kup, e.gd_up) / (T(1) + d_exp(-pd[j * a.n1]));
          }
        }
      }
    }
    if (a.map) {                                              // rows outside x₁ pass ȳ through
      const int span = C * (int)a.dim;
      for (int q = threadIdx.x; q < span; q += 256) {
        const int c = q / (int)a.dim, row = q - c * (int)a.dim;
        const int64_t cc = grp * C + c;
        if (cc < a.batch && a.map[row] < 0) xbar[cc * a.dim + row] = gbar[cc * a.dim + row];
      }
    }
  }
}

// ------------------------------------------------------------------ host side
constexpr int kColsThreads = 256;
constexpr int kColsBlocksPerCu = 8;

// rowmap as build_rowmap in bjx_elem.hip (-1 = copy-through row); the kernel reads x₁ through idx1 itself
__global__ void cols_rowmap_kernel(const int32_t* idx1, int64_t n1, int64_t dim, int32_t* map) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n1) {
    const int32_t r = idx1[i];
    if (r >= 0 && r < dim) map[r] = (int32_t)i;
  }
}

template <class T>
int cols_setup(bjx_ctx* ctx, const char* name, int form, const int32_t* idx1, int64_t n1, const void* p_w, const void* p_h, const void* p_d,
               int64_t ld_w, int64_t ld_h, int64_t ld_d, int K, double B, int64_t dim, int64_t batch, ColsArgs<T>* a, int* grid) {
  ColsArgs<T> c{};
  c.idx1 = idx1;
  c.map = nullptr;
  c.pw = (const T*)p_w; c.ph = (const T*)p_h; c.pd = (form == BJX_COLS_RAW && K == 1) ? nullptr : (const T*)p_d;
  c.ldw = ld_w; c.ldh = ld_h; c.ldd = ld_d;
  c.n1 = n1; c.dim = dim; c.batch = batch; c.K = K; c.B = (T)B;
  int G = 1;
  while (G < 64 && G < n1) G <<= 1;
  c.G = G;
  const int C = kColsThreads / G;
  c.groups = (batch + C - 1) / C;
  if (idx1 && n1 < dim) {
    BJX_REQUIRE(ctx, (size_t)dim * sizeof(int32_t) + 16 <= BJX_SCRATCH_BYTES, BJX_ERR_UNSUPPORTED, "%s: dim %lld too large for the context scratch", name, (long long)dim);
    int32_t* map = static_cast<int32_t*>(ctx->scratch);
    BJX_HIP(ctx, hipMemsetAsync(map, 0xFF, (size_t)dim * sizeof(int32_t), ctx->stream));
    if (n1 > 0) {
      hipLaunchKernelGGL(cols_rowmap_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, ctx->stream, idx1, n1, dim, map);
      BJX_CHECK_LAUNCH(ctx);
    }
    c.map = map;
  }
  const int64_t cap = (int64_t)ctx->num_cu * kColsBlocksPerCu;
  *grid = (int)(c.groups < cap ? c.groups : cap);
  *a = c;
  return BJX_OK;
}

int cols_check(bjx_ctx* ctx, const char* name, bjx_dtype dt, int form, const int32_t* idx1, int64_t n1, const void* p_w, const void* p_h,
               const void* p_d, int64_t ld_w, int64_t ld_h, int64_t ld_d, int K, double B, int64_t dim, int64_t batch) {
  BJX_REQUIRE(ctx, dt == BJX_F32 || dt == BJX_F64, BJX_ERR_ARG, "%s: bad dtype %d", name, (int)dt);
  BJX_REQUIRE(ctx, form == BJX_COLS_KNOTS || form == BJX_COLS_RAW, BJX_ERR_ARG, "%s: bad form %d", name, form);
  BJX_REQUIRE(ctx, K >= 1 && K <= BJX_COLS_MAX_BINS, BJX_ERR_UNSUPPORTED, "%s: %d bins (1 ... %d supported)", name, K, BJX_COLS_MAX_BINS);
  BJX_REQUIRE(ctx, dim >= 0 && batch >= 0 && n1 >= 0 && n1 <= dim, BJX_ERR_SHAPE, "%s: bad size (n1=%lld, dim=%lld, batch=%lld)", name, (long long)n1,
              (long long)dim, (long long)batch);
  BJX_REQUIRE(ctx, idx1 || n1 == dim, BJX_ERR_SHAPE, "%s: without idx1 every row is transformed (n1=%lld, dim=%lld)", name, (long long)n1, (long long)dim);
  BJX_REQUIRE(ctx, dim < ((int64_t)1 << 22), BJX_ERR_UNSUPPORTED, "%s: dim %lld too large", name, (long long)dim);
  const int64_t mw = form == BJX_COLS_RAW ? K : K + 1, md = form == BJX_COLS_RAW ? K - 1 : K + 1;
  BJX_REQUIRE(ctx, ld_w >= n1 * mw && ld_h >= n1 * mw && (md == 0 || ld_d >= n1 * md), BJX_ERR_SHAPE,
              "%s: column strides (%lld, %lld, %lld) below n1 x m (%lld x %lld, %lld x %lld)", name, (long long)ld_w, (long long)ld_h, (long long)ld_d,
              (long long)n1, (long long)mw, (long long)n1, (long long)md);
  BJX_REQUIRE(ctx, p_w && p_h && (p_d || md == 0), BJX_ERR_ARG, "%s: null parameter pointer", name);
  BJX_REQUIRE(ctx, form == BJX_COLS_KNOTS || B > 0.0, BJX_ERR_ARG, "%s: the B constructor needs B > 0 (got %g)", name, B);
  return BJX_OK;
}

template <class T, bool INV, int FORM>
void launch_fwd(bjx_ctx* ctx, const ColsArgs<T>& a, int grid, const T* in, T* out, T* ladj_ps, int accum, double* partials) {
#define RC(KC_) hipLaunchKernelGGL((rqs_cols_kernel<T, KC_, FORM, INV>), dim3((unsigned)grid), dim3(kColsThreads), 0, ctx->stream, a, in, out, ladj_ps, accum, partials)
  switch (a.K) {
    case 4: RC(4); break;
    case 8: RC(8); break;
    case 16: RC(16); break;
    default: RC(0); break;
  }
#undef RC
}

template <class T>
int rqs_cols_impl(bjx_ctx* ctx, int inverse, int form, const int32_t* idx1, int64_t n1, const void* p_w, const void* p_h, const void* p_d, int64_t ld_w,
                  int64_t ld_h, int64_t ld_d, int K, double B, const T* in, T* out, T* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (batch == 0) {
    if (ladj_sum && !(flags & BJX_ACCUMULATE)) BJX_HIP(ctx, hipMemsetAsync(ladj_sum, 0, sizeof(double), ctx->stream));
    return BJX_OK;
  }
  ColsArgs<T> a;
  int grid = 0;
  int rc = cols_setup<T>(ctx, "bjx_rqs_cols", form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, dim, batch, &a, &grid);
  if (rc) return rc;
  if (ladj_sum) { rc = bjx_ensure_partials(ctx, (size_t)grid); if (rc) return rc; }
  double* partials = ladj_sum ? ctx->partials : nullptr;
  const int accum = (flags & BJX_ACCUMULATE) ? 1 : 0;
  {
    BjxProf prof_(ctx);
    if (form == BJX_COLS_RAW) { if (inverse) launch_fwd<T, true, BJX_COLS_RAW>(ctx, a, grid, in, out, ladj_ps, accum, partials); else launch_fwd<T, false, BJX_COLS_RAW>(ctx, a, grid, in, out, ladj_ps, accum, partials); }
    else { if (inverse) launch_fwd<T, true, BJX_COLS_KNOTS>(ctx, a, grid, in, out, ladj_ps, accum, partials); else launch_fwd<T, false, BJX_COLS_KNOTS>(ctx, a, grid, in, out, ladj_ps, accum, partials); }
  }
  BJX_CHECK_LAUNCH(ctx);
  if (ladj_sum) return bjx_launch_finalize(ctx, grid, ladj_sum, 0.0, 0, 0.0, flags);
  return BJX_OK;
}

template <class T, bool INV, int FORM>
void launch_vjp(bjx_ctx* ctx, const ColsArgs<T>& a, int grid, const T* in, const T* gb, const T* lb, T* xb, T* wb, T* hb, T* db) {
#define RV(KC_) hipLaunchKernelGGL((rqs_cols_vjp_kernel<T, KC_, FORM, INV>), dim3((unsigned)grid), dim3(kColsThreads), 0, ctx->stream, a, in, gb, lb, xb, wb, hb, db)
  switch (a.K) {
    case 4: RV(4); break;
    case 8: RV(8); break;
    case 16: RV(16); break;
    default: RV(0); break;
  }
#undef RV
}

template <class T>
int rqs_cols_vjp_impl(bjx_ctx* ctx, int inverse, int form, const int32_t* idx1, int64_t n1, const void* p_w, const void* p_h, const void* p_d,
                      int64_t ld_w, int64_t ld_h, int64_t ld_d, int K, double B, const T* in, const T* gb, const T* lb, T* xb, T* wb, T* hb, T* db,
                      int64_t dim, int64_t batch) {
  if (batch == 0 || dim == 0) return BJX_OK;
  ColsArgs<T> a;
  int grid = 0;
  int rc = cols_setup<T>(ctx, "bjx_rqs_cols_vjp", form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, dim, batch, &a, &grid);
  if (rc) return rc;
  if (form == BJX_COLS_RAW && K == 1) db = nullptr;          // no raw derivative parameters
  {
    BjxProf prof_(ctx);
    if (form == BJX_COLS_RAW) { if (inverse) launch_vjp<T, true, BJX_COLS_RAW>(ctx, a, grid, in, gb, lb, xb, wb, hb, db); else launch_vjp<T, false, BJX_COLS_RAW>(ctx, a, grid, in, gb, lb, xb, wb, hb, db); }
    else { if (inverse) launch_vjp<T, true, BJX_COLS_KNOTS>(ctx, a, grid, in, gb, lb, xb, wb, hb, db); else launch_vjp<T, false, BJX_COLS_KNOTS>(ctx, a, grid, in, gb, lb, xb, wb, hb, db); }
  }
  BJX_CHECK_LAUNCH(ctx);
  return BJX_OK;
}
}  // namespace

BJX_API int bjx_rqs_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, int form, const int32_t* idx1, int64_t n1, const void* p_w, const void* p_h,
                         const void* p_d, int64_t ld_w, int64_t ld_h, int64_t ld_d, int K, double B, const void* in, void* out, void* ladj_ps,
                         double* ladj_sum, int64_t dim, int64_t batch, uint32_t flags) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = cols_check(ctx, "bjx_rqs_cols", dt, form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out) || dim * batch == 0, BJX_ERR_ARG, "bjx_rqs_cols: null pointer");
  if (dt == BJX_F32)
    return rqs_cols_impl<float>(ctx, inverse, form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, (const float*)in, (float*)out, (float*)ladj_ps, ladj_sum, dim, batch, flags);
  return rqs_cols_impl<double>(ctx, inverse, form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, (const double*)in, (double*)out, (double*)ladj_ps, ladj_sum, dim, batch, flags);
}

BJX_API int bjx_rqs_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, int form, const int32_t* idx1, int64_t n1, const void* p_w, const void* p_h,
                             const void* p_d, int64_t ld_w, int64_t ld_h, int64_t ld_d, int K, double B, const void* in, const void* out_bar,
                             const void* ladj_bar, void* in_bar, void* w_bar, void* h_bar, void* d_bar, int64_t dim, int64_t batch) {
  if (!ctx) return BJX_ERR_ARG;
  int rc = cols_check(ctx, "bjx_rqs_cols_vjp", dt, form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, dim, batch);
  if (rc) return rc;
  BJX_REQUIRE(ctx, (in && out_bar && in_bar) || dim * batch == 0, BJX_ERR_ARG, "bjx_rqs_cols_vjp: null pointer");
  if (dt == BJX_F32)
    return rqs_cols_vjp_impl<float>(ctx, inverse, form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, (const float*)in, (const float*)out_bar,
                                    (const float*)ladj_bar, (float*)in_bar, (float*)w_bar, (float*)h_bar, (float*)d_bar, dim, batch);
  return rqs_cols_vjp_impl<double>(ctx, inverse, form, idx1, n1, p_w, p_h, p_d, ld_w, ld_h, ld_d, K, B, (const double*)in, (const double*)out_bar,
                                   (const double*)ladj_bar, (double*)in_bar, (double*)w_bar, (double*)h_bar, (double*)d_bar, dim, batch);
}
