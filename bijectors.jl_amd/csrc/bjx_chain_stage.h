// Stage kinds and closed-form partials of the elementwise-chain pullbacks, shared by bjx_coupling_chain.hip (per-sample parameters,
// per-column cotangents) and bjx_chain_vjp.hip (shared parameters, cotangents summed over the batch).  Included INSIDE the anonymous
// namespace of each translation unit (after `using namespace bjx;`), like bjx_linkmath.h.
// stage kinds inside the kernels: the ABI kinds plus the inverses that have no ABI kind of their own (a per-sample Shift cannot
// be negated on the host)
enum : int { CK_ID = 0, CK_EXP, CK_LOG, CK_SHIFT, CK_SHIFT_INV, CK_SCALE, CK_SCALE_INV, CK_LOGIT, CK_LOGIT_INV, CK_LEAKY, CK_LEAKY_INV, CK_FLIP, CK_AFFINE, CK_AFFINE_INV };

// value and closed-form partials of one stage at its input u (the derivatives of oracle.chain_vjp, plus the parameter partials)
template <class T> struct StageD { T dy, dl, ya, la, yb, lb; };

template <class T> __device__ __forceinline__ StageD<T> stage_partials(const int kind, T& v, const T a, const T b) {
  StageD<T> d;
  d.dy = T(1); d.dl = T(0); d.ya = T(0); d.la = T(0); d.yb = T(0); d.lb = T(0);
  const T u = v;
  switch (kind) {
    case CK_EXP: v = d_exp(u); d.dy = v; d.dl = T(1); break;
    case CK_LOG: { const T iu = T(1) / u; v = d_log(u); d.dy = iu; d.dl = -iu; } break;
    case CK_SHIFT: v = a + u; d.ya = T(1); break;
    case CK_SCALE: v = a * u; d.dy = a; d.ya = u; d.la = T(1) / a; break;
    case CK_SCALE_INV: { const T ia = T(1) / a; v = ia * u; d.dy = ia; d.ya = -u * ia * ia; d.la = -ia; } break;
    case CK_LOGIT: {
      const T ixa = T(1) / (u - a), ixb = T(1) / (b - u), iw = T(1) / (b - a);
      v = d_log((u - a) * ixb);
      d.dy = ixa + ixb; d.dl = ixb - ixa;                  // ladj = -log(u-a) - log(b-u) + log(b-a)
      d.ya = -ixa; d.yb = -ixb; d.la = ixa - iw; d.lb = iw - ixb;
    } break;
    case CK_LOGIT_INV: {
      const T w = b - a, sg = d_logistic(u), iw = T(1) / w;
      v = w * sg + a;
      d.dy = w * sg * (T(1) - sg); d.dl = T(1) - 2 * sg;   // ladj = log(sg (1 - sg)) + log(b - a)
      d.ya = T(1) - sg; d.yb = sg; d.la = -iw; d.lb = iw;
    } break;
    case CK_LEAKY: {
      const bool neg = u < T(0);
      const T J = neg ? a : T(1);
      v = J * u; d.dy = J; d.ya = neg ? u : T(0); d.la = neg ? T(1) / a : T(0);
    } break;
    case CK_FLIP: v = -u; d.dy = T(-1); break;
    case CK_AFFINE: v = b + a * u; d.dy = a; d.ya = u; d.la = T(1) / a; d.yb = T(1); break;
    default: break;
  }
  return d;
}

