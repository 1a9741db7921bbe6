// bjx_flow_cols.inc — lane helpers of the column-tile Planar kernels (bjx_flow_cols.hip, bjx_planar_logpdf.hip).  Included inside
// the including file's anonymous namespace, after bjx_flow_common.inc.
__device__ __forceinline__ float lane_bcast(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ double lane_bcast(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
template <int G> __device__ __forceinline__ float group_sum_fast(float v) { return group_sum_f32_dpp<G>(v); }
template <int G> __device__ __forceinline__ double group_sum_fast(double v) { return group_sum<G>(v); }
// C values per lane -> lane L holds the wave sum of value L / (64 / C): log2(C) halving exchanges (C/2 + C/4 + ... shuffles in all)
// and one butterfly over the 64 / C lanes that are left, instead of C full butterflies (6·C shuffles).
template <class T, int C, int G> __device__ __forceinline__ T wave_sum_scatter_rec(const T (&s)[C], int lane) {
  if constexpr (C == 1) return group_sum_fast<G>(s[0]);
  else {
    constexpr int H = G / 2;
    const bool hi = lane & H;
    T a[C / 2];
#pragma unroll
    for (int i = 0; i < C / 2; ++i) a[i] = (hi ? s[C / 2 + i] : s[i]) + shfl_xor(hi ? s[i] : s[C / 2 + i], H);
    return wave_sum_scatter_rec<T, C / 2, H>(a, lane);
  }
}
template <class T, int C> __device__ __forceinline__ T wave_sum_scatter(const T (&s)[C], int lane) {
  static_assert(C == 1 || C == 2 || C == 4 || C == 8 || C == 16, "C");
  return wave_sum_scatter_rec<T, C, 64>(s, lane);
}
