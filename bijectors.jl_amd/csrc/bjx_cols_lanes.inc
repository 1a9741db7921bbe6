// bjx_cols_lanes.inc — the lane geometry of the per-column flow kernels (bjx_planar_cols.hip, bjx_radial_cols.hip): the packs a
// lane of a column's group holds, and their loads and stores in the vector (AL) and the element form.  Included INSIDE each
// file's anonymous namespace (after `using namespace bjx;`), so every translation unit has its own internal copies.

// the packs of one lane: pack r starts at row off[r] and has nrow[r] live rows (0: the pack does not exist)
template <int V, int R> struct LanePacks {
  int off[R], nrow[R];
  __device__ __forceinline__ LanePacks(int gl, int G, int dim) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = (gl + r * G) * V;
      off[r] = row;
      nrow[r] = dim - row <= 0 ? 0 : (dim - row < V ? dim - row : V);
    }
  }
};

// streamed once (x, ȳ): nontemporal; AL: whole packs on 16-byte aligned addresses
template <class T, int V, int R, bool AL> __device__ __forceinline__ void load_data(const T* col, const LanePacks<V, R>& lp, Pack<T, V> (&p)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lp.nrow[r] > 0) {
      if constexpr (AL) p[r] = load_pack<T, V, true>(col + lp.off[r]);
      else p[r] = load_pack_part<T, V>(col + lp.off[r], lp.nrow[r]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) p[r].v[j] = T(0);
    }
  }
}
// parameters: through the caches (the pullback reads every row twice; short columns share cache lines between layers)
template <class T, int V, int R, bool AL> __device__ __forceinline__ void load_param(const T* col, const LanePacks<V, R>& lp, Pack<T, V> (&p)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lp.nrow[r] > 0) {
      if constexpr (AL) p[r] = load_pack<T, V, false>(col + lp.off[r]);
      else p[r] = load_pack_part_cached<T, V>(col + lp.off[r], lp.nrow[r]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) p[r].v[j] = T(0);
    }
  }
}
template <class T, int V, int R, bool AL> __device__ __forceinline__ void store_data(T* col, const LanePacks<V, R>& lp, const Pack<T, V> (&p)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lp.nrow[r] > 0) {
      if constexpr (AL) store_pack<T, V, true>(col + lp.off[r], p[r]);
      else store_pack_part<T, V>(col + lp.off[r], p[r], lp.nrow[r]);
    }
  }
}
