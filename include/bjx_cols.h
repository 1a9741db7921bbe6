/* bjx_cols.h — companion of bjx.h: the RationalQuadraticSpline law with one parameter set per COLUMN.
 *
 * Coupling(θ, mask) (coupling.jl:206-259) evaluates θ on each sample's x₂; when θ returns
 * RationalQuadraticSpline(w, h, d[, B]) every column of a batch has its own knots (the neural spline coupling of
 * Durkan et al., 2019).  bjx_rqs / bjx_coupling_rqs take ONE knot table shared by the batch; these two entries take
 * a table per column.  bjx.h itself is unchanged (its prototypes are pinned by the Julia binding's tests); the
 * Julia side does not bind these entries yet.
 *
 * Layout: parameter j of x₁-row r in column n is at p[r + j*n1 + n*ld] — each column is an (n1 x m) column-major
 * matrix, ld >= n1*m.  The three ld's are separate, so three slices of ONE network head [n1, 3K-1, batch] are
 * passed with no copy.
 *   BJX_COLS_KNOTS: p_w, p_h, p_d have m = K+1 (knot arrays as for bjx_rqs).
 *   BJX_COLS_RAW:   p_w, p_h have m = K, p_d has m = K-1, plus B > 0: the B constructor
 *                   (rational_quadratic_spline.jl:109-123) evaluated in registers inside the spline kernel, in the
 *                   order of operations of bjx_rqs_params.  No pass writes normalised knots.  With K = 1, p_d holds
 *                   no values and may be NULL.
 * The bin of an input is the number of knots below it — Base.searchsortedfirst on the (non-decreasing) knot vector,
 * the same `<` comparisons and the same bin at ties on a knot.  Outside the first / last knot the map is the identity
 * with log-det 0·x.
 *
 * 1 <= K <= 64 bins (BJX_ERR_UNSUPPORTED otherwise).  Float32 and Float64.  No host synchronisation and no allocation
 * beyond the context's scratch, so a step that uses them can be captured (run it once outside the capture first). */
#ifndef BJX_COLS_H
#define BJX_COLS_H

#include "bjx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BJX_COLS_KNOTS = 0, BJX_COLS_RAW = 1 };
#define BJX_COLS_MAX_BINS 64

/* Spline law with one parameter set per column.  idx1: int32[n1] transformed rows (0-based), or NULL with n1 == dim
 * (plain per-column spline over every row).  Rows outside idx1 are copied through (coupling.jl:125).
 * inverse, ladj_ps, ladj_sum, flags: as bjx_coupling_rqs (BJX_ACCUMULATE honoured; the summed log-det is a
 * deterministic, fixed-order reduction). */
int bjx_rqs_cols(bjx_ctx* ctx, bjx_dtype dt, int inverse, int form, const int32_t* idx1, int64_t n1,
                 const void* p_w, const void* p_h, const void* p_d, int64_t ld_w, int64_t ld_h, int64_t ld_d, int K,
                 double B, const void* in, void* out, void* ladj_ps, double* ladj_sum, int64_t dim, int64_t batch,
                 uint32_t flags);

/* Pullback of the same call.  in = x (inverse=0) or y (inverse=1: implicit function theorem at x = f^-1(y), like
 * bjx_rqs_vjp_knots).  in_bar: [dim, batch] (rows outside idx1 pass out_bar through).  w_bar / h_bar / d_bar:
 * PER-COLUMN cotangents of the parameters in the call's form, dense [n1, m, batch], NOT summed over the batch; any
 * of them may be NULL.  ladj_bar: T[batch] or NULL (= 0). */
int bjx_rqs_cols_vjp(bjx_ctx* ctx, bjx_dtype dt, int inverse, int form, const int32_t* idx1, int64_t n1,
                     const void* p_w, const void* p_h, const void* p_d, int64_t ld_w, int64_t ld_h, int64_t ld_d, int K,
                     double B, const void* in, const void* out_bar, const void* ladj_bar, void* in_bar, void* w_bar,
                     void* h_bar, void* d_bar, int64_t dim, int64_t batch);

#ifdef __cplusplus
}
#endif

#endif /* BJX_COLS_H */
