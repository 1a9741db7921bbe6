"""Seeded inputs, Float64 references and the form / edge tables of tests/test_gpu_vec_cholesky_abi.py (the four VecCholesky entry points
of include/bjx.h through the C ABI).  tests/test_host_vec_cholesky_ref.py checks on the CPU that every input and reference is finite,
that the Float32 oracle stays within a tenth of the flat bar of the Float64 one on these inputs (the bar then measures the kernel, not
the conditioning of the data) and that every table shape reaches the form written next to it.  No GPU, no torch.

Reference: always the Float64 oracle on the dt-rounded inputs — `oracle.vec_cholesky`, `oracle.vec_cholesky_inv_vjp`,
`oracle.vec_cholesky_fwd_vjp` (pinned by tests/test_oracle_golden.py on golden files and finite differences).

Draws are functions of (dtype, K, batch) alone and are made for uplo = 'U'; the 'L' operand is the transpose of the 'U' one per sample
(`for_uplo`), so that the 'L' result must be the transpose of the 'U' result bit for bit.

The form functions restate the dispatchers at the end of csrc/bjx_seq.hip (chol_impl, chol_inv_vjp_impl, chol_fwd_vjp_impl) for the
DEFAULT tuning switches; the tables below name, per form, the smallest and the largest K that reaches it."""
import functools
import math
import zlib

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTS = (F32, F64)
LOG_DET_FLOOR = math.log(math.cosh(0.5))
"""floor of the per-element bar of a log-det, 0.12: ONE logcosh term at the scale of the draws (y = 0.5·normal).  A log-det is a sum of such
terms of one sign, each evaluated as |y| + log1p(exp(−2|y|)) − log 2 (LogExpFunctions.logcosh, the form the reference and the kernels use)
with an absolute error of an ulp of log 2; at K = 2 it is one term counted twice and can be arbitrarily near zero, so a log-det below
one typical term is compared on that term.  From K = 3 on |log-det| exceeds the floor and its own magnitude rules."""


def vw(dt):
    """elements of a 16-byte pack"""
    return 16 // np.dtype(dt).itemsize


def nvec(K):
    return K * (K - 1) // 2


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ the dispatchers, restated
# NOTHING ties these three functions to the C++ but the reader: they were compared with chol_impl, chol_inv_vjp_impl and chol_fwd_vjp_impl
# by hand.  The host test checks the tables against THEM only, so whoever changes the dispatch in csrc/bjx_seq.hip (a threshold, a
# (V, CHV) ladder, an LDS limit) must change them and the tables with it, or the GPU file quietly reaches other forms than it names.
LANE_MAX = 11
LDS_MAX = 160 * 1024


def _chunk_cfg(dt, K, packs_ok):
    """(V, CHV) of the chunk / tile kernels: lane L owns CHV packs of V entries of the packed vector"""
    n, w = nvec(K), vw(dt)
    ch = (n + 63) // 64
    if packs_ok and n % w == 0:
        need = (ch + w - 1) // w
        return w, (1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else 16)
    return 1, (2 if ch <= 2 else 8 if ch <= 8 else 16 if ch <= 16 else 32)


def value_form(dt, K, inverse, aligned=True, out=True):
    """bjx_vec_cholesky.  `aligned`: the 16-byte alignment of the pointer that decides V — BOTH `in` and `out` for the lane kernels, the
    packed vector (`in` of the inverse, `out` of the forward) for the chunk kernels.
    -> ("lane", V) | ("chunk", V, CHV) | ("generic",)"""
    sz, n = np.dtype(dt).itemsize, nvec(K)
    if 2 <= K <= LANE_MAX and 64 * ((K * K) | 1) * sz <= 36 * 1024:
        return "lane", (vw(dt) if aligned else 1)
    v, chv = _chunk_cfg(dt, K, aligned)
    chn = v * chv
    if inverse:
        cmax = K
        while cmax * (cmax + 1) // 2 <= 64 * chn - 1:
            cmax += 1
        words = max(cmax * (K + 1) + 1, K * K, 64 * (chn + v))
        words = (words + 4) // 4 * 4
        tile = 2 * words * sz if out else 0
    else:
        tile = 2 * max((K * K + 3) // 4 * 4, 64 * (chn + v)) * sz
    if K >= 2 and chn <= 32 and n <= 64 * 32 and tile <= 80 * 1024:
        return "chunk", v, chv
    return ("generic",)


def inv_vjp_form(dt, K, aligned=True):
    """bjx_vec_cholesky_inv_vjp.  `aligned`: y AND y_bar (and W_bar for the lane kernel).  -> ("lane", V) | ("chunk", V, CHV) | ("refused",)"""
    sz, n = np.dtype(dt).itemsize, nvec(K)
    if K <= LANE_MAX and 64 * (((n + K) | 1) + ((K * K) | 1)) * sz <= 56 * 1024:
        return "lane", (vw(dt) if aligned else 1)
    v, chv = _chunk_cfg(dt, K, aligned)
    chn = v * chv
    tile = 2 * max((K * K + 3) // 4 * 4, 64 * (chn + v)) * sz
    if chn <= 32 and n <= 64 * 32 and tile <= LDS_MAX:
        return "chunk", v, chv
    return ("refused",)


def fwd_vjp_form(dt, K, aligned=True):
    """bjx_vec_cholesky_fwd_vjp.  `aligned`: W, y_bar AND W_bar.  -> ("lane", V) | ("swizzled",) | ("pack",) | ("scalar",) | ("refused",)"""
    sz, n, w = np.dtype(dt).itemsize, nvec(K), vw(dt)
    if K <= LANE_MAX and 64 * (((K * K) | 1) + (n | 1)) * sz <= 56 * 1024:
        return "lane", (w if aligned else 1)
    if ((K * (K + 1) + 3) // 4 * 4 + n + 4) * sz > LDS_MAX:
        return ("refused",)
    v_ok = aligned and (K * K) % w == 0 and n % w == 0
    if v_ok and K & (K - 1) == 0 and K >= w:
        return ("swizzled",)
    return ("pack",) if v_ok else ("scalar",)


# ------------------------------------------------------------------ the tables
# form -> (smallest K, largest K) with every pointer aligned: bjx_vec_cholesky in both directions (with and without `out`) and
# bjx_vec_cholesky_inv_vjp, where ("generic",) reads ("refused",).  K = 17, 33 and 41 (Float32) have an odd K·K: the dense W of every
# second sample of an aligned call is off the 16-byte boundary (the per-sample `bjx_aligned16_dev(Ws)` branch of the chunk kernels).
VALUE_FORMS = {
    F32: [(("lane", 4), (2, 11)), (("chunk", 1, 2), (12, 15)), (("chunk", 4, 1), (16, 17)), (("chunk", 4, 2), (24, 32)), (("chunk", 1, 8), (18, 31)),
          (("chunk", 4, 4), (33, 41)), (("chunk", 4, 8), (48, 64)), (("chunk", 1, 16), (34, 45)), (("chunk", 1, 32), (46, 63)), (("generic",), (65, 100))],
    F64: [(("lane", 2), (2, 8)), (("chunk", 1, 2), (10, 15)), (("chunk", 2, 1), (9, 16)), (("chunk", 2, 2), (17, 21)), (("chunk", 1, 8), (18, 31)),
          (("chunk", 2, 4), (24, 32)), (("chunk", 2, 8), (33, 45)), (("chunk", 1, 16), (34, 43)), (("chunk", 1, 32), (46, 63)), (("chunk", 2, 16), (48, 64)),
          (("generic",), (65, 100))],
}
# K -> form with the deciding base pointer one element off the 16-byte boundary (V = 1 at every K)
OFFSET_FORMS = {
    F32: [(2, ("lane", 1)), (11, ("lane", 1)), (16, ("chunk", 1, 2)), (17, ("chunk", 1, 8)), (32, ("chunk", 1, 8)), (33, ("chunk", 1, 16)), (64, ("chunk", 1, 32))],
    F64: [(2, ("lane", 1)), (8, ("lane", 1)), (16, ("chunk", 1, 2)), (17, ("chunk", 1, 8)), (32, ("chunk", 1, 8)), (33, ("chunk", 1, 16)), (64, ("chunk", 1, 32))],
}
MIXED_KS = (16, 33, 64)               # only the y side offset, only the dense-W side offset, both
# (K, aligned, form) of bjx_vec_cholesky_fwd_vjp; aligned == False: one of the three pointers offset (the test takes each in turn at the
# lane shapes and W_bar at the others)
FWD_VJP_SHAPES = {
    F32: [(2, True, ("lane", 4)), (11, True, ("lane", 4)), (2, False, ("lane", 1)), (11, False, ("lane", 1)),
          (16, True, ("swizzled",)), (64, True, ("swizzled",)), (128, True, ("swizzled",)), (24, True, ("pack",)), (160, True, ("pack",)),
          (12, True, ("scalar",)), (13, True, ("scalar",)), (165, True, ("scalar",)), (16, False, ("scalar",)), (24, False, ("scalar",))],
    F64: [(2, True, ("lane", 2)), (8, True, ("lane", 2)), (2, False, ("lane", 1)), (8, False, ("lane", 1)),
          (16, True, ("swizzled",)), (64, True, ("swizzled",)), (12, True, ("pack",)), (116, True, ("pack",)),
          (9, True, ("scalar",)), (13, True, ("scalar",)), (115, True, ("scalar",)), (16, False, ("scalar",)), (24, False, ("scalar",))],
}
INV_VJP_SERVED, INV_VJP_REFUSED = 64, 65
FWD_VJP_SERVED = {F32: 165, F64: 116}
FWD_VJP_REFUSED = {F32: 166, F64: 117}
LANE_TRIP_KS = (2, 3)                 # the lane kernels' `s0` loop, second and third trip


def table_ks(dt):
    """every K of the tables of `dt`, ascending"""
    dt = np.dtype(dt)
    ks = {k for _, lohi in VALUE_FORMS[dt] for k in lohi} | {k for k, _ in OFFSET_FORMS[dt]} | set(MIXED_KS) | {k for k, _, _ in FWD_VJP_SHAPES[dt]}
    return sorted(ks | {1, 3, FWD_VJP_REFUSED[dt]})


def batches(form):
    """the smallest batches that reach each edge: the lane kernels take 64 samples per wave (one short, one full, a second wave with one
    sample, a third); the chunk kernels 2 per block (the last block's second wave idles on an odd batch); the generic kernels 4."""
    return {"lane": (1, 63, 64, 65, 129), "chunk": (1, 2, 3, 5), "generic": (1, 4, 5), "refused": (1,)}[form[0]]


def fwd_vjp_batches(K, form):
    """chol_fwd_vjp_kernel: one wave = one block per sample; the oracle's pullback loops in Python per sample"""
    if form[0] == "lane":
        return batches(form)
    return (2,) if K >= 115 else (1, 3)


def lane_trip_batch(num_cu):
    """the lane kernels cap their grid at 32 tiles of 64 samples per CU: every block takes a second trip, the first 2 a third (1 sample in the last)"""
    return 2 * (32 * num_cu) * 64 + 65


# ------------------------------------------------------------------ draws
def _f(a, dt):
    return np.asfortranarray(np.asarray(a).astype(dt))


def _keep(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def _draw(dtname, K, batch):
    from oracle import oracle

    dt, n = np.dtype(dtname), nvec(K)
    r = rng_for("vec_cholesky", dtname, K, batch)
    y = _f(0.5 * r.normal(size=(n, batch)), dt)
    W64, _ = oracle.vec_cholesky(np.asfortranarray(y.astype(np.float64)), inverse=True, uplo="U")      # valid factors: the Float64 inverse of the rounded y
    return _keep(dict(y=y, W=_f(W64, dt), W_bar=_f(r.normal(size=(K, K, batch)), dt), y_bar=_f(r.normal(size=(n, batch)), dt),
                      logJ_bar=r.normal(size=batch).astype(dt)))


_draw_cached = functools.lru_cache(maxsize=None)(_draw)


def draw(dtname, K, batch):
    """y = 0.5·normal (n, batch); W (K, K, batch): upper factors, the Float64 oracle inverse of the rounded y, rounded; W_bar (K, K, batch),
    y_bar (n, batch), logJ_bar (batch,): standard normal.  All rounded to the type, read-only, kept (the batches of the `s0` trips are not)."""
    dtname = np.dtype(dtname).name
    return _draw(dtname, K, batch) if batch > 4096 else _draw_cached(dtname, K, batch)


FIRST_ROW_MAGNITUDES = (1e-6, 3e-6, 1e-5, 1e-4, 5.0, 5.25, 5.5, 6.0)
FIRST_ROW_KS = {F32: (2, 11), F64: (2, 8)}        # K = 2, where that entry is the whole sample, and the largest lane K


@functools.lru_cache(maxsize=None)
def draw_first_row_edges(dtname, K):
    """The first-row entries W[1, j] = tanh(y) of the forward link at both ends of atanh, both signs: sample 2m has every first-row y at
    +FIRST_ROW_MAGNITUDES[m] (|w| down to 1e-6, and up to 1 − 1.2e-5 at y = 6: 200 ulp of Float32 from 1), the other entries 0.5·normal;
    sample 2m + 1 is its negative, entry by entry, so W differs from its neighbour by the sign of the strict triangle only and the link,
    odd in every entry, must return the negated y bit for bit.  -> y (n, 16), W (K, K, 16) upper, the Float64 oracle inverse of the rounded
    y, rounded."""
    from oracle import oracle

    dt, n = np.dtype(dtname), nvec(K)
    r = rng_for("first_row_edges", dtname, K)
    y = np.empty((n, 2 * len(FIRST_ROW_MAGNITUDES)))
    first = [c * (c - 1) // 2 for c in range(1, K)]
    for m, mag in enumerate(FIRST_ROW_MAGNITUDES):
        col = 0.5 * r.normal(size=n)
        col[first] = mag
        y[:, 2 * m], y[:, 2 * m + 1] = col, -col
    y = _f(y, dt)
    W64, _ = oracle.vec_cholesky(np.asfortranarray(y.astype(np.float64)), inverse=True, uplo="U")
    return _keep(dict(y=y, W=_f(W64, dt)))


def for_uplo(mat, uplo):
    """the (K, K, batch) operand of `uplo` from the 'U' one: its transpose per sample for 'L'"""
    return mat if uplo == "U" else np.asfortranarray(np.transpose(mat, (1, 0, 2)))


def f64(a):
    return np.asfortranarray(np.asarray(a, np.float64))


# ------------------------------------------------------------------ references (Float64 oracle on the rounded inputs)
def ref_inverse(y, uplo):
    """-> W (K, K, batch), logJ (batch,)"""
    from oracle import oracle

    return oracle.vec_cholesky(f64(y), inverse=True, uplo=uplo)


def ref_forward(W, uplo):
    """-> y (n, batch), log-det (batch,)"""
    from oracle import oracle

    return oracle.vec_cholesky(f64(W), inverse=False, uplo=uplo)


def ref_inv_vjp(y, W_bar, logJ_bar, uplo):
    from oracle import oracle

    return oracle.vec_cholesky_inv_vjp(f64(y), f64(W_bar), None if logJ_bar is None else np.asarray(logJ_bar, np.float64), uplo=uplo)


def ref_fwd_vjp(W, y_bar, uplo, period=None):
    """The oracle's pullback loops in Python per sample.  `period`: the caller states that sample s holds the data of sample s % period
    (the `s0`-trip batches, period prime): the reference of the first `period` samples, tiled."""
    from oracle import oracle

    W, y_bar = np.asarray(W), np.asarray(y_bar)
    if period is None or period >= W.shape[2]:
        return oracle.vec_cholesky_fwd_vjp(f64(W), f64(y_bar), uplo=uplo)
    base = oracle.vec_cholesky_fwd_vjp(f64(W[:, :, :period]), f64(y_bar[:, :period]), uplo=uplo)
    return base[:, :, np.arange(W.shape[2]) % period]


def unused_triangle(K, uplo):
    """index arrays (rows, cols) of the strict triangle that `uplo` does not name"""
    return np.tril_indices(K, -1) if uplo == "U" else np.triu_indices(K, 1)
