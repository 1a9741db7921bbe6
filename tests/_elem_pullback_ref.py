"""numpy Float64 references and the seeded inputs of the C-ABI edge suites of the one-pass kernels in csrc/bjx_elem.hip:
tests/test_gpu_batchnorm_train_abi.py (bjx_batchnorm_stats / _train / _train_apply, bjx_row_moments -> bjx_batchnorm_train_vjp) and
tests/test_gpu_coupling_affine_vjp.py (bjx_coupling_affine_vjp).  tests/test_host_elem_pullback_ref.py pins the coupling reference on
central differences of the oracle and checks that every reference output is finite on every input drawn here; the training values and
their pullback are `oracle.batchnorm_train` / `oracle.batchnorm_train_vjp` (the latter pinned by central differences in
tests/test_oracle_golden.py), called with Float64 copies of the dt-rounded inputs.  No GPU, no torch.

Every input is a function of (dtype, dim, batch, seed) alone, drawn once and kept (treat the arrays as read-only)."""
import functools
import zlib

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


def vw(dt):
    """elements of a 16-byte pack"""
    return 16 // np.dtype(dt).itemsize


def lanes(dt, dim, aligned=True):
    """(V, G) of col_launch_cfg / coupling_affine_vjp_impl: V = the pack width when the columns are whole aligned packs, else 1;
    G = the lanes a column gets, the power of two >= dim / V, at most 64."""
    v = vw(dt) if (aligned and dim % vw(dt) == 0) else 1
    packs, g = dim // v, 1
    while g < 64 and g < packs:
        g <<= 1
    return v, g


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f(a, dt):
    return np.asfortranarray(np.asarray(a).astype(dt))


# ------------------------------------------------------------------ training-mode InvertibleBatchNorm
# (dim, aligned): `aligned == False` = the (dim, batch) array is viewed one element into its buffer
STATS_SHAPES = {F32: [(1, True), (5, True), (64, True), (100, True), (101, True), (130, True), (300, True), (520, True), (1024, True), (256, False)],
                F64: [(3, True), (64, True), (129, True), (130, True), (258, True), (512, True)]}
# columns of more than 256 packs: refused before the windows of bjx_row_moments were given the per-row shift
LIFTED_SHAPES = {F32: [(257, True), (301, True), (1028, True), (2051, True), (300, False)], F64: [(257, True), (514, True), (1030, True)]}
LIFTED_BATCHES = (2, 65, 300)
VJP_DIMS = {F32: [5, 13, 64, 257, 300, 1024], F64: [5, 64, 257, 258]}
VJP_BATCHES = (2, 37, 257, 1000)
EPS, MTM = 1e-5, 0.1


def stats_form(dt, dim, aligned=True):
    """what bn_stats_impl launches: (V, G, R) of bn_stats_kernel, or (VW, 64, 0) for the windows of more than 256 packs"""
    v, g = lanes(dt, dim, aligned)
    nvc = dim // v
    if nvc > 256:
        return vw(dt), 64, 0
    return v, g, 1 if nvc <= g else (2 if nvc <= 2 * g else 4)


def stats_launches(dt, dim, aligned=True):
    """kernel launches of one bjx_batchnorm_stats call (include/bjx.h), whatever the batch"""
    if stats_form(dt, dim, aligned)[2]:
        return 2
    return 2 if dim % vw(dt) == 0 else 4


def stats_batches(dt, dim, aligned=True):
    """c = 256 / G columns per block, u = 16 c columns per block and trip of the grid: the tail loop only, one block, two blocks with one
    trip of the unrolled loop, three and five blocks (the empty quarters and the k-tail of bn_stats_reduce_kernel)"""
    g = stats_form(dt, dim, aligned)[1]
    c = 256 // g
    u = 16 * c
    return sorted({b for b in (1, 2, c - 1, c + 1, u - 1, u + 1, 2 * u + 7, 4 * u + 3) if b >= 1})


@functools.lru_cache(maxsize=None)
def draw_bn(dtname, dim, batch, seed=0):
    """x: every row with its own mean in [-2, 2] and a spread (standard deviation over the batch) in [0.5, 1.5]; b, logs; the moving statistics m0 (near the row means), v0;
    the cotangents g (of out) and lb (of the log-det).  All rounded to the type."""
    dt = np.dtype(dtname)
    r = rng_for("bn", dtname, dim, batch, seed)
    mu, sd = r.uniform(-2.0, 2.0, size=dim), r.uniform(0.5, 1.5, size=dim)
    z = r.normal(size=(dim, batch))
    if batch >= 2:                                       # the spread of every row is `sd` at any batch, two columns included
        z = (z - z.mean(axis=1, keepdims=True)) / z.std(axis=1, keepdims=True)
    d = dict(x=_f(mu[:, None] + sd[:, None] * z, dt), b=r.normal(size=dim).astype(dt), logs=(0.3 * r.normal(size=dim)).astype(dt),
             m0=(mu + 0.1 * r.normal(size=dim)).astype(dt), v0=r.uniform(0.5, 2.0, size=dim).astype(dt),
             g=_f(r.normal(size=(dim, batch)), dt), lb=r.normal(size=batch).astype(dt))
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def draw_bn_constant_row(dtname, dim, batch, seed=0):
    """draw_bn with ONE exactly constant row: x = 0.5, moving mean 0.25 — every sum of that row is exact, its variance exactly 0"""
    d = {k: v.copy(order="K") for k, v in draw_bn(dtname, dim, batch, seed).items()}
    row = dim // 2
    d["x"][row, :] = 0.5
    d["m0"][row] = 0.25
    d["row"] = row
    return d


@functools.lru_cache(maxsize=None)
def draw_bn_conditioned(dtname, dim, batch, seed=0):
    """|mean| >> std.  Float32: mean = 100 std, moving mean 0.  Float64: mean 1e6, std 1e-2, moving mean 1e6, eps 1e-12 (the data of
    test_batchnorm_training_large_mean_float64).  `center`: a value c with x - c exact in Float64 — the reference is evaluated on x - c."""
    dt = np.dtype(dtname)
    r = rng_for("bn_cond", dtname, dim, batch, seed)
    if dt == F32:
        sd = r.uniform(0.5, 1.5, size=dim)
        x, m0, eps, center = _f(100.0 * sd[:, None] + sd[:, None] * r.normal(size=(dim, batch)), dt), np.zeros(dim, dt), EPS, 0.0
    else:
        x, m0, eps, center = _f(1e6 + 1e-2 * r.normal(size=(dim, batch)), dt), np.full(dim, 1e6, dt), 1e-12, 1e6
    return dict(x=x, b=r.normal(size=dim).astype(dt), logs=(0.3 * r.normal(size=dim)).astype(dt), m0=m0, v0=np.ones(dim, dt),
                g=_f(r.normal(size=(dim, batch)), dt), lb=r.normal(size=batch).astype(dt), eps=eps, center=center)


def ref_stats(x, shift):
    """(Σ_n (x − shift), Σ_n (x − shift)², N) per row, Float64 (shift None = 0)"""
    d = np.asarray(x, np.float64)
    if shift is not None:
        d = d - np.asarray(shift, np.float64)[:, None]
    return d.sum(axis=1), (d * d).sum(axis=1), d.shape[1]


def ref_moments(a, b):
    """bjx_row_moments: (Σ_n a, Σ_n a·b) per row, Float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.sum(axis=1), (a * b).sum(axis=1)


def batch_mean_var(x, center=0.0):
    """the batch statistics the forward pass normalises with, two passes in Float64 on x − center (exact for the conditioned draws)"""
    d = np.asarray(x, np.float64) - center
    dm = d.mean(axis=1)
    return dm + center, ((d - dm[:, None]) ** 2).sum(axis=1) / d.shape[1], d - dm[:, None]


# ------------------------------------------------------------------ affine coupling pullback
# (dim, aligned): `aligned == False` = `in` starts one element into its buffer
COUPLING_SHAPES = {F32: [(1, True), (3, True), (12, True), (64, True), (67, True), (256, True), (260, True), (64, False)],
                   F64: [(7, True), (12, True), (130, True), (128, True)]}
MASKS = ("scattered", "range", "unsorted", "all", "none")


def coupling_batches(dt, dim, aligned=True):
    """c = 256 / G columns per block and step of the four-column unroll: one, two or three of the four columns in flight, the block edge, a
    second block with one column, a third block"""
    c = 256 // lanes(dt, dim, aligned)[1]
    return sorted({b for b in (1, c - 1, c + 1, 2 * c + 1, 4 * c - 1, 4 * c, 4 * c + 1, 8 * c + 3) if b >= 1})


def mask_rows(kind, dim, seed=0):
    """idx1 (int32, 0-based): scattered sorted rows, a contiguous range, an unsorted permutation of a subset, every row, none"""
    r = rng_for("mask", kind, dim, seed)
    n1 = max(1, dim // 2)
    if kind == "scattered":
        idx = np.sort(r.choice(dim, size=n1, replace=False))
    elif kind == "range":
        lo = (dim - n1) // 2
        idx = np.arange(lo, lo + n1)
    elif kind == "unsorted":
        idx = r.permutation(r.choice(dim, size=n1, replace=False))
        if n1 > 1 and (np.diff(idx) > 0).all():
            idx = idx[::-1]
    elif kind == "all":
        idx = np.arange(dim)
    elif kind == "none":
        idx = np.zeros(0, np.int64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(idx, np.int32)


@functools.lru_cache(maxsize=None)
def draw_coupling(dtname, dim, batch, seed=0, mask="scattered"):
    """idx1; scale with |s| in [0.5, 2] and a random sign, shift: (n1, batch); x, gbar: (dim, batch); lbar: (batch,)"""
    dt = np.dtype(dtname)
    idx1 = mask_rows(mask, dim, seed)
    n1 = len(idx1)
    r = rng_for("coupling", dtname, dim, batch, seed, mask)
    d = dict(idx1=idx1, scale=_f(r.uniform(0.5, 2.0, size=(n1, batch)) * r.choice([-1.0, 1.0], size=(n1, batch)), dt), shift=_f(r.normal(size=(n1, batch)), dt),
             x=_f(r.normal(size=(dim, batch)), dt), gbar=_f(r.normal(size=(dim, batch)), dt), lbar=r.normal(size=batch).astype(dt))
    for a in d.values():
        a.setflags(write=False)
    return d


def ref_coupling_affine_vjp(idx1, scale, shift, x, gbar, lbar, inverse):
    """The closed forms above coupling_affine_vjp_kernel (coupling.jl:206-259 with b = Shift(t) ∘ Scale(s)), Float64:
      forward:  x̄₁ = s ȳ₁,   s̄ = ȳ₁ x₁ + ℓ̄/s,          t̄ = ȳ₁
      inverse:  ȳ₁ = x̄₁/s,   s̄ = −(x̄₁/s) x₁ − ℓ̄/s,     t̄ = −x̄₁/s      (x₁ = (y₁ − t)/s)
    scale None = 1, shift None = 0, lbar None = 0; row idx1[k] uses parameter row k; the other rows pass gbar through.
    -> (in_bar (dim, batch), scale_bar (n1, batch), shift_bar (n1, batch))"""
    x, g = np.asarray(x, np.float64), np.asarray(gbar, np.float64)
    idx1 = np.asarray(idx1, np.int64)
    n1, batch = len(idx1), x.shape[1]
    s = np.ones((n1, batch)) if scale is None else np.asarray(scale, np.float64)
    t = np.zeros((n1, batch)) if shift is None else np.asarray(shift, np.float64)
    lb = np.zeros(batch) if lbar is None else np.asarray(lbar, np.float64)
    in_bar = g.copy()
    g1 = g[idx1]
    if not inverse:
        in_bar[idx1] = s * g1
        return in_bar, g1 * x[idx1] + lb / s, g1.copy()
    x1 = (x[idx1] - t) / s
    in_bar[idx1] = g1 / s
    return in_bar, -(g1 / s) * x1 - lb / s, -g1 / s


def scale_bar_term_scale(idx1, scale, shift, x, gbar, lbar, inverse):
    """Per column, the largest summand of s̄ = ±(ȳ₁ x₁ + ℓ̄/s): the two terms have either sign, and the rounding of their sum is relative to the
    larger TERM, not to a sum that cancels (`term_scale` of _tol.flat_close; with n1 == 1 a column of s̄ is that one sum)."""
    idx1 = np.asarray(idx1, np.int64)
    n1, batch = len(idx1), np.shape(x)[1]
    s = np.ones((n1, batch)) if scale is None else np.asarray(scale, np.float64)
    t = np.zeros((n1, batch)) if shift is None else np.asarray(shift, np.float64)
    lb = np.zeros(batch) if lbar is None else np.asarray(lbar, np.float64)
    x1, g1 = np.asarray(x, np.float64)[idx1], np.asarray(gbar, np.float64)[idx1]
    a = np.abs(g1 * x1) if not inverse else np.abs(g1 / s * (x1 - t) / s)
    return np.maximum(a, np.abs(lb / s)).max(axis=0) if n1 else np.zeros(batch)
