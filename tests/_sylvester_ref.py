"""Float64 reference of the shared Sylvester layer (include/bjx_sylvester.h, `SylvesterLayer`): the closed forms in numpy over all
columns at once, with ONE parameter set.  Inputs are rounded to the tested dtype first, so the reference and the kernel start from the
same numbers.  tests/test_host_sylvester.py holds this module to central differences in every shared parameter and every input, and to
the per-column sibling's reference (tests/_sylvester_cols_ref.py, whose module docstring writes out the per-column forms) on expanded
parameters.

With U = triu(R), Ũ = triu(R̃) (diagonal included; the strict lower triangles are never read), Q (dim, M), b (M,), z, ȳ (dim, N), ℓ̄ (N,):
    s = Qᵀz;  t = Ũs + b;  a = tanh t;  p = Ua;  y = z + Qp;  d = 1 + (1 − a²)⊙diag(R̃)⊙diag(R);  ladj = Σ_m log|d_m|
    p̄ = Qᵀȳ;  ā = Uᵀp̄;  t̄ = ā⊙hp − ℓ̄·2a⊙hp⊙diag(R̃)⊙diag(R)/d;  s̄ = Ũᵀt̄;  z̄ = ȳ + Qs̄
    Q̄ = Σ_n ȳpᵀ + z s̄ᵀ;  R̄ = Σ_n triu(p̄aᵀ) + diag(ℓ̄·hp⊙diag(R̃)/d);  R̃̄ = Σ_n triu(t̄sᵀ) + diag(ℓ̄·hp⊙diag(R)/d);  b̄ = Σ_n t̄.
The summands are kept next to the sums (`qb_cols` (dim, M, N), `rb_cols`, `rtb_cols` (M, M, N), `bb_cols` (M, N)); `summed(n)` adds
them over the first n columns only, so one draw serves every batch size of a test.  `term_scale(n)` is the largest, over those
columns, of the sibling's per-column term scale (RefAll.scale: the parts of every summand taken by absolute value, and the summands
themselves): what a sum over the batch rounds on is the size of the terms it adds, not of their possibly cancelling sum.

Draws (`draws`): the sibling's recipe with one parameter set — Q the thin QR factor of a normal matrix, off-diagonals of R and R̃
~ N(0, 1)/√M, diagonals 0.9·tanh(N(0, 1)) (|R_mm R̃_mm| <= 0.81, so every d >= 0.19), b ~ 0.5·N(0, 1), z, ȳ, ℓ̄ ~ N(0, 1); the strict lower
triangles are drawn too (they must not matter); seeded per case by the siblings' `seed`.

The negative-determinant recipe (`draws(..., negdet=True)`): a shared layer cannot pin a unit's pre-activation through b per column,
so R_00 = −2, R̃_00 = 1.5, row 0 of triu(R̃) is zero off the diagonal (t_0 = 1.5·s_0 + b_0) and every column's z is moved along q_0
until t_0 takes, cycling over the columns, the values NEGDET_T0.  d_0 = 1 − 3(1 − tanh²t_0): <= −1.5 for the small values, >= 0.7 for the
large ones — columns of both signs, none near d = 0.  It holds the absolute value in the log-det and the sign of the diagonal terms.

`GPU_DRAWS` lists every draw the GPU test uses; the host test asserts min|d| >= 0.2 over them and its own."""
import numpy as np

from _radial_cols_ref import rounded, seed  # noqa: F401  (re-exported: the siblings' seeding)

NEGDET_T0 = (0.1, -0.3, 2.0, -2.5, 0.4, -0.2, 3.0)


def draws(rng, dim, M, N, dt, negdet=False):
    """-> Q (dim, M), R, R̃ (M, M), b (M,), z, ȳ (dim, N), ℓ̄ (N,) rounded to `dt`, as float64 arrays."""
    assert 1 <= M <= dim
    Q = np.linalg.qr(rng.normal(size=(dim, M)))[0]
    R = rng.normal(size=(M, M)) / np.sqrt(M)
    Rt = rng.normal(size=(M, M)) / np.sqrt(M)
    idx = np.arange(M)
    R[idx, idx] = 0.9 * np.tanh(rng.normal(size=M))
    Rt[idx, idx] = 0.9 * np.tanh(rng.normal(size=M))
    b = 0.5 * rng.normal(size=M)
    z, g, lb = rng.normal(size=(dim, N)), rng.normal(size=(dim, N)), rng.normal(size=N)
    Q, R, Rt, b, z, g, lb = (rounded(a, dt) for a in (Q, R, Rt, b, z, g, lb))
    if negdet:
        R[0, 0], Rt[0, 0] = -2.0, 1.5
        Rt[0, 1:] = 0.0
        q0 = Q[:, 0]
        want = np.array([NEGDET_T0[n % len(NEGDET_T0)] for n in range(N)])
        delta = ((want - b[0]) / 1.5 - q0 @ z) / (q0 @ q0)
        z = rounded(z + q0[:, None] * delta[None, :], dt)
    return Q, R, Rt, b, z, g, lb


def _amax(a):
    return np.abs(a).reshape(-1, a.shape[-1]).max(axis=0)


class RefShared:
    """Everything the layer returns: out (dim, N), ladj (N,), d (M, N), in_bar (dim, N), the summands `qb_cols`, `rb_cols`, `rtb_cols`,
    `bb_cols`, their sums over all columns qb (dim, M), rb, rtb (M, M), bb (M,), and `scale_cols` (N,), the per-column term scale."""

    def __init__(self, Q, R, Rt, b, z, g, lb=None):
        dim, M = Q.shape
        N = z.shape[1]
        lb = np.zeros(N) if lb is None else lb
        upper = np.triu(np.ones((M, M))) > 0
        U, Ut = np.where(upper, R, 0.0), np.where(upper, Rt, 0.0)        # where, not a product: a NaN below the diagonal is never read
        rd, rtd = np.diag(R)[:, None], np.diag(Rt)[:, None]
        s = Q.T @ z
        t = Ut @ s + b[:, None]
        a = np.tanh(t)
        p = U @ a
        hp = 1.0 - a * a
        self.d = 1.0 + hp * rtd * rd
        self.out = z + Q @ p
        self.ladj = np.log(np.abs(self.d)).sum(axis=0)
        pb = Q.T @ g
        ab = U.T @ pb
        t1, t2 = ab * hp, lb * (-2.0 * a * hp * rtd * rd / self.d)
        tb = t1 + t2
        sb = Ut.T @ tb
        self.in_bar = g + Q @ sb
        er, ert = lb * hp * rtd / self.d, lb * hp * rd / self.d
        up3 = upper[:, :, None]
        idx = np.arange(M)
        self.qb_cols = g[:, None, :] * p[None, :, :] + z[:, None, :] * sb[None, :, :]
        self.rb_cols = np.where(up3, pb[:, None, :] * a[None, :, :], 0.0)
        self.rb_cols[idx, idx, :] += er
        self.rtb_cols = np.where(up3, tb[:, None, :] * s[None, :, :], 0.0)
        self.rtb_cols[idx, idx, :] += ert
        self.bb_cols = tb
        scale = _amax(g) * _amax(p) + _amax(z) * _amax(sb)
        scale = np.maximum(scale, _amax(pb) * _amax(a) + _amax(er))
        scale = np.maximum(scale, _amax(tb) * _amax(s) + _amax(ert))
        scale = np.maximum(scale, _amax(np.abs(t1) + np.abs(t2)))
        for c_ in (self.qb_cols, self.rb_cols, self.rtb_cols, self.bb_cols):
            scale = np.maximum(scale, _amax(c_))
        self.scale_cols = scale
        self.N = N
        self.qb, self.rb, self.rtb, self.bb = self.summed(N)

    def summed(self, n):
        """-> (Q̄, R̄, R̃̄, b̄) of the FIRST n columns alone: the same summands, added over fewer columns."""
        return self.qb_cols[:, :, :n].sum(axis=2), self.rb_cols[:, :, :n].sum(axis=2), self.rtb_cols[:, :, :n].sum(axis=2), self.bb_cols[:, :n].sum(axis=1)

    def term_scale(self, n=None):
        """The largest per-column term scale over the first n columns (all of them by default); 0 for an empty sum."""
        n = self.N if n is None else n
        with np.errstate(invalid="ignore"):
            return float(np.nanmax(self.scale_cols[:n])) if n and np.isfinite(self.scale_cols[:n]).any() else 0.0


class Draw:
    """One draw and its reference, computed once; the tests slice its first n columns."""

    def __init__(self, dt, dim, M, N, key, negdet=False):
        self.dt, self.dim, self.M, self.N, self.key, self.negdet = dt, dim, M, N, key, negdet
        self.Q, self.R, self.Rt, self.b, self.z, self.g, self.lb = draws(seed(*key), dim, M, N, dt, negdet)
        self.ref = RefShared(self.Q, self.R, self.Rt, self.b, self.z, self.g, self.lb)


# ------------------------------------------------------------------ every draw of tests/test_gpu_zz_sylvester_shared.py
F32, F64 = np.float32, np.float64
DIMS = {F32: [1, 2, 3, 5, 4, 8, 16, 64, 65, 260, 261, 516, 765, 1024], F64: [1, 2, 3, 5, 4, 8, 16, 64, 65, 256, 257, 384, 512]}
UNITS = (1, 2, 3, 5, 16)
SYL_TILES_MIN, SYL_FOLD_CHUNK = 4, 32          # the constants of bijectors.jl_amd/csrc/bjx_sylvester.hip
REDUCTION_SHAPES = ((F32, 2, 2), (F32, 64, 16), (F64, 5, 3))


def lanes(dim, dt):
    packs = -(-dim // (16 // np.dtype(dt).itemsize))
    G = 1
    while G < 64 and G < packs:
        G *= 2
    return G


def batches(C):
    return sorted({n for n in (1, C - 1, C, C + 1) if n >= 1})


def reduction_batches(C):
    return [SYL_TILES_MIN * C, 3 * SYL_TILES_MIN * C - 5, (SYL_FOLD_CHUNK + 1) * SYL_TILES_MIN * C - 3]


def edge_draws(dt):
    """(dim, M, N, key) of the dispatcher edges of one dtype."""
    for dim in DIMS[dt]:
        for M in UNITS:
            if M <= dim:
                yield dim, M, max(batches(256 // lanes(dim, dt))), ("sylvester-shared", np.dtype(dt).name, dim, M)


def gpu_draws():
    """(dt, dim, M, N, key, negdet) of every draw the GPU test makes through `Draw`."""
    for dt in (F32, F64):
        for dim, M, N, key in edge_draws(dt):
            yield dt, dim, M, N, key, False
    for dt, dim, M in REDUCTION_SHAPES:
        yield dt, dim, M, max(reduction_batches(256 // lanes(dim, dt))), ("sylvester-shared-reduce", np.dtype(dt).name, dim), False
    for dt in (F32, F64):
        yield dt, 8, 3, 45, ("sylvester-shared-negdet", np.dtype(dt).name), True
        for tag in ("nan-low", "nan-col", "bits", "unaligned"):
            yield dt, 12, 3, 70, ("sylvester-shared-" + tag, np.dtype(dt).name), False
    yield F64, 6, 3, 50, ("sylvester-shared-route",), False
    yield F64, 6, 2, 50, ("sylvester-shared-route2",), False
    yield F64, 5, 1, 9, ("sylvester-shared-vector",), False
    yield F32, 8, 2, 5, ("sylvester-shared-abi",), False
    for dt, dim, M in ((F32, 128, 13), (F32, 128, 14), (F64, 256, 7), (F64, 256, 8)):
        yield dt, dim, M, 256 // lanes(dim, dt) + 1, ("sylvester-shared-lds", np.dtype(dt).name, dim, M), False
