"""Float64 reference of the amortised Sylvester layer (include/bjx_sylvester_cols.h): the closed forms in numpy over all columns at
once.  Inputs are rounded to the tested dtype first, so the reference and the kernel start from the same numbers.
tests/test_host_sylvester_cols.py holds this module to an independent evaluation (the dense finite-difference Jacobian's slogdet,
central differences in every parameter).

Per column, with U = triu(R), Ũ = triu(R̃) (diagonal included; the strict lower triangles are never read):
    s = Qᵀz;  t = Ũs + b;  a = tanh t;  p = Ua;  y = z + Qp;  d = 1 + (1 − a²)⊙diag(R̃)⊙diag(R);  ladj = Σ log|d|
and the pullback of (ȳ, ℓ̄), hp = 1 − a²:
    p̄ = Qᵀȳ;  ā = Uᵀp̄;  t̄ = ā⊙hp − ℓ̄·2a⊙hp⊙diag(R̃)⊙diag(R)/d;  s̄ = Ũᵀt̄;  z̄ = ȳ + Qs̄;  Q̄ = ȳpᵀ + z s̄ᵀ;
    R̄ = triu(p̄aᵀ) + diag(ℓ̄·hp⊙diag(R̃)/d);  R̃̄ = triu(t̄sᵀ) + diag(ℓ̄·hp⊙diag(R)/d);  b̄ = t̄.
Shapes: Q (dim, M, N); R, R̃ (M, M, N); b (M, N); z, ȳ (dim, N); ℓ̄ (N,).

Draws: Q = the thin QR factor of a normal matrix per column, off-diagonals of R and R̃ ~ N(0, 1)/√M, diagonals 0.9·tanh(N(0, 1)),
b ~ 0.5·N(0, 1), z, ȳ, ℓ̄ ~ N(0, 1); seeded per case by zlib.crc32 of the case's key (the siblings' `seed`).  The strict lower
triangles are drawn too (they must not matter).  Two fixed columns are part of every draw:
  column 0   R = 0: the identity, log-det 0, Q̄ = z s̄ᵀ;
  column 1   (when N >= 2) R̃_00 = 1.5, R_00 = −2 (product −3) and b_0 set so that the pre-activation of unit 0 is 0.1 (Ũ_0·s + b_0 =
             0.1; with z, Q of unit scale a b_0 left at its draw would let tanh saturate and d_0 → 1): d_0 = 1 − 3(1 − tanh²0.1) ≈ −1.97,
             negative with |d_0| >= 0.2 — it holds the absolute value in the log-det and the sign of the diagonal terms."""
import numpy as np

from _radial_cols_ref import rounded, seed  # noqa: F401  (re-exported: the siblings' seeding)


def draws(rng, dim, M, N, dt):
    """-> Q, R, R̃, b, z, ȳ, ℓ̄ rounded to `dt`, as float64 arrays, with the two fixed columns."""
    assert 1 <= M <= dim
    Q = np.empty((dim, M, N))
    for n in range(N):
        Q[:, :, n] = np.linalg.qr(rng.normal(size=(dim, M)))[0]
    R = rng.normal(size=(M, M, N)) / np.sqrt(M)
    Rt = rng.normal(size=(M, M, N)) / np.sqrt(M)
    idx = np.arange(M)
    R[idx, idx, :] = 0.9 * np.tanh(rng.normal(size=(M, N)))
    Rt[idx, idx, :] = 0.9 * np.tanh(rng.normal(size=(M, N)))
    b = 0.5 * rng.normal(size=(M, N))
    z, g, lb = rng.normal(size=(dim, N)), rng.normal(size=(dim, N)), rng.normal(size=N)
    Q, R, Rt, z, g, lb = (rounded(a, dt) for a in (Q, R, Rt, z, g, lb))
    R[:, :, 0] = 0.0
    if N >= 2:
        R[0, 0, 1], Rt[0, 0, 1] = -2.0, 1.5
        s1 = Q[:, :, 1].T @ z[:, 1]
        b[0, 1] = 0.1 - np.triu(Rt[:, :, 1])[0] @ s1
    b = rounded(b, dt)
    return Q, R, Rt, b, z, g, lb


def _amax(a):
    return np.abs(a).reshape(-1, a.shape[-1]).max(axis=0)


class RefAll:
    """Everything the layer returns: out (dim, N), ladj (N,), d (M, N), in_bar (dim, N), qb (dim, M, N), rb, rtb (M, M, N), bb (M, N),
    and `scale` (N,): the per-column TERM scale of the parameter cotangents — the largest of ‖ȳ‖∞‖p‖∞ + ‖z‖∞‖s̄‖∞ (Q̄), ‖p̄‖∞‖a‖∞ + the
    diagonal term (R̄), ‖t̄‖∞‖s‖∞ + the diagonal term (R̃̄), |ā⊙hp| + |ℓ̄·2a hp R̃_mm R_mm/d| (b̄ = t̄) and of the reference cotangents
    themselves: the rounding of a cotangent lives on the scale of its summands, not of their (possibly cancelling) sum."""

    def __init__(self, Q, R, Rt, b, z, g, lb=None):
        dim, M, N = Q.shape
        lb = np.zeros(N) if lb is None else lb
        mask = np.triu(np.ones((M, M)))[:, :, None]
        U, Ut = np.where(mask > 0, R, 0.0), np.where(mask > 0, Rt, 0.0)      # where, not a product: a NaN below the diagonal is never read
        idx = np.arange(M)
        rd, rtd = R[idx, idx, :], Rt[idx, idx, :]
        s = np.einsum("rmn,rn->mn", Q, z)
        t = np.einsum("ijn,jn->in", Ut, s) + b
        a = np.tanh(t)
        p = np.einsum("ijn,jn->in", U, a)
        hp = 1.0 - a * a
        self.d = 1.0 + hp * rtd * rd
        self.out = z + np.einsum("rmn,mn->rn", Q, p)
        self.ladj = np.log(np.abs(self.d)).sum(axis=0)
        pb = np.einsum("rmn,rn->mn", Q, g)
        ab = np.einsum("ijn,in->jn", U, pb)
        t1, t2 = ab * hp, lb * (-2.0 * a * hp * rtd * rd / self.d)
        tb = t1 + t2
        sb = np.einsum("ijn,in->jn", Ut, tb)
        self.in_bar = g + np.einsum("rmn,mn->rn", Q, sb)
        self.qb = g[:, None, :] * p[None, :, :] + z[:, None, :] * sb[None, :, :]
        er, ert = lb * hp * rtd / self.d, lb * hp * rd / self.d
        self.rb = pb[:, None, :] * a[None, :, :] * mask
        self.rb[idx, idx, :] += er
        self.rtb = tb[:, None, :] * s[None, :, :] * mask
        self.rtb[idx, idx, :] += ert
        self.bb = tb
        scale = _amax(g) * _amax(p) + _amax(z) * _amax(sb)
        scale = np.maximum(scale, _amax(pb) * _amax(a) + _amax(er))
        scale = np.maximum(scale, _amax(tb) * _amax(s) + _amax(ert))
        scale = np.maximum(scale, _amax(np.abs(t1) + np.abs(t2)))
        for c_ in (self.qb, self.rb, self.rtb, self.bb):
            scale = np.maximum(scale, _amax(c_))
        self.scale = scale
