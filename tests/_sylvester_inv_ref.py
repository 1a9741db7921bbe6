"""Float64 reference of the INVERSE of the shared Sylvester layer (include/bjx_sylvester_inv.h, `SylvesterLayer(..., orthonormal=True)`):
the back-substitution, the inverse's input pullback and, through the implicit-function rule, its parameter pullback, in numpy over all
columns at once.  tests/test_host_sylvester_inv.py holds this module to the forward reference (tests/_sylvester_ref.py), to the
transposed Jacobian through the forward reference's `in_bar`, and to central differences over a dense Newton solve of the forward forms.

With U = triu(R), Ũ = triu(R̃), k_m = R_mm·R̃_mm and QᵀQ = I, per column y:
    s′ = Qᵀy;  for m = M−1 … 0:  c_m = b_m + Σ_{j>m} Ũ_mj s_j,  ρ_m = s′_m − Σ_{j>m} U_mj a_j,
               α + k_m·tanh(α + c_m) = R̃_mm·ρ_m,  a_m = tanh(α + c_m),  s_m = ρ_m − R_mm·a_m
    z = y − Q(s′ − s);  d = 1 + (1 − a²)⊙k;  ladj = −Σ_m log|d_m|          (of the inverse)
The pullback of (z̄, c) on (z, ladj), hp = 1 − a²:
    e = −2a⊙hp⊙k/d;  η = Qᵀz̄ − c·Ũᵀe;  for m = 0 … M−1:  σ_m = Σ_{j<m} U_jm π_j,
               π_m = (η_m − Ũ_mm·hp_m·σ_m − Σ_{i<m} Ũ_im τ_i)/d_m,  τ_m = hp_m·(U_mm·π_m + σ_m)
    ȳ = z̄ − Q·Ũᵀ(c·e + τ)
and the parameter cotangents are MINUS the forward parameter pullback (RefShared) at z with the cotangents (ȳ, c): `fwd` is that forward
reference, `summed(n)` negates its sums over the first n columns, `term_scale(n)` is its term scale.

The scalar equation is solved by a safeguarded Newton iteration on [w − |k|, w + |k|] (the left side is increasing for k > −1 and
|k·tanh| <= |k|) to a step below one Float64 ulp.

Draws (`inv_draws`): the forward recipe of tests/_sylvester_ref.py; the data y is the forward reference's image of the drawn z, rounded to
the tested dtype, so y lies in the layer's range at unit scale.  The near-singular recipe (`near_singular`): R̃_00 = 1.25,
R_00 = −(1 − 2⁻¹⁰)/1.25 (k_0 = −1 + 2⁻¹⁰), row 0 of triu(R̃) zero off the diagonal, and z moved along q_0 until t_0 = 1.25·s_0 + b_0 spans
±0.05 over the columns: min d ≈ 1e-3."""
import numpy as np

from _sylvester_ref import RefShared, draws, lanes, rounded, seed  # noqa: F401

F32, F64 = np.float32, np.float64


def solve_alpha(w, k, c, iters=200):
    """α with α + k·tanh(α + c) = w, elementwise; NaN in, NaN out."""
    w, k, c = np.broadcast_arrays(np.asarray(w, np.float64), np.asarray(k, np.float64), np.asarray(c, np.float64))
    lo, hi = w - np.abs(k), w + np.abs(k)
    a = np.clip(w - k * np.tanh(w + c), lo, hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(iters):
            t = np.tanh(a + c)
            f = a + k * t - w
            lo, hi = np.where(f < 0, a, lo), np.where(f > 0, a, hi)
            an = a - f / (1.0 + k * (1.0 - t * t))
            an = np.where((an >= lo) & (an <= hi), an, 0.5 * (lo + hi))
            if np.array_equal(an, a, equal_nan=True):
                break
            a = an
    return a


def inverse_map(Q, R, Rt, b, y):
    """-> z (dim, N), s′, s, a (M, N) by the back-substitution; only the upper triangles are read."""
    M = Q.shape[1]
    sp = Q.T @ y
    s, a = np.zeros_like(sp), np.zeros_like(sp)
    for m in range(M - 1, -1, -1):
        c, rho = b[m] + np.zeros(y.shape[1]), sp[m].copy()
        for j in range(m + 1, M):
            c += Rt[m, j] * s[j]
            rho -= R[m, j] * a[j]
        al = solve_alpha(Rt[m, m] * rho, R[m, m] * Rt[m, m], c)
        a[m] = np.tanh(al + c)
        s[m] = rho - R[m, m] * a[m]
    return y - Q @ (sp - s), sp, s, a


class RefInv:
    """Everything inverse(layer) returns at y: out = z (dim, N), ladj (N,), d (M, N), in_bar = ȳ (dim, N), and `fwd`, the forward reference
    at z with the cotangents (ȳ, c), whose parameter sums are minus the inverse's."""

    def __init__(self, Q, R, Rt, b, y, zb, c=None):
        dim, M = Q.shape
        N = y.shape[1]
        c = np.zeros(N) if c is None else c
        z, sp, s, a = inverse_map(Q, R, Rt, b, y)
        k = (np.diag(R) * np.diag(Rt))[:, None]
        hp = 1.0 - a * a
        d = 1.0 + hp * k
        self.out, self.d, self.a, self.s = z, d, a, s
        self.ladj = -np.log(np.abs(d)).sum(axis=0)
        e = -2.0 * a * hp * k / d
        eta = Q.T @ zb
        for m in range(M):
            for i in range(m + 1):
                eta[m] -= c * Rt[i, m] * e[i]
        pi, tau = np.zeros_like(a), np.zeros_like(a)
        for m in range(M):
            sg, st = np.zeros(N), np.zeros(N)
            for j in range(m):
                sg += R[j, m] * pi[j]
                st += Rt[j, m] * tau[j]
            pi[m] = (eta[m] - Rt[m, m] * hp[m] * sg - st) / d[m]
            tau[m] = hp[m] * (R[m, m] * pi[m] + sg)
        v = np.zeros_like(a)
        for m in range(M):
            for i in range(m + 1):
                v[m] += Rt[i, m] * (c * e[i] + tau[i])
        self.in_bar = zb - Q @ v
        self.N = N
        self.fwd = RefShared(Q, R, Rt, b, z, self.in_bar, c)

    def summed(self, n):
        """-> (q̄, r̄, r̃̄, b̄) of the inverse summed over the first n columns."""
        return tuple(-t for t in self.fwd.summed(n))

    def term_scale(self, n=None):
        return self.fwd.term_scale(n)


def inv_draws(rng, dim, M, N, dt, zero_diag=False):
    """-> Q, R, R̃, b, z (the pre-image), y (the data: the layer's image of z, rounded to `dt`), z̄, c.  `zero_diag` (M >= 3): R̃_11 = 0 and
    R_22 = 0 exactly — units whose scalar equation has k = 0, one with a zero right-hand side factor."""
    Q, R, Rt, b, z, g, lb = draws(rng, dim, M, N, dt)
    if zero_diag:
        Rt[1, 1], R[2, 2] = 0.0, 0.0
    y = rounded(RefShared(Q, R, Rt, b, z, g, lb).out, dt)
    return Q, R, Rt, b, z, y, g, lb


def near_singular(rng, dim, M, N, dt):
    """The near-singular recipe of the module docstring -> Q, R, R̃, b, z, y, z̄, c."""
    Q, R, Rt, b, z, g, lb = draws(rng, dim, M, N, dt)
    Rt[0, 0] = 1.25
    R[0, 0] = -(1.0 - 2.0 ** -10) / 1.25
    Rt[0, 1:] = 0.0
    R, Rt = rounded(R, dt), rounded(Rt, dt)
    q0 = Q[:, 0]
    want = np.linspace(-0.05, 0.05, N)
    delta = ((want - b[0]) / 1.25 - q0 @ z) / (q0 @ q0)
    z = rounded(z + q0[:, None] * delta[None, :], dt)
    y = rounded(RefShared(Q, R, Rt, b, z, g, lb).out, dt)
    return Q, R, Rt, b, z, y, g, lb


class InvDraw:
    """One draw and its reference, computed once; the tests slice its first n columns."""

    def __init__(self, dt, dim, M, N, key, recipe="plain"):
        self.dt, self.dim, self.M, self.N, self.key = dt, dim, M, N, key
        make = {"plain": inv_draws, "singular": near_singular, "zero-diag": lambda *a: inv_draws(*a, zero_diag=True)}[recipe]
        self.Q, self.R, self.Rt, self.b, self.z, self.y, self.g, self.lb = make(seed(*key), dim, M, N, dt)
        self.ref = RefInv(self.Q, self.R, self.Rt, self.b, self.y, self.g, self.lb)
