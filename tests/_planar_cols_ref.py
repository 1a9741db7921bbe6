"""Float64 reference of the amortised planar flow (include/bjx_planar_cols.h): the CPU oracle applied COLUMN BY COLUMN — `orc.planar`
for the maps, `orc.planar_vjp` / `orc.planar_inv_vjp` / `orc.planar_param_vjp` with N = 1 for the pullbacks (with one column the
batch sums of `planar_param_vjp` are that column's cotangents).  Inputs are rounded to the tested dtype first, so the oracle and
the kernel start from the same numbers.  Shapes: w, u (dim, L, N); b (L, N); x, ȳ (dim, N); ℓ̄ (N,).

Draws: w, u ~ 0.8·dim^(−1/4)·N(0, 1), so wᵀu has a standard deviation of about 0.64 at every dim; b, z, ȳ, ℓ̄ ~ N(0, 1); seeded per
case by zlib.crc32 of the case's key."""
import zlib

import numpy as np


def seed(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rounded(a, dt):
    return np.asarray(a, dt).astype(np.float64)


def draws(rng, dim, L, N, dt):
    """-> w, u, b, z, ȳ, ℓ̄ rounded to `dt`, as float64 arrays."""
    s = 0.8 * dim ** -0.25
    w = rounded(s * rng.normal(size=(dim, L, N)), dt)
    u = rounded(s * rng.normal(size=(dim, L, N)), dt)
    b = rounded(rng.normal(size=(L, N)), dt)
    z = rounded(rng.normal(size=(dim, N)), dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    return w, u, b, z, g, lb


def _col(a, n):
    return np.asfortranarray(a[:, n:n + 1])


def ref_map(orc, w, u, b, x, inverse=False):
    """-> (out (dim, N), per-column log-det (N,)); the inverse undoes layer L−1 first."""
    dim, N = x.shape
    out, ladj = np.empty((dim, N)), np.empty(N)
    for n in range(N):
        o, l = orc.planar(w[:, :, n], u[:, :, n], b[:, n], _col(x, n), inverse=inverse)
        out[:, n], ladj[n] = np.asarray(o)[:, 0], np.asarray(l)[0]
    return out, ladj


def ref_vjp(orc, w, u, b, x, g, lb=None, inverse=False):
    """Input pullback at x (forward) or y (inverse: the implicit-function rule)."""
    dim, N = x.shape
    fn = orc.planar_inv_vjp if inverse else orc.planar_vjp
    out = np.empty((dim, N))
    for n in range(N):
        out[:, n] = fn(w[:, :, n], u[:, :, n], b[:, n], _col(x, n), _col(g, n), None if lb is None else lb[n:n + 1])[:, 0]
    return out


def ref_param_vjp(orc, w, u, b, x, g, lb=None):
    """Per-column (w̄ (dim, L, N), ū (dim, L, N), b̄ (L, N)) of the forward flow."""
    dim, L, N = w.shape
    wb, ub, bb = np.empty((dim, L, N)), np.empty((dim, L, N)), np.empty((L, N))
    for n in range(N):
        wb[:, :, n], ub[:, :, n], bb[:, n] = orc.planar_param_vjp(w[:, :, n], u[:, :, n], b[:, n], _col(x, n), _col(g, n), None if lb is None else lb[n:n + 1])
    return wb, ub, bb


def ref_inverse_param_vjp(orc, w, u, b, y, xbar, lb=None):
    """inverse(flow): ȳ by the implicit-function rule, then the forward parameter pullback at x = f⁻¹(y) with (−ȳ, −ℓ̄).
    -> (ȳ, w̄, ū, b̄)."""
    x, _ = ref_map(orc, w, u, b, y, inverse=True)
    yb = ref_vjp(orc, w, u, b, y, xbar, lb, inverse=True)
    return (yb,) + ref_param_vjp(orc, w, u, b, x, -yb, None if lb is None else -lb)


def trajectory_scale(w, u, b, x, y):
    """Per column: the largest entry of any state z_0 = x, z_1, ..., z_L = f(x) of the forward flow.  x = f(x) − Σ_k û_k t_k is a sum that
    can cancel (a layer with a tiny ‖w‖ has û ~ 1/‖w‖): whoever evaluates the round trip in `dt` rounds at the size of these terms.
    A scale, not a reference: the layers are written out in numpy over all columns at once (û = u + (log1pexp(−wᵀu) − 1)·w/‖w‖²), and
    the last state is held to `y`, the oracle's f(x), at 1e-12."""
    cur, top = x, np.abs(x).max(axis=0)
    for k in range(w.shape[1]):
        wk, uk = w[:, k, :], u[:, k, :]
        u_hat = uk + (np.logaddexp(0.0, -(wk * uk).sum(axis=0)) - 1.0) / (wk * wk).sum(axis=0) * wk
        cur = cur + u_hat * np.tanh((wk * cur).sum(axis=0) + b[k])
        top = np.maximum(top, np.abs(cur).max(axis=0))
    assert np.abs(cur - y).max() <= 1e-12 * max(1.0, np.abs(top).max()), "trajectory_scale's layers disagree with the oracle"
    return top


def joint_scale(wb, ub, bb):
    """Per column: the largest entry of the three parameter cotangents together (a single b̄ near zero has no scale of its own)."""
    N = bb.shape[-1]
    return np.abs(np.concatenate([wb.reshape(-1, N), ub.reshape(-1, N), bb.reshape(-1, N)])).max(axis=0)


def inverse_amp(orc, amp, w, u, b, x, dt):
    """tests/_tol.planar_inverse_amp (`amp`) column by column at the pre-images x -> (N,)."""
    return np.array([amp(orc, w[:, :, n], u[:, :, n], b[:, n], _col(x, n), dt)[0] for n in range(x.shape[1])])
