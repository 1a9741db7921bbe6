"""Float64 reference for the value and gradients of the log-density of transformed(N(μ, diag σ²), l_L ∘ … ∘ l_1) with PlanarLayers
(include/bjx_planar_logpdf.h, `logpdf_vjp_params`), shared by the CPU and the GPU tests.

With x = f⁻¹(y), w = (x − μ)/σ, ℓ = logabsdetjac(inverse(f), y) per column and the cotangent c of lp:
    lp = −½‖w‖² − Σ log σ − (d/2) log 2π + ℓ;   x̄ = −c·w/σ, ℓ̄ = c;   μ̄ = Σ c·w/σ;   σ̄ = Σ c·(w² − 1)/σ
The oracle's inverse map, layer by layer, gives x and ℓ; `orc.planar_inv_vjp` on (x̄, c) gives ȳ; and — the implicit function theorem on
the whole stack — `orc.planar_param_vjp` at x with the cotangents (−ȳ, −c) gives (w̄, ū, b̄).  tests/test_host_planar_logpdf_grad.py pins
all of it against central differences of Σ c·lp taken through the oracle's maps alone."""
import math

import numpy as np


def inverse_run(orc, w, u, b, Y):
    """(x, ℓ) of inverse(l_L ∘ … ∘ l_1) at Y through the oracle's single-layer inverse, Float64.  w, u: (dim, L); b: (L,)."""
    x = np.asfortranarray(np.asarray(Y, np.float64))
    ell = np.zeros(x.shape[1])
    for k in range(w.shape[1] - 1, -1, -1):
        x, l = orc.planar(np.ascontiguousarray(w[:, k]), np.ascontiguousarray(u[:, k]), b[k:k + 1], x, inverse=True)
        x = np.asfortranarray(np.asarray(x, np.float64))
        ell = ell + np.asarray(l, np.float64)
    return x, ell


def _base(mu, sigma, dim):
    mu = np.zeros(dim) if mu is None else np.asarray(mu, np.float64)
    sigma = np.ones(dim) if sigma is None else np.asarray(sigma, np.float64)
    return mu.reshape(-1, 1), sigma.reshape(-1, 1)


def _f64(w, u, b):
    w, u = np.asarray(w, np.float64), np.asarray(u, np.float64)
    return w.reshape(w.shape[0], -1), u.reshape(u.shape[0], -1), np.asarray(b, np.float64).reshape(-1)


def logpdf_values(orc, w, u, b, mu, sigma, Y):
    """lp per column through the oracle's maps alone (no derivative): what the central differences are taken of."""
    w, u, b = _f64(w, u, b)
    x, ell = inverse_run(orc, w, u, b, Y)
    dim = x.shape[0]
    m, s = _base(mu, sigma, dim)
    ww = (x - m) / s
    return -0.5 * (ww * ww).sum(axis=0) - np.log(s).sum() - 0.5 * dim * math.log(2.0 * math.pi) + ell


def objective(orc, w, u, b, mu, sigma, Y, c):
    return float((np.asarray(c, np.float64) * logpdf_values(orc, w, u, b, mu, sigma, Y)).sum())


def ref_planar_logpdf_grad(orc, w, u, b, mu, sigma, Y, c):
    """-> dict(lp, y_bar, w_bar [dim, L], u_bar [dim, L], b_bar [L], mu_bar, sigma_bar, t_mu, t_sigma (max-norms of the summands), x, x_bar);
    c: (batch,) or None (= 1)."""
    w, u, b = _f64(w, u, b)
    x, ell = inverse_run(orc, w, u, b, Y)
    dim, N = x.shape
    c = np.ones(N) if c is None else np.asarray(c, np.float64)
    m, s = _base(mu, sigma, dim)
    ww = (x - m) / s
    lp = -0.5 * (ww * ww).sum(axis=0) - np.log(s).sum() - 0.5 * dim * math.log(2.0 * math.pi) + ell
    xbar = np.asfortranarray(-c * ww / s)
    yb = orc.planar_inv_vjp(w, u, b, np.asfortranarray(np.asarray(Y, np.float64)), xbar, c)
    wb, ub, bb = orc.planar_param_vjp(w, u, b, x, -yb, -c)
    mterm, sterm = c * ww / s, c * (ww * ww - 1.0) / s
    return dict(lp=lp, y_bar=yb, w_bar=wb.reshape(dim, -1), u_bar=ub.reshape(dim, -1), b_bar=bb.reshape(-1), mu_bar=mterm.sum(axis=1),
                sigma_bar=sterm.sum(axis=1), t_mu=float(np.abs(mterm).max()) if N else 0.0, t_sigma=float(np.abs(sterm).max()) if N else 0.0,
                x=x, x_bar=xbar)
