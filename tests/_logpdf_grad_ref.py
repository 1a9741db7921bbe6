"""Float64 reference for the value and gradients of the log-density of transformed(N(μ, diag σ²), l_L ∘ … ∘ l_1) with RadialLayers
(include/bjx_radial_stack_logpdf.h, `logpdf_vjp_params`), shared by the CPU and the GPU tests.

With x = f⁻¹(y), w = (x − μ)/σ, ℓ = logabsdetjac(inverse(f), y) per column and the cotangent c of lp:
    lp = −½‖w‖² − Σ log σ − (d/2) log 2π + ℓ;   x̄ = −c·w/σ, ℓ̄ = c;   μ̄ = Σ c·w/σ;   σ̄ = Σ c·(w² − 1)/σ
The oracle's inverse run, layer by layer, gives x and ℓ; `_radial_params_ref.ref_run_params(…, inverse=True)` on (x̄, c) gives ȳ and
the layers' cotangents with the max-norm of their summands."""
import math

import numpy as np

from _radial_params_ref import ref_run_params


def inverse_run(orc, al, be, z0, Y):
    """(x, ℓ) of inverse(l_L ∘ … ∘ l_1) at Y through the oracle's single-layer inverse, Float64."""
    x = np.asfortranarray(np.asarray(Y, np.float64))
    ell = np.zeros(x.shape[1])
    for k in range(len(al) - 1, -1, -1):
        x, l = orc.radial(np.float64(al[k]), np.float64(be[k]), np.ascontiguousarray(z0[:, k], dtype=np.float64), x, True)
        x = np.asfortranarray(x)
        ell = ell + l
    return x, ell


def _base(mu, sigma, dim):
    mu = np.zeros(dim) if mu is None else np.asarray(mu, np.float64)
    sigma = np.ones(dim) if sigma is None else np.asarray(sigma, np.float64)
    return mu.reshape(-1, 1), sigma.reshape(-1, 1)


def logpdf_values(orc, al, be, z0, mu, sigma, Y):
    """lp per column through the oracle's maps alone (no derivative): what the central differences are taken of."""
    x, ell = inverse_run(orc, al, be, z0, Y)
    dim = x.shape[0]
    m, s = _base(mu, sigma, dim)
    w = (x - m) / s
    return -0.5 * (w * w).sum(axis=0) - np.log(s).sum() - 0.5 * dim * math.log(2.0 * math.pi) + ell


def objective(orc, al, be, z0, mu, sigma, Y, c):
    return float((np.asarray(c, np.float64) * logpdf_values(orc, al, be, z0, mu, sigma, Y)).sum())


def ref_logpdf_grad(orc, al, be, z0, mu, sigma, Y, c):
    """-> dict(lp, y_bar, alpha_bar [L], beta_bar [L], z0_bar [dim, L], mu_bar, sigma_bar, terms = (ta, tb, tz per layer), t_mu, t_sigma,
    x, x_bar); c: (batch,) or None (= 1)."""
    al, be, z0 = np.asarray(al, np.float64), np.asarray(be, np.float64), np.asarray(z0, np.float64)
    x, ell = inverse_run(orc, al, be, z0, Y)
    dim, N = x.shape
    c = np.ones(N) if c is None else np.asarray(c, np.float64)
    m, s = _base(mu, sigma, dim)
    w = (x - m) / s
    lp = -0.5 * (w * w).sum(axis=0) - np.log(s).sum() - 0.5 * dim * math.log(2.0 * math.pi) + ell
    xbar = np.asfortranarray(-c * w / s)
    yb, ab, bb, zb, terms = ref_run_params(orc, al, be, z0, Y, xbar, c, inverse=True)
    mterm, sterm = c * w / s, c * (w * w - 1.0) / s
    return dict(lp=lp, y_bar=yb, alpha_bar=ab, beta_bar=bb, z0_bar=zb, mu_bar=mterm.sum(axis=1), sigma_bar=sterm.sum(axis=1), terms=terms,
                t_mu=float(np.abs(mterm).max()) if N else 0.0, t_sigma=float(np.abs(sterm).max()) if N else 0.0, x=x, x_bar=xbar)
