"""Reference for the parameter pullback of a run of RadialLayers (include/bjx_radial_stack_params.h), shared by the CPU and the GPU
tests: the oracle composed layer by layer in Float64.

Forward run: `oracle.radial` for the layer inputs, `oracle.radial_vjp` to carry ḡ from the last layer back, `oracle.radial_param_vjp`
per layer.  Inverse run: per layer the oracle's inverse for the pre-image, `radial_vjp(..., inverse=True)` for ḡ′, then
`radial_param_vjp(pre-image, −ḡ′, −ℓ̄)` (the implicit-function rule).  Next to the sums the max-norm of their SUMMANDS is returned
(`terms`: the only growth factor `flat_close` takes, for sums that cancel)."""
import numpy as np


def _sp(v):
    return np.logaddexp(0.0, v)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _summand_norms(al, be, z0, z, g, gin, lb):
    """max |summand| of (ᾱ_, β̄, z̄₀) of one forward layer at input z with output cotangent g and input cotangent gin."""
    d = z.shape[0]
    a_hat = _sp(al)
    bh = _sp(be) - a_hat
    dl = z - z0.reshape(-1, 1)
    r = np.sqrt((dl * dl).sum(axis=0))
    dg = (dl * g).sum(axis=0)
    h = 1.0 / (a_hat + r)
    a = 1.0 + bh * h
    D = a - bh * h * h * r
    gb = h * dg + lb * ((d - 1) * h / a + (h - h * h * r) / D)
    ga = -h * h * (bh * dg + lb * ((d - 1) * bh / a + (bh - 2.0 * bh * h * r) / D))
    return float(np.abs(_sig(al) * (ga - gb)).max()), float(np.abs(_sig(be) * gb).max()), float(np.abs(g - gin).max())


def ref_run_params(orc, al, be, z0, X, G, lbar, inverse=False):
    """-> (x_bar, alpha_bar [L], beta_bar [L], z0_bar [dim, L], terms) in Float64; terms = (max |summand|) per output, each [L]."""
    al, be, z0 = np.asarray(al, np.float64), np.asarray(be, np.float64), np.asarray(z0, np.float64)
    nl = len(al)
    x = np.asfortranarray(np.asarray(X, np.float64))
    N = x.shape[1]
    lb = np.zeros(N) if lbar is None else np.asarray(lbar, np.float64)
    order = list(range(nl - 1, -1, -1) if inverse else range(nl))
    inputs = []
    for k in order:
        inputs.append(x)
        x = np.asfortranarray(orc.radial(al[k], be[k], z0[:, k], x, inverse)[0])
    g = np.asarray(G, np.float64)
    ab, bb, zb = np.zeros(nl), np.zeros(nl), np.zeros_like(z0)
    ta, tb, tz = np.zeros(nl), np.zeros(nl), np.zeros(nl)
    for k, xin in zip(reversed(order), reversed(inputs)):
        z0k = np.ascontiguousarray(z0[:, k])
        if not inverse:
            ab[k], bb[k], zb[:, k] = orc.radial_param_vjp(al[k], be[k], z0k, xin, g, lb)
            gin = orc.radial_vjp(al[k], be[k], z0k, xin, g, lb)
            ta[k], tb[k], tz[k] = _summand_norms(al[k], be[k], z0k, xin, g, gin, lb)
        else:
            pre = np.asfortranarray(orc.radial(al[k], be[k], z0k, xin, True)[0])
            gin = orc.radial_vjp(al[k], be[k], z0k, xin, g, lb, inverse=True)
            ab[k], bb[k], zb[:, k] = orc.radial_param_vjp(al[k], be[k], z0k, pre, -gin, -lb)
            ta[k], tb[k], tz[k] = _summand_norms(al[k], be[k], z0k, pre, -gin, -g, -lb)
        g = gin
    return g, ab, bb, zb, (ta, tb, tz)


def run_objective(orc, al, be, z0, X, G, lbar, inverse=False):
    """Σ ȳ·y(θ) + Σ ℓ̄·ladj(θ) of the run through the oracle's maps alone (no closed-form derivative): what a central difference in
    one parameter is taken of."""
    x = np.asfortranarray(np.asarray(X, np.float64))
    nl = len(al)
    ladj = np.zeros(x.shape[1])
    for k in (range(nl - 1, -1, -1) if inverse else range(nl)):
        x, l = orc.radial(np.float64(al[k]), np.float64(be[k]), np.ascontiguousarray(z0[:, k], dtype=np.float64), x, inverse)
        x = np.asfortranarray(x)
        ladj = ladj + l
    return float((np.asarray(G, np.float64) * x).sum() + (0.0 if lbar is None else (np.asarray(lbar, np.float64) * ladj).sum()))
