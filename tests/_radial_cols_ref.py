"""Float64 reference of the amortised radial flow (include/bjx_radial_cols.h): the CPU oracle applied COLUMN BY COLUMN and layer by
layer, as tests/_radial_params_ref.py composes a run — `orc.radial` for the layer inputs, `orc.radial_vjp(…, inverse=…)` to carry the
cotangent, `orc.radial_param_vjp` with N = 1 for the parameters (with one column its batch sums are that column's cotangents; in the
forward direction the carried cotangent is read off its z̄₀ = ȳ − radial_vjp(…), which saves calling radial_vjp twice per layer and is
held to the direct call at 1e-14 in tests/test_host_radial_cols.py).
The inverse is the implicit-function rule: per layer the pre-image, ḡ′ = radial_vjp(inverse=True), then radial_param_vjp(pre-image, −ḡ′, −ℓ̄).
Inputs are rounded to the tested dtype first, so the oracle and the kernel start from the same numbers.
Shapes: α_, β (L, N); z₀ (dim, L, N); x, ȳ (dim, N); ℓ̄ (N,).

Draws (those of tests/test_gpu_radial_stack.py, made per column): α_ ~ 0.5·N(0, 1), β ~ N(0, 1), z₀ ~ 0.3·N(0, 1); z, ȳ, ℓ̄ ~ N(0, 1);
seeded per case by zlib.crc32 of the case's key.  Column 0 of every draw has z == z₀ of layer 0 exactly (r = 0 at the first layer
of the forward flow: 1/r is read as 0 there)."""
import zlib

import numpy as np


def seed(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rounded(a, dt):
    return np.asarray(a, dt).astype(np.float64)


def draws(rng, dim, L, N, dt):
    """-> α_, β, z₀, z, ȳ, ℓ̄ rounded to `dt`, as float64 arrays; z[:, 0] == z₀[:, 0, 0]."""
    al = rounded(0.5 * rng.normal(size=(L, N)), dt)
    be = rounded(rng.normal(size=(L, N)), dt)
    z0 = rounded(0.3 * rng.normal(size=(dim, L, N)), dt)
    z = rounded(rng.normal(size=(dim, N)), dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    z[:, 0] = z0[:, 0, 0]
    return al, be, z0, z, g, lb


def _column(orc, al, be, z0, x, g, lb, inverse):
    """One column (x, g: (dim, 1); lb: (1,)) -> (out, ladj, in_bar, ᾱ_ [L], β̄ [L], z̄₀ [dim, L])."""
    L = len(al)
    order = range(L - 1, -1, -1) if inverse else range(L)
    states, ladj = [], 0.0
    for k in order:
        states.append(x)
        x, l = orc.radial(al[k], be[k], z0[:, k], x, inverse)
        x = np.asfortranarray(x)
        ladj += float(l[0])
    out = x
    states.append(out)
    ab, bb, zb = np.zeros(L), np.zeros(L), np.zeros_like(z0)
    for i in range(L - 1, -1, -1):
        k = order[i]
        if not inverse:
            ab[k], bb[k], zb[:, k] = orc.radial_param_vjp(al[k], be[k], z0[:, k], states[i], g, lb)
            g = g - zb[:, k:k + 1]           # radial_param_vjp returns z̄₀ = ȳ − radial_vjp(…) of its one column: z̄ without a second radial_vjp call
        else:
            gin = orc.radial_vjp(al[k], be[k], z0[:, k], states[i], g, lb, inverse=True)
            ab[k], bb[k], zb[:, k] = orc.radial_param_vjp(al[k], be[k], z0[:, k], states[i + 1], -gin, -lb)   # states[i + 1]: the pre-image
            g = gin
    return out[:, 0], ladj, g[:, 0], ab, bb, zb


class RefAll:
    """Everything one direction of the flow returns, column by column: out (dim, N), ladj (N,), in_bar (dim, N), ab, bb (L, N),
    zb (dim, L, N)."""

    def __init__(self, orc, al, be, z0, x, g, lb, inverse=False):
        dim, N = x.shape
        L = al.shape[0]
        self.out, self.ladj, self.in_bar = np.empty((dim, N)), np.empty(N), np.empty((dim, N))
        self.ab, self.bb, self.zb = np.empty((L, N)), np.empty((L, N)), np.empty((dim, L, N))
        for n in range(N):
            r = _column(orc, np.ascontiguousarray(al[:, n]), np.ascontiguousarray(be[:, n]), np.ascontiguousarray(z0[:, :, n]),
                        np.asfortranarray(x[:, n:n + 1]), np.asfortranarray(g[:, n:n + 1]), np.zeros(1) if lb is None else lb[n:n + 1], inverse)
            self.out[:, n], self.ladj[n], self.in_bar[:, n], self.ab[:, n], self.bb[:, n], self.zb[:, :, n] = r
        self.scale = joint_scale(self.ab, self.bb, self.zb)


def joint_scale(ab, bb, zb):
    """Per column: the largest entry of the three parameter cotangents together (a single ᾱ_ near zero has no scale of its own)."""
    N = ab.shape[-1]
    return np.abs(np.concatenate([ab.reshape(-1, N), bb.reshape(-1, N), zb.reshape(-1, N)])).max(axis=0)


# ------------------------------------------------------------------ the same closed forms over all columns at once
def _sp(v):
    return np.logaddexp(0.0, v)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _layer_forms(al, be, z0, z):
    """δ, r and the scalars of one layer at its forward input z, every column at once (oracle.radial_vjp's docstring)."""
    d = z.shape[0]
    a_hat = _sp(al)
    bh = _sp(be) - a_hat
    dl = z - z0
    r = np.sqrt((dl * dl).sum(axis=0))
    h = 1.0 / (a_hat + r)
    a = 1.0 + bh * h
    with np.errstate(divide="ignore", invalid="ignore"):
        rinv = np.where(r > 0, 1.0 / r, 0.0)
    c = -bh * h * h * rinv
    D = a - bh * h * h * r
    lr = (d - 1) * (-bh * h * h) / a + (-2.0 * bh * h * h + 2.0 * bh * h ** 3 * r) / D
    return d, a_hat, bh, dl, r, h, a, rinv, c, D, lr


def _forward_pullback(al, be, z0, z, s, lbs):
    """(z̄, ᾱ_, β̄, z̄₀) of one forward layer at z with the output cotangent s and the log-det cotangent lbs."""
    d, a_hat, bh, dl, r, h, a, rinv, c, D, lr = _layer_forms(al, be, z0, z)
    dg = (dl * s).sum(axis=0)
    zin = a * s + c * dg * dl + lbs * lr * rinv * dl
    gb = h * dg + lbs * ((d - 1) * h / a + (h - h * h * r) / D)
    ga = -h * h * (bh * dg + lbs * ((d - 1) * bh / a + (bh - 2.0 * bh * h * r) / D))
    return zin, _sig(al) * (ga - gb), _sig(be) * gb, s - zin


class VecAll:
    """RefAll's fields from a numpy restatement over all columns at once — NOT a reference of its own: whoever uses it holds it to
    RefAll on some columns first (the grid-stride test: the first 64)."""

    def __init__(self, al, be, z0, x, g, lb, inverse=False):
        dim, N = x.shape
        L = al.shape[0]
        lb = np.zeros(N) if lb is None else lb
        self.ab, self.bb, self.zb = np.empty((L, N)), np.empty((L, N)), np.empty((dim, L, N))
        ladj, cur, states = np.zeros(N), x, [None] * L
        if not inverse:
            for k in range(L):
                d, a_hat, bh, dl, r, h, a, rinv, c, D, lr = _layer_forms(al[k], be[k], z0[:, k], cur)
                states[k] = cur
                ladj = ladj + (d - 1) * np.log(a) + np.log(D)
                cur = cur + bh * h * dl
            self.out = cur
            for k in range(L - 1, -1, -1):
                g, self.ab[k], self.bb[k], self.zb[:, k] = _forward_pullback(al[k], be[k], z0[:, k], states[k], g, lb)
        else:
            for k in range(L - 1, -1, -1):
                a_hat, apb = _sp(al[k]), _sp(be[k])
                dl = cur - z0[:, k]
                gam = np.sqrt((dl * dl).sum(axis=0))                 # compute_r, radial_layer.jl:124-129
                aa = apb - gam
                r = (np.sqrt(aa * aa + 4.0 * a_hat * gam) - aa) / 2.0
                cur = z0[:, k] + (a_hat + r) / (apb + r) * dl
                states[k] = cur                                      # the pre-image: the forward input of layer k
                d, _, bh, _, r, h, a, _, _, D, _ = _layer_forms(al[k], be[k], z0[:, k], cur)
                ladj = ladj - ((d - 1) * np.log(a) + np.log(D))
            self.out = cur
            for k in range(L):
                d, a_hat, bh, dl, r, h, a, rinv, c, D, lr = _layer_forms(al[k], be[k], z0[:, k], states[k])
                v = g - lb * lr * rinv * dl
                yb = (v - c * (dl * v).sum(axis=0) * dl / (a + c * r * r)) / a
                _, self.ab[k], self.bb[k], self.zb[:, k] = _forward_pullback(al[k], be[k], z0[:, k], states[k], -yb, -lb)
                g = yb
        self.ladj, self.in_bar = ladj, g
        self.scale = joint_scale(self.ab, self.bb, self.zb)
