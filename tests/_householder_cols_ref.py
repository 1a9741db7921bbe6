"""Float64 reference of the amortised Householder flow (include/bjx_householder_cols.h): the closed forms in numpy over all columns
at once.  Inputs are rounded to the tested dtype first, so the reference and the kernel start from the same numbers.
tests/test_host_householder_cols.py holds this module to an independent evaluation (dense matrices, slogdet, central differences).

Per column:  u = exp(s)⊙x;  z_{k+1} = z_k − t_k (v_kᵀz_k) v_k, t_k = 2/v_kᵀv_k (0 where v_kᵀv_k == 0);  y = z_L + m;  ladj = Σ s.
The inverse is x = exp(−s)⊙H_0⋯H_{L−1}(y − m) with the log-det −Σ s.  One reverse step at the layer's input z_k with the cotangent g
of its output:  a = vᵀz_k, c = vᵀg,  v̄ = −t(a g + c z_k − t a c v),  g ← g − t c v.
Shapes: v (dim, L, N); s, m (dim, N) or None; x, ȳ (dim, N); ℓ̄ (N,).

Draws: v ~ N(0, 1), log_scale ~ 0.5·N(0, 1), shift, z, ȳ, ℓ̄ ~ N(0, 1); seeded per case by zlib.crc32 of the case's key (the siblings'
`seed`).  Column 0 of every draw has v[:, 0, 0] == 0 exactly: a degenerate first layer."""
import numpy as np

from _radial_cols_ref import rounded, seed  # noqa: F401  (re-exported: the siblings' seeding)

HEADS = ("none", "scale", "shift", "both")


def draws(rng, dim, L, N, dt, head="both"):
    """-> v, s, m, z, ȳ, ℓ̄ rounded to `dt`, as float64 arrays (s and / or m None as `head` says); v[:, 0, 0] == 0."""
    assert head in HEADS
    v = rounded(rng.normal(size=(dim, L, N)), dt)
    s = rounded(0.5 * rng.normal(size=(dim, N)), dt)
    m = rounded(rng.normal(size=(dim, N)), dt)
    z = rounded(rng.normal(size=(dim, N)), dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    v[:, 0, 0] = 0.0
    return v, (s if head in ("scale", "both") else None), (m if head in ("shift", "both") else None), z, g, lb


def _tau(vk):
    ss = (vk * vk).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ss == 0, 0.0, 2.0 / ss)


def _reflect(vk, z):
    return z - _tau(vk) * (vk * z).sum(axis=0) * vk


def _amax(a):
    return np.abs(a).max(axis=0)


class RefAll:
    """Everything one direction of the flow returns: out (dim, N), ladj (N,), in_bar (dim, N), vb (dim, L, N), sb, mb (dim, N) or None,
    and `scale` (N,): the per-column TERM scale of the parameter cotangents — the largest of |t|(|a|‖g‖∞ + |c|‖z_k‖∞ + |t a c|‖v_k‖∞)
    over the layers, of |ū⊙u| + |ℓ̄|, and of the reference cotangents themselves (at dim 1 every H is −1 and v̄ is analytically 0; at
    dim 2 the three terms nearly cancel: the rounding of v̄ lives on the scale of its terms, not of their sum)."""

    def __init__(self, v, s, m, x, g, lb, inverse=False):
        dim, L, N = v.shape
        lb = np.zeros(N) if lb is None else lb
        es = np.ones((dim, N)) if s is None else np.exp(s)
        self.vb = np.empty((dim, L, N))
        scale = np.zeros(N)
        if not inverse:
            u = es * x
            states, cur = [None] * L, u
            for k in range(L):
                states[k] = cur
                cur = _reflect(v[:, k], cur)
            self.out = cur if m is None else cur + m
            self.ladj = np.zeros(N) if s is None else s.sum(axis=0)
            self.mb = None if m is None else g.copy()
            order = range(L - 1, -1, -1)
        else:
            cur = x if m is None else x - m
            states = [None] * L
            for k in range(L - 1, -1, -1):
                states[k] = cur                                      # the input of H_k in the inverse's order
                cur = _reflect(v[:, k], cur)
            q = cur
            self.out = q / es
            self.ladj = np.zeros(N) if s is None else -s.sum(axis=0)
            if s is None:
                self.sb = None
            else:
                self.sb = -self.out * g - lb
                scale = np.maximum(scale, _amax(self.out * g) + np.abs(lb))
            g = g / es
            order = range(L)
        for k in order:
            vk, zk = v[:, k], states[k]
            t = _tau(vk)
            a, c = (vk * zk).sum(axis=0), (vk * g).sum(axis=0)
            self.vb[:, k] = -t * (a * g + c * zk - t * a * c * vk)
            scale = np.maximum(scale, np.abs(t) * (np.abs(a) * _amax(g) + np.abs(c) * _amax(zk) + np.abs(t * a * c) * _amax(vk)))
            g = g - t * c * vk
        if not inverse:
            if s is None:
                self.sb = None
            else:
                self.sb = g * u + lb
                scale = np.maximum(scale, _amax(g * u) + np.abs(lb))
            self.in_bar = g * es
        else:
            self.in_bar = g
            self.mb = None if m is None else -g
        for c_ in (self.vb.reshape(-1, N), self.sb, self.mb):
            if c_ is not None:
                scale = np.maximum(scale, _amax(c_))
        self.scale = scale
