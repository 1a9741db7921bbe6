"""Float64 reference of the shared Householder layer (include/bjx_householder.h, `HouseholderLayer`): the closed forms in numpy over
all columns at once.  Inputs are rounded to the tested dtype first, so the reference and the kernel start from the same numbers.
tests/test_host_householder.py holds this module to an independent evaluation (dense matrices, slogdet, central differences) and to
the per-column sibling's reference (tests/_householder_cols_ref.py) on expanded parameters.

With V = [v_0 … v_{L−1}] (dim, L) shared by all columns:  t_k = 2/v_kᵀv_k (0 where v_kᵀv_k == 0);  z_0 = x, z_{k+1} = z_k − t_k(v_kᵀz_k)v_k,
y = z_L; the inverse walks k = L−1 … 0 with the same step; logabsdetjac = 0.  The input pullback of one direction is the other
direction's map of ȳ.  One reverse step at the step's input z_k with the cotangent g of its output, a_n = v_kᵀz_{k,n}, c_n = v_kᵀg_n:
    S_k = Σ_n (a_n g_n + c_n z_{k,n}),   q_k = Σ_n a_n c_n,   v̄_k = −t_k S_k + t_k² q_k v_k,   g ← g − t_k c v_k.

The summands are kept next to the sums: `s_terms` (dim, L, N) = a_n g_n + c_n z_{k,n}, `q_terms` (L, N) = a_n c_n and `vb_cols`
(dim, L, N) = −t s_terms + t² q_terms v_k, the per-column contribution to v̄_k; `summed(n)` adds them over the first n columns only (one
draw serves every batch size of a test).  `term_scale` (L,) is the max-norm over rows and columns
of the summand of v̄_k taken part by part, |t_k||s_terms| + t_k²|q_terms||v_k|: what a sum over the batch rounds on is the size of the
terms it adds, and the two parts cancel (exactly at dim 1, where every H is −1 and v̄ is analytically 0; nearly at dim 2), so the
contribution's own norm would be a scale the sums S_k and q_k never see.

Draws: V, x, ȳ ~ N(0, 1), seeded per case by the siblings' `seed`."""
import numpy as np

from _householder_cols_ref import _reflect, _tau
from _radial_cols_ref import rounded, seed  # noqa: F401  (re-exported: the siblings' seeding)


def draws(rng, dim, L, N, dt):
    """-> V (dim, L), x (dim, N), ȳ (dim, N) rounded to `dt`, as float64 arrays."""
    V = rounded(rng.normal(size=(dim, L)), dt)
    x = rounded(rng.normal(size=(dim, N)), dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    return V, x, g


def apply(V, x, inverse=False):
    """The map (or its inverse) alone: (dim, N) -> (dim, N)."""
    L = V.shape[1]
    cur = x
    for k in (range(L - 1, -1, -1) if inverse else range(L)):
        cur = _reflect(V[:, k:k + 1], cur)
    return cur


class RefShared:
    """Everything one direction returns: out (dim, N), ladj (N,) zeros, in_bar (dim, N), vb (dim, L) and the summands described in the
    module docstring."""

    def __init__(self, V, x, g, inverse=False):
        dim, L = V.shape
        N = x.shape[1]
        order = list(range(L - 1, -1, -1) if inverse else range(L))
        states, cur = {}, x
        for k in order:
            states[k] = cur                                          # the input of step k in this direction's order
            cur = _reflect(V[:, k:k + 1], cur)
        self.out = cur
        self.ladj = np.zeros(N)
        self.s_terms = np.zeros((dim, L, N))
        self.q_terms = np.zeros((L, N))
        self.vb_cols = np.zeros((dim, L, N))
        self.vb = np.zeros((dim, L))
        self.term_scale = np.zeros(L)
        self.term_cols = np.zeros((L, N))                            # the max over the rows of the parts of column n's summand of v̄_k
        self.V, self.t = V, np.zeros(L)
        for k in reversed(order):
            vk, zk = V[:, k:k + 1], states[k]
            t = float(_tau(vk)[0])
            a, c = (vk * zk).sum(axis=0), (vk * g).sum(axis=0)
            self.s_terms[:, k] = a * g + c * zk
            self.q_terms[k] = a * c
            self.vb_cols[:, k] = -t * self.s_terms[:, k] + t * t * self.q_terms[k] * vk
            self.vb[:, k] = -t * self.s_terms[:, k].sum(axis=1) + t * t * self.q_terms[k].sum() * vk[:, 0]
            self.t[k] = t
            self.term_cols[k] = (abs(t) * np.abs(self.s_terms[:, k]) + t * t * np.abs(self.q_terms[k]) * np.abs(vk)).max(axis=0)
            if N:
                self.term_scale[k] = self.term_cols[k].max()
            g = g - t * c * vk
        self.in_bar = g

    def summed(self, n):
        """-> (v̄ (dim, L), term_scale (L,)) of the FIRST n columns alone: the same summands, added over fewer columns."""
        t = self.t
        vb = -t * self.s_terms[:, :, :n].sum(axis=2) + t * t * self.q_terms[:, :n].sum(axis=1) * self.V
        return vb, (self.term_cols[:, :n].max(axis=1) if n else np.zeros(len(t)))
