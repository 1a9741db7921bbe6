"""The amortised Sylvester layer (`AmortizedSylvesterLayer`, include/bjx_sylvester_cols.h) against the Float64 closed forms of
tests/_sylvester_cols_ref.py (held to the finite-difference Jacobian's slogdet and central differences in
tests/test_host_sylvester_cols.py), on tests/_tol.py's flat bar (1e-3 Float32 / 1e-6 Float64), no conditioned bar anywhere: values and
x̄ per="sample" (with floor=1.0 at dim 1: a column of one entry has no scale of its own; the inputs are unit-scale draws), log-dets
per="element" with a floor of 1, q̄ / r̄ / r̃̄ / b̄ on the column's TERM scale (`RefAll.scale`).  No column is left out of any comparison;
column 0 of every draw has R = 0 (the identity) and column 1 has R_00·R̃_00 = −3 with d_0 < 0.

Dispatcher edges by dim (V = 4 / 2 elements per 16-byte pack in Float32 / Float64, G lanes per column, R packs per lane) are the
siblings' (tests/test_gpu_householder_cols.py): 1, 2, 3, 5 element form; 4, 8, 16, 64 vector form; 65 partial last pack; 260 / 256
R = 2; 261 / 257, 516, 765 / 384 the R = 4 kernels with dead or partial packs; 1 024 / 512 the limits.  At every dim M = 1, 3, 16 where
M <= dim; at dims 8, 64, 65 and the limit also M = 2, 4, 5, 8, 9: every padded instantiation (1, 2, 4, 8, 16) both full and with dead
units.  Every case runs the batches 1, C − 1, C, C + 1 with C = 256/G columns per block.

The GPU suite is kept near 5 000 test ids, so the cases are THREE ids here: the parts below are plain functions called in turn (every
failure names its part in the traceback and its dtype, dim, M and batch in the message)."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _householder_cols_ref import RefAll as HouseholderRefAll  # noqa: E402
from _householder_cols_ref import draws as householder_draws  # noqa: E402
from _sylvester_cols_ref import RefAll, draws, seed  # noqa: E402
from _tol import flat_close  # noqa: E402

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
DIMS = {F32: [1, 2, 3, 5, 4, 8, 16, 64, 65, 260, 261, 516, 765, 1024], F64: [1, 2, 3, 5, 4, 8, 16, 64, 65, 256, 257, 384, 512]}
NAMES = ("q", "r", "r_tilde", "b")


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def lanes(dim, dt):
    packs = -(-dim // (16 // np.dtype(dt).itemsize))
    G = 1
    while G < 64 and G < packs:
        G *= 2
    return G


def units(dim, dt):
    ms = {1, 3, 16}
    if dim in (8, 64, 65, DIMS[dt][-1]):
        ms |= {2, 4, 5, 8, 9}
    return sorted(m for m in ms if m <= dim)


def dev3(a, dt):
    """(A, B, N) numpy -> cuda tensor laid out column-major per column (a permute(2, 1, 0) view of a (N, B, A) array)."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 1, 0))).astype(dt)).cuda().permute(2, 1, 0)


def dev2(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def close_cols(got, ref, dt, what):
    """Values and input cotangents (dim, n): per sample; a column of ONE entry on a floor of 1."""
    return flat_close(got, ref, dt, what, per="sample", floor=1.0 if ref.shape[0] == 1 else 0.0)


class Ref:
    """Every reference quantity of one parameter draw, computed once; the tests slice its first n columns."""

    def __init__(self, dt, dim, M, N, key):
        self.dt, self.dim, self.M, self.N = dt, dim, M, N
        self.Q, self.R, self.Rt, self.b, self.z, self.g, self.lb = self.np = draws(seed(*key), dim, M, N, dt)
        self.F = RefAll(*self.np)

    def layer(self, bj, n=None, R=None, b=None):
        n, dt = self.N if n is None else n, self.dt
        return bj.AmortizedSylvesterLayer(dev3(self.Q[..., :n], dt), dev3((self.R if R is None else R)[..., :n], dt), dev3(self.Rt[..., :n], dt),
                                          dev2((self.b if b is None else b)[..., :n], dt))

    def data(self, n=None):
        n = self.N if n is None else n
        return dev2(self.z[:, :n], self.dt), dev2(self.g[:, :n], self.dt), dev1(self.lb[:n], self.dt)


def check_params(grads, F, n, dt, what, scale=None):
    assert set(grads) == set(NAMES), (what, sorted(grads))
    for k, r in zip(NAMES, (F.qb, F.rb, F.rtb, F.bb)):
        got = host(grads[k])
        assert got.shape == r[..., :n].shape, (what, k, got.shape)
        flat_close(got.reshape(-1, n), r[..., :n].reshape(-1, n), dt, f"{what} {k} cotangent", term_scale=(F.scale if scale is None else scale)[:n])
    low = np.tril(np.ones(F.rb.shape[:2]), -1) > 0
    assert not host(grads["r"])[low].any() and not host(grads["r_tilde"])[low].any(), what + ": the strict lower triangles are not exact zeros"


def check_all(bj, R, n, what):
    """The map and the pullbacks of the first n columns of the draw R."""
    dt = R.dt
    layer = R.layer(bj, n)
    zd, gd, lbd = R.data(n)
    y, l = bj.with_logabsdet_jacobian(layer, zd, per_sample=True)
    close_cols(host(y), R.F.out[:, :n], dt, what + " values")
    flat_close(host(l), R.F.ladj[:n], dt, what + " ladj", per="element", floor=1.0)
    assert torch.equal(y[:, 0], zd[:, 0]) and float(l[0]) == 0.0, what + ": column 0 (R = 0) is not the identity with log-det 0"
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    close_cols(host(xb), R.F.in_bar[:, :n], dt, what + " input cotangent")
    assert torch.equal(bj.vjp(layer, zd, gd, lbd), xb), what + ": vjp and vjp_params disagree on the input cotangent"
    check_params(grads, R.F, n, dt, what)


def batches(C, more=()):
    return sorted({n for n in (1, C - 1, C, C + 1) + tuple(more) if n >= 1})


def maps_and_pullbacks_match_reference(bj, dt):
    for dim in DIMS[dt]:
        C = 256 // lanes(dim, dt)
        ns = batches(C)
        for M in units(dim, dt):
            R = Ref(dt, dim, M, max(ns), ("cols", np.dtype(dt).name, dim, M))
            if max(ns) >= 2:
                assert R.F.d[0, 1] < 0
            for n in ns:
                check_all(bj, R, n, f"sylvester_cols {np.dtype(dt).name} dim={dim} M={M} batch={n}")


# ------------------------------------------------------------------ layouts
def _outputs(bj, layer, zd, gd, lbd):
    y, l = bj.with_logabsdet_jacobian(layer, zd, per_sample=True)
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    return [y, l, xb] + [grads[k] for k in NAMES]


def parameter_layouts_give_the_same_bits(bj):
    """The permuted network outputs (no copy), contiguous (dim, M, batch) tensors (copied once) and the four slices of one head
    [dim·M + 2M² + M + pad, batch] (no copy; pad = 0 … 3 so that the column stride is and is not a multiple of the pack: vector and
    element form): every output bit for bit the dense call's."""
    for dt, dim, M, N in ((F32, 64, 5, 37), (F64, 64, 5, 37), (F32, 65, 3, 21), (F64, 8, 8, 130), (F32, 260, 16, 9)):
        R = Ref(dt, dim, M, N, ("layout", np.dtype(dt).name, dim, M))
        what = f"sylvester_cols layouts {np.dtype(dt).name} dim={dim} M={M} batch={N}"
        zd, gd, lbd = R.data()
        dense = R.layer(bj)
        want = _outputs(bj, dense, zd, gd, lbd)
        close_cols(host(want[0]), R.F.out, dt, what + " values")
        cont = bj.AmortizedSylvesterLayer(*(t.contiguous() for t in (dense.q, dense.r, dense.r_tilde, dense.b)))
        assert cont._col_params(zd, dim, N)[0].data_ptr() != cont.q.data_ptr()
        for a, b_ in zip(want, _outputs(bj, cont, zd, gd, lbd)):
            assert torch.equal(a, b_), what + ": contiguous parameters give other bits"
        o1, o2, o3 = dim * M, dim * M + M * M, dim * M + 2 * M * M
        for pad in range(4):
            rows = o3 + M + pad
            head = torch.zeros((N, rows), dtype=TDT[dt], device="cuda")
            head[:, :o1] = dense.q.permute(2, 1, 0).reshape(N, o1)
            head[:, o1:o2] = dense.r.permute(2, 1, 0).reshape(N, M * M)
            head[:, o2:o3] = dense.r_tilde.permute(2, 1, 0).reshape(N, M * M)
            head[:, o3:o3 + M] = dense.b.T
            sl = bj.AmortizedSylvesterLayer(head[:, :o1].view(N, M, dim).permute(2, 1, 0), head[:, o1:o2].view(N, M, M).permute(2, 1, 0),
                                            head[:, o2:o3].view(N, M, M).permute(2, 1, 0), head[:, o3:o3 + M].T)
            cp = sl._col_params(zd, dim, N)
            es = head.element_size()
            assert [t.data_ptr() for t in cp[:4]] == [head.data_ptr() + o * es for o in (0, o1, o2, o3)] and cp[4:] == [rows] * 4, what
            for a, b_ in zip(want, _outputs(bj, sl, zd, gd, lbd)):
                assert torch.equal(a, b_), f"{what}: the slices of one head (pad {pad}) give other bits"


def one_unit_given_as_vectors_and_a_vector_input(bj):
    """q (dim, batch), r, r_tilde, b (batch,): M = 1; the cotangents come back in those shapes.  A 1-D input is one column."""
    dt, dim, N = F64, 5, 9
    R = Ref(dt, dim, 1, N, ("one-unit",))
    layer = bj.AmortizedSylvesterLayer(dev2(R.Q[:, 0, :], dt), dev1(R.R[0, 0], dt), dev1(R.Rt[0, 0], dt), dev1(R.b[0], dt))
    zd, gd, lbd = R.data()
    what = f"sylvester_cols float64 dim={dim} M=1 batch={N} one unit"
    y, l = bj.with_logabsdet_jacobian(layer, zd)                # the siblings' shape: a per-column vector
    flat_close(host(y), R.F.out, dt, what + " values")
    flat_close(host(l), R.F.ladj, dt, what + " ladj", per="element", floor=1.0)
    flat_close(host(bj.logabsdetjac(layer, zd)), R.F.ladj, dt, what + " logabsdetjac", per="element", floor=1.0)
    flat_close(host(bj.transform(layer, zd)), R.F.out, dt, what + " transform")
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    assert grads["q"].shape == (dim, N) and grads["r"].shape == (N,) and grads["r_tilde"].shape == (N,) and grads["b"].shape == (N,)
    flat_close(host(xb), R.F.in_bar, dt, what + " input cotangent")
    for k, r in (("q", R.F.qb[:, 0, :]), ("r", R.F.rb[0, 0]), ("r_tilde", R.F.rtb[0, 0]), ("b", R.F.bb[0])):
        flat_close(host(grads[k]).reshape(-1, N), r.reshape(-1, N), dt, f"{what} {k} cotangent", term_scale=R.F.scale)
    one = bj.AmortizedSylvesterLayer(dev2(R.Q[:, 0, 1:2], dt), dev1(R.R[0, 0, 1:2], dt), dev1(R.Rt[0, 0, 1:2], dt), dev1(R.b[0, 1:2], dt))
    yv, lv = bj.with_logabsdet_jacobian(one, dev1(R.z[:, 1], dt), per_sample=True)
    assert yv.shape == (dim,)
    flat_close(host(yv).reshape(dim, 1), R.F.out[:, 1:2], dt, what + " vector input values")
    flat_close(host(lv).reshape(1), R.F.ladj[1:2], dt, what + " vector input ladj", per="element", floor=1.0)


def in_place_summed_log_det_and_ladj_bar(bj):
    """transform_ / with_logabsdet_jacobian_ write into the caller's buffer; the summed log-det is the Float64 sum of the per-sample
    one (1e-12: both are Float64 sums of the same Float values in another order) and two calls return the same bits; ladj_bar as None,
    as a number and as a tensor."""
    for dt, dim, M, N in ((F32, 8, 3, 300), (F64, 65, 9, 30), (F32, 260, 4, 9)):          # 3, 8 and 3 blocks: the sum crosses blocks
        R = Ref(dt, dim, M, N, ("misc", np.dtype(dt).name, dim, M))
        what = f"sylvester_cols {np.dtype(dt).name} dim={dim} M={M} batch={N}"
        layer = R.layer(bj)
        zd, gd, lbd = R.data()
        y, l = bj.with_logabsdet_jacobian(layer, zd, per_sample=True)
        buf = zd.clone()
        assert bj.transform_(layer, buf) is buf and torch.equal(buf, y), what + " transform_"
        buf, out = zd.clone(), torch.empty_like(zd)
        o2, l2 = bj.with_logabsdet_jacobian_(layer, buf, out)
        assert o2 is out and torch.equal(out, y) and torch.equal(buf, zd), what + " with_logabsdet_jacobian_"
        _, (lps, tot) = bj.with_logabsdet_jacobian(layer, zd, per_sample="both")
        assert torch.equal(lps, l), what
        want = float(host(l.double().sum()))
        assert abs(float(tot) - want) <= 1e-12 * max(1.0, abs(want)), (what, float(tot), want)
        _, (lps2, tot2) = bj.with_logabsdet_jacobian(layer, zd, per_sample="both")
        assert torch.equal(lps2, lps) and torch.equal(torch.as_tensor(tot2), torch.as_tensor(tot)), what + ": two calls differ in the bits of the summed log-det"
        flat_close(host(torch.as_tensor(tot).reshape(1)), np.array([R.F.ladj.sum()]), dt, what + " summed ladj", per="element", floor=1.0)
        for name, lbar, lbn in (("None", None, np.zeros(N)), ("number", 0.75, np.full(N, 0.75)), ("tensor", lbd, R.lb)):
            F = RefAll(R.Q, R.R, R.Rt, R.b, R.z, R.g, lbn)
            xb, grads = bj.vjp_params(layer, zd, gd, lbar)
            close_cols(host(xb), F.in_bar, dt, f"{what} ladj_bar={name} input cotangent")
            check_params(grads, F, N, dt, f"{what} ladj_bar={name}")


def a_nan_stays_in_its_column_and_the_lower_triangles_are_never_read(bj):
    """A NaN in b[M−1] of one column: a_{M−1} is NaN, so every p_i, every row of y, the log-det, every row of x̄ and of q̄ of THAT column
    are NaN and r̄, r̃̄, b̄ hold NaNs; every other column keeps its bits.  A NaN everywhere below the diagonal of r and r̃: no bit moves."""
    for dt, dim, M in ((F32, 3, 2), (F32, 64, 16), (F64, 65, 5), (F32, 516, 9)):
        N = 2 * (256 // lanes(dim, dt)) + 3
        R = Ref(dt, dim, M, N, ("nan", np.dtype(dt).name, dim, M))
        what = f"sylvester_cols NaN {np.dtype(dt).name} dim={dim} M={M} batch={N}"
        zd, gd, lbd = R.data()
        clean = _outputs(bj, R.layer(bj), zd, gd, lbd)
        close_cols(host(clean[2]), R.F.in_bar, dt, what + " input cotangent")
        bad = N // 2
        b = R.b.copy()
        b[M - 1, bad] = np.nan
        got = _outputs(bj, R.layer(bj, b=b), zd, gd, lbd)
        keep = torch.from_numpy(np.arange(N) != bad).cuda()
        for k, (a, c) in enumerate(zip(got, clean)):
            assert torch.equal(a[..., keep], c[..., keep]), f"{what}: output {k} of another column changed"
            assert bool(torch.isnan(a[..., bad]).any()), f"{what}: output {k} of the poisoned column holds no NaN"
        for k in (0, 1, 2, 3):
            assert bool(torch.isnan(got[k][..., bad]).all()), f"{what}: output {k} of the poisoned column is not NaN everywhere"
        low = np.tril(np.ones((M, M)), -1) > 0
        Rn, Rtn = R.R.copy(), R.Rt.copy()
        Rn[low], Rtn[low] = np.nan, np.nan
        lay = bj.AmortizedSylvesterLayer(dev3(R.Q, dt), dev3(Rn, dt), dev3(Rtn, dt), dev2(R.b, dt))
        for k, (a, c) in enumerate(zip(_outputs(bj, lay, zd, gd, lbd), clean)):
            assert torch.equal(a, c), f"{what}: output {k} moved with a NaN below the diagonal"


# ------------------------------------------------------------------ host routing
def composition_with_a_householder_head(bj):
    """layer ∘ AmortizedHouseholderFlow: each stays a stage of its own, and vjp_params of the composition is the stage-by-stage chain rule
    on the two references; a stack of two Sylvester layers the same way."""
    for dt in (F32, F64):
        dim, M, L, N = 6, 3, 2, 50
        R = Ref(dt, dim, M, N, ("compose", np.dtype(dt).name))
        v, s, m, _, _, _ = householder_draws(seed("compose-hh", np.dtype(dt).name), dim, L, N, dt)
        hh = bj.AmortizedHouseholderFlow(dev3(v, dt), dev2(s, dt), dev2(m, dt))
        layer = R.layer(bj)
        comp = layer @ hh
        assert [type(st).__name__ for st in comp._plan()[0]] == ["AmortizedHouseholderFlow", "AmortizedSylvesterLayer"]
        zd, gd, lbd = R.data()
        what = f"sylvester_cols ∘ householder_cols {np.dtype(dt).name} dim={dim} M={M} batch={N}"
        H = HouseholderRefAll(v, s, m, R.z, R.g, R.lb)
        S = RefAll(R.Q, R.R, R.Rt, R.b, H.out, R.g, R.lb)
        B = HouseholderRefAll(v, s, m, R.z, S.in_bar, R.lb)
        y, l = bj.with_logabsdet_jacobian(comp, zd, per_sample=True)
        flat_close(host(y), S.out, dt, what + " values")
        flat_close(host(l), S.ladj + H.ladj, dt, what + " ladj", per="element", floor=1.0)
        xb, G = bj.vjp_params(comp, zd, gd, lbd)
        flat_close(host(xb), B.in_bar, dt, what + " input cotangent")
        assert torch.equal(bj.vjp(comp, zd, gd, lbd), xb), what
        check_params(G["stages"][1], S, N, dt, what)
        for k, r in (("v", B.vb), ("log_scale", B.sb), ("shift", B.mb)):
            flat_close(host(G["stages"][0][k]).reshape(-1, N), r.reshape(-1, N), dt, f"{what} {k} cotangent", term_scale=B.scale)
        R2 = Ref(dt, dim, 2, N, ("compose-2", np.dtype(dt).name))
        stack = R2.layer(bj) @ layer
        S1 = RefAll(R.Q, R.R, R.Rt, R.b, R.z, R.g, R.lb)
        S2 = RefAll(R2.Q, R2.R, R2.Rt, R2.b, S1.out, R.g, R.lb)
        B1 = RefAll(R.Q, R.R, R.Rt, R.b, R.z, S2.in_bar, R.lb)
        what = f"sylvester_cols stack of two {np.dtype(dt).name} dim={dim} batch={N}"
        y, l = bj.with_logabsdet_jacobian(stack, zd, per_sample=True)
        flat_close(host(y), S2.out, dt, what + " values")
        flat_close(host(l), S1.ladj + S2.ladj, dt, what + " ladj", per="element", floor=1.0)
        xb, G = bj.vjp_params(stack, zd, gd, lbd)
        flat_close(host(xb), B1.in_bar, dt, what + " input cotangent")
        check_params(G["stages"][0], B1, N, dt, what + " first layer")
        check_params(G["stages"][1], S2, N, dt, what + " second layer")


def the_pullback_is_one_launch(bj):
    R = Ref(F32, 16, 3, 20, ("launches",))
    layer = R.layer(bj)
    zd, gd, lbd = R.data()
    bj.vjp_params(layer, zd, gd, lbd)
    _, _, k = bj.kernel_timed(lambda: bj.vjp_params(layer, zd, gd, lbd))
    assert k == 1, f"AmortizedSylvesterLayer: {k} hot launches"


def sizes_beyond_the_limits_and_the_inverse_are_refused(bj):
    for tdt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        q = torch.ones((1, 1, lim + 1), dtype=tdt, device="cuda").permute(2, 1, 0)
        one = torch.ones(1, dtype=tdt, device="cuda")
        layer = bj.AmortizedSylvesterLayer(q, one, one, one)
        x = torch.zeros((1, lim + 1), dtype=tdt, device="cuda").T
        for call in (lambda: bj.transform(layer, x), lambda: bj.vjp(layer, x, x), lambda: bj.vjp_params(layer, x, x)):
            with pytest.raises(ValueError, match=str(lim)):
                call()
    for M in (0, 17):
        with pytest.raises(ValueError, match="16"):
            bj.AmortizedSylvesterLayer(torch.zeros((32, M, 4), device="cuda"), torch.zeros((M, M, 4), device="cuda"), torch.zeros((M, M, 4), device="cuda"),
                                       torch.zeros((M, 4), device="cuda"))
    with pytest.raises(ValueError, match="above dim 2"):
        bj.AmortizedSylvesterLayer(torch.zeros((2, 3, 4), device="cuda"), torch.zeros((3, 3, 4), device="cuda"), torch.zeros((3, 3, 4), device="cuda"),
                                   torch.zeros((3, 4), device="cuda"))
    R = Ref(F32, 3, 2, 4, ("refuse",))
    layer = R.layer(bj)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((4, 5), device="cuda").T)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((3, 3), device="cuda").T)
    zd, gd, lbd = R.data()
    inv = bj.inverse(layer)
    td = bj.transformed(bj.MvNormal(3), layer)
    for call in (lambda: bj.transform(inv, zd), lambda: bj.with_logabsdet_jacobian(inv, zd), lambda: bj.vjp(inv, zd, gd), lambda: bj.vjp_params(inv, zd, gd),
                 lambda: bj.logpdf(td, zd), lambda: bj.logpdf_vjp_params(td, zd)):
        with pytest.raises(NotImplementedError, match="inverse map is not built"):
            call()


# ------------------------------------------------------------------ the C ABI
def cols(a, dt):
    """(A, B, N) / (rows, N) / (N,) numpy -> flat cuda tensor in the dense ABI layout: the first index fastest, the column slowest."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T).reshape(-1)).cuda()


class Call:
    """One parameter draw on the device in the dense ABI layout, and the two entries bound to it."""

    def __init__(self, bj, dt, dim, M, N, key):
        self.bj, self.dt, self.dim, self.M, self.N = bj, dt, dim, M, N
        self.np = draws(seed(*key), dim, M, N, dt)
        self.q, self.r, self.rt, self.b, self.z, self.g, self.lb = (cols(a, dt) for a in self.np)
        self.ctx = bj.context(self.q.device)
        self.lib = bj._lib.load()
        self.code = bj._lib.BJX_F32 if dt == F32 else bj._lib.BJX_F64
        self.what = f"{np.dtype(dt).name} dim={dim} M={M} batch={N}"

    def empty(self, n):
        return torch.full((n,), float("nan"), dtype=TDT[self.dt], device="cuda")

    def bars(self):
        return [self.empty(self.N * self.M * self.dim), self.empty(self.N * self.M * self.M), self.empty(self.N * self.M * self.M), self.empty(self.N * self.M)]

    def _params(self, lds, null):
        p = self.bj.interface._ptr
        ptrs = [None if k == null else p(t) for k, t in enumerate((self.q, self.r, self.rt, self.b))]
        return ptrs + list(lds or (self.dim * self.M, self.M * self.M, self.M * self.M, self.M))

    def map(self, x, out, ps, sm, flags=0, batch=None, M=None, dim=None, lds=None, null=None, code=None):
        p = self.bj.interface._ptr
        rc = self.lib.bjx_sylvester_cols(self.ctx.h, self.code if code is None else code, *self._params(lds, null), self.M if M is None else M, p(x), p(out),
                                         p(ps), p(sm), self.dim if dim is None else dim, self.N if batch is None else batch, flags)
        torch.cuda.synchronize()
        return rc

    def vjp(self, x, g, lb, xb, qb, rb, rtb, bb, batch=None, M=None, dim=None, lds=None, null=None, code=None):
        p = self.bj.interface._ptr
        rc = self.lib.bjx_sylvester_cols_vjp(self.ctx.h, self.code if code is None else code, *self._params(lds, null), self.M if M is None else M, p(x), p(g),
                                             p(lb), p(xb), p(qb), p(rb), p(rtb), p(bb), self.dim if dim is None else dim, self.N if batch is None else batch)
        torch.cuda.synchronize()
        return rc

    def mat(self, t):
        """flat device tensor -> (rows, N) numpy"""
        return host(t).reshape(self.N, -1).T


def accumulate_in_place_and_the_summed_log_det(bj):
    for dt, dim, M, N in ((F32, 8, 3, 300), (F64, 5, 2, 200), (F32, 260, 16, 9), (F64, 64, 8, 40)):
        c = Call(bj, dt, dim, M, N, ("abi-acc", np.dtype(dt).name, dim, M))
        ref = RefAll(*c.np)
        what = "bjx_sylvester_cols " + c.what
        out, ps = c.empty(N * dim), c.empty(N)
        sm = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        assert c.map(c.z, out, ps, sm) == 0
        flat_close(c.mat(out), ref.out, dt, what + " values")
        flat_close(host(ps), ref.ladj, dt, what + " ladj", per="element", floor=1.0)
        total = float(host(ps.double().sum()))
        assert abs(float(host(sm)[0]) - total) <= 1e-12 * max(1.0, abs(total)), (what, float(host(sm)[0]), total)
        sm2 = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        out2, ps2 = c.empty(N * dim), c.empty(N)
        assert c.map(c.z, out2, ps2, sm2) == 0
        assert torch.equal(sm2, sm) and torch.equal(ps2, ps) and torch.equal(out2, out), what + ": two calls differ in their bits"
        sm3 = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        assert c.map(c.z, out2, None, sm3) == 0 and torch.equal(sm3, sm)
        assert c.map(c.z, out2, ps2, None) == 0 and torch.equal(ps2, ps)
        assert c.map(c.z, out2, None, None) == 0 and torch.equal(out2, out)
        p0 = torch.from_numpy(np.asarray(seed("p0", N).normal(size=N), dt)).cuda()
        ps_acc, sm_acc = p0.clone(), torch.full((1,), 2.5, dtype=torch.float64, device="cuda")
        assert c.map(c.z, out2, ps_acc, sm_acc, flags=bj._lib.BJX_ACCUMULATE) == 0
        assert torch.equal(ps_acc, p0 + ps), what + " BJX_ACCUMULATE"
        assert abs(float(host(sm_acc)[0]) - (2.5 + float(host(sm)[0]))) <= 1e-12 * (2.5 + abs(total)), what + " BJX_ACCUMULATE"
        # out == in and in_bar == out_bar
        buf, ps2 = c.z.clone(), c.empty(N)
        assert c.map(buf, buf, ps2, None) == 0
        assert torch.equal(buf, out) and torch.equal(ps2, ps), what + ": out == in differs"
        xb, bars = c.empty(N * dim), c.bars()
        assert c.vjp(c.z, c.g, c.lb, xb, *bars) == 0
        gbuf, bars2 = c.g.clone(), c.bars()
        assert c.vjp(c.z, gbuf, c.lb, gbuf, *bars2) == 0
        assert torch.equal(gbuf, xb) and all(torch.equal(s, t) for s, t in zip(bars, bars2)), what + ": in_bar == out_bar differs"
        xb0, xbz = c.empty(N * dim), c.empty(N * dim)             # ladj_bar = NULL is a zero cotangent
        assert c.vjp(c.z, c.g, None, xb0, None, None, None, None) == 0 and c.vjp(c.z, c.g, torch.zeros_like(c.lb), xbz, None, None, None, None) == 0
        assert torch.equal(xb0, xbz), what


def null_cotangent_outputs_in_every_combination(bj):
    for dt, dim, M, N in ((F32, 5, 3, 130), (F64, 64, 2, 20), (F64, 257, 16, 5), (F32, 8, 8, 70)):
        c = Call(bj, dt, dim, M, N, ("abi-null", np.dtype(dt).name, dim, M))
        full = c.bars()
        xb = c.empty(N * dim)
        assert c.vjp(c.z, c.g, c.lb, xb, *full) == 0
        what = "bjx_sylvester_cols_vjp " + c.what
        ref = RefAll(*c.np)
        flat_close(c.mat(xb), ref.in_bar, dt, what + " input cotangent")
        for name, got, r in zip(NAMES, full, (ref.qb, ref.rb, ref.rtb, ref.bb)):
            flat_close(c.mat(got), np.ascontiguousarray(r.transpose(2, 1, 0) if r.ndim == 3 else r.T).reshape(N, -1).T, dt, f"{what} {name} cotangent",
                       term_scale=ref.scale)
        for want in itertools.product((True, False), repeat=4):
            if all(want):
                continue
            outs = [c.empty(t.numel()) if w_ else None for t, w_ in zip(full, want)]
            xb2 = c.empty(N * dim)
            assert c.vjp(c.z, c.g, c.lb, xb2, *outs) == 0
            assert torch.equal(xb2, xb), f"{what}: the input cotangent changes with outputs {want}"
            for o, f_ in zip(outs, full):
                assert o is None or torch.equal(o, f_), f"{what}: a cotangent changes with outputs {want}"


def batch_zero(bj):
    c = Call(bj, F32, 4, 2, 3, ("abi-empty",))
    sm = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    out = c.empty(12)
    assert c.map(c.z, out, None, sm, batch=0) == 0
    assert float(host(sm)[0]) == 0.0 and bool(torch.isnan(out).all())
    sm.fill_(7.0)
    assert c.map(c.z, out, None, sm, batch=0, flags=bj._lib.BJX_ACCUMULATE) == 0 and float(host(sm)[0]) == 7.0
    for null in range(4):
        assert c.map(None, None, None, None, batch=0, null=null) == 0         # nothing to read: null pointers are fine
    xb, bars = c.empty(12), c.bars()
    assert c.vjp(c.z, c.g, c.lb, xb, *bars, batch=0) == 0
    assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars)


def refusals_happen_before_any_launch(bj):
    Lb = bj._lib
    for dt, lim in ((F32, 1024), (F64, 512)):
        c = Call(bj, dt, 4, 2, 6, ("abi-refuse", np.dtype(dt).name))
        out, ps = c.empty(24), c.empty(6)
        sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
        xb, bars = c.empty(24), c.bars()
        err = lambda: (Lb.load().bjx_last_error(c.ctx.h) or b"").decode()
        both = (lambda **kw: c.map(c.z, out, ps, sm, **kw), lambda **kw: c.vjp(c.z, c.g, c.lb, xb, *bars, **kw))
        for f in both:
            # units outside 1 ... 16, more units than rows, dim above the limit: UNSUPPORTED
            for M in (0, 17):
                assert f(M=M, dim=32, lds=(32 * 17, 17 * 17, 17 * 17, 17)) == Lb.ERR_UNSUPPORTED and "16" in err()
            assert f(M=5, lds=(20, 25, 25, 5)) == Lb.ERR_UNSUPPORTED and "above dim 4" in err()
            assert f(dim=lim + 1, lds=((lim + 1) * 2, 4, 4, 2)) == Lb.ERR_UNSUPPORTED and str(lim) in err()
            # strides below the minimum, dim < 1, batch < 0: SHAPE
            for lds in ((7, 4, 4, 2), (8, 3, 4, 2), (8, 4, 3, 2), (8, 4, 4, 1)):
                assert f(lds=lds) == Lb.ERR_SHAPE
            assert f(dim=0) == Lb.ERR_SHAPE and f(batch=-1) == Lb.ERR_SHAPE
            # null required pointers with batch > 0, a bad dtype: ARG
            for null in range(4):
                assert f(null=null) == Lb.ERR_ARG
            assert f(code=77) == Lb.ERR_ARG
        assert c.map(None, out, ps, sm) == Lb.ERR_ARG and c.map(c.z, None, ps, sm) == Lb.ERR_ARG
        assert c.vjp(None, c.g, c.lb, xb, *bars) == Lb.ERR_ARG and c.vjp(c.z, None, c.lb, xb, *bars) == Lb.ERR_ARG
        assert c.vjp(c.z, c.g, c.lb, None, *bars) == Lb.ERR_ARG
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ps).all()) and float(host(sm)[0]) == 3.0, "a refused call wrote something"
        assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars), "a refused call wrote something"
        assert c.vjp(c.z, c.g, c.lb, xb, *bars) == 0 and bool(torch.isfinite(xb).all()) and all(bool(torch.isfinite(t).all()) for t in bars)


# ------------------------------------------------------------------ the three test ids
def test_kernels_at_every_form_edge_padded_unit_count_layout_and_special_input(bj):
    for dt in (F32, F64):
        maps_and_pullbacks_match_reference(bj, dt)
    parameter_layouts_give_the_same_bits(bj)
    one_unit_given_as_vectors_and_a_vector_input(bj)
    in_place_summed_log_det_and_ladj_bar(bj)
    a_nan_stays_in_its_column_and_the_lower_triangles_are_never_read(bj)


def test_host_class_composition_launch_count_and_refusals(bj):
    composition_with_a_householder_head(bj)
    the_pullback_is_one_launch(bj)
    sizes_beyond_the_limits_and_the_inverse_are_refused(bj)


def test_c_abi_contract(bj):
    accumulate_in_place_and_the_summed_log_det(bj)
    null_cotangent_outputs_in_every_combination(bj)
    batch_zero(bj)
    refusals_happen_before_any_launch(bj)
