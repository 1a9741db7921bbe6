"""bjx_planar_cols / bjx_planar_cols_vjp (include/bjx_planar_cols.h) called through the C ABI: BJX_ACCUMULATE on ladj_ps and ladj_sum,
the summed log-det against the Float64 sum of the per-column values and bit-identical from call to call, in-place calls,
batch == 0, NULL parameter-cotangent outputs in every combination, and every refusal with its status code and nothing written.
Values are held to tests/_tol.py's flat bar against the oracle column by column (tests/_planar_cols_ref.py), as in
tests/test_gpu_planar_cols.py."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _planar_cols_ref import draws, joint_scale, ref_map, ref_param_vjp, ref_vjp, seed  # noqa: E402
from _tol import flat_close  # noqa: E402

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def host(t):
    return t.detach().cpu().numpy()


def cols(a, dt):
    """(dim, L, N) / (rows, N) / (N,) numpy -> flat cuda tensor in the dense ABI layout: the first index fastest, the column slowest."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T).reshape(-1)).cuda()


class Call:
    """One parameter draw on the device in the dense ABI layout, and the two entries bound to it."""

    def __init__(self, bj, dt, dim, L, N, key):
        self.bj, self.dt, self.dim, self.L, self.N = bj, dt, dim, L, N
        self.np = draws(seed(*key), dim, L, N, dt)
        self.w, self.u, self.b, self.z, self.g, self.lb = (cols(a, dt) for a in self.np)
        self.ctx = bj.context(self.w.device)
        self.lib = bj._lib.load()
        self.code = bj._lib.BJX_F32 if dt == F32 else bj._lib.BJX_F64

    def empty(self, *shape):
        return torch.full(shape, float("nan"), dtype=TDT[self.dt], device="cuda")

    def map(self, inverse, x, out, ps, sm, flags=0, batch=None, L=None, dim=None, lds=None, w="w", u="u", b="b"):
        p = self.bj.interface._ptr
        L_, dim_ = self.L if L is None else L, self.dim if dim is None else dim
        lw, lu, lb = lds or (self.dim * self.L, self.dim * self.L, self.L)
        rc = self.lib.bjx_planar_cols(self.ctx.h, self.code, int(inverse), p(getattr(self, w) if w else None), p(getattr(self, u) if u else None),
                                      p(getattr(self, b) if b else None), lw, lu, lb, L_, p(x), p(out), p(ps), p(sm), dim_, self.N if batch is None else batch, flags)
        torch.cuda.synchronize()
        return rc

    def vjp(self, inverse, x, g, lb, xb, wb, ub, bb, batch=None):
        p = self.bj.interface._ptr
        rc = self.lib.bjx_planar_cols_vjp(self.ctx.h, self.code, int(inverse), p(self.w), p(self.u), p(self.b), self.dim * self.L, self.dim * self.L, self.L, self.L,
                                          p(x), p(g), p(lb), p(xb), p(wb), p(ub), p(bb), self.dim, self.N if batch is None else batch)
        torch.cuda.synchronize()
        return rc

    def mat(self, t):
        """flat device tensor -> (rows, N) numpy"""
        return host(t).reshape(self.N, -1).T

    def cube(self, t):
        """flat device tensor [dim, L, N] -> (dim·L, N) numpy in the row order of a (dim, L, N) array"""
        return host(t).reshape(self.N, self.L, -1).transpose(2, 1, 0).reshape(-1, self.N)


@pytest.mark.parametrize("inverse", [False, True])
def test_accumulate_and_the_summed_log_det(bj, orc, inverse):
    for dt, dim, L, N in ((F32, 8, 3, 1000), (F64, 5, 2, 700), (F32, 260, 2, 9)):
        _accumulate_and_the_summed_log_det(bj, orc, dt, dim, L, N, inverse)


def _accumulate_and_the_summed_log_det(bj, orc, dt, dim, L, N, inverse):
    c = Call(bj, dt, dim, L, N, ("abi-acc", np.dtype(dt).name, dim, L, inverse))
    w, u, b, z, _, _ = c.np
    y_ref, l_ref = ref_map(orc, w, u, b, z, inverse=inverse)
    what = f"bjx_planar_cols {np.dtype(dt).name} dim={dim} L={L} inv={inverse}"
    out, ps = c.empty(N * dim), c.empty(N)
    sm = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    assert c.map(inverse, c.z, out, ps, sm) == 0
    flat_close(c.mat(out), y_ref, dt, what + " values")
    flat_close(host(ps), l_ref, dt, what + " ladj", per="element", floor=1.0)
    total = float(host(ps.double().sum()))
    assert abs(float(host(sm)[0]) - total) <= 1e-12 * abs(total), (float(host(sm)[0]), total)
    sm2 = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    out2, ps2 = c.empty(N * dim), c.empty(N)
    assert c.map(inverse, c.z, out2, ps2, sm2) == 0
    assert torch.equal(sm2, sm) and torch.equal(ps2, ps) and torch.equal(out2, out), what + ": two calls differ in their bits"
    # only the sum, only the per-column values, neither
    sm3 = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    assert c.map(inverse, c.z, out2, None, sm3) == 0 and torch.equal(sm3, sm)
    assert c.map(inverse, c.z, out2, ps2, None) == 0 and torch.equal(ps2, ps)
    assert c.map(inverse, c.z, out2, None, None) == 0 and torch.equal(out2, out)
    # BJX_ACCUMULATE adds to both
    p0 = torch.from_numpy(np.asarray(seed("p0", N).normal(size=N), dt)).cuda()
    ps_acc, sm_acc = p0.clone(), torch.full((1,), 2.5, dtype=torch.float64, device="cuda")
    assert c.map(inverse, c.z, out2, ps_acc, sm_acc, flags=bj._lib.BJX_ACCUMULATE) == 0
    assert torch.equal(ps_acc, p0 + ps)
    assert abs(float(host(sm_acc)[0]) - (2.5 + float(host(sm)[0]))) <= 1e-12 * (2.5 + abs(total))


def test_in_place_calls_give_the_same_bits(bj):
    for dt, dim, L, N in ((F32, 64, 2, 40), (F64, 3, 4, 300)):
        _in_place_calls_give_the_same_bits(bj, dt, dim, L, N)


def _in_place_calls_give_the_same_bits(bj, dt, dim, L, N):
    c = Call(bj, dt, dim, L, N, ("abi-inplace", np.dtype(dt).name, dim))
    for inverse in (False, True):
        out, ps = c.empty(N * dim), c.empty(N)
        assert c.map(inverse, c.z, out, ps, None) == 0
        buf, ps2 = c.z.clone(), c.empty(N)
        assert c.map(inverse, buf, buf, ps2, None) == 0
        assert torch.equal(buf, out) and torch.equal(ps2, ps), f"out == in differs (dim={dim} inverse={inverse})"
        xb = c.empty(N * dim)
        assert c.vjp(inverse, c.z, c.g, c.lb, xb, None, None, None) == 0
        gbuf = c.g.clone()
        assert c.vjp(inverse, c.z, gbuf, c.lb, gbuf, None, None, None) == 0
        assert torch.equal(gbuf, xb), f"in_bar == out_bar differs (dim={dim} inverse={inverse})"
        xb0 = c.empty(N * dim)                                   # ladj_bar = NULL is a zero cotangent
        assert c.vjp(inverse, c.z, c.g, None, xb0, None, None, None) == 0
        xbz = c.empty(N * dim)
        assert c.vjp(inverse, c.z, c.g, torch.zeros_like(c.lb), xbz, None, None, None) == 0
        assert torch.equal(xb0, xbz)


def test_null_cotangent_outputs_in_every_combination(bj, orc):
    for dt, dim, L, N in ((F32, 5, 3, 130), (F64, 64, 2, 20), (F64, 257, 1, 5)):
        _null_cotangent_outputs_in_every_combination(bj, orc, dt, dim, L, N)


def _null_cotangent_outputs_in_every_combination(bj, orc, dt, dim, L, N):
    c = Call(bj, dt, dim, L, N, ("abi-null", np.dtype(dt).name, dim))
    w, u, b, z, g, lb = c.np
    full = [c.empty(N * L * dim), c.empty(N * L * dim), c.empty(N * L)]
    xb = c.empty(N * dim)
    assert c.vjp(False, c.z, c.g, c.lb, xb, *full) == 0
    what = f"bjx_planar_cols_vjp {np.dtype(dt).name} dim={dim} L={L}"
    flat_close(c.mat(xb), ref_vjp(orc, w, u, b, z, g, lb), dt, what + " x̄")
    refs = ref_param_vjp(orc, w, u, b, z, g, lb)
    ts = joint_scale(*refs)
    for name, got, ref in zip("wub", full, refs):
        flat_close(c.mat(got) if name == "b" else c.cube(got), ref.reshape(-1, N), dt, f"{what} {name}̄", term_scale=ts)
    for want in itertools.product((True, False), repeat=3):
        if all(want):
            continue
        outs = [c.empty(t.numel()) if w_ else None for t, w_ in zip(full, want)]
        xb2 = c.empty(N * dim)
        assert c.vjp(False, c.z, c.g, c.lb, xb2, *outs) == 0
        assert torch.equal(xb2, xb), f"{what}: x̄ changes with outputs {want}"
        for o, f_ in zip(outs, full):
            assert o is None or torch.equal(o, f_), f"{what}: a cotangent changes with outputs {want}"


def test_batch_zero(bj):
    c = Call(bj, F32, 4, 2, 3, ("abi-empty",))
    sm = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    out = c.empty(12)
    assert c.map(False, c.z, out, None, sm, batch=0) == 0
    assert float(host(sm)[0]) == 0.0 and bool(torch.isnan(out).all())
    sm.fill_(7.0)
    assert c.map(True, c.z, out, None, sm, batch=0, flags=bj._lib.BJX_ACCUMULATE) == 0 and float(host(sm)[0]) == 7.0
    assert c.map(False, None, None, None, None, batch=0, w=None, u=None, b=None) == 0          # nothing to read: null pointers are fine
    xb = c.empty(12)
    assert c.vjp(False, c.z, c.g, c.lb, xb, None, None, None, batch=0) == 0 and bool(torch.isnan(xb).all())


def test_refusals_happen_before_any_launch(bj):
    Lb = bj._lib
    for dt, lim in ((F32, 1024), (F64, 512)):
        c = Call(bj, dt, 4, 2, 6, ("abi-refuse", np.dtype(dt).name))
        out, ps = c.empty(24), c.empty(6)
        sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
        err = lambda: (Lb.load().bjx_last_error(c.ctx.h) or b"").decode()
        for L in (0, 65):
            assert c.map(False, c.z, out, ps, sm, L=L) == Lb.ERR_UNSUPPORTED and "64" in err()
        assert c.map(False, c.z, out, ps, sm, dim=lim + 1, lds=((lim + 1) * 2, (lim + 1) * 2, 2)) == Lb.ERR_UNSUPPORTED and str(lim) in err()
        for lds in ((7, 8, 2), (8, 7, 2), (8, 8, 1)):
            assert c.map(True, c.z, out, ps, sm, lds=lds) == Lb.ERR_SHAPE
        for miss in ("w", "u", "b"):
            assert c.map(False, c.z, out, ps, sm, **{miss: None}) == Lb.ERR_ARG
        assert c.map(False, None, out, ps, sm) == Lb.ERR_ARG and c.map(False, c.z, None, ps, sm) == Lb.ERR_ARG
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ps).all()) and float(host(sm)[0]) == 3.0, "a refused call wrote something"
        # the pullback: the inverse has no parameter outputs; null data pointers
        xb, bars = c.empty(24), [c.empty(48), c.empty(48), c.empty(12)]
        for k in range(3):
            outs = [bars[j] if j == k else None for j in range(3)]
            assert c.vjp(True, c.z, c.g, c.lb, xb, *outs) == Lb.ERR_ARG
        assert c.vjp(False, None, c.g, c.lb, xb, *bars) == Lb.ERR_ARG
        assert c.vjp(False, c.z, None, c.lb, xb, *bars) == Lb.ERR_ARG
        assert c.vjp(False, c.z, c.g, c.lb, None, *bars) == Lb.ERR_ARG
        assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars), "a refused call wrote something"
        assert c.vjp(True, c.z, c.g, c.lb, xb, None, None, None) == 0 and bool(torch.isfinite(xb).all())
