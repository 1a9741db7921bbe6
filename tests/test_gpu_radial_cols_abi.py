"""bjx_radial_cols / bjx_radial_cols_vjp (include/bjx_radial_cols.h) called through the C ABI: BJX_ACCUMULATE on ladj_ps and ladj_sum,
the summed log-det against the Float64 sum of the per-column values and bit-identical from call to call, in-place calls,
batch == 0, NULL parameter-cotangent outputs in every combination and in both directions, and every refusal with its status code
and nothing written.  Values are held to tests/_tol.py's flat bar against the oracle column by column
(tests/_radial_cols_ref.py), as in tests/test_gpu_radial_cols.py."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _radial_cols_ref import RefAll, draws, seed  # noqa: E402
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
        self.a, self.b, self.z0, self.z, self.g, self.lb = (cols(a, dt) for a in self.np)
        self.ctx = bj.context(self.a.device)
        self.lib = bj._lib.load()
        self.code = bj._lib.BJX_F32 if dt == F32 else bj._lib.BJX_F64

    def empty(self, *shape):
        return torch.full(shape, float("nan"), dtype=TDT[self.dt], device="cuda")

    def map(self, inverse, x, out, ps, sm, flags=0, batch=None, L=None, dim=None, lds=None, a="a", b="b", z0="z0", code=None):
        p = self.bj.interface._ptr
        L_, dim_ = self.L if L is None else L, self.dim if dim is None else dim
        la, lb, lz = lds or (self.L, self.L, self.dim * self.L)
        rc = self.lib.bjx_radial_cols(self.ctx.h, self.code if code is None else code, int(inverse), p(getattr(self, a) if a else None),
                                      p(getattr(self, b) if b else None), p(getattr(self, z0) if z0 else None), la, lb, lz, L_, p(x), p(out), p(ps), p(sm), dim_,
                                      self.N if batch is None else batch, flags)
        torch.cuda.synchronize()
        return rc

    def vjp(self, inverse, x, g, lb, xb, ab, bb, zb, batch=None, L=None, dim=None, lds=None, code=None):
        p = self.bj.interface._ptr
        la, lb_, lz = lds or (self.L, self.L, self.dim * self.L)
        rc = self.lib.bjx_radial_cols_vjp(self.ctx.h, self.code if code is None else code, int(inverse), p(self.a), p(self.b), p(self.z0), la, lb_, lz,
                                          self.L if L is None else L, p(x), p(g), p(lb), p(xb), p(ab), p(bb), p(zb), self.dim if dim is None else dim,
                                          self.N if batch is None else batch)
        torch.cuda.synchronize()
        return rc

    def mat(self, t):
        """flat device tensor -> (rows, N) numpy"""
        return host(t).reshape(self.N, -1).T

    def cube(self, t):
        """flat device tensor [dim, L, N] -> (dim·L, N) numpy in the row order of a (dim, L, N) array"""
        return host(t).reshape(self.N, self.L, -1).transpose(2, 1, 0).reshape(-1, self.N)


def test_accumulate_and_the_summed_log_det(bj, orc):
    for dt, dim, L, N in ((F32, 8, 3, 300), (F64, 5, 2, 200), (F32, 260, 2, 9)):          # 3, 4 and 3 blocks: the summed log-det crosses blocks
        for inverse in (False, True):
            _accumulate_and_the_summed_log_det(bj, orc, dt, dim, L, N, inverse)


def _accumulate_and_the_summed_log_det(bj, orc, dt, dim, L, N, inverse):
    c = Call(bj, dt, dim, L, N, ("abi-acc", np.dtype(dt).name, dim, L, inverse))
    al, be, z0, z, g, lb = c.np
    ref = RefAll(orc, al, be, z0, z, g, lb, inverse)
    what = f"bjx_radial_cols {np.dtype(dt).name} dim={dim} L={L} inv={inverse}"
    out, ps = c.empty(N * dim), c.empty(N)
    sm = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    assert c.map(inverse, c.z, out, ps, sm) == 0
    flat_close(c.mat(out), ref.out, dt, what + " values")
    flat_close(host(ps), ref.ladj, dt, what + " ladj", per="element", floor=1.0)
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
        xb, bars = c.empty(N * dim), [c.empty(N * L), c.empty(N * L), c.empty(N * L * dim)]
        assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars) == 0
        gbuf, bars2 = c.g.clone(), [c.empty(N * L), c.empty(N * L), c.empty(N * L * dim)]
        assert c.vjp(inverse, c.z, gbuf, c.lb, gbuf, *bars2) == 0
        assert torch.equal(gbuf, xb) and all(torch.equal(s, t) for s, t in zip(bars, bars2)), f"in_bar == out_bar differs (dim={dim} inverse={inverse})"
        xb0 = c.empty(N * dim)                                   # ladj_bar = NULL is a zero cotangent
        assert c.vjp(inverse, c.z, c.g, None, xb0, None, None, None) == 0
        xbz = c.empty(N * dim)
        assert c.vjp(inverse, c.z, c.g, torch.zeros_like(c.lb), xbz, None, None, None) == 0
        assert torch.equal(xb0, xbz)


def test_null_cotangent_outputs_in_every_combination(bj, orc):
    for dt, dim, L, N in ((F32, 5, 3, 130), (F64, 64, 2, 20), (F64, 257, 1, 5)):
        for inverse in (False, True):
            _null_cotangent_outputs_in_every_combination(bj, orc, dt, dim, L, N, inverse)


def _null_cotangent_outputs_in_every_combination(bj, orc, dt, dim, L, N, inverse):
    c = Call(bj, dt, dim, L, N, ("abi-null", np.dtype(dt).name, dim))
    al, be, z0, z, g, lb = c.np
    full = [c.empty(N * L), c.empty(N * L), c.empty(N * L * dim)]
    xb = c.empty(N * dim)
    assert c.vjp(inverse, c.z, c.g, c.lb, xb, *full) == 0
    what = f"bjx_radial_cols_vjp {np.dtype(dt).name} dim={dim} L={L} inv={inverse}"
    ref = RefAll(orc, al, be, z0, z, g, lb, inverse)
    flat_close(c.mat(xb), ref.in_bar, dt, what + " input cotangent")
    for name, got, r in zip(("alpha_", "beta", "z_0"), full, (ref.ab, ref.bb, ref.zb)):
        flat_close(c.cube(got) if name == "z_0" else c.mat(got), r.reshape(-1, N), dt, f"{what} {name} cotangent", term_scale=ref.scale)
    for want in itertools.product((True, False), repeat=3):
        if all(want):
            continue
        outs = [c.empty(t.numel()) if w_ else None for t, w_ in zip(full, want)]
        xb2 = c.empty(N * dim)
        assert c.vjp(inverse, c.z, c.g, c.lb, xb2, *outs) == 0
        assert torch.equal(xb2, xb), f"{what}: the input cotangent changes with outputs {want}"
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
    assert c.map(False, None, None, None, None, batch=0, a=None, b=None, z0=None) == 0         # nothing to read: null pointers are fine
    xb, bars = c.empty(12), [c.empty(6), c.empty(6), c.empty(24)]
    for inverse in (False, True):
        assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, batch=0) == 0
    assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars)


def test_refusals_happen_before_any_launch(bj):
    Lb = bj._lib
    for dt, lim in ((F32, 1024), (F64, 512)):
        c = Call(bj, dt, 4, 2, 6, ("abi-refuse", np.dtype(dt).name))
        out, ps = c.empty(24), c.empty(6)
        sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
        xb, bars = c.empty(24), [c.empty(12), c.empty(12), c.empty(48)]
        err = lambda: (Lb.load().bjx_last_error(c.ctx.h) or b"").decode()
        for inverse in (False, True):
            # layers outside 1 ... 64 and dim above the limit: UNSUPPORTED
            for L in (0, 65):
                assert c.map(inverse, c.z, out, ps, sm, L=L, lds=(65, 65, 4 * 65)) == Lb.ERR_UNSUPPORTED and "64" in err()
                assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, L=L, lds=(65, 65, 4 * 65)) == Lb.ERR_UNSUPPORTED and "64" in err()
            big = (2, 2, (lim + 1) * 2)
            assert c.map(inverse, c.z, out, ps, sm, dim=lim + 1, lds=big) == Lb.ERR_UNSUPPORTED and str(lim) in err()
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, dim=lim + 1, lds=big) == Lb.ERR_UNSUPPORTED and str(lim) in err()
            # strides below the minimum, dim < 1, batch < 0: SHAPE
            for lds in ((1, 2, 8), (2, 1, 8), (2, 2, 7)):
                assert c.map(inverse, c.z, out, ps, sm, lds=lds) == Lb.ERR_SHAPE
                assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, lds=lds) == Lb.ERR_SHAPE
            assert c.map(inverse, c.z, out, ps, sm, dim=0) == Lb.ERR_SHAPE and c.map(inverse, c.z, out, ps, sm, batch=-1) == Lb.ERR_SHAPE
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, dim=0) == Lb.ERR_SHAPE and c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, batch=-1) == Lb.ERR_SHAPE
            # null pointers with batch > 0, a bad dtype: ARG
            for miss in ("a", "b", "z0"):
                assert c.map(inverse, c.z, out, ps, sm, **{miss: None}) == Lb.ERR_ARG
            assert c.map(inverse, None, out, ps, sm) == Lb.ERR_ARG and c.map(inverse, c.z, None, ps, sm) == Lb.ERR_ARG
            assert c.map(inverse, c.z, out, ps, sm, code=77) == Lb.ERR_ARG
            assert c.vjp(inverse, None, c.g, c.lb, xb, *bars) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, None, c.lb, xb, *bars) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, c.g, c.lb, None, *bars) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, code=77) == Lb.ERR_ARG
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ps).all()) and float(host(sm)[0]) == 3.0, "a refused call wrote something"
        assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars), "a refused call wrote something"
        # unlike the planar entry, the inverse takes parameter outputs
        assert c.vjp(True, c.z, c.g, c.lb, xb, *bars) == 0 and bool(torch.isfinite(xb).all()) and all(bool(torch.isfinite(t).all()) for t in bars)
