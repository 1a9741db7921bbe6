"""bjx_householder_cols / bjx_householder_cols_vjp (include/bjx_householder_cols.h) called through the C ABI: BJX_ACCUMULATE on ladj_ps
and ladj_sum, the summed log-det against the Float64 sum of the per-column values and bit-identical from call to call, in-place
calls, batch == 0, NULL parameter-cotangent outputs in every combination and in both directions with identical x̄ bits, absent p_s /
p_m, and every refusal with its status code and nothing written.  Values are held to tests/_tol.py's flat bar against the Float64
closed forms (tests/_householder_cols_ref.py), as in tests/test_gpu_householder_cols.py.
The GPU suite is kept at 5 000 test ids, so the parts below are plain functions called in turn by ONE test id."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _householder_cols_ref import HEADS, RefAll, draws, seed  # noqa: E402
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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T).reshape(-1)).cuda()


class Call:
    """One parameter draw on the device in the dense ABI layout, and the two entries bound to it."""

    def __init__(self, bj, dt, dim, L, N, key, head="both"):
        self.bj, self.dt, self.dim, self.L, self.N = bj, dt, dim, L, N
        self.np = draws(seed(*key), dim, L, N, dt, head)
        self.v, self.s, self.m, self.z, self.g, self.lb = (cols(a, dt) for a in self.np)
        self.ctx = bj.context(self.v.device)
        self.lib = bj._lib.load()
        self.code = bj._lib.BJX_F32 if dt == F32 else bj._lib.BJX_F64

    def empty(self, *shape):
        return torch.full(shape, float("nan"), dtype=TDT[self.dt], device="cuda")

    def bars(self):
        return [self.empty(self.N * self.L * self.dim), self.empty(self.N * self.dim) if self.s is not None else None,
                self.empty(self.N * self.dim) if self.m is not None else None]

    def map(self, inverse, x, out, ps, sm, flags=0, batch=None, L=None, dim=None, lds=None, v="v", s="s", m="m", code=None):
        p = self.bj.interface._ptr
        L_, dim_ = self.L if L is None else L, self.dim if dim is None else dim
        lv, ls, lm = lds or (self.dim * self.L, self.dim, self.dim)
        rc = self.lib.bjx_householder_cols(self.ctx.h, self.code if code is None else code, int(inverse), p(getattr(self, v) if v else None),
                                           p(getattr(self, s) if s else None), p(getattr(self, m) if m else None), lv, ls, lm, L_, p(x), p(out), p(ps), p(sm),
                                           dim_, self.N if batch is None else batch, flags)
        torch.cuda.synchronize()
        return rc

    def vjp(self, inverse, x, g, lb, xb, vb, sb, mb, batch=None, L=None, dim=None, lds=None, code=None, s="s", m="m"):
        p = self.bj.interface._ptr
        lv, ls, lm = lds or (self.dim * self.L, self.dim, self.dim)
        rc = self.lib.bjx_householder_cols_vjp(self.ctx.h, self.code if code is None else code, int(inverse), p(self.v), p(getattr(self, s) if s else None),
                                               p(getattr(self, m) if m else None), lv, ls, lm, self.L if L is None else L, p(x), p(g), p(lb), p(xb), p(vb),
                                               p(sb), p(mb), self.dim if dim is None else dim, self.N if batch is None else batch)
        torch.cuda.synchronize()
        return rc

    def mat(self, t):
        """flat device tensor -> (rows, N) numpy"""
        return host(t).reshape(self.N, -1).T

    def cube(self, t):
        """flat device tensor [dim, L, N] -> (dim·L, N) numpy in the row order of a (dim, L, N) array"""
        return host(t).reshape(self.N, self.L, -1).transpose(2, 1, 0).reshape(-1, self.N)


def accumulate_and_the_summed_log_det(bj):
    for dt, dim, L, N in ((F32, 8, 3, 300), (F64, 5, 2, 200), (F32, 260, 2, 9)):          # 3, 4 and 3 blocks: the summed log-det crosses blocks
        for inverse in (False, True):
            _accumulate_and_the_summed_log_det(bj, dt, dim, L, N, inverse)


def _accumulate_and_the_summed_log_det(bj, dt, dim, L, N, inverse):
    c = Call(bj, dt, dim, L, N, ("abi-acc", np.dtype(dt).name, dim, L, inverse))
    ref = RefAll(*c.np, inverse)
    what = f"bjx_householder_cols {np.dtype(dt).name} dim={dim} L={L} inv={inverse}"
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
    # without p_s: exact zeros, or left accumulated
    ps0 = c.empty(N)
    sm0 = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    assert c.map(inverse, c.z, out2, ps0, sm0, s=None) == 0
    assert not host(ps0).any() and float(host(sm0)[0]) == 0.0, what + ": the log-det without p_s is not an exact zero"
    ps_acc, sm_acc = p0.clone(), torch.full((1,), 2.5, dtype=torch.float64, device="cuda")
    assert c.map(inverse, c.z, out2, ps_acc, sm_acc, s=None, flags=bj._lib.BJX_ACCUMULATE) == 0
    assert torch.equal(ps_acc, p0) and float(host(sm_acc)[0]) == 2.5


def in_place_calls_give_the_same_bits(bj):
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
        xb, bars = c.empty(N * dim), c.bars()
        assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars) == 0
        gbuf, bars2 = c.g.clone(), c.bars()
        assert c.vjp(inverse, c.z, gbuf, c.lb, gbuf, *bars2) == 0
        assert torch.equal(gbuf, xb) and all(torch.equal(s, t) for s, t in zip(bars, bars2)), f"in_bar == out_bar differs (dim={dim} inverse={inverse})"
        xb0 = c.empty(N * dim)                                   # ladj_bar = NULL is a zero cotangent
        assert c.vjp(inverse, c.z, c.g, None, xb0, None, None, None) == 0
        xbz = c.empty(N * dim)
        assert c.vjp(inverse, c.z, c.g, torch.zeros_like(c.lb), xbz, None, None, None) == 0
        assert torch.equal(xb0, xbz)


def null_cotangent_outputs_in_every_combination(bj):
    for dt, dim, L, N in ((F32, 5, 3, 130), (F64, 64, 2, 20), (F64, 257, 1, 5)):
        for inverse in (False, True):
            _null_cotangent_outputs_in_every_combination(bj, dt, dim, L, N, inverse)


def _null_cotangent_outputs_in_every_combination(bj, dt, dim, L, N, inverse):
    c = Call(bj, dt, dim, L, N, ("abi-null", np.dtype(dt).name, dim))
    full = c.bars()
    xb = c.empty(N * dim)
    assert c.vjp(inverse, c.z, c.g, c.lb, xb, *full) == 0
    what = f"bjx_householder_cols_vjp {np.dtype(dt).name} dim={dim} L={L} inv={inverse}"
    ref = RefAll(*c.np, inverse)
    flat_close(c.mat(xb), ref.in_bar, dt, what + " input cotangent")
    for name, got, r in zip(("v", "log_scale", "shift"), full, (ref.vb, ref.sb, ref.mb)):
        flat_close(c.cube(got) if name == "v" else c.mat(got), r.reshape(-1, N), dt, f"{what} {name} cotangent", term_scale=ref.scale)
    for want in itertools.product((True, False), repeat=3):
        if all(want):
            continue
        outs = [c.empty(t.numel()) if w_ else None for t, w_ in zip(full, want)]
        xb2 = c.empty(N * dim)
        assert c.vjp(inverse, c.z, c.g, c.lb, xb2, *outs) == 0
        assert torch.equal(xb2, xb), f"{what}: the input cotangent changes with outputs {want}"
        for o, f_ in zip(outs, full):
            assert o is None or torch.equal(o, f_), f"{what}: a cotangent changes with outputs {want}"


def absent_scale_and_shift(bj, head):
    """p_s and / or p_m NULL (their ld's are then ignored: a nonsense value is passed), dim 8 (vector form) and 5 (element form), both
    directions: the values, the input cotangent and the cotangents of the present parameters."""
    for dt, dim in ((F32, 8), (F64, 5)):
        L, N = 2, 70
        c = Call(bj, dt, dim, L, N, ("abi-head", np.dtype(dt).name, dim, head), head)
        lds = (dim * L, dim if c.s is not None else -7, dim if c.m is not None else -7)
        for inverse in (False, True):
            ref = RefAll(*c.np, inverse)
            what = f"bjx_householder_cols {np.dtype(dt).name} dim={dim} head={head} inv={inverse}"
            out, ps = c.empty(N * dim), c.empty(N)
            assert c.map(inverse, c.z, out, ps, None, lds=lds, s="s" if c.s is not None else None, m="m" if c.m is not None else None) == 0
            flat_close(c.mat(out), ref.out, dt, what + " values")
            flat_close(host(ps), ref.ladj, dt, what + " ladj", per="element", floor=1.0)
            xb, bars = c.empty(N * dim), c.bars()
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, lds=lds, s="s" if c.s is not None else None, m="m" if c.m is not None else None) == 0
            flat_close(c.mat(xb), ref.in_bar, dt, what + " input cotangent")
            for name, got, r in zip(("v", "log_scale", "shift"), bars, (ref.vb, ref.sb, ref.mb)):
                assert (got is None) == (r is None)
                if got is not None:
                    flat_close(c.cube(got) if name == "v" else c.mat(got), r.reshape(-1, N), dt, f"{what} {name} cotangent", term_scale=ref.scale)


def batch_zero(bj):
    c = Call(bj, F32, 4, 2, 3, ("abi-empty",))
    sm = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    out = c.empty(12)
    assert c.map(False, c.z, out, None, sm, batch=0) == 0
    assert float(host(sm)[0]) == 0.0 and bool(torch.isnan(out).all())
    sm.fill_(7.0)
    assert c.map(True, c.z, out, None, sm, batch=0, flags=bj._lib.BJX_ACCUMULATE) == 0 and float(host(sm)[0]) == 7.0
    assert c.map(False, None, None, None, None, batch=0, v=None, s=None, m=None) == 0         # nothing to read: null pointers are fine
    xb, bars = c.empty(12), c.bars()
    for inverse in (False, True):
        assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, batch=0) == 0
    assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars)


def refusals_happen_before_any_launch(bj):
    Lb = bj._lib
    for dt, lim in ((F32, 1024), (F64, 512)):
        c = Call(bj, dt, 4, 2, 6, ("abi-refuse", np.dtype(dt).name))
        out, ps = c.empty(24), c.empty(6)
        sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
        xb, bars = c.empty(24), c.bars()
        err = lambda: (Lb.load().bjx_last_error(c.ctx.h) or b"").decode()
        for inverse in (False, True):
            # layers outside 1 ... 64 and dim above the limit: UNSUPPORTED
            for L in (0, 65):
                assert c.map(inverse, c.z, out, ps, sm, L=L, lds=(4 * 65, 4, 4)) == Lb.ERR_UNSUPPORTED and "64" in err()
                assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, L=L, lds=(4 * 65, 4, 4)) == Lb.ERR_UNSUPPORTED and "64" in err()
            big = ((lim + 1) * 2, lim + 1, lim + 1)
            assert c.map(inverse, c.z, out, ps, sm, dim=lim + 1, lds=big) == Lb.ERR_UNSUPPORTED and str(lim) in err()
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, dim=lim + 1, lds=big) == Lb.ERR_UNSUPPORTED and str(lim) in err()
            # strides below the minimum, dim < 1, batch < 0: SHAPE
            for lds in ((7, 4, 4), (8, 3, 4), (8, 4, 3)):
                assert c.map(inverse, c.z, out, ps, sm, lds=lds) == Lb.ERR_SHAPE
                assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, lds=lds) == Lb.ERR_SHAPE
            assert c.map(inverse, c.z, out, ps, sm, dim=0) == Lb.ERR_SHAPE and c.map(inverse, c.z, out, ps, sm, batch=-1) == Lb.ERR_SHAPE
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, dim=0) == Lb.ERR_SHAPE and c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, batch=-1) == Lb.ERR_SHAPE
            # null required pointers with batch > 0, a bad dtype, a cotangent output of an absent parameter: ARG
            assert c.map(inverse, c.z, out, ps, sm, v=None) == Lb.ERR_ARG
            assert c.map(inverse, None, out, ps, sm) == Lb.ERR_ARG and c.map(inverse, c.z, None, ps, sm) == Lb.ERR_ARG
            assert c.map(inverse, c.z, out, ps, sm, code=77) == Lb.ERR_ARG
            assert c.vjp(inverse, None, c.g, c.lb, xb, *bars) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, None, c.lb, xb, *bars) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, c.g, c.lb, None, *bars) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, code=77) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, s=None) == Lb.ERR_ARG
            assert c.vjp(inverse, c.z, c.g, c.lb, xb, *bars, m=None) == Lb.ERR_ARG
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ps).all()) and float(host(sm)[0]) == 3.0, "a refused call wrote something"
        assert bool(torch.isnan(xb).all()) and all(bool(torch.isnan(t).all()) for t in bars), "a refused call wrote something"
        assert c.vjp(True, c.z, c.g, c.lb, xb, *bars) == 0 and bool(torch.isfinite(xb).all()) and all(bool(torch.isfinite(t).all()) for t in bars)


def test_c_abi_contract(bj):
    accumulate_and_the_summed_log_det(bj)
    in_place_calls_give_the_same_bits(bj)
    null_cotangent_outputs_in_every_combination(bj)
    for head in HEADS:
        absent_scale_and_shift(bj, head)
    batch_zero(bj)
    refusals_happen_before_any_launch(bj)
