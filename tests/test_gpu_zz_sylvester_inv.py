"""The inverse of the shared Sylvester layer (`SylvesterLayer(..., orthonormal=True)`, include/bjx_sylvester_inv.h) through bijectors_amd and
through the C entries against the Float64 reference of tests/_sylvester_inv_ref.py (held to the forward reference, to the transposed
Jacobian and to central differences over a dense solve in tests/test_host_sylvester_inv.py), on tests/_tol.py's flat bar (1e-3 Float32 /
1e-6 Float64) with nothing multiplying it and no conditioned bar: z, ȳ and ladj per="sample" (floor=1.0 where a sample has ONE entry),
each of q̄, r̄, r̃̄, b̄ per="tensor" with the reference's `term_scale(n)` of the columns the call sums over.  No column is left out.

The data y of a draw is the layer's image of a unit-scale z (the sibling's draws: every d >= 0.19), rounded to the tested dtype.
Dispatcher edges: every dim of `DIMS[dt]` (element and vector form, R = 1, 2, 4, dead packs, the limits) at M = 1, 2, 3, 5, 16 where
M <= dim (MP = 1, 2, 4, 8 with padded units, 16), the batches C − 1, C, C + 1 with C = 256/G columns per tile.

The near-singular draws (k_0 = −1 + 2⁻¹⁰, t_0 within ±0.05: min d ≈ 1e-3) assert the RESIDUAL on the flat bar: the forward reference at
the returned z gives y back on y's per-column scale and minus the returned log-det; ȳ carries 1/d² there and is not compared.

The file is named to collect after every existing GPU test file.  Its parts are plain functions called in turn (every failure names
its part in the traceback and its dtype, dim, M and batch in the message)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _sylvester_inv_ref import InvDraw, RefInv  # noqa: E402
from _sylvester_ref import DIMS, UNITS, RefShared, batches, draws, lanes, seed  # noqa: E402, F401
from _tol import flat_close  # noqa: E402

F32, F64 = np.float32, np.float64
KEYS = ("q", "r", "r_tilde", "b")


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def dev2(a, dt):
    """(rows, n) numpy -> cuda tensor with the column-major layout of the library."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def name(dt):
    return np.dtype(dt).name


def tdt(dt):
    return torch.float32 if dt == F32 else torch.float64


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def close_cols(got, ref, dt, what):
    return flat_close(got, ref, dt, what, per="sample", floor=1.0 if ref.shape[0] == 1 else 0.0)


def close_ladj(got, ref, dt, what):
    return close_cols(np.asarray(got).reshape(1, -1), np.asarray(ref).reshape(1, -1), dt, what)


def close_sum(got, ref_ladj, dt, what):
    return flat_close(host(got).reshape(1, 1), np.array([[ref_ladj.sum()]]), dt, what, per="sample", floor=1.0, term_scale=float(np.abs(ref_ladj).max()))


def close_params(grads, sums, ts, dt, what):
    assert set(grads) == set(KEYS), (what, sorted(grads))
    for k, ref in zip(KEYS, sums):
        got = host(grads[k])
        assert got.shape == ref.shape, (what, k, got.shape, ref.shape)
        flat_close(got, ref, dt, f"{what} cotangent of {k}", per="tensor", term_scale=ts)
    for k in ("r", "r_tilde"):
        g = host(grads[k])
        if g.ndim == 2:
            low = np.tril(np.ones(g.shape), -1) > 0
            assert not g[low].any() and not np.signbit(g[low]).any(), f"{what}: the strict lower triangle of the cotangent of {k} is not exact zeros"


def make_layer(bj, D, R=None, Rt=None):
    dt = D.dt
    return bj.SylvesterLayer(dev2(D.Q, dt), dev2(D.R if R is None else R, dt), dev2(D.Rt if Rt is None else Rt, dt), dev1(D.b, dt), orthonormal=True)


def served(bj, dim, M):
    return bj._lib.sylvester_lds_bytes(dim, M) <= bj._lib.BJX_SYLVESTER_LDS_BUDGET


def check_all(bj, D, n, what):
    """The inverse map (out == in included), the log-dets per sample and summed, BJX_ACCUMULATE, the round trip, vjp, `pre` and vjp_params
    of the first n columns."""
    dt, ref = D.dt, D.ref
    layer = make_layer(bj, D)
    inv = bj.inverse(layer)
    yd, gd, ld = dev2(D.y[:, :n], dt), dev2(D.g[:, :n], dt), dev1(D.lb[:n], dt)
    z, (l, tot) = bj.with_logabsdet_jacobian(inv, yd, per_sample="both")
    close_cols(host(z), ref.out[:, :n], dt, what + " values")
    close_ladj(host(l), ref.ladj[:n], dt, what + " ladj")
    assert tot.dtype == torch.float64
    close_sum(tot, ref.ladj[:n], dt, what + " summed ladj")
    buf = yd.clone()
    assert bj.transform_(inv, buf) is buf and torch.equal(buf, z), what + ": out == in"
    # the round trip inverse(layer)(layer(z)) against z
    back = bj.transform(inv, bj.transform(layer, dev2(D.z[:, :n], dt)))
    close_cols(host(back), D.z[:, :n], dt, what + " round trip")
    # BJX_ACCUMULATE through the C entry: the log-dets are added to what is there
    lib = bj._lib.load()
    ctx = bj.context(yd.device)
    q, r, rt, b = layer._tables(yd, D.dim)
    code = 0 if dt == F32 else 1
    ps, sm, out = torch.full((n,), 7.0, dtype=yd.dtype, device="cuda"), torch.full((1,), 3.0, dtype=torch.float64, device="cuda"), torch.empty_like(yd)
    assert lib.bjx_sylvester_inv(ctx.h, code, p(q), p(r), p(rt), p(b), D.M, p(yd), p(out), p(ps), p(sm), D.dim, n, bj._lib.BJX_ACCUMULATE) == 0
    assert torch.equal(out, z), what + ": BJX_ACCUMULATE changed the values"
    close_ladj(host(ps) - 7.0, ref.ladj[:n], dt, what + " accumulated ladj")
    flat_close(host(sm).reshape(1, 1) - 3.0, np.array([[ref.ladj[:n].sum()]]), dt, what + " accumulated summed ladj", per="sample", floor=1.0,
               term_scale=float(np.abs(ref.ladj[:n]).max()))
    # pullbacks
    yb = bj.vjp(inv, yd, gd, ld)
    close_cols(host(yb), ref.in_bar[:, :n], dt, what + " vjp")
    yb_c, pre = torch.empty_like(yd), torch.empty_like(yd)
    assert lib.bjx_sylvester_inv_vjp(ctx.h, code, p(q), p(r), p(rt), p(b), D.M, p(yd), p(gd), p(ld), p(yb_c), p(pre), D.dim, n) == 0
    assert torch.equal(pre, z), what + ": pre does not have the bits of the map"
    assert torch.equal(yb_c, yb), what + ": ȳ depends on whether pre is asked for"
    yb2, grads = bj.vjp_params(inv, yd, gd, ld)
    assert torch.equal(yb, yb2), what + ": ȳ of vjp and of vjp_params differ in their bits"
    close_params(grads, ref.summed(n), ref.term_scale(n), dt, what)
    key = (tdt(dt), D.dim, D.M)
    assert (key in bj.interface._SYL_LDS_REFUSED) == (not served(bj, D.dim, D.M)), what + ": fallback taken where the LDS rule admits the shape, or not where it does not"


# ------------------------------------------------------------------ 1. kernels
def dispatcher_edges(bj, dt):
    for dim in DIMS[dt]:
        for M in UNITS:
            if M > dim:
                continue
            ns = batches(256 // lanes(dim, dt))
            D = InvDraw(dt, dim, M, max(ns), ("sylvester-inv", name(dt), dim, M))
            assert np.abs(D.ref.d).min() >= 0.19
            for n in ns:
                check_all(bj, D, n, f"sylvester inverse {name(dt)} dim={dim} M={M} batch={n}")


def zero_diagonals(bj):
    for dt in (F32, F64):
        D = InvDraw(dt, 8, 3, 45, ("sylvester-inv-zero-diag", name(dt)), recipe="zero-diag")
        assert D.R[2, 2] == 0.0 and D.Rt[1, 1] == 0.0
        check_all(bj, D, 45, f"sylvester inverse zero diagonals {name(dt)} dim=8 M=3 batch=45")


def near_singular(bj):
    for dt in (F32, F64):
        for dim, M in ((8, 3), (64, 16)):
            n = 64
            D = InvDraw(dt, dim, M, n, ("sylvester-inv-singular", name(dt), dim), recipe="singular")
            what = f"sylvester inverse near-singular {name(dt)} dim={dim} M={M} batch={n}"
            assert 2e-4 <= np.abs(D.ref.d).min() <= 4e-3, (what, np.abs(D.ref.d).min())
            layer = make_layer(bj, D)
            z, l = bj.with_logabsdet_jacobian(bj.inverse(layer), dev2(D.y, dt), per_sample=True)
            F = RefShared(D.Q, D.R, D.Rt, D.b, host(z).astype(np.float64), D.g)       # the forward reference at the returned z
            worst = close_cols(F.out, D.y, dt, what + " residual")
            print(f"{what}: residual {worst:.3g} of the column scale, z within {np.abs(host(z) - D.ref.out).max():.3g}")
            close_ladj(-F.ladj, host(l).astype(np.float64), dt, what + " log-det residual")


def nan_handling(bj):
    for dt in (F32, F64):
        dim, M, n = 12, 3, 70
        D = InvDraw(dt, dim, M, n, ("sylvester-inv-nan", name(dt)))
        what = f"sylvester inverse NaN {name(dt)} dim={dim} M={M} batch={n}"
        yd, gd, ld = dev2(D.y, dt), dev2(D.g, dt), dev1(D.lb, dt)
        low = np.tril(np.ones((M, M)), -1) > 0
        outs = []
        for fill in (np.nan, 0.0):
            R, Rt = D.R.copy(), D.Rt.copy()
            R[low], Rt[low] = fill, fill
            inv = bj.inverse(make_layer(bj, D, R, Rt))
            z, l = bj.with_logabsdet_jacobian(inv, yd, per_sample=True)
            yb, grads = bj.vjp_params(inv, yd, gd, ld)
            outs.append([z, l, yb, bj.vjp(inv, yd, gd, ld)] + [grads[k] for k in KEYS])
        for a, b_ in zip(*outs):
            assert torch.isfinite(a).all() and torch.equal(a, b_), what + ": NaN below the diagonals changed a bit"
        clean = outs[1]
        inv = bj.inverse(make_layer(bj, D))
        bad = n // 2
        keep = torch.ones(n, dtype=torch.bool, device="cuda")
        keep[bad] = False
        # a NaN in one column of y: z, ladj and ȳ of that column are NaN, every other column keeps its bits
        y2 = D.y.copy()
        y2[1, bad] = np.nan
        z, l = bj.with_logabsdet_jacobian(inv, dev2(y2, dt), per_sample=True)
        yb = bj.vjp(inv, dev2(y2, dt), gd, ld)
        assert torch.isnan(z[:, bad]).all() and torch.isnan(l[bad]) and torch.isnan(yb[:, bad]).all(), what + ": NaN column of y"
        assert torch.equal(z[:, keep], clean[0][:, keep]) and torch.equal(l[keep], clean[1][keep]) and torch.equal(yb[:, keep], clean[2][:, keep]), what + ": a NaN of y left its column"
        # a NaN in one column of z̄: ȳ of that column is NaN, every other column keeps its bits
        g2 = D.g.copy()
        g2[3, bad] = np.nan
        yb = bj.vjp(inv, yd, dev2(g2, dt), ld)
        assert torch.isnan(yb[:, bad]).all() and torch.equal(yb[:, keep], clean[2][:, keep]), what + ": a NaN of z̄ left its column"


def bit_equality(bj):
    lib = bj._lib.load()
    for dt in (F32, F64):
        dim, M, n = 12, 3, 70
        D = InvDraw(dt, dim, M, n, ("sylvester-inv-bits", name(dt)))
        what = f"sylvester inverse bits {name(dt)} dim={dim} M={M} batch={n}"
        code = 0 if dt == F32 else 1
        layer = make_layer(bj, D)
        inv = bj.inverse(layer)
        yd, gd, ld = dev2(D.y, dt), dev2(D.g, dt), dev1(D.lb, dt)
        z1, l1 = bj.with_logabsdet_jacobian(inv, yd, per_sample=True)
        z2, l2 = bj.with_logabsdet_jacobian(inv, yd, per_sample=True)
        yb1, g1 = bj.vjp_params(inv, yd, gd, ld)
        yb2, g2 = bj.vjp_params(inv, yd, gd, ld)
        assert torch.equal(z1, z2) and torch.equal(l1, l2) and torch.equal(yb1, yb2) and all(torch.equal(g1[k], g2[k]) for k in KEYS), what + ": two identical calls differ"
        assert torch.equal(yb1, bj.vjp(inv, yd, gd, ld)), what + ": ȳ of vjp and of vjp_params differ"
        # in_bar == out_bar through the C entry
        ctx = bj.context(yd.device)
        q, r, rt, b = layer._tables(yd, dim)
        alias = gd.clone()
        assert lib.bjx_sylvester_inv_vjp(ctx.h, code, p(q), p(r), p(rt), p(b), M, p(yd), p(alias), p(ld), p(alias), None, dim, n) == 0
        assert torch.equal(alias, yb1), what + ": in_bar == out_bar"
        # base pointers one element past a 16-byte boundary (the element form) against the dense call
        def flat(a, shift):
            f = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T).reshape(-1)).cuda()
            buf = torch.empty(f.numel() + 4, dtype=tdt(dt), device="cuda")
            out = buf[shift:shift + f.numel()]
            out.copy_(f)
            assert (out.data_ptr() % 16 != 0) == bool(shift)
            return out

        res = []
        for shift in (0, 1):
            q_, y_, g_ = flat(D.Q, shift), flat(D.y, shift), flat(D.g, shift)
            o_, yb_, pre_ = (flat(np.zeros((dim, n)), shift) for _ in range(3))
            ps = torch.empty(n, dtype=tdt(dt), device="cuda")
            assert lib.bjx_sylvester_inv(ctx.h, code, p(q_), p(r), p(rt), p(b), M, p(y_), p(o_), p(ps), None, dim, n, 0) == 0
            assert lib.bjx_sylvester_inv_vjp(ctx.h, code, p(q_), p(r), p(rt), p(b), M, p(y_), p(g_), p(ld), p(yb_), p(pre_), dim, n) == 0
            torch.cuda.synchronize()
            res.append([host(o_).reshape(n, dim).T, host(ps), host(yb_).reshape(n, dim).T, host(pre_).reshape(n, dim).T])
        for k, (al, un) in enumerate(zip(*res)):
            assert np.array_equal(al, un), f"{what}: output {k} depends on the form"
        assert np.array_equal(res[0][0], host(z1)) and np.array_equal(res[0][2], host(yb1)) and np.array_equal(res[0][3], host(z1)), what
        close_cols(res[1][0], D.ref.out, dt, what + " unaligned values")
        close_ladj(res[1][1], D.ref.ladj, dt, what + " unaligned ladj")
        close_cols(res[1][2], D.ref.in_bar, dt, what + " unaligned input cotangent")


def test_sylvester_inverse_kernels_float32(bj):
    dispatcher_edges(bj, F32)


def test_sylvester_inverse_kernels_float64(bj):
    dispatcher_edges(bj, F64)


def test_sylvester_inverse_special_inputs_and_bits(bj):
    zero_diagonals(bj)
    near_singular(bj)
    nan_handling(bj)
    bit_equality(bj)


# ------------------------------------------------------------------ 2. host class
def launch_counts_and_shapes(bj):
    lib = bj._lib.load()
    for dt in (F32, F64):
        dim, M, n = 12, 3, 70
        D = InvDraw(dt, dim, M, n, ("sylvester-inv-bits", name(dt)))
        inv = bj.inverse(make_layer(bj, D))
        yd, gd = dev2(D.y, dt), dev2(D.g, dt)
        what = f"sylvester inverse launches {name(dt)}"
        for call, want in ((lambda: bj.transform(inv, yd), 1), (lambda: bj.with_logabsdet_jacobian(inv, yd, per_sample=True), 1),
                           (lambda: bj.with_logabsdet_jacobian(inv, yd, per_sample="both"), 2), (lambda: bj.logabsdetjac(inv, yd), None),
                           (lambda: bj.vjp(inv, yd, gd, 0.5), 1), (lambda: bj.vjp_params(inv, yd, gd, 0.5), 3)):
            before = lib.bjx_launch_count()
            call()
            k = lib.bjx_launch_count() - before
            assert (k == want) if want is not None else (1 <= k <= 2), (what, k, want)
        close_ladj(host(bj.logabsdetjac(inv, yd)), D.ref.ladj, dt, what + " logabsdetjac")
        buf = yd.clone()
        zb_, lj = bj.with_logabsdet_jacobian_(inv, buf)
        assert zb_ is buf and torch.equal(buf, bj.transform(inv, yd)), what
        # a vector input and the M = 1 shorthand shapes
        zv, lv = bj.with_logabsdet_jacobian(inv, dev1(D.y[:, 1], dt))
        assert zv.shape == (dim,)
        close_cols(host(zv).reshape(dim, 1), D.ref.out[:, 1:2], dt, what + " vector input values")
        close_ladj(host(torch.as_tensor(lv)).reshape(1), D.ref.ladj[1:2], dt, what + " vector input ladj")
        e = torch.empty((0, dim), dtype=tdt(dt), device="cuda").T
        z0, l0 = bj.with_logabsdet_jacobian(inv, e, per_sample=True)
        assert z0.shape == (dim, 0) and l0.shape == (0,) and bj.vjp(inv, e, e).shape == (dim, 0)
        eyb, eg = bj.vjp_params(inv, e, e)
        assert eyb.shape == (dim, 0) and all(not host(eg[k]).any() for k in KEYS)
    D = InvDraw(F64, 5, 1, 9, ("sylvester-inv-vector",))
    one = bj.SylvesterLayer(dev1(D.Q[:, 0], F64), dev1(D.R.reshape(-1), F64), dev1(D.Rt.reshape(-1), F64), dev1(D.b, F64), orthonormal=True)
    yb, grads = bj.vjp_params(bj.inverse(one), dev2(D.y, F64), dev2(D.g, F64), dev1(D.lb, F64))
    assert grads["q"].shape == (5,) and grads["r"].shape == (1,) and grads["r_tilde"].shape == (1,) and grads["b"].shape == (1,)
    close_cols(host(yb), D.ref.in_bar, F64, "sylvester inverse M = 1 shorthand input cotangent")
    close_params({k: grads[k].reshape(s.shape) for k, s in zip(KEYS, D.ref.summed(9))}, D.ref.summed(9), D.ref.term_scale(9), F64, "sylvester inverse M = 1 shorthand")


def lds_fallback(bj):
    for dt, dim, M in ((F32, 128, 14), (F64, 256, 8)):
        assert not served(bj, dim, M)
        n = 256 // lanes(dim, dt) + 1
        D = InvDraw(dt, dim, M, n, ("sylvester-inv-lds", name(dt), dim, M))
        check_all(bj, D, n, f"sylvester inverse over the LDS rule {name(dt)} dim={dim} M={M} batch={n}")
        assert (tdt(dt), dim, M) in bj.interface._SYL_LDS_REFUSED


def log_density(bj):
    dt, dim, M, n = F64, 6, 3, 50
    D = InvDraw(dt, dim, M, n, ("sylvester-inv-logpdf",))
    what = f"sylvester logpdf {name(dt)} dim={dim} M={M} batch={n}"
    rng = seed("sylvester-inv-logpdf-base")
    mu, sigma = rng.normal(size=dim), np.exp(0.3 * rng.normal(size=dim))
    layer = make_layer(bj, D)
    td = bj.transformed(bj.MvNormal(dev1(mu, dt), dev1(sigma, dt)), layer)
    yd = dev2(D.y, dt)
    I = RefInv(D.Q, D.R, D.Rt, D.b, D.y, D.g)
    w = (I.out - mu[:, None]) / sigma[:, None]
    lp_ref = -0.5 * (w * w).sum(axis=0) - np.log(sigma).sum() - 0.5 * dim * np.log(2 * np.pi) + I.ladj
    flat_close(host(bj.logpdf(td, yd)), lp_ref, dt, what, per="element", floor=1.0)
    c = D.lb
    G = RefInv(D.Q, D.R, D.Rt, D.b, D.y, -c[None, :] * w / sigma[:, None], c)     # x̄ = −c·w/σ, ℓ̄ = c
    lp, yb, grads = bj.logpdf_vjp_params(td, yd, dev1(c, dt))
    flat_close(host(lp), lp_ref, dt, what + " (with gradients)", per="element", floor=1.0)
    close_cols(host(yb), G.in_bar, dt, what + " input cotangent")
    close_params(grads["transform"], G.summed(n), G.term_scale(n), dt, what)
    mg = c[None, :] * w / sigma[:, None]
    flat_close(host(grads["base"]["mu"]), mg.sum(axis=1), dt, what + " cotangent of mu", per="tensor", term_scale=float(np.abs(mg).max()))
    sg = mg * w - c[None, :] / sigma[:, None]
    flat_close(host(grads["base"]["sigma"]), sg.sum(axis=1), dt, what + " cotangent of sigma", per="tensor", term_scale=float(np.abs(sg).max()))
    lp2, yb2, none = bj.logpdf_vjp_params(td, yd, dev1(c, dt), params=False)
    assert none == {} and torch.equal(lp2, lp) and torch.equal(yb2, yb), what + ": params=False"
    # a layer that does not declare an orthonormal q still refuses
    plain = bj.SylvesterLayer(dev2(D.Q, dt), dev2(D.R, dt), dev2(D.Rt, dt), dev1(D.b, dt))
    with pytest.raises(NotImplementedError, match="inverse map is not built"):
        bj.logpdf(bj.transformed(bj.MvNormal(dim), plain), yd)


def composition(bj):
    dt, dim, n = F64, 6, 50
    D1 = InvDraw(dt, dim, 3, n, ("sylvester-inv-route",))
    D2 = InvDraw(dt, dim, 2, n, ("sylvester-inv-route2",))
    l1, l2 = make_layer(bj, D1), make_layer(bj, D2)
    what = f"sylvester inverse of a stack {name(dt)} dim={dim} batch={n}"
    both = bj.inverse(l2 @ l1)
    yd, gd, ld = dev2(D1.y, dt), dev2(D1.g, dt), dev1(D1.lb, dt)
    # inverse(l2 ∘ l1) = inverse(l1) ∘ inverse(l2): the references in sequence
    A = RefInv(D2.Q, D2.R, D2.Rt, D2.b, D1.y, D1.g, D1.lb)
    B = RefInv(D1.Q, D1.R, D1.Rt, D1.b, A.out, D1.g, D1.lb)
    A = RefInv(D2.Q, D2.R, D2.Rt, D2.b, D1.y, B.in_bar, D1.lb)
    assert min(np.abs(A.d).min(), np.abs(B.d).min()) >= 0.1
    z, l = bj.with_logabsdet_jacobian(both, yd, per_sample=True)
    close_cols(host(z), B.out, dt, what + " values")
    close_ladj(host(l), A.ladj + B.ladj, dt, what + " ladj")
    step = bj.transform(bj.inverse(l1), bj.transform(bj.inverse(l2), yd))
    close_cols(host(z), host(step).astype(np.float64), dt, what + " against the two inverses in sequence")
    close_cols(host(bj.vjp(both, yd, gd, ld)), A.in_bar, dt, what + " vjp")
    yb, grads = bj.vjp_params(both, yd, gd, ld)
    close_cols(host(yb), A.in_bar, dt, what + " input cotangent")
    assert set(grads) == {"stages"} and len(grads["stages"]) == 2, what
    close_params(grads["stages"][0], A.summed(n), A.term_scale(n), dt, what + ", inverse(l2)")
    close_params(grads["stages"][1], B.summed(n), B.term_scale(n), dt, what + ", inverse(l1)")


def test_sylvester_inverse_host_class(bj):
    launch_counts_and_shapes(bj)
    lds_fallback(bj)
    log_density(bj)
    composition(bj)


# ------------------------------------------------------------------ 3. the C entries called directly
def test_sylvester_inverse_c_abi(bj):
    lib, lb_ = bj._lib.load(), bj._lib
    dim, M, n = 8, 2, 5
    D = InvDraw(F32, dim, M, n, ("sylvester-inv-abi",))
    Qd, Rd, Rtd, bd, yd, gd = dev2(D.Q, F32), dev2(D.R, F32), dev2(D.Rt, F32), dev1(D.b, F32), dev2(D.y, F32), dev2(D.g, F32)
    out, pre = torch.empty_like(yd), torch.empty_like(yd)
    ctx = bj.context(yd.device)

    def fmap(ctx_=ctx.h, dt=0, q=Qd, r=Rd, rt=Rtd, b=bd, m=M, i=yd, o=out, d=dim, n_=n):
        return lib.bjx_sylvester_inv(ctx_, dt, p(q), p(r), p(rt), p(b), m, p(i), p(o), None, None, d, n_, 0)

    def fvjp(ctx_=ctx.h, dt=0, q=Qd, r=Rd, rt=Rtd, b=bd, m=M, i=yd, gb=gd, xb=out, pr=pre, d=dim, n_=n):
        return lib.bjx_sylvester_inv_vjp(ctx_, dt, p(q), p(r), p(rt), p(b), m, p(i), p(gb), None, p(xb), p(pr), d, n_)

    before = lib.bjx_launch_count()
    for f in (fmap, fvjp):
        assert f(ctx_=None) == lb_.ERR_ARG
        assert f(dt=2) == lb_.ERR_ARG
        assert f(m=0) == lb_.ERR_UNSUPPORTED and f(m=17) == lb_.ERR_UNSUPPORTED
        assert f(m=9) == lb_.ERR_UNSUPPORTED                      # M > dim
        assert f(d=0) == lb_.ERR_SHAPE and f(n_=-1) == lb_.ERR_SHAPE
        assert f(d=1025) == lb_.ERR_UNSUPPORTED and f(dt=1, d=513) == lb_.ERR_UNSUPPORTED
        for k in ("q", "r", "rt", "b", "i"):
            assert f(**{k: None}) == lb_.ERR_ARG, k
    assert fmap(o=None) == lb_.ERR_ARG
    assert fvjp(gb=None) == lb_.ERR_ARG
    assert lib.bjx_launch_count() == before, "a refusal launched a kernel"
    # batch == 0 launches nothing; ladj_sum is zeroed unless BJX_ACCUMULATE is set
    sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    assert fmap(n_=0) == 0 and fmap(n_=0, i=None, o=None) == 0 and fvjp(n_=0) == 0 and fvjp(n_=0, i=None, gb=None, xb=None, pr=None) == 0
    assert lib.bjx_sylvester_inv(ctx.h, 0, p(Qd), p(Rd), p(Rtd), p(bd), M, None, None, None, p(sm), dim, 0, 0) == 0
    assert fvjp(xb=None, pr=None) == 0                             # nothing asked for
    assert lib.bjx_launch_count() == before
    assert float(sm) == 0.0
    sm.fill_(3.0)
    assert lib.bjx_sylvester_inv(ctx.h, 0, p(Qd), p(Rd), p(Rtd), p(bd), M, None, None, None, p(sm), dim, 0, lb_.BJX_ACCUMULATE) == 0 and float(sm) == 3.0
    # the served calls and their launch counts
    for call, want in ((fmap, 1), (fvjp, 1), (lambda: fvjp(pr=None), 1), (lambda: fvjp(xb=None), 1), (lambda: fvjp(xb=gd.clone()), 1)):
        before = lib.bjx_launch_count()
        assert call() == 0
        assert lib.bjx_launch_count() - before == want, (want, lib.bjx_launch_count() - before)
    ps = torch.empty(n, device="cuda")
    before = lib.bjx_launch_count()
    assert lib.bjx_sylvester_inv(ctx.h, 0, p(Qd), p(Rd), p(Rtd), p(bd), M, p(yd), p(out), p(ps), p(sm), dim, n, 0) == 0
    assert lib.bjx_launch_count() - before == 2                   # the summed log-det: the map and the fixed-order reduction
    torch.cuda.synchronize()
    Z = RefInv(D.Q, D.R, D.Rt, D.b, D.y, D.g, None)               # ladj_bar = NULL reads as 0
    close_cols(host(out), Z.out, F32, "sylvester inverse C entry values")
    close_ladj(host(ps), Z.ladj, F32, "sylvester inverse C entry ladj")
    close_sum(sm, Z.ladj, F32, "sylvester inverse C entry summed ladj")
    assert fvjp() == 0
    torch.cuda.synchronize()
    close_cols(host(out), Z.in_bar, F32, "sylvester inverse C entry input cotangent, ladj_bar = NULL")
    close_cols(host(pre), Z.out, F32, "sylvester inverse C entry pre")
