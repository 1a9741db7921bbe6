"""The shared Sylvester layer (`SylvesterLayer`, include/bjx_sylvester.h) through bijectors_amd and through the C entries against the
Float64 closed forms of tests/_sylvester_ref.py (held to central differences and to the per-column sibling's reference in
tests/test_host_sylvester.py), on tests/_tol.py's flat bar (1e-3 Float32 / 1e-6 Float64) with nothing multiplying it and no conditioned
bar: values, x̄ and ladj per="sample" (with floor=1.0 where a sample has ONE entry — dim 1, and the log-det, one number per column: a
column of one entry has no scale of its own; the inputs are unit-scale draws), each of q̄, r̄, r̃̄, b̄ per="tensor" with the reference's
`term_scale(n)` of the columns the call sums over.  No column is left out of any comparison.

Dispatcher edges by dim (V = 4 / 2 elements per 16-byte pack in Float32 / Float64, G lanes per column, R packs per lane): 1, 2, 3, 5
element form; 4, 8, 16, 64 vector form; 65 partial last pack; 260 / 256 R = 2; 261 / 257, 516, 765 / 384 the R = 4 kernels with dead
packs; 1 024 / 512 the limits — at M = 1, 2, 3, 5, 16 where M <= dim (MP = 1, 2, 4 and 8 with padded units, and 16), the batches
1, C − 1, C, C + 1 with C = 256/G columns per tile.  Where the LDS rule (BJX_SYLVESTER_LDS_BYTES(dim, M) <= 64 KiB) does not admit the
fused parameter pullback the host's chunked fallback answers, on the same bar.

Reduction edges, from the constants of bijectors.jl_amd/csrc/bjx_sylvester.hip — a tile is C = 256/G columns, the persistent grid of the
pullback is min(ceil(tiles / SYL_TILES_MIN), 4·CUs) blocks with SYL_TILES_MIN = 4, one Float64 partial per block, and the first fold
runs when there are more than SYL_FOLD_CHUNK = 32 partials:
  batch = 4·C            4 tiles, 1 block: the block walks four tiles and keeps its sums on chip between them
  batch = 12·C − 5       12 tiles, 3 blocks of 4 tiles each, the last tile ragged (C − 5 live columns)
  batch = 132·C − 3      132 tiles, 33 blocks > 32: two fold chunks (32 + 1 partials), so the first fold launch runs; ragged too
at dim 2 Float32 with M = 2 (G = 1), dim 64 Float32 with M = 16 (G = 16) and dim 5 Float64 with M = 3 (G = 4).

The file is named to collect after every existing GPU test file, so the ids of those files keep their positions in the collection.
Three test ids; their parts are plain functions called in turn (every failure names its part in the traceback and its dtype, dim, M
and batch in the message)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _sylvester_ref import (DIMS, F32, F64, REDUCTION_SHAPES, SYL_FOLD_CHUNK, SYL_TILES_MIN, Draw, RefShared, batches, edge_draws, lanes,  # noqa: E402
                            reduction_batches, rounded, seed)
from _tol import flat_close  # noqa: E402

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


def close_cols(got, ref, dt, what):
    return flat_close(got, ref, dt, what, per="sample", floor=1.0 if ref.shape[0] == 1 else 0.0)


def close_ladj(got, ref, dt, what):
    return close_cols(np.asarray(got).reshape(1, -1), np.asarray(ref).reshape(1, -1), dt, what)


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


def make_layer(bj, D, dt=None):
    dt = D.dt if dt is None else dt
    return bj.SylvesterLayer(dev2(D.Q, dt), dev2(D.R, dt), dev2(D.Rt, dt), dev1(D.b, dt))


def served(bj, dim, M):
    return bj._lib.sylvester_lds_bytes(dim, M) <= bj._lib.BJX_SYLVESTER_LDS_BUDGET


def check_all(bj, D, n, what, lib=None):
    """The map (out == in included), the log-dets per sample and summed, BJX_ACCUMULATE, vjp and vjp_params of the first n columns."""
    dt, ref = D.dt, D.ref
    layer = make_layer(bj, D)
    xd, gd, ld = dev2(D.z[:, :n], dt), dev2(D.g[:, :n], dt), dev1(D.lb[:n], dt)
    y, (l, tot) = bj.with_logabsdet_jacobian(layer, xd, per_sample="both")
    close_cols(host(y), ref.out[:, :n], dt, what + " values")
    close_ladj(host(l), ref.ladj[:n], dt, what + " ladj")
    assert tot.dtype == torch.float64
    flat_close(host(tot).reshape(1, 1), np.array([[ref.ladj[:n].sum()]]), dt, what + " summed ladj", per="sample", floor=1.0,
               term_scale=float(np.abs(ref.ladj[:n]).max()))
    buf = xd.clone()
    assert bj.transform_(layer, buf) is buf and torch.equal(buf, y), what + ": out == in"
    # BJX_ACCUMULATE through the C entry: the log-dets are added to what is there
    lib = bj._lib.load()
    ctx = bj.context(xd.device)
    q, r, rt, b = layer._tables(xd, D.dim)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ps, sm, out = torch.full((n,), 7.0, dtype=xd.dtype, device="cuda"), torch.full((1,), 3.0, dtype=torch.float64, device="cuda"), torch.empty_like(xd)
    assert lib.bjx_sylvester(ctx.h, 0 if dt == F32 else 1, p(q), p(r), p(rt), p(b), D.M, p(xd), p(out), p(ps), p(sm), D.dim, n, bj._lib.BJX_ACCUMULATE) == 0
    assert torch.equal(out, y), what + ": BJX_ACCUMULATE changed the values"
    close_ladj(host(ps) - 7.0, ref.ladj[:n], dt, what + " accumulated ladj")
    flat_close(host(sm).reshape(1, 1) - 3.0, np.array([[ref.ladj[:n].sum()]]), dt, what + " accumulated summed ladj", per="sample", floor=1.0,
               term_scale=float(np.abs(ref.ladj[:n]).max()))
    # pullbacks
    xb = bj.vjp(layer, xd, gd, ld)
    close_cols(host(xb), ref.in_bar[:, :n], dt, what + " vjp")
    xb2, grads = bj.vjp_params(layer, xd, gd, ld)
    assert torch.equal(xb, xb2), what + ": x̄ of vjp and of vjp_params differ in their bits"
    close_params(grads, ref.summed(n), ref.term_scale(n), dt, what)
    key = (tdt(dt), D.dim, D.M)
    assert (key in bj.interface._SYL_LDS_REFUSED) == (not served(bj, D.dim, D.M)), what + ": fallback taken where the LDS rule admits the shape, or not where it does not"


# ------------------------------------------------------------------ 1. kernels
def dispatcher_edges(bj, dt):
    for dim, M, N, key in edge_draws(dt):
        D = Draw(dt, dim, M, N, key)
        for n in batches(256 // lanes(dim, dt)):
            check_all(bj, D, n, f"sylvester {name(dt)} dim={dim} M={M} batch={n}")


def reduction_edges(bj):
    lib = bj._lib.load()
    for dt, dim, M in REDUCTION_SHAPES:
        Cc = 256 // lanes(dim, dt)
        ns = reduction_batches(Cc)
        assert -(-(-(-ns[2] // Cc)) // SYL_TILES_MIN) == SYL_FOLD_CHUNK + 1 and ns[1] % Cc and ns[2] % Cc
        D = Draw(dt, dim, M, max(ns), ("sylvester-shared-reduce", name(dt), dim))
        for n in ns:
            check_all(bj, D, n, f"sylvester reduction {name(dt)} dim={dim} M={M} batch={n}")
        layer = make_layer(bj, D)
        for n, want in ((ns[0], 2), (ns[2], 3)):      # the fold path is three launches, the short one two; never more
            xd, gd = dev2(D.z[:, :n], dt), dev2(D.g[:, :n], dt)
            before = lib.bjx_launch_count()
            bj.vjp_params(layer, xd, gd)
            assert lib.bjx_launch_count() - before == want, f"sylvester reduction {name(dt)} dim={dim} M={M} batch={n}: {lib.bjx_launch_count() - before} launches"


def special_inputs(bj):
    for dt in (F32, F64):
        dim, M, n = 8, 3, 45
        D = Draw(dt, dim, M, n, ("sylvester-shared-negdet", name(dt)), negdet=True)
        assert (D.ref.d[0] < 0).any() and (D.ref.d[0] > 0).any()
        check_all(bj, D, n, f"sylvester negative determinant {name(dt)} dim={dim} M={M} batch={n}")
        # NaN below the diagonals: bit-equal to the same call with zeros there
        dim, M, n = 12, 3, 70
        D = Draw(dt, dim, M, n, ("sylvester-shared-nan-low", name(dt)))
        what = f"sylvester NaN below the diagonals {name(dt)} dim={dim} M={M} batch={n}"
        low = np.tril(np.ones((M, M)), -1) > 0
        outs = []
        for fill in (np.nan, 0.0):
            R, Rt = D.R.copy(), D.Rt.copy()
            R[low], Rt[low] = fill, fill
            layer = bj.SylvesterLayer(dev2(D.Q, dt), dev2(R, dt), dev2(Rt, dt), dev1(D.b, dt))
            xd, gd, ld = dev2(D.z, dt), dev2(D.g, dt), dev1(D.lb, dt)
            y, l = bj.with_logabsdet_jacobian(layer, xd, per_sample=True)
            xb, grads = bj.vjp_params(layer, xd, gd, ld)
            outs.append([y, l, xb, bj.vjp(layer, xd, gd, ld)] + [grads[k] for k in KEYS])
        for a, b_ in zip(*outs):
            assert torch.isfinite(a).all() and torch.equal(a, b_), what
        close_params(dict(zip(KEYS, outs[0][4:])), D.ref.summed(n), D.ref.term_scale(n), dt, what)
        # a NaN column in `in`: its own y and x̄ are NaN, the other columns are untouched, the summed cotangents are NaN
        D = Draw(dt, dim, M, n, ("sylvester-shared-nan-col", name(dt)))
        what = f"sylvester NaN column {name(dt)} dim={dim} M={M} batch={n}"
        z = D.z.copy()
        bad = n // 2
        z[1, bad] = np.nan
        ref = RefShared(D.Q, D.R, D.Rt, D.b, z, D.g, D.lb)
        layer = make_layer(bj, D)
        xd, gd, ld = dev2(z, dt), dev2(D.g, dt), dev1(D.lb, dt)
        y, l = bj.with_logabsdet_jacobian(layer, xd, per_sample=True)
        assert np.isnan(host(y)[:, bad]).all() and np.isnan(host(l)[bad]), what
        close_cols(host(y), ref.out, dt, what + " values")
        close_ladj(host(l), ref.ladj, dt, what + " ladj")
        xb, grads = bj.vjp_params(layer, xd, gd, ld)
        assert np.isnan(host(xb)[:, bad]).all(), what
        close_cols(host(xb), ref.in_bar, dt, what + " input cotangent")
        close_params(grads, ref.summed(n), ref.term_scale(n), dt, what)
        assert np.isnan(host(grads["q"])).all() and np.isnan(host(grads["b"])).all() and np.isnan(host(grads["r"])[~low]).all(), what
        # a dead column of a ragged tile next to it does not leak: the first `bad` columns alone are finite
        xb, grads = bj.vjp_params(layer, dev2(z[:, :bad], dt), dev2(D.g[:, :bad], dt), dev1(D.lb[:bad], dt))
        close_params(grads, ref.summed(bad), float(np.nanmax(ref.scale_cols[:bad])), dt, what + " (the columns before it)")


def bit_equality(bj):
    for dt, dim, M, n in ((F32, 12, 3, 70), (F64, 12, 3, 70), (F32, 64, 16, 16 * 40 + 3), (F32, 2, 2, 256 * 5 + 1)):
        D = Draw(dt, dim, M, n, ("sylvester-shared-bits", name(dt))) if dim == 12 else Draw(dt, dim, M, n, ("sylvester-shared-reduce", name(dt), dim))
        what = f"sylvester bits {name(dt)} dim={dim} M={M} batch={n}"
        layer = make_layer(bj, D)
        xd, gd, ld = dev2(D.z[:, :n], dt), dev2(D.g[:, :n], dt), dev1(D.lb[:n], dt)
        xb1, g1 = bj.vjp_params(layer, xd, gd, ld)
        xb2, g2 = bj.vjp_params(layer, xd, gd, ld)
        assert torch.equal(xb1, xb2) and all(torch.equal(g1[k], g2[k]) for k in KEYS), what + ": two identical calls differ"
        assert torch.equal(xb1, bj.vjp(layer, xd, gd, ld)), what + ": x̄ of vjp and of vjp_params differ"


def test_shared_sylvester_kernels(bj):
    for dt in (F32, F64):
        dispatcher_edges(bj, dt)
    reduction_edges(bj)
    special_inputs(bj)
    bit_equality(bj)


# ------------------------------------------------------------------ 2. host class
def shorthand_and_launch_counts(bj):
    lib = bj._lib.load()
    D = Draw(F64, 5, 1, 9, ("sylvester-shared-vector",))
    for r_shape in ((), (1,), (1, 1)):
        shaped = lambda a, shape: dev1(a.reshape(-1), F64).reshape(shape)      # (np.ascontiguousarray would make a 0-d array 1-d)
        one = bj.SylvesterLayer(dev1(D.Q[:, 0], F64), shaped(D.R, r_shape), shaped(D.Rt, r_shape), shaped(D.b, r_shape[:1]))
        xb, grads = bj.vjp_params(one, dev2(D.z, F64), dev2(D.g, F64), dev1(D.lb, F64))
        assert grads["q"].shape == (5,) and grads["r"].shape == r_shape and grads["r_tilde"].shape == r_shape and grads["b"].shape == r_shape[:1]
        close_cols(host(xb), D.ref.in_bar, F64, "sylvester M = 1 shorthand input cotangent")
        close_params({k: grads[k].reshape(s.shape) for k, s in zip(KEYS, D.ref.summed(9))}, D.ref.summed(9), D.ref.term_scale(9), F64, "sylvester M = 1 shorthand")
    yv, lv = bj.with_logabsdet_jacobian(one, dev1(D.z[:, 1], F64))
    assert yv.shape == (5,)
    close_cols(host(yv).reshape(5, 1), D.ref.out[:, 1:2], F64, "sylvester vector input values")
    close_ladj(host(torch.as_tensor(lv)).reshape(1), D.ref.ladj[1:2], F64, "sylvester vector input ladj")
    for dt, dim, M, n in ((F32, 12, 3, 70), (F64, 12, 3, 70)):
        D = Draw(dt, dim, M, n, ("sylvester-shared-bits", name(dt)))
        layer = make_layer(bj, D)
        xd, gd = dev2(D.z, dt), dev2(D.g, dt)
        what = f"sylvester launches {name(dt)}"
        for call, want in ((lambda: bj.transform(layer, xd), 1), (lambda: bj.with_logabsdet_jacobian(layer, xd, per_sample=True), 1),
                           (lambda: bj.with_logabsdet_jacobian(layer, xd, per_sample="both"), 2), (lambda: bj.logabsdetjac(layer, xd), None),
                           (lambda: bj.vjp(layer, xd, gd, 0.5), 1), (lambda: bj.vjp_params(layer, xd, gd, 0.5), 2)):
            before = lib.bjx_launch_count()
            call()
            k = lib.bjx_launch_count() - before
            assert (k == want) if want is not None else (1 <= k <= 2), (what, k, want)
        close_ladj(host(bj.logabsdetjac(layer, xd)), D.ref.ladj, dt, what + " logabsdetjac")
        buf = xd.clone()
        yb_, lj = bj.with_logabsdet_jacobian_(layer, buf)
        assert yb_ is buf and torch.equal(buf, bj.transform(layer, xd)), what


def composition_and_stack(bj, orc):
    dt, dim, M, n = F64, 6, 3, 50
    D = Draw(dt, dim, M, n, ("sylvester-shared-route",))
    layer = make_layer(bj, D)
    xd, gd, ld = dev2(D.z, dt), dev2(D.g, dt), dev1(D.lb, dt)
    what = f"sylvester routing {name(dt)} dim={dim} M={M} batch={n}"
    # Shift ∘ SylvesterLayer ∘ PlanarLayer: a parameter stage between two others, held to the references composed
    rng = seed("sylvester-shared-compose")
    w, u, b = rounded(rng.normal(size=dim) / 2, dt), rounded(rng.normal(size=dim) / 2, dt), rounded(rng.normal(size=1), dt)
    sh = rounded(rng.normal(size=dim), dt)
    comp = bj.Shift(dev1(sh, dt)) @ layer @ bj.PlanarLayer(dev1(w, dt), dev1(u, dt), dev1(b, dt))
    assert [type(s).__name__ for s in comp._plan()[0]][1:] == ["SylvesterLayer", "Shift"]
    mid, lmid = orc.planar(w, u, b, np.asfortranarray(D.z))
    mid = np.asarray(mid, np.float64)
    S = RefShared(D.Q, D.R, D.Rt, D.b, mid, D.g, D.lb)
    assert np.abs(S.d).min() >= 0.1, np.abs(S.d).min()
    y, l = bj.with_logabsdet_jacobian(comp, xd, per_sample=True)
    close_cols(host(y), S.out + sh[:, None], dt, what + " composition values")
    close_ladj(host(l), np.asarray(lmid, np.float64) + S.ladj, dt, what + " composition ladj")
    xb, grads = bj.vjp_params(comp, xd, gd, ld)
    assert set(grads) == {"stages"} and len(grads["stages"]) == 3, what
    close_params(grads["stages"][1], S.summed(n), S.term_scale(n), dt, what + " composition")
    close_cols(host(xb), orc.planar_vjp(w, u, b, D.z, S.in_bar, D.lb), dt, what + " composition input cotangent")
    wb, ub, bb = orc.planar_param_vjp(w, u, b, D.z, S.in_bar, D.lb)
    for k, r in (("w", wb), ("u", ub), ("b", bb)):
        flat_close(host(grads["stages"][0][k]).reshape(-1), np.asarray(r).reshape(-1), dt, f"{what} composition planar {k}", per="tensor")
    sg = grads["stages"][2]
    flat_close(host(sg["shift"] if isinstance(sg, dict) else sg).reshape(-1), D.g.sum(axis=1), dt, what + " composition shift", per="tensor", term_scale=float(np.abs(D.g).max()))
    close_cols(host(bj.vjp(comp, xd, gd, ld)), orc.planar_vjp(w, u, b, D.z, S.in_bar, D.lb), dt, what + " composition vjp")
    # a stack of two layers: l2 @ l1
    D2 = Draw(dt, dim, 2, n, ("sylvester-shared-route2",))
    l2 = make_layer(bj, D2)
    stack = l2 @ layer
    assert [type(s).__name__ for s in stack._plan()[0]] == ["SylvesterLayer", "SylvesterLayer"]
    S1 = RefShared(D.Q, D.R, D.Rt, D.b, D.z, D.g, D.lb)
    S2 = RefShared(D2.Q, D2.R, D2.Rt, D2.b, S1.out, D.g, D.lb)
    S1 = RefShared(D.Q, D.R, D.Rt, D.b, D.z, S2.in_bar, D.lb)
    assert min(np.abs(S1.d).min(), np.abs(S2.d).min()) >= 0.1
    y, l = bj.with_logabsdet_jacobian(stack, xd, per_sample=True)
    close_cols(host(y), S2.out, dt, what + " stack values")
    close_ladj(host(l), S1.ladj + S2.ladj, dt, what + " stack ladj")
    xb, grads = bj.vjp_params(stack, xd, gd, ld)
    close_cols(host(xb), S1.in_bar, dt, what + " stack input cotangent")
    close_params(grads["stages"][0], S1.summed(n), S1.term_scale(n), dt, what + " stack, first layer")
    close_params(grads["stages"][1], S2.summed(n), S2.term_scale(n), dt, what + " stack, second layer")


def agreement_with_the_per_column_sibling(bj):
    for dt, dim, M, n in ((F32, 12, 3, 70), (F64, 12, 3, 70)):
        D = Draw(dt, dim, M, n, ("sylvester-shared-bits", name(dt)))
        what = f"sylvester against the per-column layer {name(dt)} dim={dim} M={M} batch={n}"
        layer = make_layer(bj, D)
        q, r, rt, b = (t.reshape(s) for t, s in zip(layer._tables(dev2(D.z, dt), dim), ((dim, M), (M, M), (M, M), (M,))))
        sib = bj.AmortizedSylvesterLayer(q.unsqueeze(-1).expand(dim, M, n), r.unsqueeze(-1).expand(M, M, n), rt.unsqueeze(-1).expand(M, M, n), b.unsqueeze(-1).expand(M, n))
        xd, gd, ld = dev2(D.z, dt), dev2(D.g, dt), dev1(D.lb, dt)
        y, l = bj.with_logabsdet_jacobian(layer, xd, per_sample=True)
        ys, ls = bj.with_logabsdet_jacobian(sib, xd, per_sample=True)
        close_cols(host(y), host(ys).astype(np.float64), dt, what + " values")
        close_ladj(host(l), host(ls).astype(np.float64), dt, what + " ladj")
        xb, grads = bj.vjp_params(layer, xd, gd, ld)
        xs, gs = bj.vjp_params(sib, xd, gd, ld)
        close_cols(host(xb), host(xs).astype(np.float64), dt, what + " input cotangent")
        close_params(grads, [host(gs[k]).astype(np.float64).sum(axis=-1) for k in KEYS], D.ref.term_scale(n), dt, what)


def fallback_empty_batch_and_errors(bj):
    lb_ = bj._lib
    for dt, dim, fits in ((F32, 128, 13), (F64, 256, 7)):
        assert served(bj, dim, fits) and not served(bj, dim, fits + 1)
        for M in (fits, fits + 1):
            n = 256 // lanes(dim, dt) + 1
            D = Draw(dt, dim, M, n, ("sylvester-shared-lds", name(dt), dim, M))
            check_all(bj, D, n, f"sylvester LDS boundary {name(dt)} dim={dim} M={M} batch={n}")
            assert ((tdt(dt), dim, M) in bj.interface._SYL_LDS_REFUSED) == (M > fits)
    for dt in (F32, F64):
        D = Draw(dt, 12, 3, 70, ("sylvester-shared-bits", name(dt)))
        layer = make_layer(bj, D)
        e = torch.empty((0, 12), dtype=tdt(dt), device="cuda").T
        y, l = bj.with_logabsdet_jacobian(layer, e, per_sample=True)
        assert y.shape == (12, 0) and l.shape == (0,)
        assert bj.vjp(layer, e, e).shape == (12, 0)
        exb, eg = bj.vjp_params(layer, e, e)
        assert exb.shape == (12, 0) and all(eg[k].shape == s.shape and not host(eg[k]).any() for k, s in zip(KEYS, D.ref.summed(0)))
    with pytest.raises(ValueError, match="16"):
        bj.SylvesterLayer(torch.zeros((32, 17), device="cuda"), torch.zeros((17, 17), device="cuda"), torch.zeros((17, 17), device="cuda"), torch.zeros(17, device="cuda"))
    with pytest.raises(ValueError, match="above dim 2"):
        bj.SylvesterLayer(torch.zeros((2, 3), device="cuda"), torch.zeros((3, 3), device="cuda"), torch.zeros((3, 3), device="cuda"), torch.zeros(3, device="cuda"))
    for t, lim in ((torch.float32, 1024), (torch.float64, 512)):
        one = torch.ones(1, dtype=t, device="cuda")
        big = bj.SylvesterLayer(torch.ones(lim + 1, dtype=t, device="cuda"), one, one, one)
        x = torch.zeros((1, lim + 1), dtype=t, device="cuda").T
        for call in (lambda: bj.transform(big, x), lambda: bj.vjp(big, x, x), lambda: bj.vjp_params(big, x, x)):
            with pytest.raises(ValueError, match=str(lim)):
                call()
    D = Draw(F64, 6, 3, 50, ("sylvester-shared-route",))
    layer = make_layer(bj, D)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((4, 7), dtype=torch.float64, device="cuda").T)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.vjp_params(layer, dev2(D.z, F64), dev2(D.g[:, :5], F64))
    for call in (lambda: bj.transform(bj.inverse(layer), dev2(D.z, F64)), lambda: bj.vjp_params(bj.inverse(layer), dev2(D.z, F64), dev2(D.g, F64))):
        with pytest.raises(NotImplementedError, match="inverse map is not built"):
            call()


def test_shared_sylvester_host_class(bj, orc):
    shorthand_and_launch_counts(bj)
    composition_and_stack(bj, orc)
    agreement_with_the_per_column_sibling(bj)
    fallback_empty_batch_and_errors(bj)


# ------------------------------------------------------------------ 3. the C entries called directly
def test_shared_sylvester_c_abi(bj):
    lib, lb_ = bj._lib.load(), bj._lib
    dim, M, n = 8, 2, 5
    D = Draw(F32, dim, M, n, ("sylvester-shared-abi",))
    Qd, Rd, Rtd, bd, xd, gd = dev2(D.Q, F32), dev2(D.R, F32), dev2(D.Rt, F32), dev1(D.b, F32), dev2(D.z, F32), dev2(D.g, F32)
    out = torch.empty_like(xd)
    qb, rb, rtb, bb = torch.empty((M, dim), device="cuda").T, torch.empty((M, M), device="cuda").T, torch.empty((M, M), device="cuda").T, torch.empty(M, device="cuda")
    ctx = bj.context(xd.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def fmap(ctx_=ctx.h, dt=0, q=Qd, r=Rd, rt=Rtd, b=bd, m=M, i=xd, o=out, d=dim, n_=n):
        return lib.bjx_sylvester(ctx_, dt, p(q), p(r), p(rt), p(b), m, p(i), p(o), None, None, d, n_, 0)

    def fvjp(ctx_=ctx.h, dt=0, q=Qd, r=Rd, rt=Rtd, b=bd, m=M, i=xd, gb=gd, xb=out, bars=(qb, rb, rtb, bb), d=dim, n_=n):
        return lib.bjx_sylvester_vjp_params(ctx_, dt, p(q), p(r), p(rt), p(b), m, p(i), p(gb), None, p(xb), *(p(t) for t in bars), d, n_)

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
    for mask in range(1, 15):                                       # a mixture of null and non-null cotangents
        bars = tuple(t if mask >> k & 1 else None for k, t in enumerate((qb, rb, rtb, bb)))
        assert fvjp(bars=bars) == lb_.ERR_ARG, mask
    assert fvjp(d=128, m=14) == lb_.ERR_UNSUPPORTED               # the LDS rule (the pointers are not read before it answers)
    assert b"LDS" in lib.bjx_last_error(ctx.h)
    assert lib.bjx_launch_count() == before, "a refusal launched a kernel"
    assert fvjp(d=128, m=14, bars=(None,) * 4, n_=0) == 0          # the plain input pullback is not subject to the LDS rule
    # the served calls and their launch counts
    for call, want in ((fmap, 1), (fvjp, 2), (lambda: fvjp(xb=None), 2), (lambda: fvjp(bars=(None,) * 4), 1), (lambda: fvjp(xb=gd.clone()), 2)):
        before = lib.bjx_launch_count()
        assert call() == 0
        assert lib.bjx_launch_count() - before == want, (want, lib.bjx_launch_count() - before)
    torch.cuda.synchronize()
    Z = RefShared(D.Q, D.R, D.Rt, D.b, D.z, D.g, None)            # ladj_bar = NULL reads as 0
    close_cols(host(out), Z.in_bar, F32, "sylvester C entry input cotangent, ladj_bar = NULL")
    close_params(dict(zip(KEYS, (qb, rb, rtb, bb))), Z.summed(n), Z.term_scale(n), F32, "sylvester C entry, ladj_bar = NULL")
    # in_bar == out_bar, and in_bar has the same bits whether or not the parameter cotangents are asked for
    alias = gd.clone()
    assert fvjp(gb=alias, xb=alias) == 0
    plain = torch.empty_like(xd)
    assert fvjp(xb=plain, bars=(None,) * 4) == 0
    assert torch.equal(alias, out) and torch.equal(plain, out)
    # batch == 0 zeroes the cotangents and ladj_sum and launches nothing
    for t in (qb, rb, rtb, bb):
        t.fill_(float("nan"))
    sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    before = lib.bjx_launch_count()
    assert fvjp(n_=0) == 0 and fvjp(n_=0, i=None, gb=None, xb=None) == 0
    assert lib.bjx_sylvester(ctx.h, 0, p(Qd), p(Rd), p(Rtd), p(bd), M, None, None, None, p(sm), dim, 0, 0) == 0
    assert lib.bjx_launch_count() == before
    assert float(sm) == 0.0 and not any(host(t).any() for t in (qb, rb, rtb, bb))
    sm.fill_(3.0)
    assert lib.bjx_sylvester(ctx.h, 0, p(Qd), p(Rd), p(Rtd), p(bd), M, None, None, None, p(sm), dim, 0, lb_.BJX_ACCUMULATE) == 0 and float(sm) == 3.0
    # unaligned base pointers (the element form) give the values of the aligned call on the bar
    for dt in (F32, F64):
        dim, M, n = 12, 3, 70
        D = Draw(dt, dim, M, n, ("sylvester-shared-unaligned", name(dt)))
        code = 0 if dt == F32 else 1

        def flat(a, shift):                                         # a dense column-major copy as a flat buffer, aligned or one element past
            f = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T).reshape(-1)).cuda()
            buf = torch.empty(f.numel() + 4, dtype=tdt(dt), device="cuda")
            out = buf[shift:shift + f.numel()]
            out.copy_(f)
            assert (out.data_ptr() % 16 != 0) == bool(shift)
            return out

        R_, Rt_, b_ = dev2(D.R, dt), dev2(D.Rt, dt), dev1(D.b, dt)
        lbd = dev1(D.lb, dt)
        res = []
        for mk in (lambda a: flat(a, 0), lambda a: flat(a, 1)):
            q_, x_, g_ = mk(D.Q), mk(D.z), mk(D.g)
            o_, xb_ = mk(np.zeros((dim, n))), mk(np.zeros((dim, n)))
            ps = torch.empty(n, dtype=tdt(dt), device="cuda")
            bars = [torch.empty(k, dtype=tdt(dt), device="cuda") for k in (dim * M, M * M, M * M, M)]
            assert lib.bjx_sylvester(ctx.h, code, p(q_), p(R_), p(Rt_), p(b_), M, p(x_), p(o_), p(ps), None, dim, n, 0) == 0
            assert lib.bjx_sylvester_vjp_params(ctx.h, code, p(q_), p(R_), p(Rt_), p(b_), M, p(x_), p(g_), p(lbd), p(xb_), *(p(t) for t in bars), dim, n) == 0
            torch.cuda.synchronize()
            res.append([host(o_).reshape(n, dim).T, host(ps), host(xb_).reshape(n, dim).T, host(bars[0]).reshape(M, dim).T,
                        host(bars[1]).reshape(M, M).T, host(bars[2]).reshape(M, M).T, host(bars[3])])
        what = f"sylvester unaligned pointers {name(dt)}"
        for k, (al, un) in enumerate(zip(*res)):
            assert np.array_equal(al, un), f"{what}: output {k} depends on the form"
        al = res[1]
        close_cols(al[0], D.ref.out, dt, what + " values")
        close_ladj(al[1], D.ref.ladj, dt, what + " ladj")
        close_cols(al[2], D.ref.in_bar, dt, what + " input cotangent")
        for got, ref, k in zip(al[3:], D.ref.summed(n), KEYS):
            flat_close(got, ref, dt, f"{what} cotangent of {k}", per="tensor", term_scale=D.ref.term_scale(n))
