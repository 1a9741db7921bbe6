"""The shared Householder layer (`HouseholderLayer`, include/bjx_householder.h) through bijectors_amd and through the C entries against the
Float64 closed forms of tests/_householder_ref.py (held to dense matrices, slogdet, central differences and the per-column sibling's
reference in tests/test_host_householder.py), on tests/_tol.py's flat bar (1e-3 Float32 / 1e-6 Float64) with nothing multiplying it:
values and x̄ per="sample" (with floor=1.0 at dim 1: a column of one entry has no scale of its own; the inputs are unit-scale draws),
v̄ per="tensor" one layer at a time with the reference's `term_scale` of the columns the call sums over.  No column is left out of any
comparison.

Dispatcher edges by dim (V = 4 / 2 elements per 16-byte pack in Float32 / Float64, G lanes per column, R packs per lane): the table of
tests/test_gpu_householder_cols.py — 1, 2, 3, 5 element form; 4, 8, 16, 64 vector form; 65 partial last pack; 260 / 256 R = 2;
261 / 257, 516, 765 / 384 the R = 4 kernels with dead packs; 1 024 / 512 the limits — at L = 1, 2, 8, both directions, the batches
1, C − 1, C, C + 1 with C = 256/G columns per tile.  Where the LDS rule (BJX_HOUSEHOLDER_LDS_BYTES(dim, L) <= 64 KiB) does not admit the
fused parameter pullback the host's chunked fallback answers, on the same bar.

Reduction edges, from the constants of bijectors.jl_amd/csrc/bjx_householder.hip — a tile is C = 256/G columns, the persistent grid of
the pullback is min(ceil(tiles / HH_TILES_MIN), 4·CUs) blocks with HH_TILES_MIN = 4, one Float64 partial per block, and the first fold
runs when there are more than HH_FOLD_CHUNK = 32 partials:
  batch = 4·C            4 tiles, 1 block: the block walks four tiles and keeps its sums on chip between them
  batch = 12·C − 5       12 tiles, 3 blocks of 4 tiles each (tile = block + 3·i), the last tile ragged (C − 5 live columns)
  batch = 132·C − 3      132 tiles, 33 blocks > 32: two fold chunks (32 + 1 partials), so the second fold launch runs; ragged too
at dim 2 Float32 (G = 1, C = 256: the butterfly over 64 column groups of a wave), dim 64 Float32 (G = 16) and dim 5 Float64 (G = 4).

Long stack: L = 64 at dim 3 and dim 16, both dtypes, 70 columns, on the flat bar (the steps are orthogonal and the rewind is the
reflection itself; measured on an MI355X: Float32 within 3.0e-6 of every scale, Float64 within 6.7e-15; numpy Float32 of the same
operation order: 2e-6).

The file is named to collect after every existing GPU test file, so the ids of those files keep their positions in the collection.

The GPU suite is kept at its count of test ids, so everything here is ONE id: the parts below are plain functions called in turn
(every failure names its part in the traceback and its dtype, dim, L and batch in the message)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _householder_ref import RefShared, draws, rounded, seed  # noqa: E402
from _tol import flat_close  # noqa: E402

F32, F64 = np.float32, np.float64
DIMS = {F32: [1, 2, 3, 5, 4, 8, 16, 64, 65, 260, 261, 516, 765, 1024], F64: [1, 2, 3, 5, 4, 8, 16, 64, 65, 256, 257, 384, 512]}
HH_TILES_MIN, HH_FOLD_CHUNK = 4, 32


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


def dev2(a, dt):
    """(rows, n) numpy -> cuda tensor with the column-major layout of the library."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def name(dt):
    return np.dtype(dt).name


def close_cols(got, ref, dt, what):
    return flat_close(got, ref, dt, what, per="sample", floor=1.0 if ref.shape[0] == 1 else 0.0)


def close_vbar(got, ref_vb, term_scale, dt, what):
    assert got.shape == ref_vb.shape, (what, got.shape)
    for k in range(ref_vb.shape[1]):
        flat_close(got[:, k], ref_vb[:, k], dt, f"{what} v̄ of layer {k}", per="tensor", term_scale=float(term_scale[k]))


class Ref:
    """One draw and both directions' references, computed once; the parts slice its first n columns."""

    def __init__(self, dt, dim, L, N, key):
        self.dt, self.dim, self.L, self.N = dt, dim, L, N
        self.V, self.x, self.g = draws(seed(*key), dim, L, N, dt)
        self.F = RefShared(self.V, self.x, self.g)
        self.I = RefShared(self.V, self.x, self.g, inverse=True)


def check_all(bj, R, n, what):
    """Maps, log-dets, round trip and parameter pullbacks of the first n columns of the draw R, both directions."""
    dt = R.dt
    layer = bj.HouseholderLayer(dev2(R.V, dt))
    inv = bj.inverse(layer)
    xd, gd = dev2(R.x[:, :n], dt), dev2(R.g[:, :n], dt)
    y, l = bj.with_logabsdet_jacobian(layer, xd, per_sample=True)
    close_cols(host(y), R.F.out[:, :n], dt, what + " values")
    xi, li = bj.with_logabsdet_jacobian(inv, xd, per_sample=True)
    close_cols(host(xi), R.I.out[:, :n], dt, what + " inverse values")
    assert l.shape == (n,) and li.shape == (n,) and l.dtype == xd.dtype and not host(l).any() and not host(li).any(), what + ": the log-det is not exact zeros"
    close_cols(host(bj.transform(inv, y)), R.x[:, :n], dt, what + " round trip")
    for f, ref, d in ((layer, R.F, "forward"), (inv, R.I, "inverse")):
        xb, grads = bj.vjp_params(f, xd, gd)
        close_cols(host(xb), ref.in_bar[:, :n], dt, f"{what} {d} input cotangent")
        assert set(grads) == {"v"}, (what, sorted(grads))
        vb, ts = ref.summed(n)
        close_vbar(host(grads["v"]), vb, ts, dt, f"{what} {d}")


def batches(C):
    return sorted({n for n in (1, C - 1, C, C + 1) if n >= 1})


def dispatcher_edges(bj, dt):
    for L in (1, 2, 8):
        for dim in DIMS[dt]:
            ns = batches(256 // lanes(dim, dt))
            R = Ref(dt, dim, L, max(ns), ("shared", name(dt), dim, L))
            for n in ns:
                check_all(bj, R, n, f"householder {name(dt)} dim={dim} L={L} batch={n}")


def reduction_edges(bj):
    for dt, dim, L in ((F32, 2, 2), (F32, 64, 3), (F64, 5, 2)):
        Cc = 256 // lanes(dim, dt)
        ns = [HH_TILES_MIN * Cc, 3 * HH_TILES_MIN * Cc - 5, (HH_FOLD_CHUNK + 1) * HH_TILES_MIN * Cc - 3]
        assert -(-(-(-ns[2] // Cc)) // HH_TILES_MIN) == HH_FOLD_CHUNK + 1 and ns[1] % Cc and ns[2] % Cc
        R = Ref(dt, dim, L, max(ns), ("shared-reduce", name(dt), dim))
        for n in ns:
            check_all(bj, R, n, f"householder reduction {name(dt)} dim={dim} L={L} batch={n}")
        # the fold path is three launches, the short one two; never more
        lib = bj._lib.load()
        layer = bj.HouseholderLayer(dev2(R.V, dt))
        for n, want in ((ns[0], 2), (ns[2], 3)):
            xd, gd = dev2(R.x[:, :n], dt), dev2(R.g[:, :n], dt)
            before = lib.bjx_launch_count()
            bj.vjp_params(layer, xd, gd)
            assert lib.bjx_launch_count() - before == want, f"householder reduction {name(dt)} dim={dim} L={L} batch={n}: {lib.bjx_launch_count() - before} launches"


def long_stack(bj):
    for dt in (F32, F64):
        for dim in (3, 16):
            R = Ref(dt, dim, 64, 70, ("shared-long", name(dt), dim))
            check_all(bj, R, 70, f"householder {name(dt)} dim={dim} L=64 batch=70")


# ------------------------------------------------------------------ the C entries called directly
def c_params(bj, dt, inverse, V, x, g, *, in_bar="own", ladj_bar=None, v_ptr="own"):
    """bjx_householder_vjp_params on device copies -> (rc, launches, x̄ or None, v̄); in_bar: "own", "alias" (= out_bar) or None."""
    lib = bj._lib.load()
    dim, L = V.shape
    n = x.shape[1]
    Vd, xd, gd = dev2(V, dt), dev2(x, dt), dev2(g, dt)
    ctx = bj.context(xd.device)
    vb = torch.full((L, dim), float("nan"), dtype=xd.dtype, device="cuda").T
    xb = gd if in_bar == "alias" else (torch.full((max(n, 1), dim), float("nan"), dtype=xd.dtype, device="cuda").T[:, :n] if in_bar == "own" else None)
    lb = None if ladj_bar is None else dev1(ladj_bar, dt)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    before = lib.bjx_launch_count()
    rc = lib.bjx_householder_vjp_params(ctx.h, 0 if dt == F32 else 1, int(inverse), p(Vd) if v_ptr == "own" else None, L, p(xd), p(gd), p(lb), p(xb), p(vb), dim, n)
    launches = lib.bjx_launch_count() - before
    torch.cuda.synchronize()
    return rc, launches, xb, vb


def lds_boundary(bj):
    """At dim 64 and at the tallest dim: the largest L the fused pullback serves, and the first it refuses (BJX_ERR_UNSUPPORTED, nothing
    launched) — there the host's fallback returns the same dictionary on the same bar and remembers the shape."""
    lb_ = bj._lib
    for dt, dims in ((F32, (64, 1024)), (F64, (64, 512))):
        for dim in dims:
            Lmax = max(l for l in range(1, 65) if lb_.householder_lds_bytes(dim, l) <= lb_.BJX_HOUSEHOLDER_LDS_BUDGET)
            assert Lmax < 64 and lb_.householder_lds_bytes(dim, Lmax + 1) > lb_.BJX_HOUSEHOLDER_LDS_BUDGET
            n = 256 // lanes(dim, dt) + 1
            for L, served in ((Lmax, True), (Lmax + 1, False)):
                R = Ref(dt, dim, L, n, ("shared-lds", name(dt), dim, L))
                layer = bj.HouseholderLayer(dev2(R.V, dt))
                for inverse, ref in ((False, R.F), (True, R.I)):
                    what = f"householder LDS boundary {name(dt)} dim={dim} L={L} batch={n} inverse={inverse}"
                    rc, launches, xb, vb = c_params(bj, dt, inverse, R.V, R.x, R.g)
                    if served:
                        assert rc == 0 and 2 <= launches <= 3, (what, rc, launches)
                        close_cols(host(xb), ref.in_bar, dt, what + " input cotangent (C entry)")
                        close_vbar(host(vb), ref.vb, ref.term_scale, dt, what + " (C entry)")
                    else:
                        assert rc == lb_.ERR_UNSUPPORTED and launches == 0, (what, rc, launches)
                    xb, grads = bj.vjp_params(bj.inverse(layer) if inverse else layer, dev2(R.x, dt), dev2(R.g, dt))
                    assert set(grads) == {"v"}, what
                    close_cols(host(xb), ref.in_bar, dt, what + " input cotangent")
                    close_vbar(host(grads["v"]), ref.vb, ref.term_scale, dt, what)
                    key = (torch.float32 if dt == F32 else torch.float64, dim, L)
                    assert (key in bj.interface._HH_LDS_REFUSED) == (not served), what


def degenerate_cases(bj):
    for dt in (F32, F64):
        for dim in (3, 64):
            L, n = 3, 2 * (256 // lanes(dim, dt)) + 3
            what = f"householder {name(dt)} dim={dim} L={L} batch={n}"
            # v_1 == 0 exactly: that layer is the identity and its cotangent exactly 0
            V, x, g = draws(seed("shared-zero", name(dt), dim), dim, L, n, dt)
            V[:, 1] = 0.0
            layer = bj.HouseholderLayer(dev2(V, dt))
            for f, ref, d in ((layer, RefShared(V, x, g), "forward"), (bj.inverse(layer), RefShared(V, x, g, True), "inverse")):
                close_cols(host(bj.transform(f, dev2(x, dt))), ref.out, dt, f"{what} zero layer {d} values")
                xb, grads = bj.vjp_params(f, dev2(x, dt), dev2(g, dt))
                close_cols(host(xb), ref.in_bar, dt, f"{what} zero layer {d} input cotangent")
                vb = host(grads["v"])
                assert not vb[:, 1].any(), f"{what} {d}: the cotangent of the zero layer is not exactly 0"
                close_vbar(vb, ref.vb, ref.term_scale, dt, f"{what} zero layer {d}")
            # a NaN in one input column: its y is NaN and v̄ (a sum over the batch) is NaN; x̄ does not read x, and the log-det is 0
            V, x, g = draws(seed("shared-nan", name(dt), dim), dim, L, n, dt)
            bad = n // 2
            x[0, bad] = np.nan
            keep = np.arange(n) != bad
            layer = bj.HouseholderLayer(dev2(V, dt))
            for f, ref, d in ((layer, RefShared(V, x, g), "forward"), (bj.inverse(layer), RefShared(V, x, g, True), "inverse")):
                y, l = bj.with_logabsdet_jacobian(f, dev2(x, dt), per_sample=True)
                y = host(y)
                assert np.isnan(y[:, bad]).all() and not host(l).any(), f"{what} NaN column {d}"
                close_cols(y[:, keep], ref.out[:, keep], dt, f"{what} NaN column {d} values")
                xb, grads = bj.vjp_params(f, dev2(x, dt), dev2(g, dt))
                close_cols(host(xb), ref.in_bar, dt, f"{what} NaN column {d} input cotangent of every column")
                assert np.isnan(host(grads["v"])).all(), f"{what} NaN column {d}: v̄ is not NaN"


def semantics(bj):
    lib = bj._lib.load()
    for dt, dim, L, n in ((F32, 5, 2, 37), (F32, 64, 2, 40), (F64, 8, 3, 70)):
        what = f"householder semantics {name(dt)} dim={dim} L={L} batch={n}"
        R = Ref(dt, dim, L, n, ("shared-sem", name(dt), dim))
        layer = bj.HouseholderLayer(dev2(R.V, dt))
        Vd, xd = dev2(R.V, dt), dev2(R.x, dt)
        ctx = bj.context(xd.device)
        code = 0 if dt == F32 else 1
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        # log-dets: exact zeros, per column and summed; left untouched under BJX_ACCUMULATE; one launch; out == in
        for inverse, ref in ((0, R.F), (1, R.I)):
            y, (l, tot) = bj.with_logabsdet_jacobian(bj.inverse(layer) if inverse else layer, xd, per_sample="both")
            assert not host(l).any() and float(tot) == 0.0 and tot.dtype == torch.float64, what
            assert float(bj.logabsdetjac(bj.inverse(layer) if inverse else layer, xd).sum()) == 0.0, what
            ps, sm = torch.full((n,), 7.0, dtype=xd.dtype, device="cuda"), torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
            out = torch.empty_like(xd)
            before = lib.bjx_launch_count()
            assert lib.bjx_householder(ctx.h, code, inverse, p(Vd), L, p(xd), p(out), p(ps), p(sm), dim, n, bj._lib.BJX_ACCUMULATE) == 0
            assert lib.bjx_launch_count() - before == 1, what
            assert torch.equal(out, y) and (host(ps) == 7.0).all() and float(sm) == 3.0, what + ": BJX_ACCUMULATE"
            assert lib.bjx_householder(ctx.h, code, inverse, p(Vd), L, p(xd), p(out), p(ps), p(sm), dim, n, 0) == 0
            assert not host(ps).any() and float(sm) == 0.0, what
            same = xd.clone()
            assert lib.bjx_householder(ctx.h, code, inverse, p(Vd), L, p(same), p(same), None, None, dim, n, 0) == 0
            assert torch.equal(same, y), what + ": out == in"
            close_cols(host(y), ref.out, dt, what + " values")
        # in-place host forms
        buf = xd.clone()
        assert bj.transform_(layer, buf) is buf and torch.equal(buf, bj.transform(layer, xd)), what
        buf = xd.clone()
        yb_, lj = bj.with_logabsdet_jacobian_(layer, buf)
        assert yb_ is buf and torch.equal(buf, bj.transform(layer, xd)) and float(torch.as_tensor(lj).sum()) == 0.0, what
        close_cols(host(bj.inverse(layer)(layer(xd))), R.x, dt, what + " inverse(layer)(layer(x))")
        # the pullback's calling forms: all the same bits
        for inverse in (False, True):
            rc, k, xb, vb = c_params(bj, dt, inverse, R.V, R.x, R.g)
            assert rc == 0 and k == 2, (what, rc, k)
            rc2, _, xb2, vb2 = c_params(bj, dt, inverse, R.V, R.x, R.g)
            assert rc2 == 0 and torch.equal(xb, xb2) and torch.equal(vb, vb2), what + ": two identical calls differ"
            rc3, _, xb3, vb3 = c_params(bj, dt, inverse, R.V, R.x, R.g, in_bar="alias")
            assert rc3 == 0 and torch.equal(xb, xb3) and torch.equal(vb, vb3), what + ": in_bar == out_bar"
            rc4, _, _, vb4 = c_params(bj, dt, inverse, R.V, R.x, R.g, in_bar=None)
            assert rc4 == 0 and torch.equal(vb, vb4), what + ": in_bar = NULL"
            rc5, _, xb5, vb5 = c_params(bj, dt, inverse, R.V, R.x, R.g, ladj_bar=rounded(seed("lb").normal(size=n) + 2.0, dt))
            assert rc5 == 0 and torch.equal(xb, xb5) and torch.equal(vb, vb5), what + ": a non-zero ladj_bar changed an output"
            f = bj.inverse(layer) if inverse else layer
            hx, hg = bj.vjp_params(f, xd, dev2(R.g, dt), 1.5)
            assert torch.equal(hx, xb) and torch.equal(hg["v"], vb), what + ": host and C entry differ"
            # an empty batch: zeros, nothing launched
            rc6, k6, _, vb6 = c_params(bj, dt, inverse, R.V, R.x[:, :0], R.g[:, :0])
            assert rc6 == 0 and k6 == 0 and not host(vb6).any(), what + ": empty batch"
        sm = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
        before = lib.bjx_launch_count()
        assert lib.bjx_householder(ctx.h, code, 0, p(Vd), L, None, None, None, p(sm), dim, 0, 0) == 0 and lib.bjx_launch_count() == before and float(sm) == 0.0, what
        e = torch.empty((0, dim), dtype=xd.dtype, device="cuda").T
        assert bj.transform(layer, e).shape == (dim, 0), what
        exb, eg = bj.vjp_params(layer, e, e)
        assert exb.shape == (dim, 0) and eg["v"].shape == (dim, L) and not host(eg["v"]).any(), what
    # one layer given as a vector: its cotangent comes back in that shape
    R = Ref(F64, 5, 1, 9, ("shared-vector",))
    one = bj.HouseholderLayer(dev1(R.V[:, 0], F64))
    xb, grads = bj.vjp_params(one, dev2(R.x, F64), dev2(R.g, F64))
    assert grads["v"].shape == (5,)
    close_cols(host(xb), R.F.in_bar, F64, "householder one layer input cotangent")
    close_vbar(host(grads["v"]).reshape(5, 1), R.F.vb, R.F.term_scale, F64, "householder one layer")
    yv = bj.transform(one, dev1(R.x[:, 1], F64))
    assert yv.shape == (5,)
    close_cols(host(yv).reshape(5, 1), R.F.out[:, 1:2], F64, "householder vector input values")


def host_routing(bj, orc):
    dt, dim, L, n = F64, 6, 3, 50
    R = Ref(dt, dim, L, n, ("shared-route",))
    layer = bj.HouseholderLayer(dev2(R.V, dt))
    inv = bj.inverse(layer)
    xd, gd = dev2(R.x, dt), dev2(R.g, dt)
    what = f"householder routing {name(dt)} dim={dim} L={L} batch={n}"
    # vjp is the other direction's map of out_bar
    assert torch.equal(bj.vjp(layer, xd, gd, 0.5), bj.transform(inv, gd)) and torch.equal(bj.vjp(inv, xd, gd), bj.transform(layer, gd)), what
    close_cols(host(bj.vjp(layer, xd, gd)), R.F.in_bar, dt, what + " vjp")
    close_cols(host(bj.vjp(inv, xd, gd)), R.I.in_bar, dt, what + " vjp of the inverse")
    # Shift ∘ HouseholderLayer ∘ PlanarLayer: a parameter stage between two others, held to the references composed
    rng = seed("shared-compose")
    w, u, b = rounded(rng.normal(size=dim) / 2, dt), rounded(rng.normal(size=dim) / 2, dt), rounded(rng.normal(size=1), dt)
    sh = rounded(rng.normal(size=dim), dt)
    lbar = rounded(rng.normal(size=n), dt)
    comp = bj.Shift(dev1(sh, dt)) @ layer @ bj.PlanarLayer(dev1(w, dt), dev1(u, dt), dev1(b, dt))
    assert [type(s).__name__ for s in comp._plan()[0]][1:] == ["HouseholderLayer", "Shift"]
    mid, lmid = orc.planar(w, u, b, np.asfortranarray(R.x))
    mid = np.asarray(mid, np.float64)
    H = RefShared(R.V, mid, R.g)
    y, l = bj.with_logabsdet_jacobian(comp, xd, per_sample=True)
    close_cols(host(y), H.out + sh[:, None], dt, what + " composition values")
    flat_close(host(l), np.asarray(lmid, np.float64), dt, what + " composition ladj", per="element", floor=1.0)
    xb, grads = bj.vjp_params(comp, xd, gd, dev1(lbar, dt))
    assert set(grads) == {"stages"} and len(grads["stages"]) == 3 and set(grads["stages"][1]) == {"v"}, what
    close_vbar(host(grads["stages"][1]["v"]), H.vb, H.term_scale, dt, what + " composition")
    close_cols(host(xb), orc.planar_vjp(w, u, b, R.x, H.in_bar, lbar), dt, what + " composition input cotangent")
    wb, ub, bb = orc.planar_param_vjp(w, u, b, R.x, H.in_bar, lbar)
    for k, r in (("w", wb), ("u", ub), ("b", bb)):
        flat_close(host(grads["stages"][0][k]).reshape(-1), np.asarray(r).reshape(-1), dt, f"{what} composition planar {k}", per="tensor")
    sg = grads["stages"][2]
    flat_close(host(sg["shift"] if isinstance(sg, dict) else sg).reshape(-1), R.g.sum(axis=1), dt, what + " composition shift", per="tensor", term_scale=float(np.abs(R.g).max()))
    # logpdf of a transformed normal: the base density at the pre-image; its gradients are the inverse's parameter pullback
    td = bj.transformed(bj.MvNormal(dim), layer)
    lp_ref = -0.5 * (R.I.out ** 2).sum(axis=0) - 0.5 * dim * np.log(2 * np.pi)
    flat_close(host(bj.logpdf(td, xd)), lp_ref, dt, what + " logpdf", per="element", floor=1.0)
    lp, yb, G = bj.logpdf_vjp_params(td, xd)
    flat_close(host(lp), lp_ref, dt, what + " logpdf (with gradients)", per="element", floor=1.0)
    pre = bj.transform(inv, xd)
    wb_, wg = bj.vjp_params(inv, xd, -pre, 1.0)
    assert set(G["transform"]) == {"v"} and torch.equal(G["transform"]["v"], wg["v"]) and torch.equal(yb, wb_), what + ": logpdf_vjp_params"
    D = RefShared(R.V, R.x, -R.I.out, inverse=True)
    close_cols(host(yb), D.in_bar, dt, what + " logpdf input cotangent")
    close_vbar(host(G["transform"]["v"]), D.vb, D.term_scale, dt, what + " logpdf")
    # size refusals are ValueErrors naming the limit
    with pytest.raises(ValueError, match="64"):
        bj.HouseholderLayer(torch.zeros((3, 65), device="cuda"))
    for tdt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        big = bj.HouseholderLayer(torch.ones(lim + 1, dtype=tdt, device="cuda"))
        x = torch.zeros((1, lim + 1), dtype=tdt, device="cuda").T
        for call in (lambda: bj.transform(big, x), lambda: bj.transform(bj.inverse(big), x), lambda: bj.vjp(big, x, x), lambda: bj.vjp_params(big, x, x),
                     lambda: bj.vjp_params(bj.inverse(big), x, x)):
            with pytest.raises(ValueError, match=str(lim)):
                call()
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((4, dim + 1), dtype=torch.float64, device="cuda").T)


def c_abi_refusals(bj):
    """Every refusal code of include/bjx_householder.h, from both entries, with no launch on any of them."""
    lib, lb_ = bj._lib.load(), bj._lib
    dim, L, n = 8, 2, 5
    V, x, g = draws(seed("shared-abi"), dim, L, n, F32)
    Vd, xd, gd = dev2(V, F32), dev2(x, F32), dev2(g, F32)
    out, vb = torch.empty_like(xd), torch.empty((L, dim), dtype=xd.dtype, device="cuda").T
    ctx = bj.context(xd.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def fmap(ctx_=ctx.h, dt=0, v=Vd, nl=L, i=xd, o=out, d=dim, b=n):
        return lib.bjx_householder(ctx_, dt, 0, p(v), nl, p(i), p(o), None, None, d, b, 0)

    def fvjp(ctx_=ctx.h, dt=0, v=Vd, nl=L, i=xd, gb=gd, xb=out, vbar=vb, d=dim, b=n):
        return lib.bjx_householder_vjp_params(ctx_, dt, 1, p(v), nl, p(i), p(gb), None, p(xb), p(vbar), d, b)

    before = lib.bjx_launch_count()
    for f in (fmap, fvjp):
        assert f(ctx_=None) == lb_.ERR_ARG
        assert f(dt=2) == lb_.ERR_ARG
        assert f(nl=0) == lb_.ERR_UNSUPPORTED and f(nl=65) == lb_.ERR_UNSUPPORTED
        assert f(d=0) == lb_.ERR_SHAPE and f(b=-1) == lb_.ERR_SHAPE
        assert f(d=1025) == lb_.ERR_UNSUPPORTED and f(dt=1, d=513) == lb_.ERR_UNSUPPORTED
        assert f(v=None) == lb_.ERR_ARG and f(i=None) == lb_.ERR_ARG
    assert fmap(o=None) == lb_.ERR_ARG
    assert fvjp(gb=None) == lb_.ERR_ARG and fvjp(vbar=None) == lb_.ERR_ARG
    assert fvjp(d=64, nl=32) == lb_.ERR_UNSUPPORTED                 # the LDS rule (the pointers are not read before it answers)
    assert lib.bjx_launch_count() == before, "a refusal launched a kernel"
    assert b"LDS" in lib.bjx_last_error(ctx.h)
    assert fmap() == 0 and fvjp() == 0 and fvjp(xb=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the one test id
def test_shared_householder_layer_kernels_host_class_and_c_abi(bj, orc):
    c_abi_refusals(bj)
    for dt in (F32, F64):
        dispatcher_edges(bj, dt)
    reduction_edges(bj)
    long_stack(bj)
    lds_boundary(bj)
    degenerate_cases(bj)
    semantics(bj)
    host_routing(bj, orc)
