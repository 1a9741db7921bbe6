"""The numpy references of the C-ABI edge suites of csrc/bjx_elem.hip (tests/_elem_pullback_ref.py), checked on the CPU: the coupling
pullback against central differences of Σ ȳ·y + Σ ℓ̄·logabsdetjac through `oracle.coupling_affine` (Float64, h = 1e-6, the bar of
test_coupling_affine_vjp: 1e-5·max(1, |ref|)), and every reference output finite on every input the GPU files draw.  No GPU, no torch."""
import numpy as np
import pytest

import _elem_pullback_ref as R

H, BAR = 1e-6, 1e-5


def _loss(orc, idx1, s, t, x, g, lb, inverse):
    y, l = orc.coupling_affine(idx1, None if s is None else np.asfortranarray(s), None if t is None else np.asfortranarray(t), np.asfortranarray(x), inverse=inverse)
    return float((np.asarray(y, np.float64) * g).sum() + (np.asarray(l, np.float64) * lb).sum())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("mask", ["scattered", "range", "unsorted", "all"])
@pytest.mark.parametrize("nulls", ["", "scale", "shift", "scale+shift", "lbar"])
def test_coupling_reference_is_the_gradient_of_the_oracle(orc, inverse, mask, nulls):
    dim, batch = 7, 5
    d = R.draw_coupling("float64", dim, batch, 3, mask)
    idx1, x, g = d["idx1"], d["x"].copy(), d["gbar"]
    if mask == "unsorted":
        assert not (np.diff(idx1) > 0).all()
    n1 = len(idx1)
    s = None if "scale" in nulls else d["scale"].copy()
    t = None if "shift" in nulls else d["shift"].copy()
    lb = None if nulls == "lbar" else d["lbar"]
    lb0 = np.zeros(batch) if lb is None else lb
    xb, sb, tb = R.ref_coupling_affine_vjp(idx1, s, t, x, g, lb, inverse)
    assert xb.shape == (dim, batch) and sb.shape == (n1, batch) and tb.shape == (n1, batch)
    # a NULL scale / shift is the constant 1 / 0: its cotangent is the derivative at that constant
    s_full = np.ones((n1, batch)) if s is None else s
    t_full = np.zeros((n1, batch)) if t is None else t
    r = R.rng_for("fd", inverse, mask, nulls)

    def fd(arr, which, i, n):
        vals = []
        for sgn in (1.0, -1.0):
            a = arr.copy()
            a[i, n] += sgn * H
            args = {"x": (s_full, t_full, a), "s": (a, t_full, x), "t": (s_full, a, x)}[which]
            vals.append(_loss(orc, idx1, args[0], args[1], args[2], g, lb0, inverse))
        return (vals[0] - vals[1]) / (2 * H)

    for _ in range(6):
        i, n = int(r.integers(dim)), int(r.integers(batch))
        assert abs(fd(x, "x", i, n) - xb[i, n]) <= BAR * max(1.0, abs(xb[i, n])), ("x", i, n)
        k = int(r.integers(n1))
        assert abs(fd(s_full, "s", k, n) - sb[k, n]) <= BAR * max(1.0, abs(sb[k, n])), ("scale", k, n)
        assert abs(fd(t_full, "t", k, n) - tb[k, n]) <= BAR * max(1.0, abs(tb[k, n])), ("shift", k, n)
    # NULL parameters through the oracle's own NULL handling give the same loss
    assert _loss(orc, idx1, s, t, x, g, lb0, inverse) == pytest.approx(_loss(orc, idx1, s_full, t_full, x, g, lb0, inverse), rel=1e-14)


def test_empty_mask_passes_the_cotangent_through():
    d = R.draw_coupling("float64", 6, 4, 0, "none")
    xb, sb, tb = R.ref_coupling_affine_vjp(d["idx1"], None, None, d["x"], d["gbar"], d["lbar"], False)
    assert np.array_equal(xb, d["gbar"]) and sb.shape == (0, 4) and tb.shape == (0, 4)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_coupling_reference_is_finite_on_every_input_of_the_gpu_suite(dt):
    dt = np.dtype(dt)
    for dim, aligned in R.COUPLING_SHAPES[dt]:
        for batch in R.coupling_batches(dt, dim, aligned):
            for mask in R.MASKS:
                d = R.draw_coupling(dt.name, dim, batch, 0, mask)
                assert d["x"].dtype == dt and d["x"].shape == (dim, batch)
                a = np.abs(d["scale"])
                assert a.size == 0 or (a.min() >= 0.49 and a.max() <= 2.01)
                assert mask in ("all", "none") or dim == 1 or (d["scale"] < 0).any()
                for inverse in (False, True):
                    for out in R.ref_coupling_affine_vjp(d["idx1"], d["scale"], d["shift"], d["x"], d["gbar"], d["lbar"], inverse):
                        assert np.isfinite(out).all() and np.isfinite(out.astype(dt)).all(), (dim, batch, mask, inverse)


def _bn_finite(orc, d, dt, eps=R.EPS, center=0.0):
    x64 = np.asarray(d["x"], np.float64)
    for shift in (None, d["m0"]):
        s1, s2, n = R.ref_stats(x64, shift)
        assert np.isfinite(s1).all() and np.isfinite(s2).all() and n == x64.shape[1]
    if x64.shape[1] < 2:
        return
    y, l, m, v = orc.batchnorm_train(*(np.asarray(d[k], np.float64) for k in ("b", "logs", "m0", "v0")), eps, R.MTM, x64 - center)
    xb, bb, lgb = orc.batchnorm_train_vjp(np.asarray(d["logs"], np.float64), eps, x64 - center, d["g"], d["lb"])
    for out in (y, l, m, v, xb, bb, lgb):
        assert np.isfinite(out).all() and np.isfinite(np.asarray(out).astype(dt)).all()
    return y


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_batchnorm_references_are_finite_on_every_input_of_the_gpu_suite(orc, dt):
    dt = np.dtype(dt)
    for dim, aligned in R.STATS_SHAPES[dt]:
        for batch in R.stats_batches(dt, dim, aligned):
            d = R.draw_bn(dt.name, dim, batch)
            assert d["x"].dtype == dt and d["x"].shape == (dim, batch)
            if batch >= 2:       # every row has a spread of order one
                sd = np.asarray(d["x"], np.float64).std(axis=1)
                assert sd.min() > 0.49 and sd.max() < 1.51, (dim, batch)
            _bn_finite(orc, d, dt)
    for dim, aligned in R.LIFTED_SHAPES[dt]:
        for batch in R.LIFTED_BATCHES:
            _bn_finite(orc, R.draw_bn(dt.name, dim, batch), dt)
    for dim in R.VJP_DIMS[dt]:
        for batch in R.VJP_BATCHES:
            _bn_finite(orc, R.draw_bn(dt.name, dim, batch), dt)
    # the exactly constant row: variance 0 -> out == b, its log-det term -log(eps)/2
    d = R.draw_bn_constant_row(dt.name, 12, 33)
    y = _bn_finite(orc, d, dt)
    assert np.array_equal(y[d["row"]], np.full(33, np.float64(d["b"][d["row"]])))
    for dim in (8, 257):
        c = R.draw_bn_conditioned(dt.name, dim, 1000)
        _bn_finite(orc, c, dt, c["eps"], c["center"])


def test_forms_cover_the_kernel_branches():
    """The shapes of the GPU suite reach every template form of bn_stats_kernel and both pack widths of the coupling pullback."""
    f32 = {(d, a): R.stats_form(R.F32, d, a) for d, a in R.STATS_SHAPES[R.F32]}
    f64 = {(d, a): R.stats_form(R.F64, d, a) for d, a in R.STATS_SHAPES[R.F64]}
    assert f32[(1, True)] == (1, 1, 1) and f32[(5, True)] == (1, 8, 1) and f32[(64, True)] == (4, 16, 1) and f32[(100, True)] == (4, 32, 1)
    assert f32[(101, True)] == (1, 64, 2) and f32[(130, True)] == (1, 64, 4) and f32[(300, True)] == (4, 64, 2) and f32[(520, True)] == (4, 64, 4)
    assert f32[(1024, True)] == (4, 64, 4) and f32[(256, False)] == (1, 64, 4)
    assert f64[(3, True)] == (1, 4, 1) and f64[(64, True)] == (2, 32, 1) and f64[(129, True)] == (1, 64, 4) and f64[(130, True)] == (2, 64, 2)
    assert f64[(258, True)] == (2, 64, 4) and f64[(512, True)] == (2, 64, 4)
    assert {(v, r) for v, _, r in f32.values()} == {(1, 1), (1, 2), (1, 4), (4, 1), (4, 2), (4, 4)}
    for dt in (R.F32, R.F64):
        assert all(R.stats_form(dt, d, a)[2] == 0 for d, a in R.LIFTED_SHAPES[dt])
    assert [R.stats_launches(R.F32, d, a) for d, a in R.LIFTED_SHAPES[R.F32]] == [4, 4, 2, 4, 2]
    assert [R.stats_launches(R.F64, d, a) for d, a in R.LIFTED_SHAPES[R.F64]] == [4, 2, 2]
    assert R.stats_batches(R.F32, 1024) == [1, 2, 3, 5, 63, 65, 135, 259]
    cg = {(d, a): R.lanes(R.F32, d, a) for d, a in R.COUPLING_SHAPES[R.F32]}
    assert cg[(1, True)] == (1, 1) and cg[(3, True)] == (1, 4) and cg[(12, True)] == (4, 4) and cg[(64, True)] == (4, 16) and cg[(67, True)] == (1, 64)
    assert cg[(256, True)] == (4, 64) and cg[(260, True)] == (4, 64) and cg[(64, False)] == (1, 64)
    assert [R.lanes(R.F64, d, a) for d, a in R.COUPLING_SHAPES[R.F64]] == [(1, 8), (2, 8), (2, 64), (2, 64)]
    assert R.coupling_batches(R.F32, 256) == [1, 3, 5, 9, 15, 16, 17, 35]
