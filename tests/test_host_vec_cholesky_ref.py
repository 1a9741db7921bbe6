"""The inputs, references and tables of tests/test_gpu_vec_cholesky_abi.py (tests/_vec_cholesky_ref.py), checked on the CPU:
  * every drawn input and every reference output is finite, in Float64 and rounded to the type;
  * forward(inverse(y)) == y in Float64 to 1e-12 at every K of the tables;
  * the Float32 oracle agrees with the Float64 oracle ON THE SAME ROUNDED INPUTS to a tenth of the flat bar (1e-4 of the scale the GPU file
    compares on) for W, y, both log-dets and the inverse's pullback, at every K of the tables: the bar of the GPU file then measures
    the kernel and not the conditioning of the data (measured: y 1.0e-7 ... 1.7e-7 of the sample's max-norm, W <= 3.7e-7, log-dets <= 3.1e-6), also on the draw of the first row at both ends of atanh;
  * the forward oracle and `vec_cholesky_fwd_vjp` give identical bits whether the unused triangle holds zeros or NaN, and the pullback
    is exactly zero on the diagonal and in the unused triangle; 'L' is the transpose of 'U' bit for bit;
  * every table shape reaches the form written next to it, and is the smallest / largest K that does.
No GPU, no torch."""
import numpy as np
import pytest

import _vec_cholesky_ref as R

TENTH = 0.1 * 1e-3          # a tenth of the flat Float32 bar of tests/_tol.py
BATCH = 5


def _ks(dt, limit=None):
    return [k for k in R.table_ks(dt) if k >= 2 and (limit is None or k <= limit)]


def _sample_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    n = ref.shape[-1]
    return float((np.abs(got - ref).reshape(-1, n).max(axis=0) / np.abs(ref).reshape(-1, n).max(axis=0)).max())


def _element_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + R.LOG_DET_FLOOR)).max())


@pytest.mark.parametrize("dt", R.DTS, ids=lambda d: d.name)
def test_every_input_and_reference_is_finite(orc, dt):
    for K in _ks(dt):
        d = R.draw(dt.name, K, 2 if K >= 115 else BATCH)
        assert all(a.dtype == dt and np.isfinite(a).all() for a in d.values())
        assert d["y"].shape[0] == R.nvec(K) and d["W"].shape[:2] == (K, K)
        for uplo in "UL":
            outs = list(R.ref_inverse(d["y"], uplo)) + list(R.ref_forward(R.for_uplo(d["W"], uplo), uplo))
            if K <= R.INV_VJP_SERVED:
                outs += [R.ref_inv_vjp(d["y"], R.for_uplo(d["W_bar"], uplo), d["logJ_bar"], uplo), R.ref_inv_vjp(d["y"], R.for_uplo(d["W_bar"], uplo), None, uplo)]
            if K <= R.FWD_VJP_SERVED[dt] and (uplo == "U" or K <= 64):
                outs.append(R.ref_fwd_vjp(R.for_uplo(d["W"], uplo), d["y_bar"], uplo))
            for o in outs:
                assert np.isfinite(o).all() and np.isfinite(np.asarray(o).astype(dt)).all(), (K, uplo)


def test_forward_of_inverse_is_the_identity_in_float64(orc):
    for K in sorted(set(_ks(R.F32)) | set(_ks(R.F64))):
        y = R.f64(R.draw("float64", K, 2 if K >= 115 else BATCH)["y"])
        for uplo in "UL":
            W, lj = orc.vec_cholesky(y, inverse=True, uplo=uplo)
            y2, lf = orc.vec_cholesky(W, inverse=False, uplo=uplo)
            assert np.abs(y2 - y).max() <= 1e-12, (K, uplo)
            assert np.abs(lf + lj).max() <= 1e-12 * np.abs(lj).max() + 1e-12, (K, uplo)      # the forward's log-det is minus the inverse's


def test_float32_oracle_is_within_a_tenth_of_the_bar_of_the_float64_oracle(orc):
    worst = {"W": 0.0, "logJ": 0.0, "y": 0.0, "ladj": 0.0, "inv_vjp": 0.0}
    for K in _ks(R.F32):
        d = R.draw("float32", K, 2 if K >= 115 else BATCH)
        for uplo in "UL":
            W32, l32 = orc.vec_cholesky(d["y"], inverse=True, uplo=uplo)
            assert W32.dtype == np.float32
            W64, l64 = R.ref_inverse(d["y"], uplo)
            Wu = R.for_uplo(d["W"], uplo)
            y32, f32 = orc.vec_cholesky(Wu, inverse=False, uplo=uplo)
            y64, f64 = R.ref_forward(Wu, uplo)
            errs = {"W": _sample_err(W32, W64), "logJ": _element_err(l32, l64), "y": _sample_err(y32, y64), "ladj": _element_err(f32, f64)}
            if K <= R.INV_VJP_SERVED:
                Wb = R.for_uplo(d["W_bar"], uplo)
                g32 = orc.vec_cholesky_inv_vjp(d["y"], Wb, d["logJ_bar"], uplo=uplo)
                assert g32.dtype == np.float32
                errs["inv_vjp"] = _sample_err(g32, R.ref_inv_vjp(d["y"], Wb, d["logJ_bar"], uplo))
            for k, e in errs.items():
                assert e <= TENTH, f"K={K} {uplo} {k}: the Float32 oracle is {e:.3g} of the scale off the Float64 one (a tenth of the bar: {TENTH:g})"
                worst[k] = max(worst[k], e)
    print("Float32 oracle vs Float64 oracle, worst over the tables:", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("uplo", ["U", "L"])
def test_unused_triangle_is_not_read_and_the_pullback_is_zero_outside_the_strict_triangle(orc, uplo):
    K = 7
    d = R.draw("float64", K, 4)
    W = R.for_uplo(d["W"], uplo)
    idx = R.unused_triangle(K, uplo)
    assert (W[idx] == 0).all()
    Wn = np.array(W, order="F")
    Wn[idx] = np.nan
    a, b = orc.vec_cholesky(W, inverse=False, uplo=uplo), orc.vec_cholesky(np.asfortranarray(Wn), inverse=False, uplo=uplo)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ga, gb = R.ref_fwd_vjp(W, d["y_bar"], uplo), R.ref_fwd_vjp(Wn, d["y_bar"], uplo)
    assert np.array_equal(ga, gb)
    assert (ga[idx] == 0).all() and (ga[np.arange(K), np.arange(K)] == 0).all()


def test_lower_is_the_transpose_of_upper_bit_for_bit(orc):
    for dt in R.DTS:
        for K in (7, 34):
            d = R.draw(dt.name, K, BATCH)
            for y in (d["y"], R.f64(d["y"])):
                WU, lU = orc.vec_cholesky(y, inverse=True, uplo="U")
                WL, lL = orc.vec_cholesky(y, inverse=True, uplo="L")
                assert np.array_equal(WL, np.transpose(WU, (1, 0, 2))) and np.array_equal(lU, lL) and (WU[0, 0] == 1).all()
            yU, fU = orc.vec_cholesky(d["W"], inverse=False, uplo="U")
            yL, fL = orc.vec_cholesky(R.for_uplo(d["W"], "L"), inverse=False, uplo="L")
            assert np.array_equal(yU, yL) and np.array_equal(fU, fL)
            assert np.array_equal(R.ref_inv_vjp(d["y"], d["W_bar"], d["logJ_bar"], "U"), R.ref_inv_vjp(d["y"], R.for_uplo(d["W_bar"], "L"), d["logJ_bar"], "L"))
            assert np.array_equal(R.ref_fwd_vjp(R.for_uplo(d["W"], "L"), d["y_bar"], "L"), np.transpose(R.ref_fwd_vjp(d["W"], d["y_bar"], "U"), (1, 0, 2)))


@pytest.mark.parametrize("dt", R.DTS, ids=lambda d: d.name)
def test_first_row_edge_draw_is_odd_and_within_a_tenth_of_the_bar(orc, dt):
    """the draw of the forward link's first row at |y| = 1e-6 ... 6, both signs: finite, W of the negated y is W with the strict triangle
    negated (so the kernel must return −y bit for bit), the Float64 forward recovers y, and the Float32 oracle stays within a tenth of the bar"""
    for K in R.FIRST_ROW_KS[dt]:
        d = R.draw_first_row_edges(dt.name, K)
        y, W = d["y"], d["W"]
        assert np.isfinite(y).all() and np.isfinite(W).all() and np.array_equal(y[:, 1::2], -y[:, ::2])
        iu = np.triu_indices(K, 1)
        assert np.array_equal(W[iu][:, 1::2], -W[iu][:, ::2]) and np.array_equal(np.diagonal(W)[1::2], np.diagonal(W)[::2])
        assert np.abs(W[0, 1]).min() < 2e-6 and np.abs(W[0, 1]).max() > 1 - 2e-5 and np.abs(W[0, 1]).max() < 1
        for uplo in "UL":
            Wu = R.for_uplo(W, uplo)
            y64, l64 = R.ref_forward(Wu, uplo)
            assert np.isfinite(y64).all() and np.isfinite(l64).all()
            assert np.array_equal(y64[:, 1::2], -y64[:, ::2]) and np.array_equal(l64[1::2], l64[::2])
            if dt == R.F64:
                assert _sample_err(y64, y) <= 1e-9, (K, uplo)             # 1 − w carries 1e-16 / 1.2e-5 at y = 6
            else:
                y32, l32 = orc.vec_cholesky(Wu, inverse=False, uplo=uplo)
                assert y32.dtype == np.float32
                assert _sample_err(y32, y64) <= TENTH and _element_err(l32, l64) <= TENTH, (K, uplo, _sample_err(y32, y64), _element_err(l32, l64))


def test_tiled_fwd_vjp_reference_is_the_reference_of_the_tiled_input(orc):
    d = R.draw("float64", 3, 7)
    idx = np.arange(17) % 7
    W, g = np.asfortranarray(d["W"][:, :, idx]), np.asfortranarray(d["y_bar"][:, idx])
    assert np.array_equal(R.ref_fwd_vjp(W, g, "U", period=7), R.ref_fwd_vjp(W, g, "U"))


@pytest.mark.parametrize("dt", R.DTS, ids=lambda d: d.name)
def test_every_table_shape_reaches_its_form_and_is_the_edge_of_it(dt):
    scan = range(2, 101)
    for form, (lo, hi) in R.VALUE_FORMS[dt]:
        for variant in ((True, True), (True, False), (False, True)):                    # inverse, inverse without `out`, forward
            ks = [K for K in scan if R.value_form(dt, K, variant[0], True, variant[1]) == form]
            assert (ks[0], ks[-1]) == (lo, hi), (form, variant, ks)
        want = ("refused",) if form == ("generic",) else form
        ks = [K for K in scan if R.inv_vjp_form(dt, K) == want]
        assert (ks[0], ks[-1]) == (lo, hi), (want, ks)
    assert {f for f, _ in R.VALUE_FORMS[dt]} == {R.value_form(dt, K, True) for K in scan}       # no form of the dispatcher is left out
    for K, form in R.OFFSET_FORMS[dt]:
        assert R.value_form(dt, K, True, False) == R.value_form(dt, K, True, False, False) == R.value_form(dt, K, False, False) == R.inv_vjp_form(dt, K, False) == form
    assert {f for _, f in R.OFFSET_FORMS[dt]} == {R.value_form(dt, K, True, False) for K in range(2, 65)}
    assert R.inv_vjp_form(dt, R.INV_VJP_SERVED)[0] == "chunk" and R.inv_vjp_form(dt, R.INV_VJP_REFUSED) == ("refused",)
    for K, aligned, form in R.FWD_VJP_SHAPES[dt]:
        assert R.fwd_vjp_form(dt, K, aligned) == form, (K, aligned)
    full = range(2, 260)
    for form in (("swizzled",), ("pack",), ("scalar",)):
        ks = [K for K in full if R.fwd_vjp_form(dt, K) == form]
        tab = [K for K, a, f in R.FWD_VJP_SHAPES[dt] if a and f == form]
        assert ks[0] == min(tab) and ks[-1] == max(tab), (form, ks[0], ks[-1], tab)
    assert R.fwd_vjp_form(dt, R.FWD_VJP_SERVED[dt]) != ("refused",) and R.fwd_vjp_form(dt, R.FWD_VJP_REFUSED[dt]) == ("refused",)
    assert R.fwd_vjp_form(dt, R.FWD_VJP_SERVED[dt], False) != ("refused",)
    # K·K odd inside an aligned call: the dense W alternates between aligned and unaligned samples
    assert dt != R.F32 or all(R.value_form(dt, K, True)[1] == 4 for K in (17, 33, 41))
    assert R.lane_trip_batch(256) == 1048641 and R.batches(("chunk", 1, 16)) == (1, 2, 3, 5)
