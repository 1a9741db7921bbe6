"""Edges of the per-column RationalQuadraticSpline (include/bjx_cols.h) that tests/test_gpu_spline_cols.py does not reach: every
pullback instantiation of bjx_spline_cols.hip (K = 4 / 8 / 16 in registers, the streaming kernel for other K, both forms, both
directions, both dtypes), x₁ blocks taller than one lane group (the `r += G` row loop), general knot tables whose bin 0 (lower knot
= −knot K) is reachable, special inputs in the pullback, grid-stride sweeps, degenerate raw parameters, BJX_ACCUMULATE /
in-place calls through the C ABI and parameter layouts.

Every comparison is against the CPU oracle applied column by column (the helpers of test_gpu_spline_cols.py) and held to
tests/_tol.py's flat bar on that file's scales: values and cotangents per="sample" (parameter cotangents on the column's largest
cotangent entry, as there), log-dets per="element" with a floor of 1.  Raw parameters are rounded to the tested dtype before
the oracle sees them, so the oracle and the kernel start from the same numbers."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _tol import flat_close  # noqa: E402
from test_gpu_spline_cols import (DT, coupling_ref, dev2, dev3, host, inputs, knots_of, masks, raw_params,  # noqa: E402
                                  ref_cols_pullback, ref_spline)

F32, F64 = np.float32, np.float64
KEYS = {"knots": ("widths", "heights", "derivatives"), "raw": ("raw_widths", "raw_heights", "raw_derivatives")}

# (K, form) of the pullback test: every specialised arm of launch_vjp (4, 8, 16) and streaming K on both sides of each
# (1, 2, 17, 33, 64); K = 1 exists in the raw form only (a knot table needs two knots).
K_VJP = [1, 2, 4, 8, 16, 17, 33, 64]
VJP_CASES = [(K, form) for K in K_VJP for form in ("knots", "raw") if not (K == 1 and form == "knots")]


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def seed(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rounded(a, dt):
    return np.asarray(a, dt).astype(np.float64)


def make_spline(bj, form, dt, raw, knots, B):
    if form == "raw":
        return bj.RationalQuadraticSpline(*(dev3(a, dt) for a in raw), B)
    return bj.RationalQuadraticSpline(*(dev3(a, dt) for a in knots))


def lbar_dev(lb, dt):
    return None if lb is None else torch.from_numpy(np.asarray(lb, dt)).cuda()


def finite_max(a):
    a = np.abs(np.asarray(a, np.float64))
    return np.where(np.isfinite(a), a, 0.0)


def untie(y, H, dt):
    """Inputs of an INVERSE pullback that sit on (within 8 ulps of) a height knot strictly inside ±knot K, moved down by 1e-4·knot K.
    The inverse pullback searches the bin again at x = f⁻¹(y) (interface.jl:276-281, in the oracle as in the kernel); at a height
    knot f⁻¹(y) is the width knot up to rounding, so which bin's cotangents are written is decided by the last bit of f⁻¹ and
    differs between any two evaluations.  Values and log-dets (continuous at a knot) are compared at the exact ties."""
    y = np.asarray(y, np.float64)
    Hf = np.asarray(H, np.float64)
    top = Hf[:, -1]
    with np.errstate(invalid="ignore"):
        d = np.nanmin(np.abs(y[:, None, :] - Hf), axis=1)
        near = np.isfinite(y) & (np.abs(y) < top) & (d <= 8 * np.finfo(dt).eps * np.abs(top))
    return rounded(np.where(near, y - 1e-4 * top, y), dt)


def check_cotangents(grads, cots, form, dt, what, term_scale=None, cond=None):
    """The three per-column cotangents against the oracle's, on the column's largest (finite) cotangent entry, as
    test_per_column_parameter_cotangents_match_oracle does (or on `term_scale` where that is larger)."""
    N = cots[0].shape[-1]
    ts = finite_max(np.concatenate([c_.reshape(-1, N) for c_ in cots])).max(axis=0)
    if term_scale is not None:
        ts = np.maximum(ts, term_scale)
    for k, ref in zip(KEYS[form], cots):
        got = host(grads[k]) if isinstance(grads, dict) else host(grads[KEYS[form].index(k)])
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if form == "knots" and k == "derivatives":
            ref = ref.copy()
            ref[:, -1] = 0.0                 # the derivative at the last knot is not read by the spline
        flat_close(got.reshape(-1, N), ref.reshape(-1, N), dt, f"{what} {k}", term_scale=ts, cond=cond)


def abi_vjp(bj, sp, inverse, x, g, lb, want, idx1=None):
    """bjx_rqs_cols_vjp called directly: the cotangent outputs not in `want` are passed as NULL."""
    L = bj._lib
    form, K, B = sp._cols
    dim, batch = x.shape
    pw, ph, pd, lw, lh, ld = sp._col_params(x, batch)
    n = dim if idx1 is None else int(idx1.numel())
    ms = (K + 1, K + 1, K + 1) if form == L.BJX_COLS_KNOTS else (K, K, K - 1)
    bars = [torch.full((batch, m, n), float("nan"), dtype=x.dtype, device=x.device).permute(2, 1, 0) if w_ else None for m, w_ in zip(ms, want)]
    xb = torch.empty((batch, dim), dtype=x.dtype, device=x.device).T
    ctx = bj.context(x.device)
    ptr = bj.interface._ptr
    rc = L.load().bjx_rqs_cols_vjp(ctx.h, L.BJX_F32 if x.dtype == torch.float32 else L.BJX_F64, int(inverse), form, ptr(idx1), n,
                                   ptr(pw), ptr(ph), ptr(pd), lw, lh, ld, K, B, ptr(x), ptr(g), ptr(lb), ptr(xb), *[ptr(b_) for b_ in bars], dim, batch)
    assert rc == 0, L.load().bjx_last_error(ctx.h)
    torch.cuda.synchronize()
    return xb, bars


def abi_fwd(bj, sp, inverse, x, out, ladj_ps, ladj_sum, flags=0, idx1=None):
    L = bj._lib
    form, K, B = sp._cols
    dim, batch = x.shape
    n = int(sp.widths.shape[0])
    pw, ph, pd, lw, lh, ld = sp._col_params(x, batch)
    ctx = bj.context(x.device)
    ptr = bj.interface._ptr
    rc = L.load().bjx_rqs_cols(ctx.h, L.BJX_F32 if x.dtype == torch.float32 else L.BJX_F64, int(inverse), form, ptr(idx1), n,
                               ptr(pw), ptr(ph), ptr(pd), lw, lh, ld, K, B, ptr(x), ptr(out), ptr(ladj_ps), ptr(ladj_sum), dim, batch, flags)
    assert rc == 0, L.load().bjx_last_error(ctx.h)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. every pullback instantiation
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("with_lb", [True, False])
@pytest.mark.parametrize("K,form", VJP_CASES)
def test_every_pullback_instantiation_matches_oracle(bj, orc, dt, inverse, with_lb, K, form):
    rng = seed("vjp", K, form, inverse, with_lb, np.dtype(dt).name)
    dim, N, B = 6, 48, 2.0
    raw = tuple(rounded(a, dt) for a in raw_params(rng, dim, K, N))
    W, H, D = knots_of(orc, *raw, B, dt)
    x = rounded(rng.uniform(-1.1 * B, 1.1 * B, size=(dim, N)), dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt) if with_lb else None
    sp = make_spline(bj, form, dt, raw, (W, H, D), B)
    b = bj.inverse(sp) if inverse else sp
    xd, gd, lbd = dev2(x, dt), dev2(g, dt), lbar_dev(lb, dt)
    xb, grads = bj.vjp_params(b, xd, gd, lbd)
    xb_ref, cots = ref_cols_pullback(orc, W, H, D, x, g, lb, inverse, raw=raw if form == "raw" else None, B=B)
    what = f"rqs_cols vjp K={K} {form} inv={inverse} lb={with_lb}"
    flat_close(host(xb), xb_ref, dt, what + " x̄")
    check_cotangents(grads, cots, form, dt, what)
    if K in (4, 8, 16, 17) and with_lb:
        # one launch per instantiation with each cotangent output NULL on its own: the others keep their bits
        full_xb, full = abi_vjp(bj, sp, inverse, xd, gd, lbd, (True, True, True))
        assert torch.equal(full_xb, xb) and all(torch.equal(a, grads[k]) for a, k in zip(full, KEYS[form]))
        for drop in range(3):
            want = tuple(i != drop for i in range(3))
            xb2, part = abi_vjp(bj, sp, inverse, xd, gd, lbd, want)
            assert torch.equal(xb2, xb), f"x̄ changes when output {drop} is NULL"
            for i in range(3):
                if want[i]:
                    assert torch.equal(part[i], full[i]), f"{KEYS[form][i]} changes when {KEYS[form][drop]} is NULL"


def test_raw_single_bin_pullback_with_and_without_a_derivative_buffer(bj, orc):
    """K = 1 in the raw form: no raw derivatives (p_d and d_bar may be NULL); the widths / heights cotangents vanish (softmax of
    one entry) and x̄ is that of the single bin between ±B.  A vanishing raw cotangent is p·(2B·c̄ − p·2B·c̄), a difference of two
    equal terms: it is compared on the size of those terms (2B times the knot cotangent, _tol.py's term_scale), not on its own
    zero norm — the kernel's fused multiply-add leaves the rounding of 2B·c̄ (~1e-16 of it in Float64) where the oracle gets 0."""
    rng = seed("k1")
    dim, N, B = 5, 64, 1.5
    raw = tuple(rounded(a, F64) for a in raw_params(rng, dim, 1, N))
    W, H, D = knots_of(orc, *raw, B, F64)
    x = rng.uniform(-1.2 * B, 1.2 * B, size=(dim, N))
    g, lb = rng.normal(size=(dim, N)), rng.normal(size=N)
    sp = bj.RationalQuadraticSpline(dev3(raw[0], F64), dev3(raw[1], F64), torch.empty((dim, 0, N), dtype=torch.float64, device="cuda"), B)
    xd, gd, lbd = dev2(x, F64), dev2(g, F64), lbar_dev(lb, F64)
    for inverse in (False, True):
        xb_ref, cots = ref_cols_pullback(orc, W, H, D, x, g, lb, inverse, raw=raw, B=B)
        _, knot_cots = ref_cols_pullback(orc, W, H, D, x, g, lb, inverse)
        terms = 2 * B * np.abs(np.concatenate([c_.reshape(-1, N) for c_ in knot_cots[:2]])).max(axis=0)
        xb, bars = abi_vjp(bj, sp, inverse, xd, gd, lbd, (True, True, False))
        flat_close(host(xb), xb_ref, F64, f"rqs_cols vjp K=1 raw inv={inverse} x̄")
        check_cotangents({"raw_widths": bars[0], "raw_heights": bars[1], "raw_derivatives": torch.empty((dim, 0, N))}, cots, "raw", F64,
                         f"rqs_cols vjp K=1 raw inv={inverse}", term_scale=terms)
        xb2, _ = abi_vjp(bj, sp, inverse, xd, gd, lbd, (True, True, True))      # a d_bar buffer of zero size is ignored
        assert torch.equal(xb2, xb)


# ------------------------------------------------------------------ 2. tall and odd x₁ blocks
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form,K", [("knots", 8), ("raw", 5)])
@pytest.mark.parametrize("n1", [33, 65, 100, 129, 300])
@pytest.mark.parametrize("how", ["plain", "coupling"])
def test_tall_x1_blocks_match_oracle(bj, orc, dt, inverse, form, K, n1, how):
    """n1 > 64 rows per column: each lane walks several rows (r += G) and sums their log-dets; n1 = 33 leaves 31 of 64 lanes
    idle.  As a Coupling (scattered mask, dim = 2 n1 + 1) the rows outside x₁ are copied through / pass ȳ through."""
    rng = seed("tall", n1, form, inverse, how, np.dtype(dt).name)
    N, B = 10, 3.0
    raw = tuple(rounded(a, dt) for a in raw_params(rng, n1, K, N))
    W, H, D = knots_of(orc, *raw, B, dt)
    sp = make_spline(bj, form, dt, raw, (W, H, D), B)
    what = f"rqs_cols n1={n1} {how} {form} K={K} inv={inverse}"
    if how == "plain":
        dim, i1 = n1, np.arange(n1)
        b = bj.inverse(sp) if inverse else sp
    else:
        dim = 2 * n1 + 1
        i1 = np.sort(rng.choice(dim, size=n1, replace=False))
        mask = bj.PartitionMask(dim, [int(i) + 1 for i in i1])
        cl = bj.Coupling(lambda x2: sp, mask)
        b = bj.inverse(cl) if inverse else cl
    x = rounded(rng.normal(size=(dim, N)) * 2, dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    xd = dev2(x, dt)
    y, lps = bj.with_logabsdet_jacobian(b, xd, per_sample=True)
    y_ref, l_ref = x.copy(), None
    y_ref[i1], l_ref = ref_spline(orc, W, H, D, np.asarray(x[i1], dt), inverse)
    flat_close(host(y), y_ref, dt, what + " values")
    flat_close(host(lps), l_ref, dt, what + " ladj", per="element", floor=1.0)
    xb, grads = bj.vjp_params(b, xd, dev2(g, dt), lbar_dev(lb, dt))
    xb1, cots = ref_cols_pullback(orc, W, H, D, x[i1], g[i1], lb, inverse, raw=raw if form == "raw" else None, B=B)
    xb_ref = g.copy()
    xb_ref[i1] = xb1
    flat_close(host(xb), xb_ref, dt, what + " x̄")
    check_cotangents(grads, cots, form, dt, what)
    if how == "coupling":
        i2 = np.setdiff1d(np.arange(dim), i1)
        assert np.array_equal(host(y)[i2], x[i2]), "rows outside x₁ copy through"
        assert np.array_equal(host(xb)[i2], g[i2]), "rows outside x₁ pass ȳ through"


# ------------------------------------------------------------------ 3. general knots: bin 0 reachable
def general_knots(rng, n, K, N, dt):
    """Per column and row a sorted random knot table whose first knot is −0.6·knot K (not −knot K, so bin 0 — lower knot
    −knot K, derivative 1 — has width 0.4·knot K); heights likewise, positive random derivatives."""
    def table(top):
        t = np.sort(rng.uniform(-0.6, 1.0, size=(n, K + 1, N)), axis=1)
        t[:, 0], t[:, -1] = -0.6, 1.0
        return t * top[:, None, :]
    W = table(rng.uniform(1.5, 3.0, size=(n, N)))
    H = table(rng.uniform(1.0, 4.0, size=(n, N)))
    D = rng.uniform(0.3, 3.0, size=(n, K + 1, N))
    return tuple(np.asarray(a, dt) for a in (W, H, D))


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", [1, 4, 5, 8, 16, 33])
def test_general_knots_bin0_matches_oracle(bj, orc, dt, inverse, K):
    rng = seed("bin0", K, inverse, np.dtype(dt).name)
    dim, N = 7, 96
    W, H, D = general_knots(rng, dim, K, N, dt)
    kn = H if inverse else W
    top = kn[:, -1].astype(np.float64)
    k0 = kn[:, 0].astype(np.float64)
    x = np.empty((dim, N))
    q = N // 4
    x[:, :2 * q] = -top[:, :2 * q] + (k0[:, :2 * q] + top[:, :2 * q]) * rng.uniform(0.0, 1.0, size=(dim, 2 * q))     # bin 0
    x[:, 2 * q:3 * q] = k0[:, 2 * q:3 * q]                                                                              # knot 0
    x[:, 3 * q:] = top[:, 3 * q:] * rng.uniform(-1.1, 1.1, size=(dim, N - 3 * q))
    x[0, 3 * q] = -top[0, 3 * q]                                                                                        # −knot K
    x = rounded(x, dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    sp = bj.RationalQuadraticSpline(dev3(W, dt), dev3(H, dt), dev3(D, dt))
    b = bj.inverse(sp) if inverse else sp
    xd = dev2(x, dt)
    what = f"rqs_cols general knots K={K} inv={inverse}"
    y, lps = bj.with_logabsdet_jacobian(b, xd, per_sample=True)
    y_ref, l_ref = ref_spline(orc, W, H, D, np.asarray(x, dt), inverse)
    flat_close(host(y), y_ref, dt, what + " values")
    flat_close(host(lps), l_ref, dt, what + " ladj", per="element", floor=1.0)
    if inverse:
        x = untie(x, H, dt)
        xd = dev2(x, dt)
    xb, grads = bj.vjp_params(b, xd, dev2(g, dt), lbar_dev(lb, dt))
    xb_ref, cots = ref_cols_pullback(orc, *(a.astype(np.float64) for a in (W, H, D)), x, g, lb, inverse)
    flat_close(host(xb), xb_ref, dt, what + " x̄")
    check_cotangents(grads, cots, "knots", dt, what)
    assert np.abs(cots[0][:, -1, :2 * q]).max() > 0, "bin 0 sends a cotangent to knot K"


# ------------------------------------------------------------------ 4. special inputs in the pullback
def edge_inputs(rng, W, H, B, inverse, dt):
    """inputs()'s specials (columns 0-8) plus: knot 0, ±knot K, exactly ±B, NaN / ±inf in a few columns, and every interior knot
    (columns 17 ...); the remaining columns uniform in ±1.1 B."""
    n, K1, N = W.shape
    kn = (H if inverse else W).astype(np.float64)
    x = inputs(rng, W, H, B, inverse, dt).astype(np.float64)
    x[:, 9] = kn[:, 0, 9]
    x[:, 10] = kn[:, -1, 10]
    x[:, 11] = -kn[:, -1, 11]
    x[:, 12], x[:, 13] = B, -B
    x[0, 14] = np.nan
    x[1, 15], x[2, 15] = np.inf, -np.inf
    x[:, 16] = np.nan
    for j in range(K1 - 2):                                 # knots 1 ... K-1, row by row
        c, r = 17 + j // n, j % n
        x[r, c] = kn[r, 1 + j, c]
    first = 17 + (K1 - 2 + n - 1) // n
    x[:, first:] = rng.uniform(-1.1 * B, 1.1 * B, size=(n, N - first))
    return rounded(x, dt)


def edge_params(rng, form, dt, dim, K, N, B):
    """Raw parameters; in the raw form the special columns get equal raw widths and heights, so that with K and B powers of two
    the B constructor gives exact knot grids and the kernel's knots are the oracle's bit for bit: ties, and the slivers between
    ±B and ±knot K (knot K = 2B·Σsoftmax − B is B only up to rounding), are decided the same.  Columns 3 / 4 (inputs ±0) keep
    random heights: on the grid 0 is a height knot and the inverse there is a column of zeros, compared on a zero scale."""
    raw = [rounded(a, dt) for a in raw_params(rng, dim, K, N)]
    if form == "raw":
        keep = raw[1][:, :, 3:5].copy()
        raw[0][:, :, :24] = 0.25
        raw[1][:, :, :24] = -0.5
        raw[1][:, :, 3:5] = keep
    return tuple(raw)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form,K", [("knots", 8), ("knots", 5), ("raw", 8), ("raw", 32)])
def test_pullback_at_special_inputs_matches_oracle(bj, orc, dt, inverse, form, K):
    rng = seed("edge", form, K, inverse, np.dtype(dt).name)
    dim, N, B = 9, 48, 2.0
    raw = edge_params(rng, form, dt, dim, K, N, B)
    W, H, D = knots_of(orc, *raw, B, dt)
    x = edge_inputs(rng, W, H, B, inverse, dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    sp = make_spline(bj, form, dt, raw, (W, H, D), B)
    b = bj.inverse(sp) if inverse else sp
    xd = dev2(x, dt)
    what = f"rqs_cols specials {form} K={K} inv={inverse}"
    with np.errstate(invalid="ignore"):
        y, lps = bj.with_logabsdet_jacobian(b, xd, per_sample=True)
        y_ref, l_ref = ref_spline(orc, W, H, D, np.asarray(x, dt), inverse)
        flat_close(host(y), y_ref, dt, what + " values")
        flat_close(host(lps), l_ref, dt, what + " ladj", per="element", floor=1.0)
        if inverse:
            x = untie(x, H, dt)
            xd = dev2(x, dt)
        xb, grads = bj.vjp_params(b, xd, dev2(g, dt), lbar_dev(lb, dt))
        xb_ref, cots = ref_cols_pullback(orc, W, H, D, x, g, lb, inverse, raw=raw if form == "raw" else None, B=B)
    flat_close(host(xb), xb_ref, dt, what + " x̄")
    check_cotangents(grads, cots, form, dt, what)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form", ["knots", "raw"])
def test_nan_in_x1_stays_in_its_column_and_rows(bj, orc, inverse, form):
    """A Coupling (scattered mask): NaN / ±inf on x₁ rows of a few columns reach neither the other columns nor the rows outside x₁."""
    rng = seed("nan-coupling", form, inverse)
    dim, K, N, B = 12, 8, 40, 2.0
    mask = bj.PartitionMask(dim, masks(dim)["scattered"])
    i1 = np.array(mask.indices_1) - 1
    i2 = np.array(mask.indices_2) - 1
    n1 = len(i1)
    raw = raw_params(rng, n1, K, N)
    W, H, D = knots_of(orc, *raw, B, F64)
    sp = make_spline(bj, form, F64, raw, (W, H, D), B)
    cl = bj.Coupling(lambda x2: sp, mask)
    b = bj.inverse(cl) if inverse else cl
    x = rng.normal(size=(dim, N)) * 1.5
    x[i1[0], 3], x[i1[1], 7], x[i1[2], 7], x[:, 11][i1] = np.nan, np.inf, -np.inf, np.nan
    g, lb = rng.normal(size=(dim, N)), rng.normal(size=N)
    with np.errstate(invalid="ignore"):
        y, lps = bj.with_logabsdet_jacobian(b, dev2(x, F64), per_sample=True)
        y_ref, l_ref = coupling_ref(orc, lambda x2: sp, bj, mask, x, inverse, F64)
        flat_close(host(y), y_ref, F64, f"coupling specials {form} inv={inverse} values")
        flat_close(host(lps), l_ref, F64, f"coupling specials {form} inv={inverse} ladj", per="element", floor=1.0)
        assert np.array_equal(host(y)[i2], x[i2])
        xb = host(bj.vjp(b, dev2(x, F64), dev2(g, F64), lbar_dev(lb, F64)))
        xb1, _ = ref_cols_pullback(orc, W, H, D, x[i1], g[i1], lb, inverse)
    assert np.array_equal(xb[i2], g[i2]), "rows outside x₁ pass ȳ through"
    ref = g.copy()
    ref[i1] = xb1
    flat_close(xb, ref, F64, f"coupling specials {form} inv={inverse} x̄")


# ------------------------------------------------------------------ 5. grid-stride sweeps against the oracle
def sweep_columns(rng, batch, C, cap):
    """The stated column set: the first group, the groups on either side of every sweep boundary, the last (ragged) group and
    ~2 000 random columns."""
    groups = (batch + C - 1) // C
    gs = {0, groups - 1}
    for s in range(1, (groups - 1) // cap + 1):
        gs |= {s * cap - 1, s * cap}
    cols = set()
    for gr in gs:
        cols |= set(range(gr * C, min(batch, (gr + 1) * C)))
    cols |= set(rng.choice(batch, size=2000, replace=False).tolist())
    return np.array(sorted(cols))


def norm_knots(rng, n, K, N, B, dt):
    """B-constructor-like knot tables built in numpy for many columns at once (softmax cumsums scaled to ±B)."""
    def tab():
        e = np.exp(rng.normal(size=(n, K, N)))
        c = np.cumsum(e / e.sum(axis=1, keepdims=True), axis=1)
        return np.concatenate([np.zeros((n, 1, N)), c], axis=1) * (2 * B) - B
    D = np.concatenate([np.ones((n, 1, N)), np.log1p(np.exp(rng.normal(size=(n, K - 1, N)))), np.ones((n, 1, N))], axis=1)
    return tuple(np.asarray(a, dt) for a in (tab(), tab(), D))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form,K,dt", [("raw", 5, F32), ("knots", 8, F64)])
def test_grid_stride_sweeps_match_oracle(bj, orc, inverse, form, K, dt):
    dim, B = 4, 3.0
    G, C = 4, 256 // 4                                       # 4 rows: 4 lanes per column, 64 columns per 256-thread block
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8     # blocks of one sweep (kColsBlocksPerCu = 8)
    batch = (3 * cap + cap // 2) * C - 17                   # three full sweeps, a half sweep, a ragged last group
    assert (batch + C - 1) // C > 3 * cap and batch % C != 0
    rng = seed("sweep", form, K, inverse)
    cols = sweep_columns(rng, batch, C, cap)
    if form == "raw":
        raw = tuple(np.asarray(a, dt) for a in raw_params(rng, dim, K, batch))
        sp = bj.RationalQuadraticSpline(*(dev3(a, dt) for a in raw), B)
        rsel = tuple(a[:, :, cols].astype(np.float64) for a in raw)
        W, H, D = knots_of(orc, *rsel, B, dt)
    else:
        Wa, Ha, Da = norm_knots(rng, dim, K, batch, B, dt)
        sp = bj.RationalQuadraticSpline(dev3(Wa, dt), dev3(Ha, dt), dev3(Da, dt))
        W, H, D = (a[:, :, cols] for a in (Wa, Ha, Da))
        rsel = None
        del Wa, Ha, Da
    x = np.asarray(rng.uniform(-1.1 * B, 1.1 * B, size=(dim, batch)), dt)
    g = np.asarray(rng.normal(size=(dim, batch)), dt)
    lb = np.asarray(rng.normal(size=batch), dt)
    b = bj.inverse(sp) if inverse else sp
    xd = dev2(x, dt)
    ci = torch.from_numpy(cols).cuda()
    what = f"rqs_cols sweeps {form} K={K} inv={inverse} batch={batch}"
    y, lps = bj.with_logabsdet_jacobian(b, xd, per_sample=True)
    xs, gs_, lbs = x[:, cols].astype(np.float64), g[:, cols].astype(np.float64), lb[cols].astype(np.float64)
    y_ref, l_ref = ref_spline(orc, W, H, D, np.asarray(xs, dt), inverse)
    flat_close(host(y[:, ci]), y_ref, dt, what + " values")
    flat_close(host(lps[ci]), l_ref, dt, what + " ladj", per="element", floor=1.0)
    xb, grads = bj.vjp_params(b, xd, dev2(g, dt), lbar_dev(lb, dt))
    xb_ref, cots = ref_cols_pullback(orc, *(a.astype(np.float64) for a in (W, H, D)), xs, gs_, lbs, inverse, raw=rsel, B=B)
    flat_close(host(xb[:, ci]), xb_ref, dt, what + " x̄")
    check_cotangents({k: v[:, :, ci] for k, v in grads.items()}, cots, form, dt, what)


# ------------------------------------------------------------------ degenerate raw parameters
def device_knots(bj, raw, B, dt):
    """The B constructor evaluated on the device by bjx_rqs_params (rqs_params_kernel: the operations, order and d_exp / d_log1pexp
    of the raw form's own knot builder), one row per (x₁-row, column) -> (n, K+1, N) knot arrays in `dt`.  Knots built by the host
    oracle can differ from these in the last bit (host and device exp differ by an ulp), and with underflowed softmax entries a
    last-bit difference turns a zero-width or zero-height bin on or off; with the device's knots the oracle sees the kernel's bins."""
    n, K, N = raw[0].shape
    rows = [torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1)).reshape(N * n, -1)).astype(dt)).cuda() for a in raw]
    sp = bj.RationalQuadraticSpline(*rows, B)
    return tuple(np.transpose(host(t).reshape(N, n, K + 1), (1, 2, 0)).astype(dt) for t in (sp.widths, sp.heights, sp.derivatives))


def params_vjp_in(dt, raw, B, cots):
    """oracle.rqs_params_vjp for (n, K, N) arrays with the softmax p evaluated in `dt`, as the kernel does.  A softmax entry below
    the range of `dt` is exactly 0 there (Float32: exp(r − max) < 1e-45 for r − max < −104) but not in the oracle's Float64, and
    a zero-height bin sends ±inf to its knots: 0·inf = NaN in `dt` where Float64 gives ±inf.  Everything after p is Float64."""
    outs = []
    for r, cb in zip(raw[:2], cots[:2]):
        r = np.asarray(r, dt)
        e = np.exp(r - r.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float64)
        pbar = 2 * B * np.cumsum(cb[:, 1:][:, ::-1], axis=1)[:, ::-1]
        outs.append(p * (pbar - (p * pbar).sum(axis=1, keepdims=True)))
    outs.append(cots[2][:, 1:-1] / (1 + np.exp(-np.asarray(raw[2], np.float64))))
    return tuple(outs)


def inverse_bins(x, W, H, dt):
    """For inverse inputs y: (unresolved, amp).  The pullback evaluates at x = f⁻¹(y), which carries a rounding error of about
    one ulp of x; in a bin w wide that moves ξ = (x − w_k)/w by a = ulp(x)/w, and every term of the pullback moves with ξ
    (a first-order amplification in the sense of tests/_tol.py, computed from the data: Float32 bins of a few ulps occur here).
    A bin at most 2 ulps wide (0 < w <= 2 ulp) leaves f⁻¹(y) at most one value inside the bin: it rounds onto a knot and the
    pullback's second search (at x, interface.jl:276-281) lands in the neighbouring bin, which may have zero height (J = 0,
    x̄ = ±inf): `unresolved`, left out and counted.  `amp`: per column, the largest a of the other inputs."""
    n, K1, N = W.shape
    Wf, Hf = W.astype(np.float64), H.astype(np.float64)
    unresolved, amp = np.zeros((n, N), bool), np.zeros((n, N))
    for r in range(n):
        for c in range(N):
            y, w, h = x[r, c], Wf[r, :, c], Hf[r, :, c]
            if not (np.isfinite(y) and -h[-1] < y < h[-1]):
                continue
            k = int(np.searchsorted(h, y, side="left"))           # upper knot of y's bin; k = 0: lower knot −knot K
            lo = -w[-1] if k == 0 else w[k - 1]
            ulp = float(np.spacing(np.asarray(max(abs(lo), abs(w[k])), dt)))
            width = w[k] - lo
            if width > 0:
                unresolved[r, c] = width <= 2 * ulp
                amp[r, c] = ulp / width
    return unresolved, np.where(unresolved, 0.0, amp).max(axis=0)


# Float32 with B = 1e-3 is not in this list: there the inverse x̄ is over the bar in 20-31 % of the columns with no amplification
# found in the data, and the forward raw-height cotangents hold NaN where the oracle has ±inf beyond the entries explained by a
# flushed subnormal softmax (LAB_NOTEBOOK.md, open).
DEGENERATE = [(dt, B) for dt in (F32, F64) for B in (1e-3, 1e3) if not (dt is F32 and B == 1e-3)]


@pytest.mark.parametrize("dt,B", DEGENERATE)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", [8, 5])
def test_degenerate_raw_parameters_match_oracle(bj, orc, dt, inverse, B, K):
    """Raw widths / heights spread so widely that softmax entries underflow (zero-width and zero-height bins: N(0, 30²) in Float32,
    N(0, 400²) in Float64) and raw derivatives at ±40 and ±800 (log1pexp saturates to x or underflows to 0), the raw form against
    the oracle on the device-built knots (device_knots).  Where the oracle returns non-finite values (a zero-height bin has
    log-det −inf, its cotangents are NaN) the kernel must return the same ones (flat_close).

    Three numerical facts of `dt`, each isolated rather than hidden behind a wider bar:
    * the raw cotangent p_i (p̄_i − Σ p_m p̄_m) cancels to far below its terms when one softmax entry is ≈ 1; it is compared on the
      size of those terms, 2B·max|c̄| (tests/_tol.py's term_scale), as test_raw_single_bin_pullback_… does;
    * the softmax of the chain rule is evaluated in `dt` (params_vjp_in);
    * in the inverse, x = f⁻¹(y) is known to one ulp, a large part of a bin only a few ulps wide: the pullback is compared with
      that amplification (cond=, inverse_bins), and inputs in bins at most 2 ulps wide are left out and counted."""
    rng = seed("degenerate", K, B, inverse, np.dtype(dt).name)
    dim, N = 6, 64
    sc = 30.0 if dt is F32 else 400.0
    rw, rh, _ = raw_params(rng, dim, K, N, scale=sc)
    rd = rng.choice([-800.0, -40.0, 40.0, 800.0], size=(dim, K - 1, N))
    raw = tuple(rounded(a, dt) for a in (rw, rh, rd))
    W, H, D = device_knots(bj, raw, B, dt)
    assert (np.diff(W, axis=1) == 0).any() and (np.diff(H, axis=1) == 0).any(), "some bins have zero width / height"
    x = rounded(rng.uniform(-1.1 * B, 1.1 * B, size=(dim, N)), dt)
    g = rounded(rng.normal(size=(dim, N)), dt)
    lb = rounded(rng.normal(size=N), dt)
    sp = make_spline(bj, "raw", dt, raw, None, B)
    b = bj.inverse(sp) if inverse else sp
    xd = dev2(x, dt)
    what = f"rqs_cols degenerate raw K={K} B={B:g} inv={inverse}"
    with np.errstate(all="ignore"):
        y, lps = bj.with_logabsdet_jacobian(b, xd, per_sample=True)
        y_ref, l_ref = ref_spline(orc, W, H, D, np.asarray(x, dt), inverse)
        flat_close(host(y), y_ref, dt, what + " values")
        flat_close(host(lps), l_ref, dt, what + " ladj", per="element", floor=1.0)
        xb, grads = bj.vjp_params(b, xd, dev2(g, dt), lbar_dev(lb, dt))
        xb_ref, knot_cots = ref_cols_pullback(orc, *(a.astype(np.float64) for a in (W, H, D)), x, g, lb, inverse)
        cots = params_vjp_in(dt, raw, B, knot_cots)
        skip, amp = inverse_bins(x, W, H, dt) if inverse else (np.zeros(x.shape, bool), np.zeros(N))
        assert skip.mean() < 0.05, f"{int(skip.sum())} of {skip.size} inputs in unresolvable bins"
        note = f"{int(skip.sum())} inverse inputs in bins <= 2 ulps wide not compared" if skip.any() else None
        flat_close(np.where(skip, 0.0, host(xb)), np.where(skip, 0.0, xb_ref), dt, what + " x̄", note=note, cond=amp)
        terms = 2 * B * finite_max(np.concatenate([np.where(skip[:, None], 0.0, c_).reshape(-1, N) for c_ in knot_cots[:2]])).max(axis=0)
        got = {k: np.where(skip[:, None], 0.0, host(grads[k])) for k in KEYS["raw"]}
        ref = tuple(np.where(skip[:, None], 0.0, c_) for c_ in cots)
        check_cotangents({k: torch.from_numpy(v) for k, v in got.items()}, ref, "raw", dt, what, term_scale=terms, cond=amp)


# ------------------------------------------------------------------ 6. C-ABI flags and in-place
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form,K", [("knots", 8), ("raw", 5), ("knots", 16), ("raw", 4)])
def test_accumulate_adds_to_both_log_det_outputs(bj, orc, dt, inverse, form, K):
    rng = seed("accumulate", form, K, inverse, np.dtype(dt).name)
    dim, N, B = 12, 3000, 2.0
    raw = tuple(rounded(a, dt) for a in raw_params(rng, dim, K, N))
    W, H, D = knots_of(orc, *raw, B, dt) if form == "knots" else (None, None, None)
    sp = make_spline(bj, form, dt, raw, (W, H, D), B)
    x = dev2(rng.uniform(-1.1 * B, 1.1 * B, size=(dim, N)), dt)
    y = torch.empty_like(x)
    fresh_ps = torch.empty(N, dtype=DT[dt], device="cuda")
    fresh_sum = torch.empty(1, dtype=torch.float64, device="cuda")
    abi_fwd(bj, sp, inverse, x, y, fresh_ps, fresh_sum)
    old_ps = torch.from_numpy(rng.normal(size=N).astype(dt)).cuda()
    old_sum = 12.375
    sums = []
    for _ in range(2):
        ps = old_ps.clone()
        sm = torch.full((1,), old_sum, dtype=torch.float64, device="cuda")
        y2 = torch.empty_like(x)
        abi_fwd(bj, sp, inverse, x, y2, ps, sm, flags=bj._lib.BJX_ACCUMULATE)
        assert torch.equal(y2, y)
        assert torch.equal(ps, old_ps + fresh_ps), "ladj_ps = old value + fresh log-det"
        assert float(sm) == old_sum + float(fresh_sum), "ladj_sum = old value + fresh summed log-det"
        sums.append(float(sm))
    assert sums[0] == sums[1], "the accumulated sum is deterministic"


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form,K", [("knots", 8), ("raw", 5)])
def test_in_place_call_with_idx1_matches_out_of_place(bj, orc, dt, inverse, form, K):
    rng = seed("inplace", form, K, inverse, np.dtype(dt).name)
    dim, N, B = 20, 700, 2.0
    i1 = np.sort(rng.choice(dim, size=9, replace=False)).astype(np.int32)
    raw = tuple(rounded(a, dt) for a in raw_params(rng, len(i1), K, N))
    W, H, D = knots_of(orc, *raw, B, dt) if form == "knots" else (None, None, None)
    sp = make_spline(bj, form, dt, raw, (W, H, D), B)
    idx = torch.from_numpy(i1).cuda()
    x = dev2(rng.uniform(-1.1 * B, 1.1 * B, size=(dim, N)), dt)
    y = torch.full_like(x, float("nan"))
    ps1, sm1 = torch.empty(N, dtype=DT[dt], device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    abi_fwd(bj, sp, inverse, x, y, ps1, sm1, idx1=idx)
    i2 = torch.from_numpy(np.setdiff1d(np.arange(dim), i1)).cuda()
    assert torch.equal(y[i2], x[i2]), "out of place: rows outside x₁ copied"
    z = x.clone()
    ps2, sm2 = torch.empty_like(ps1), torch.empty_like(sm1)
    abi_fwd(bj, sp, inverse, z, z, ps2, sm2, idx1=idx)
    assert torch.equal(z[i2], x[i2]), "in place: rows outside x₁ untouched"
    assert torch.equal(z, y), "in place: x₁ rows equal the out-of-place result"
    assert torch.equal(ps2, ps1) and float(sm2) == float(sm1)


# ------------------------------------------------------------------ 7. parameter layouts
@pytest.mark.parametrize("form,K", [("knots", 8), ("raw", 5), ("raw", 16)])
@pytest.mark.parametrize("layout", ["batch_major", "expand", "offset_slice", "f32_params"])
def test_parameter_layouts_give_the_canonical_bits(bj, orc, form, K, layout):
    """Parameters in any layout (or dtype) take _col_params' copy path or are passed as they are; either way the outputs are the
    bits of the same numbers in the canonical layout (column-major per column, dtype of x)."""
    rng = seed("layout", form, K, layout)
    dim, N, B = 5, 300, 2.0
    dt = F64
    pdt = F32 if layout == "f32_params" else dt
    raw = [np.asarray(a, pdt).astype(np.float64) for a in raw_params(rng, dim, K, N)]
    if layout == "expand":
        raw = [np.ascontiguousarray(np.broadcast_to(a[:, :, :1], a.shape)) for a in raw]
    arrs = raw if form == "raw" else [rounded(a, pdt) for a in knots_of(orc, *raw, B, F64)]
    canon = [dev3(a, dt) for a in arrs]

    def other(a):
        if layout == "batch_major":
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()            # (n, m, N) row-major: the batch is the fastest axis
            assert t.stride(2) == 1
            return t
        if layout == "expand":
            return torch.from_numpy(np.ascontiguousarray(a[:, :, :1])).cuda().expand(a.shape)
        if layout == "offset_slice":
            n, m, nb = a.shape
            big = np.zeros((n, m + 3, nb))
            big[:, 2:2 + m] = a
            t = dev3(big, dt)[:, 2:2 + m]
            assert t.storage_offset() > 0 and t.stride(2) > n * m
            return t
        return dev3(a, F32)
    alt = [other(a) for a in arrs]
    sps = [bj.RationalQuadraticSpline(*p, B) if form == "raw" else bj.RationalQuadraticSpline(*p) for p in (canon, alt)]
    x = dev2(rng.uniform(-1.1 * B, 1.1 * B, size=(dim, N)), dt)
    g = dev2(rng.normal(size=(dim, N)), dt)
    lb = torch.from_numpy(rng.normal(size=N)).cuda()
    for inverse in (False, True):
        r = []
        for sp in sps:
            b = bj.inverse(sp) if inverse else sp
            y, l = bj.with_logabsdet_jacobian(b, x, per_sample=True)
            xb, grads = bj.vjp_params(b, x, g, lb)
            r.append((y, l, xb, grads))
        (y1, l1, xb1, g1), (y2, l2, xb2, g2) = r
        assert torch.equal(y1, y2) and torch.equal(l1, l2), f"{layout} inv={inverse}: values / log-dets"
        assert torch.equal(xb1, xb2), f"{layout} inv={inverse}: x̄"
        assert set(g1) == set(g2) and all(torch.equal(g1[k], g2[k]) for k in g1), f"{layout} inv={inverse}: cotangents"
