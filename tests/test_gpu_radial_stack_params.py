"""Parameter pullback of a run of RadialLayers in one streaming pass (include/bjx_radial_stack_params.h: bjx_radial_stack_vjp_params;
`_RadialRun._vjp_params` and `_vjp_params_composed` in bijectors.jl_amd/interface.py) against the oracle composed layer by layer in
Float64 (tests/_radial_params_ref.py: forward — `radial` for the layer inputs, `radial_vjp` to carry ḡ, `radial_param_vjp` per layer;
inverse — per layer the oracle's inverse for the pre-image, `radial_vjp(inverse=True)` for ḡ′, `radial_param_vjp(pre-image, −ḡ′, −ℓ̄)`).

Bar: `flat_close` (1e-3 Float32, 1e-6 Float64, flat).  x̄ per sample; parameter cotangents per tensor (one layer's ᾱ_, β̄ or z̄₀ at a
time), with `term_scale` = the max-norm of that sum's SUMMANDS — it only matters where the sum over the batch cancels below its
largest term, and flat_close records it.  No other factor.

Parameters and points as in tests/test_gpu_radial_stack.py (|z₀| ~ 0.3, row 0 shifted by 2: r stays away from 0); the inverse run is
evaluated at the rounded image of the forward run.

Shapes: the smallest at which each path can go wrong — group form on whole packs (a ragged tile, more than one tile, more than one
pack per lane), on a partial last pack (35 rows) and on scalar packs (an element-aligned base); the lane-per-column form (one column
past a 64-column tile, short columns, tiled ones); batches at which blocks walk several tiles and more than 32 blocks leave a partial
(the first fold runs: grid = ceil(tiles / 4), 32 partials per fold chunk — 64 rows: 32 / 16 columns per tile, N = 4 500 gives 36 / 71
blocks; 10 rows: 64 columns per tile, N = 8 300 gives 33 blocks); 17 layers; one layer against bjx_radial_vjp_params; the first
height the register kernels refuse.

Launch counts measured on an MI355X (`test_planner_takes_the_fused_pass`): `vjp_params` of a pure radial run takes 2 hot launches
(`bj.kernel_timed`: the streaming pass, and the folds under one event pair) at L = 3 and at L = 6, forward and inverse, 64 and 10 rows,
both dtypes; the C entry itself 2 or 3 kernel launches (`bjx_launch_count`)."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _radial_params_ref import ref_run_params, run_objective  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, dev, host, rng  # noqa: E402,F401  (fixtures / helpers)

DTYPES = [np.float32, np.float64]
GROUP_PACKS = [(8, 2, 5), (64, 3, 67), (128, 8, 130), (512, 2, 9)]
GROUP_V1 = [(35, 3, 67)]
WALK = [(2, 4, 65), (7, 3, 64), (10, 5, 130)]
CASES = [(d, nl, N, dt) for (d, nl, N) in GROUP_PACKS + GROUP_V1 + WALK for dt in DTYPES] + [(16, 2, 33, np.float64)]
IDS = [f"{d}x{nl}x{N}-{np.dtype(dt).name}" for d, nl, N, dt in CASES]


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


def _params(r, dim, nl, dt):
    al = (0.5 * r.normal(size=nl)).astype(dt)
    be = r.normal(size=nl).astype(dt)
    z0 = (0.3 * r.normal(size=(dim, nl))).astype(dt)
    return al, be, z0


def _points(r, dim, N, dt):
    Z = r.normal(size=(dim, N))
    Z[0] += 2.0                                           # away from every z₀ (|z₀| ~ 0.3)
    return np.asfortranarray(Z.astype(dt))


def _image(orc, al, be, z0, Z, dt):
    """The forward run's image of Z, rounded to dt: where the inverse run is evaluated."""
    x = np.asfortranarray(np.asarray(Z, np.float64))
    for k in range(len(al)):
        x = np.asfortranarray(orc.radial(np.float64(al[k]), np.float64(be[k]), z0[:, k].astype(np.float64), x)[0])
    return np.asfortranarray(x.astype(dt))


def _draw(orc, seed, dim, nl, N, dt):
    r = rng(seed)
    al, be, z0 = _params(r, dim, nl, dt)
    Z = _points(r, dim, N, dt)
    G = np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = r.normal(size=N).astype(dt)
    return dict(al=al, be=be, z0=z0, Z=Z, G=G, lbar=lbar, Yd=_image(orc, al, be, z0, Z, dt))


def _layers(bj, al, be, z0):
    mk = lambda a: torch.tensor(a).cuda()
    return [bj.RadialLayer(mk(al[k:k + 1]), mk(be[k:k + 1]), mk(np.ascontiguousarray(z0[:, k]))) for k in range(len(al))]


def _compose(ls):
    f = ls[0]
    for l in ls[1:]:
        f = l @ f
    return f


def _tables(al, be, z0):
    return torch.tensor(al).cuda(), torch.tensor(be).cuda(), torch.tensor(np.ascontiguousarray(z0.T).reshape(-1)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _launches(bj):
    return int(bj._lib.load().bjx_launch_count())


def _c_params(bj, inverse, tabs, nl, x, g, lb, xb, outs="new", dim=None, batch=None, dt=None):
    """bjx_radial_stack_vjp_params -> (status, (alpha_bar, beta_bar, z0_bar [dim, nl]) device tensors)."""
    I = bj.interface
    ctx = I.context(tabs[1].device)
    dim = x.shape[0] if dim is None else dim
    batch = x.shape[1] if batch is None else batch
    if outs == "new":
        tt = tabs[1]
        outs = (torch.full((nl,), 7.0, dtype=tt.dtype, device="cuda"), torch.full((nl,), 7.0, dtype=tt.dtype, device="cuda"),
                torch.full((max(nl, 1) * dim,), 7.0, dtype=tt.dtype, device="cuda"))
    rc = bj._lib.load().bjx_radial_stack_vjp_params(ctx.h, I._dt(tabs[1]) if dt is None else dt, int(inverse), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl,
                                                    _p(x), _p(g), _p(lb), _p(xb), _p(outs[0]), _p(outs[1]), _p(outs[2]), dim, batch)
    return rc, outs


def _check_params(got, ref, dt, what, nl, dim):
    """got: (alpha_bar, beta_bar, z0_bar flat) device; ref: (…, ab, bb, zb [dim, nl], terms).  Layer by layer, per tensor."""
    _, ab, bb, zb, (ta, tb, tz) = ref
    ga, gb, gz = host(got[0]), host(got[1]), host(got[2]).reshape(nl, dim).T
    worst = 0.0
    for k in range(nl):
        worst = max(worst, flat_close(ga[k:k + 1], ab[k:k + 1], dt, f"{what} alpha_bar[{k}]", per="tensor", term_scale=ta[k]),
                    flat_close(gb[k:k + 1], bb[k:k + 1], dt, f"{what} beta_bar[{k}]", per="tensor", term_scale=tb[k]),
                    flat_close(gz[:, k], zb[:, k], dt, f"{what} z0_bar[{k}]", per="tensor", term_scale=tz[k]))
    return worst


@pytest.fixture(scope="module")
def refs(orc):
    """Per case: the draw and the oracle's results for both directions, with and without ℓ̄ — computed once, never written to."""
    out = {}
    for i, case in enumerate(CASES):
        dim, nl, N, dt = case
        c = _draw(orc, 3000 + i, dim, nl, N, dt)
        for inverse in (False, True):
            X = c["Yd"] if inverse else c["Z"]
            c[(inverse, True)] = ref_run_params(orc, c["al"], c["be"], c["z0"], X, c["G"], c["lbar"], inverse)
            c[(inverse, False)] = ref_run_params(orc, c["al"], c["be"], c["z0"], X, c["G"], None, inverse)
        out[case] = c
    return out


# ------------------------------------------------------------------ every path against the oracle (the C entry, called directly)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_oracle(bj, refs, case, inverse):
    dim, nl, N, dt = case
    c = refs[case]
    tabs = _tables(c["al"], c["be"], c["z0"])
    Xd, Gd, lbd = dev(c["Yd"] if inverse else c["Z"]), dev(c["G"]), torch.from_numpy(c["lbar"]).cuda()
    for with_l, with_xb in ((True, True), (False, True), (True, False), (False, False)):
        ref = c[(inverse, with_l)]
        xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T if with_xb else None
        torch.cuda.synchronize()
        n0 = _launches(bj)
        rc, outs = _c_params(bj, inverse, tabs, nl, Xd, Gd, lbd if with_l else None, xb)
        assert rc == 0
        assert _launches(bj) - n0 <= 3
        what = f"radial stack params {IDS[CASES.index(case)]} inverse={inverse} lbar={with_l} in_bar={with_xb}"
        if with_xb:
            flat_close(host(xb), ref[0], dt, what + " x_bar")
        worst = _check_params(outs, ref, dt, what, nl, dim)
        print(f"{what}: worst parameter error {worst:.3g} of its scale")


def test_scalar_packs_on_an_element_aligned_base(bj, orc):
    """Group form with V = 1: 8 Float32 rows whose base is one element past a 16-byte boundary."""
    dim, nl, N, dt = 8, 3, 37, np.float32
    c = _draw(orc, 3100, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])

    def off(a):                                           # (dim, N) column-major view that starts 4 bytes into its buffer
        buf = torch.empty(dim * N + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(N, dim).T
        if a is not None:
            v.copy_(dev(a))
        assert v.data_ptr() % 16 == 4
        return v
    lbd = torch.from_numpy(c["lbar"]).cuda()
    for inverse in (False, True):
        X = c["Yd"] if inverse else c["Z"]
        x, g, xb = off(X), off(c["G"]), off(None)
        rc, outs = _c_params(bj, inverse, tabs, nl, x, g, lbd, xb)
        assert rc == 0
        ref = ref_run_params(orc, c["al"], c["be"], c["z0"], X, c["G"], c["lbar"], inverse)
        flat_close(host(xb), ref[0], dt, f"radial stack params V = 1 inverse={inverse} x_bar")
        _check_params(outs, ref, dt, f"radial stack params V = 1 inverse={inverse}", nl, dim)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dim,N,dt", [(64, 4500, np.float32), (64, 4500, np.float64), (10, 8300, np.float32), (10, 8300, np.float64)])
def test_blocks_walk_many_tiles_and_the_first_fold_runs(bj, orc, dim, N, dt, inverse):
    """More than 32 blocks of several tiles each: three launches (the pass and both folds), the oracle's values, and the same bits from a
    second call (fixed-order sums, no atomics)."""
    nl = 3
    c = _draw(orc, 3200 + dim, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])
    X = c["Yd"] if inverse else c["Z"]
    Xd, Gd, lbd = dev(X), dev(c["G"]), torch.from_numpy(c["lbar"]).cuda()
    xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, outs = _c_params(bj, inverse, tabs, nl, Xd, Gd, lbd, xb)
    assert rc == 0 and _launches(bj) - n0 == 3
    ref = ref_run_params(orc, c["al"], c["be"], c["z0"], X, c["G"], c["lbar"], inverse)
    flat_close(host(xb), ref[0], dt, f"many tiles dim={dim} inverse={inverse} x_bar")
    _check_params(outs, ref, dt, f"many tiles dim={dim} inverse={inverse}", nl, dim)
    xb2 = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
    rc, outs2 = _c_params(bj, inverse, tabs, nl, Xd, Gd, lbd, xb2)
    assert rc == 0 and torch.equal(xb, xb2) and all(torch.equal(a, b) for a, b in zip(outs, outs2))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 67), (10, 70)])
def test_seventeen_layers(bj, orc, dim, N, dt, inverse):
    nl = 17
    c = _draw(orc, 3300 + dim, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])
    X = c["Yd"] if inverse else c["Z"]
    xb = torch.empty((N, dim), dtype=dev(X).dtype, device="cuda").T
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, outs = _c_params(bj, inverse, tabs, nl, dev(X), dev(c["G"]), torch.from_numpy(c["lbar"]).cuda(), xb)
    assert rc == 0 and _launches(bj) - n0 <= 3
    ref = ref_run_params(orc, c["al"], c["be"], c["z0"], X, c["G"], c["lbar"], inverse)
    flat_close(host(xb), ref[0], dt, f"17 layers dim={dim} inverse={inverse} x_bar")
    _check_params(outs, ref, dt, f"17 layers dim={dim} inverse={inverse}", nl, dim)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 67), (10, 70), (2, 65)])
def test_one_layer_is_the_single_layer_rule(bj, orc, dim, N, dt):
    """n_layers = 1 against bjx_radial_vjp_params (forward) and the host's implicit-function rule on it (inverse), at the flat bar."""
    c = _draw(orc, 3400 + dim, dim, 1, N, dt)
    layer = _layers(bj, c["al"], c["be"], c["z0"])[0]
    tabs = _tables(c["al"], c["be"], c["z0"])
    lbd = torch.from_numpy(c["lbar"]).cuda()
    for inverse in (False, True):
        Xd, Gd = dev(c["Yd"] if inverse else c["Z"]), dev(c["G"])
        x1, g1 = bj.vjp_params(bj.inverse(layer) if inverse else layer, Xd, Gd, lbd)
        xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
        rc, outs = _c_params(bj, inverse, tabs, 1, Xd, Gd, lbd, xb)
        assert rc == 0
        flat_close(host(xb), host(x1), dt, f"stack of one vs the single layer dim={dim} inverse={inverse} x_bar")
        for got, name in zip(outs, ("alpha_", "beta", "z_0")):
            flat_close(host(got).reshape(-1), host(g1[name]).reshape(-1), dt, f"stack of one vs the single layer dim={dim} inverse={inverse} {name}", per="tensor")


BITS = [(64, 3, 67), (128, 8, 130), (35, 3, 67), (10, 5, 130), (7, 3, 64)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", BITS)
def test_x_bar_is_the_input_pullbacks_bits(bj, orc, dim, nl, N, dt):
    """x̄ is bjx_radial_stack_vjp's, bit for bit: the pullback kernels of both files evaluate the sweeps with floating-point contraction
    off and explicit fused multiply-adds, so no rounding depends on the code around them.  The differing entries and the largest
    difference in units of the last place are printed before the assertion."""
    c = _draw(orc, 3500 + dim, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])
    lbd = torch.from_numpy(c["lbar"]).cuda()
    I = bj.interface
    same = True
    for inverse in (False, True):
        Xd, Gd = dev(c["Yd"] if inverse else c["Z"]), dev(c["G"])
        xv = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
        ctx = I.context(Xd.device)
        assert bj._lib.load().bjx_radial_stack_vjp(ctx.h, I._dt(Xd), int(inverse), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl, _p(Xd), _p(Gd), _p(lbd), _p(xv),
                                                   dim, N) == 0
        xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
        rc, outs = _c_params(bj, inverse, tabs, nl, Xd, Gd, lbd, xb)
        assert rc == 0
        a, b = host(xb), host(xv)
        ulp = np.abs(a - b) / np.spacing(np.abs(b))
        print(f"x_bar bits dim={dim} layers={nl} {np.dtype(dt).name} inverse={inverse}: {int((a != b).sum())} of {a.size} entries differ, largest difference {float(ulp.max()):.3g} ulp")
        same = same and torch.equal(xb, xv)
    assert same


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 67), (10, 5, 130)])
def test_in_bar_may_alias_out_bar(bj, orc, dim, nl, N, dt):
    """in_bar == out_bar gives the bits of the call with buffers of its own, x̄ and parameters."""
    c = _draw(orc, 3550 + dim, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])
    lbd = torch.from_numpy(c["lbar"]).cuda()
    for inverse in (False, True):
        Xd, Gd = dev(c["Yd"] if inverse else c["Z"]), dev(c["G"])
        xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
        rc, outs = _c_params(bj, inverse, tabs, nl, Xd, Gd, lbd, xb)
        assert rc == 0
        ga = dev(c["G"])
        rc, outs2 = _c_params(bj, inverse, tabs, nl, Xd, ga, lbd, ga)
        assert rc == 0 and torch.equal(ga, xb) and all(torch.equal(a, b) for a, b in zip(outs, outs2))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim", [64, 10])
def test_empty_batch_writes_zeros(bj, dim, dt):
    nl = 3
    al, be, z0 = _params(rng(3600), dim, nl, dt)
    tabs = _tables(al, be, z0)
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, outs = _c_params(bj, False, tabs, nl, None, None, None, None, dim=dim, batch=0)
    assert rc == 0 and _launches(bj) - n0 <= 1
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in outs)


def test_refused_height_falls_back_to_the_layers(bj, orc):
    """2 049 Float32 rows (the first height the register kernels refuse): BJX_ERR_UNSUPPORTED, nothing launched; `vjp_params` of that
    composition goes layer by layer and still gives the oracle's values."""
    dim, nl, N, dt = 2049, 2, 3, np.float32
    c = _draw(orc, 3700, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])
    Xd, Gd, lbd = dev(c["Z"]), dev(c["G"]), torch.from_numpy(c["lbar"]).cuda()
    xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
    torch.cuda.synchronize()
    n0 = _launches(bj)
    U = bj._lib.ERR_UNSUPPORTED
    assert _c_params(bj, False, tabs, nl, Xd, Gd, lbd, xb)[0] == U and _c_params(bj, True, tabs, nl, Xd, Gd, None, None)[0] == U
    assert _launches(bj) == n0
    flow = _compose(_layers(bj, c["al"], c["be"], c["z0"]))
    xg, gr = bj.vjp_params(flow, Xd, Gd, lbd)
    ref = ref_run_params(orc, c["al"], c["be"], c["z0"], c["Z"], c["G"], c["lbar"])
    flat_close(host(xg), ref[0], dt, "fallback x_bar")
    assert len(gr["stages"]) == nl
    for k in range(nl):
        d = gr["stages"][k]
        flat_close(host(d["alpha_"]), ref[1][k:k + 1], dt, f"fallback alpha_bar[{k}]", per="tensor", term_scale=ref[4][0][k])
        flat_close(host(d["beta"]), ref[2][k:k + 1], dt, f"fallback beta_bar[{k}]", per="tensor", term_scale=ref[4][1][k])
        flat_close(host(d["z_0"]), ref[3][:, k], dt, f"fallback z0_bar[{k}]", per="tensor", term_scale=ref[4][2][k])


def test_argument_checks_launch_nothing(bj):
    dim, nl, N, dt = 8, 2, 5, np.float32
    r = rng(3800)
    al, be, z0 = _params(r, dim, nl, dt)
    tabs = _tables(al, be, z0)
    x = dev(_points(r, dim, N, dt))
    xb = torch.empty((N, dim), dtype=x.dtype, device="cuda").T
    L = bj._lib
    good = _c_params(bj, False, tabs, nl, x, x, None, xb)[1]
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_params(bj, False, tabs, 0, x, x, None, xb, outs=good)[0] == L.ERR_SHAPE and _c_params(bj, False, tabs, -1, x, x, None, xb, outs=good)[0] == L.ERR_SHAPE
    assert _c_params(bj, False, tabs, nl, x, x, None, xb, outs=good, dim=0)[0] == L.ERR_SHAPE
    assert _c_params(bj, False, tabs, nl, x, x, None, xb, outs=good, batch=-1)[0] == L.ERR_SHAPE
    assert _c_params(bj, False, (None, tabs[1], tabs[2]), nl, x, x, None, xb, outs=good)[0] == L.ERR_ARG
    assert _c_params(bj, False, (tabs[0], tabs[1], None), nl, x, x, None, xb, outs=good)[0] == L.ERR_ARG
    assert _c_params(bj, False, tabs, nl, None, x, None, xb, outs=good, dim=dim, batch=N)[0] == L.ERR_ARG
    assert _c_params(bj, False, tabs, nl, x, None, None, xb, outs=good)[0] == L.ERR_ARG
    for k in range(3):
        assert _c_params(bj, False, tabs, nl, x, x, None, xb, outs=tuple(None if j == k else good[j] for j in range(3)))[0] == L.ERR_ARG
    assert _c_params(bj, False, tabs, nl, x, x, None, xb, outs=good, dt=77)[0] == L.ERR_ARG
    assert _launches(bj) == n0


# ------------------------------------------------------------------ through the planner
def _check_stage(d, ref, k, dt, what):
    flat_close(host(d["alpha_"]).reshape(-1), ref[1][k:k + 1], dt, f"{what} alpha_bar[{k}]", per="tensor", term_scale=ref[4][0][k])
    flat_close(host(d["beta"]).reshape(-1), ref[2][k:k + 1], dt, f"{what} beta_bar[{k}]", per="tensor", term_scale=ref[4][1][k])
    flat_close(host(d["z_0"]).reshape(-1), ref[3][:, k], dt, f"{what} z0_bar[{k}]", per="tensor", term_scale=ref[4][2][k])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 130), (10, 100)])
def test_planner_takes_the_fused_pass(bj, orc, dim, N, dt):
    """`vjp_params(run of three ∘ Shift)` and `vjp_params(inverse(run))` match the oracle, and the number of hot launches
    (`bj.kernel_timed`) does not grow with the number of layers: L = 3 and L = 6 take the same count (measured: 2 and 2, forward and
    inverse, at both heights and dtypes)."""
    counts = {}
    for nl in (3, 6):
        c = _draw(orc, 3900 + dim + nl, dim, nl, N, dt)
        ls = _layers(bj, c["al"], c["be"], c["z0"])
        run = _compose(ls)
        lbd, Gd = torch.from_numpy(c["lbar"]).cuda(), dev(c["G"])
        # Shift, then the run
        flow = run @ bj.Shift(0.5)
        assert [type(s).__name__ for s in flow._plan()[0]] == ["Shift", "_RadialRun"]
        Zd = dev(c["Z"])
        xg, gr = bj.vjp_params(flow, Zd, Gd, lbd)
        ref = ref_run_params(orc, c["al"], c["be"], c["z0"], c["Z"].astype(np.float64) + 0.5, c["G"], c["lbar"])
        flat_close(host(xg), ref[0], dt, f"Shift then {nl} radial layers, x_bar")
        assert len(gr["stages"]) == nl + 1
        for k in range(nl):
            assert gr["stages"][1 + k]["z_0"].shape == ls[k].z_0.shape and gr["stages"][1 + k]["alpha_"].shape == ls[k].alpha_.shape
            _check_stage(gr["stages"][1 + k], ref, k, dt, f"Shift then {nl} radial layers")
        # the inverse run: stage j of inverse(run) is inverse(layer L-1-j)
        inv = bj.inverse(run)
        Yd = dev(c["Yd"])
        yg, gi = bj.vjp_params(inv, Yd, Gd, lbd)
        refi = ref_run_params(orc, c["al"], c["be"], c["z0"], c["Yd"], c["G"], c["lbar"], inverse=True)
        flat_close(host(yg), refi[0], dt, f"inverse of {nl} radial layers, y_bar")
        assert len(gi["stages"]) == nl
        for j in range(nl):
            _check_stage(gi["stages"][j], refi, nl - 1 - j, dt, f"inverse of {nl} radial layers")
        _, _, kf = bj.kernel_timed(lambda: bj.vjp_params(run, Zd, Gd, lbd))
        _, _, ki = bj.kernel_timed(lambda: bj.vjp_params(inv, Yd, Gd, lbd))
        counts[nl] = (kf, ki)
    print(f"dim {dim} {np.dtype(dt).name}: hot launches of vjp_params (forward, inverse): L = 3 {counts[3]}, L = 6 {counts[6]}")
    assert counts[3] == counts[6]
    assert max(counts[3]) <= 3


def test_mixed_flow_returns_one_dictionary_per_stage(bj, orc):
    """planar ∘ radial-run ∘ planar: every original stage gets its own dictionary; the radial ones are the oracle's."""
    r = rng(4000)
    dim, N, dt = 10, 333, np.float64
    al, be, z0 = _params(r, dim, 3, dt)
    rs = _layers(bj, al, be, z0)
    w = (r.normal(size=(dim, 2)) / math.sqrt(dim)).astype(dt)
    u = (r.normal(size=(dim, 2)) / math.sqrt(dim)).astype(dt)
    pb = r.normal(size=2).astype(dt)
    ps = [bj.PlanarLayer(torch.tensor(np.ascontiguousarray(w[:, k])).cuda(), torch.tensor(np.ascontiguousarray(u[:, k])).cuda(), torch.tensor(pb[k:k + 1]).cuda()) for k in range(2)]
    Z = _points(r, dim, N, dt)
    G = np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = r.normal(size=N).astype(dt)
    flow = ps[1] @ rs[2] @ rs[1] @ rs[0] @ ps[0]
    assert [type(s).__name__ for s in flow._plan()[0]] == ["PlanarLayer", "_RadialRun", "PlanarLayer"]
    xg, gr = bj.vjp_params(flow, dev(Z), dev(G), torch.from_numpy(lbar).cuda())
    assert len(gr["stages"]) == 5
    assert set(gr["stages"][0]) == {"w", "u", "b"} and set(gr["stages"][4]) == {"w", "u", "b"}
    Z1 = orc.planar(w[:, 0], u[:, 0], pb[0:1], Z)[0]
    Z2 = Z1
    for k in range(3):
        Z2 = orc.radial(al[k], be[k], z0[:, k], np.asfortranarray(Z2))[0]
    G2 = orc.planar_vjp(w[:, 1], u[:, 1], pb[1:2], Z2, G, lbar)               # cotangent on the radial run's output
    ref = ref_run_params(orc, al, be, z0, Z1, G2, lbar)
    for k in range(3):
        assert set(gr["stages"][1 + k]) == {"alpha_", "beta", "z_0"}
        _check_stage(gr["stages"][1 + k], ref, k, dt, "planar, three radial, planar")
    flat_close(host(xg), orc.planar_vjp(w[:, 0], u[:, 0], pb[0:1], Z, ref[0], lbar), dt, "planar, three radial, planar: x_bar")


# ------------------------------------------------------------------ independent of the closed forms
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dim,N", [(64, 67), (10, 70)])
def test_central_differences_of_the_objective(bj, orc, dim, N, inverse):
    """Float64: d/dθ [Σ ȳ·y(θ) + Σ ℓ̄·ladj(θ)] through the oracle's forward and inverse MAPS, central differences (step 1e-5: truncation
    ~1e-10·|f‴|, rounding ~1e-16·|f|/1e-5 ~ 1e-9 relative to the objective's terms), for α_, β and one z₀ entry of the middle layer of
    three.  Bar: 1e-6 of max(|derivative|, max |summand|) — the flat Float64 bar on the same scale as the other tests."""
    nl, dt, mid = 3, np.float64, 1
    c = _draw(orc, 4100 + dim, dim, nl, N, dt)
    tabs = _tables(c["al"], c["be"], c["z0"])
    X = c["Yd"] if inverse else c["Z"]
    rc, outs = _c_params(bj, inverse, tabs, nl, dev(X), dev(c["G"]), torch.from_numpy(c["lbar"]).cuda(), None)
    assert rc == 0
    ref = ref_run_params(orc, c["al"], c["be"], c["z0"], X, c["G"], c["lbar"], inverse)
    ga, gb, gz = host(outs[0]), host(outs[1]), host(outs[2]).reshape(nl, dim).T
    h = 1e-5

    def fd(which, row=None):
        vals = []
        for s in (+1.0, -1.0):
            al, be, z0 = c["al"].copy(), c["be"].copy(), c["z0"].copy()
            if which == "alpha_":
                al[mid] += s * h
            elif which == "beta":
                be[mid] += s * h
            else:
                z0[row, mid] += s * h
            vals.append(run_objective(orc, al, be, z0, X, c["G"], c["lbar"], inverse))
        return (vals[0] - vals[1]) / (2 * h)

    row = dim // 3
    for got, which, term, rw in ((ga[mid], "alpha_", ref[4][0][mid], None), (gb[mid], "beta", ref[4][1][mid], None), (gz[row, mid], "z_0", ref[4][2][mid], row)):
        d = fd(which, rw)
        err = abs(got - d) / max(abs(d), term)
        print(f"central difference dim={dim} inverse={inverse} {which}: kernel {got:.12g}, difference {d:.12g}, error {err:.3g} of its scale")
        assert err <= 1e-6, f"{which}: {got} vs {d}"
