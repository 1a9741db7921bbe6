"""Value and gradients of the log-density of a transformed distribution (`bj.logpdf_vjp_params`) and the fused pass for runs of
RadialLayers behind it (include/bjx_radial_stack_logpdf.h: bjx_radial_stack_logpdf_vjp_params), against Float64 numpy
(tests/_logpdf_grad_ref.py, pinned against central differences by tests/test_host_logpdf_grad.py): the oracle's inverse run layer by
layer for x and ℓ, the closed forms for lp, x̄, μ̄, σ̄, and `ref_run_params(…, inverse=True)` on (x̄, c) for ȳ and the layers' cotangents.

Bars: `flat_close` (1e-3 Float32, 1e-6 Float64, flat) — ȳ per sample; every parameter tensor (one layer's ᾱ_, β̄ or z̄₀, μ̄, σ̄) per
tensor with `term_scale` = the max-norm of that sum's summands; lp with `close` at scale n_layers + dim (the existing logpdf check of
tests/test_gpu_radial_stack.py).  Nothing else multiplies a bar.

Parameters and points are drawn as tests/test_gpu_radial_stack_params.py draws them (its helpers are imported); y is the rounded image
of the forward run.  Shapes: one per dispatch branch of that file's list — whole 16-byte packs (128 x 8 x 130, 64 x 3 x 257, and 384
rows for more than one pack per lane: 512 x 2 with the base rows is past the LDS budget, `test_lds_budget`), a partial last pack (35 rows), scalar packs / element-aligned staging (a base one element past
a 16-byte boundary), the lane-per-column form (2 and 7 rows, 10 rows x 8 layers), 17 layers, and the batches at which blocks walk
several tiles and both fold levels run (64 x 4 500, 10 x 8 300)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _logpdf_grad_ref import ref_logpdf_grad  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, close, dev, host, rng  # noqa: E402,F401  (fixtures / helpers)
from test_gpu_radial_stack_params import _compose, _image, _launches, _layers, _p, _params, _points, _tables  # noqa: E402

DTYPES = [np.float32, np.float64]
SHAPES = [(128, 8, 130), (64, 3, 257), (384, 2, 9), (35, 3, 67), (2, 4, 65), (7, 3, 64), (10, 8, 130), (64, 17, 67), (10, 17, 70)]
CASES = [(d, nl, N, dt) for (d, nl, N) in SHAPES for dt in DTYPES]
IDS = [f"{d}x{nl}x{N}-{np.dtype(dt).name}" for d, nl, N, dt in CASES]
BASES = ["standard", "standard-with-bars", "diagonal", "diagonal-no-bars"]


def _draw(orc, seed, dim, nl, N, dt):
    r = rng(seed)
    al, be, z0 = _params(r, dim, nl, dt)
    Z = _points(r, dim, N, dt)
    c = r.normal(size=N).astype(dt)
    mu = (0.2 * r.normal(size=dim)).astype(dt)
    sigma = np.exp(0.3 * r.normal(size=dim)).astype(dt)
    return dict(al=al, be=be, z0=z0, c=c, mu=mu, sigma=sigma, Y=_image(orc, al, be, z0, Z, dt))


def _force_generic(run, tdt, dim):
    """Fill the run's memory of refusals so that `logpdf_vjp_params` takes the generic path (its own fused launches stay)."""
    run._refused.update({("logpdf", tdt, dim, False), ("logpdf", tdt, dim, True)})


def _ref(orc, d, diagonal, c="own"):
    return ref_logpdf_grad(orc, d["al"], d["be"], d["z0"], d["mu"] if diagonal else None, d["sigma"] if diagonal else None, d["Y"], d["c"] if isinstance(c, str) else c)


def _c_logpdf(bj, tabs, nl, mu, sigma, y, c, dim=None, batch=None, dt=None, lp=True, lp_sum=True, y_bar=True, layers=True, base=True):
    """bjx_radial_stack_logpdf_vjp_params -> (status, dict of the outputs asked for, device tensors pre-filled with 7)."""
    I = bj.interface
    tt = tabs[1]
    ctx = I.context(tt.device)
    dim = y.shape[0] if dim is None else dim
    batch = y.shape[1] if batch is None else batch
    nb = max(batch, 0)
    full = lambda *s: torch.full(s, 7.0, dtype=tt.dtype, device="cuda")
    o = dict(lp=full(nb) if lp else None, lp_sum=torch.full((1,), 7.0, dtype=torch.float64, device="cuda") if lp_sum else None,
             y_bar=torch.full((nb, max(dim, 0)), 7.0, dtype=tt.dtype, device="cuda").T if y_bar else None,
             alpha_bar=full(nl) if layers else None, beta_bar=full(nl) if layers else None, z0_bar=full(max(nl, 1) * dim) if layers else None,
             mu_bar=full(max(dim, 0)) if base else None, sigma_bar=full(max(dim, 0)) if base else None)
    rc = bj._lib.load().bjx_radial_stack_logpdf_vjp_params(ctx.h, I._dt(tt) if dt is None else dt, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl, _p(mu), _p(sigma), _p(y), _p(c),
                                                           _p(o["lp"]), _p(o["lp_sum"]), _p(o["y_bar"]), _p(o["alpha_bar"]), _p(o["beta_bar"]), _p(o["z0_bar"]),
                                                           _p(o["mu_bar"]), _p(o["sigma_bar"]), dim, batch)
    return rc, o


def _check(o, ref, dt, what, nl, dim):
    """Every output present in `o` against the reference at the bars of the module docstring; returns the worst gradient error."""
    worst = 0.0
    if o.get("lp") is not None:
        close(host(o["lp"]), ref["lp"], dt, scale=nl + dim, what=what + " lp")
    if o.get("lp_sum") is not None:
        s, r = float(o["lp_sum"][0]), float(ref["lp"].sum())
        print(f"{what} lp_sum {s:.10g} vs {r:.10g}")
        close(np.array([s / max(len(ref["lp"]), 1)]), np.array([r / max(len(ref["lp"]), 1)]), dt, scale=nl + dim, what=what + " mean lp")
    if o.get("y_bar") is not None:
        worst = max(worst, flat_close(host(o["y_bar"]), ref["y_bar"], dt, what + " y_bar"))
    ta, tb, tz = ref["terms"]
    if o.get("z0_bar") is not None:
        ga, gb, gz = host(o["alpha_bar"]), host(o["beta_bar"]), host(o["z0_bar"]).reshape(nl, dim).T
        for k in range(nl):
            worst = max(worst, flat_close(ga[k:k + 1], ref["alpha_bar"][k:k + 1], dt, f"{what} alpha_bar[{k}]", per="tensor", term_scale=ta[k]),
                        flat_close(gb[k:k + 1], ref["beta_bar"][k:k + 1], dt, f"{what} beta_bar[{k}]", per="tensor", term_scale=tb[k]),
                        flat_close(gz[:, k], ref["z0_bar"][:, k], dt, f"{what} z0_bar[{k}]", per="tensor", term_scale=tz[k]))
    if o.get("mu_bar") is not None:
        worst = max(worst, flat_close(host(o["mu_bar"]), ref["mu_bar"], dt, what + " mu_bar", per="tensor", term_scale=ref["t_mu"]),
                    flat_close(host(o["sigma_bar"]), ref["sigma_bar"], dt, what + " sigma_bar", per="tensor", term_scale=ref["t_sigma"]))
    return worst


@pytest.fixture(scope="module")
def refs(orc):
    """Per case: the draw and the reference for the standard and the diagonal base — computed once, never written to."""
    out = {}
    for i, case in enumerate(CASES):
        dim, nl, N, dt = case
        d = _draw(orc, 5000 + i, dim, nl, N, dt)
        d["standard"] = _ref(orc, d, False)
        d["diagonal"] = _ref(orc, d, True)
        out[case] = d
    return out


# ------------------------------------------------------------------ every form of the kernel, every base variant (the C entry)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_reference(bj, refs, case):
    dim, nl, N, dt = case
    d = refs[case]
    tabs = _tables(d["al"], d["be"], d["z0"])
    yd, cd, mud, sgd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda(), torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda()
    for base in BASES:
        diag = base.startswith("diagonal")                            # standard-with-bars: mu = sigma = NULL, mu_bar and sigma_bar asked for
        torch.cuda.synchronize()
        n0 = _launches(bj)
        rc, o = _c_logpdf(bj, tabs, nl, mud if diag else None, sgd if diag else None, yd, cd, base=base in ("diagonal", "standard-with-bars"))
        assert rc == 0
        assert _launches(bj) - n0 <= 3
        what = f"radial logpdf {IDS[CASES.index(case)]} base={base}"
        worst = _check(o, d["diagonal" if diag else "standard"], dt, what, nl, dim)
        print(f"{what}: worst gradient error {worst:.3g} of its scale")


@pytest.mark.parametrize("dt", DTYPES)
def test_element_aligned_base_pointer(bj, orc, dt):
    """8 rows on a base one element past a 16-byte boundary: the group form with V = 1 (Float32) / scalar tile staging (Float64)."""
    dim, nl, N = 8, 3, 37
    d = _draw(orc, 5100, dim, nl, N, dt)
    tabs = _tables(d["al"], d["be"], d["z0"])
    tdt = torch.float32 if dt == np.float32 else torch.float64
    buf = torch.empty(dim * N + 1, dtype=tdt, device="cuda")
    y = buf[1:].view(N, dim).T
    y.copy_(dev(d["Y"]))
    assert y.data_ptr() % 16 == np.dtype(dt).itemsize
    rc, o = _c_logpdf(bj, tabs, nl, torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda(), y, torch.from_numpy(d["c"]).cuda())
    assert rc == 0
    _check(o, _ref(orc, d, True), dt, f"radial logpdf element-aligned {np.dtype(dt).name}", nl, dim)


def test_lds_budget(bj, orc):
    """512 Float32 rows x 2 layers: with the rows of μ̄ and σ̄ the four wave tables alone are 4·(2·514 + 1 + 1 024)·8 = 65 696 bytes, past
    the 64 KiB budget — BJX_ERR_UNSUPPORTED, nothing launched; without them (40.2 KiB) the entry serves the shape."""
    dim, nl, N, dt = 512, 2, 9, np.float32
    d = _draw(orc, 5150, dim, nl, N, dt)
    tabs = _tables(d["al"], d["be"], d["z0"])
    yd, cd, mud, sgd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda(), torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda()
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_logpdf(bj, tabs, nl, mud, sgd, yd, cd)[0] == bj._lib.ERR_UNSUPPORTED
    assert _launches(bj) == n0
    rc, o = _c_logpdf(bj, tabs, nl, mud, sgd, yd, cd, base=False)
    assert rc == 0
    _check(o, _ref(orc, d, True), dt, "radial logpdf 512 rows without the base rows", nl, dim)


@pytest.mark.parametrize("dim,N,dt", [(64, 4500, np.float32), (64, 4500, np.float64), (10, 8300, np.float32), (10, 8300, np.float64)])
def test_blocks_walk_many_tiles_both_folds_and_repeat_bits(bj, orc, dim, N, dt):
    """More than 32 blocks of several tiles each: three launches (the pass and both folds), the reference's values, and the same bits in
    EVERY output from a second call (fixed-order sums, no atomics)."""
    nl = 3
    d = _draw(orc, 5200 + dim, dim, nl, N, dt)
    tabs = _tables(d["al"], d["be"], d["z0"])
    args = (bj, tabs, nl, torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda(), dev(d["Y"]), torch.from_numpy(d["c"]).cuda())
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, o = _c_logpdf(*args)
    assert rc == 0 and _launches(bj) - n0 == 3
    _check(o, _ref(orc, d, True), dt, f"radial logpdf many tiles dim={dim} {np.dtype(dt).name}", nl, dim)
    rc, o2 = _c_logpdf(*args)
    assert rc == 0
    for k in o:
        assert torch.equal(o[k], o2[k]), f"{k} differs between two identical calls"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 67), (10, 5, 130)])
def test_repeat_call_bits_small(bj, orc, dim, nl, N, dt):
    d = _draw(orc, 5250 + dim, dim, nl, N, dt)
    tabs = _tables(d["al"], d["be"], d["z0"])
    args = (bj, tabs, nl, torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda(), dev(d["Y"]), torch.from_numpy(d["c"]).cuda())
    (rc, o), (rc2, o2) = _c_logpdf(*args), _c_logpdf(*args)
    assert rc == 0 and rc2 == 0
    for k in o:
        assert torch.equal(o[k], o2[k]), f"{k} differs between two identical calls"


# ------------------------------------------------------------------ lp_bar variants (public function)
def _td(bj, d, diagonal):
    ls = _layers(bj, d["al"], d["be"], d["z0"])
    flow = _compose(ls) if len(ls) > 1 else ls[0]
    base = bj.MvNormal(torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda()) if diagonal else bj.MvNormal(len(d["mu"]))
    return bj.transformed(base, flow), ls


def _public_as_outputs(lp, yb, grads, nl, dim):
    """The public function's results in the layout `_check` reads (stage j of inverse(run) is inverse(layer nl-1-j))."""
    o = dict(lp=lp, y_bar=yb)
    if grads:
        st = grads["transform"]["stages"][::-1] if "stages" in grads["transform"] else [grads["transform"]]
        o.update(alpha_bar=torch.cat([s["alpha_"].reshape(-1) for s in st]), beta_bar=torch.cat([s["beta"].reshape(-1) for s in st]),
                 z0_bar=torch.cat([s["z_0"].reshape(-1) for s in st]))
        if "mu" in grads["base"]:
            o.update(mu_bar=grads["base"]["mu"], sigma_bar=grads["base"]["sigma"])
    return o


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 67), (10, 5, 130)])
def test_lp_bar_variants(bj, orc, dim, nl, N, dt):
    """None (= 1), a Python number, a (batch,) tensor, and all zeros: ȳ and every gradient are then EXACTLY zero and lp is still right."""
    d = _draw(orc, 5300 + dim, dim, nl, N, dt)
    td, _ = _td(bj, d, True)
    yd = dev(d["Y"])
    for name, arg, cref in (("None", None, None), ("number", 0.7, np.full(N, 0.7)), ("tensor", torch.from_numpy(d["c"]).cuda(), d["c"])):
        lp, yb, g = bj.logpdf_vjp_params(td, yd, arg)
        _check(_public_as_outputs(lp, yb, g, nl, dim), _ref(orc, d, True, c=cref), dt, f"lp_bar={name} dim={dim} {np.dtype(dt).name}", nl, dim)
    for zero in (0.0, torch.zeros(N, dtype=yd.dtype, device="cuda")):
        lp, yb, g = bj.logpdf_vjp_params(td, yd, zero)
        o = _public_as_outputs(lp, yb, g, nl, dim)
        close(host(lp), _ref(orc, d, True)["lp"], dt, scale=nl + dim, what="lp with a zero cotangent")
        for k in ("y_bar", "alpha_bar", "beta_bar", "z0_bar", "mu_bar", "sigma_bar"):
            assert float(o[k].abs().max()) == 0.0, f"{k} is not exactly zero for a zero cotangent"


# ------------------------------------------------------------------ optional outputs
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 67), (10, 5, 130)])
def test_optional_outputs(bj, orc, dim, nl, N, dt):
    """y_bar = NULL leaves every parameter result bit-identical to the call that writes it; with the three layer cotangents NULL (and
    with nothing summed over the batch asked for: one launch) ȳ and lp are unchanged."""
    d = _draw(orc, 5400 + dim, dim, nl, N, dt)
    tabs = _tables(d["al"], d["be"], d["z0"])
    args = (bj, tabs, nl, torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda(), dev(d["Y"]), torch.from_numpy(d["c"]).cuda())
    rc, full = _c_logpdf(*args)
    assert rc == 0
    rc, o = _c_logpdf(*args, y_bar=False)
    assert rc == 0
    for k in ("lp", "lp_sum", "alpha_bar", "beta_bar", "z0_bar", "mu_bar", "sigma_bar"):
        assert torch.equal(o[k], full[k]), f"{k} changes when y_bar is not written"
    rc, o = _c_logpdf(*args, layers=False)
    assert rc == 0
    for k in ("lp", "lp_sum", "y_bar", "mu_bar", "sigma_bar"):
        assert torch.equal(o[k], full[k]), f"{k} changes when the layer cotangents are not written"
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, o = _c_logpdf(*args, layers=False, base=False, lp_sum=False)
    assert rc == 0 and _launches(bj) - n0 == 1
    assert torch.equal(o["y_bar"], full["y_bar"]) and torch.equal(o["lp"], full["lp"])
    # two of the three layer cotangents is an argument error
    I = bj.interface
    ctx = I.context(tabs[1].device)
    one = torch.empty(nl, dtype=tabs[1].dtype, device="cuda")
    assert bj._lib.load().bjx_radial_stack_logpdf_vjp_params(ctx.h, I._dt(tabs[1]), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl, None, None, _p(args[5]), None, None, None, None,
                                                             _p(one), _p(one), None, None, None, dim, N) == bj._lib.ERR_ARG


# ------------------------------------------------------------------ one layer: a stack of one against the generic path
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 67), (10, 70), (2, 65)])
def test_one_layer_matches_the_generic_path(bj, orc, dim, N, dt):
    d = _draw(orc, 5500 + dim, dim, 1, N, dt)
    td, ls = _td(bj, d, True)
    yd, cd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda()
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    assert set(g["transform"]) == {"alpha_", "beta", "z_0"}                      # what vjp_params(inverse(RadialLayer)) returns
    _, _, kf = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    run = ls[0].__dict__["_stack_of_one"]
    _force_generic(run, yd.dtype, dim)
    lp2, yb2, g2 = bj.logpdf_vjp_params(td, yd, cd)
    _, _, kg = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    print(f"one layer dim={dim} {np.dtype(dt).name}: hot launches fused {kf}, generic {kg}")
    assert kf <= 3 and kg > kf
    what = f"stack of one vs generic dim={dim} {np.dtype(dt).name}"
    close(host(lp), host(lp2), dt, scale=1 + dim, what=what + " lp")
    flat_close(host(yb), host(yb2), dt, what + " y_bar")
    for name in ("alpha_", "beta", "z_0"):
        assert g["transform"][name].shape == g2["transform"][name].shape
        flat_close(host(g["transform"][name]).reshape(-1), host(g2["transform"][name]).reshape(-1), dt, f"{what} {name}", per="tensor")
    for name in ("mu", "sigma"):
        flat_close(host(g["base"][name]), host(g2["base"][name]), dt, f"{what} {name}", per="tensor")
    _check(_public_as_outputs(lp, yb, g, 1, dim), _ref(orc, d, True), dt, what + " (reference)", 1, dim)


# ------------------------------------------------------------------ the public function
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("diagonal", [False, True])
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 130), (10, 4, 100)])
def test_public_function(bj, orc, dim, nl, N, diagonal, dt):
    d = _draw(orc, 5600 + dim, dim, nl, N, dt)
    td, ls = _td(bj, d, diagonal)
    yd, cd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda()
    what = f"public dim={dim} L={nl} {np.dtype(dt).name} diagonal={diagonal}"
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    ref = _ref(orc, d, diagonal)
    _check(_public_as_outputs(lp, yb, g, nl, dim), ref, dt, what, nl, dim)
    close(host(lp), host(bj.logpdf(td, yd)), dt, scale=nl + dim, what=what + " lp vs bj.logpdf")
    _, _, kf = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    assert kf <= 3, f"the fused call took {kf} hot launches"
    # keys, shapes and order of vjp_params(inverse(flow), …)
    inv = bj.inverse(td.transform)
    _, gv = bj.vjp_params(inv, yd, dev(ref["x_bar"].astype(dt)), cd)
    assert set(g) == {"transform", "base"} and set(g["base"]) == ({"mu", "sigma"} if diagonal else set())
    assert list(g["transform"]) == ["stages"] and len(g["transform"]["stages"]) == len(gv["stages"]) == nl
    for j in range(nl):
        a, b = g["transform"]["stages"][j], gv["stages"][j]
        assert set(a) == set(b) == {"alpha_", "beta", "z_0"}
        for name in a:
            assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype
            flat_close(host(a[name]).reshape(-1), host(b[name]).reshape(-1), dt, f"{what} stage {j} {name} vs vjp_params", per="tensor",
                       term_scale=ref["terms"][("alpha_", "beta", "z_0").index(name)][nl - 1 - j])
    # params=False: only the input pullback; want_y_bar=False
    lp3, yb3, g3 = bj.logpdf_vjp_params(td, yd, cd, params=False)
    assert g3 == {} and torch.equal(yb3, yb) and torch.equal(lp3, lp)
    lp4, yb4, g4 = bj.logpdf_vjp_params(td, yd, cd, want_y_bar=False)
    assert yb4 is None and torch.equal(lp4, lp)
    # vector input
    lpv, ybv, gvv = bj.logpdf_vjp_params(td, yd[:, 0].contiguous(), float(d["c"][0]))
    assert ybv.shape == (dim,)
    close(host(lpv).reshape(-1), ref["lp"][:1], dt, scale=nl + dim, what=what + " vector lp")
    flat_close(host(ybv).reshape(dim, 1), ref["y_bar"][:, :1], dt, what + " vector y_bar")
    # the generic path, forced: the same answers at the flat bar, through more launches
    run = bj.interface._td_inverse(td)._plan()[0][0].orig
    assert type(run).__name__ == "_RadialRun"
    _force_generic(run, yd.dtype, dim)
    lp2, yb2, g2 = bj.logpdf_vjp_params(td, yd, cd)
    _, _, kg = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    print(f"{what}: hot launches fused {kf}, generic {kg}")
    assert kg > kf
    o, o2 = _public_as_outputs(lp, yb, g, nl, dim), _public_as_outputs(lp2, yb2, g2, nl, dim)
    close(host(lp), host(lp2), dt, scale=nl + dim, what=what + " fused vs generic lp")
    flat_close(host(yb), host(yb2), dt, what + " fused vs generic y_bar")
    _check(o2, ref, dt, what + " generic", nl, dim)
    ta, tb, tz = ref["terms"]
    for k in range(nl):
        flat_close(host(o["alpha_bar"])[k:k + 1], host(o2["alpha_bar"])[k:k + 1], dt, f"{what} fused vs generic alpha_bar[{k}]", per="tensor", term_scale=ta[k])
        flat_close(host(o["beta_bar"])[k:k + 1], host(o2["beta_bar"])[k:k + 1], dt, f"{what} fused vs generic beta_bar[{k}]", per="tensor", term_scale=tb[k])
        flat_close(host(o["z0_bar"])[k * dim:(k + 1) * dim], host(o2["z0_bar"])[k * dim:(k + 1) * dim], dt, f"{what} fused vs generic z0_bar[{k}]", per="tensor", term_scale=tz[k])
    if diagonal:
        flat_close(host(o["mu_bar"]), host(o2["mu_bar"]), dt, what + " fused vs generic mu_bar", per="tensor", term_scale=ref["t_mu"])
        flat_close(host(o["sigma_bar"]), host(o2["sigma_bar"]), dt, what + " fused vs generic sigma_bar", per="tensor", term_scale=ref["t_sigma"])


# ------------------------------------------------------------------ edges of the C entry
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim", [64, 10])
def test_empty_batch_writes_zeros_and_launches_nothing(bj, dim, dt):
    nl = 3
    al, be, z0 = _params(rng(5700), dim, nl, dt)
    tabs = _tables(al, be, z0)
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, o = _c_logpdf(bj, tabs, nl, None, None, None, None, dim=dim, batch=0)
    assert rc == 0 and _launches(bj) == n0
    torch.cuda.synchronize()
    for k in ("lp_sum", "alpha_bar", "beta_bar", "z0_bar", "mu_bar", "sigma_bar"):
        assert float(o[k].abs().max()) == 0.0, k


def test_refused_height_goes_through_the_layers(bj, orc):
    """4 096 Float32 rows: BJX_ERR_UNSUPPORTED from the C entry, nothing launched; the public function remembers it and still returns
    the reference's values through the layers."""
    dim, nl, N, dt = 4096, 2, 3, np.float32
    d = _draw(orc, 5800, dim, nl, N, dt)
    tabs = _tables(d["al"], d["be"], d["z0"])
    yd, cd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda()
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_logpdf(bj, tabs, nl, None, None, yd, cd)[0] == bj._lib.ERR_UNSUPPORTED
    assert _launches(bj) == n0
    td, _ = _td(bj, d, True)
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    _check(_public_as_outputs(lp, yb, g, nl, dim), _ref(orc, d, True), dt, "refused height, through the layers", nl, dim)
    run = bj.interface._td_inverse(td)._plan()[0][0].orig
    assert ("logpdf", yd.dtype, dim, True) in run._refused


def test_public_function_remembers_the_lds_refusal_per_request(bj, orc):
    """512 Float32 rows x 2 layers on a diagonal base: with the parameters asked for the entry refuses (the rows of μ̄ / σ̄ put its tables
    past the LDS budget) — the function answers through the generic path and remembers THAT request; `params=False` on the same
    distribution still takes the fused pass (one hot launch), and both give the reference's values."""
    dim, nl, N, dt = 512, 2, 9, np.float32
    d = _draw(orc, 5850, dim, nl, N, dt)
    td, _ = _td(bj, d, True)
    yd, cd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda()
    ref = _ref(orc, d, True)
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    _check(_public_as_outputs(lp, yb, g, nl, dim), ref, dt, "512 x 2 with the base rows, generic", nl, dim)
    run = bj.interface._td_inverse(td)._plan()[0][0].orig
    assert ("logpdf", yd.dtype, dim, True) in run._refused and ("logpdf", yd.dtype, dim, False) not in run._refused
    (lp2, yb2, g2), _, k = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd, params=False))
    assert g2 == {} and k == 1, f"params=False took {k} hot launches"
    assert ("logpdf", yd.dtype, dim, False) not in run._refused
    _check(dict(lp=lp2, y_bar=yb2), ref, dt, "512 x 2, params=False, fused", nl, dim)


def test_argument_checks_launch_nothing(bj):
    dim, nl, N, dt = 8, 2, 5, np.float32
    r = rng(5900)
    al, be, z0 = _params(r, dim, nl, dt)
    tabs = _tables(al, be, z0)
    y = dev(_points(r, dim, N, dt))
    Lb = bj._lib
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_logpdf(bj, tabs, nl, None, None, y, None, dim=0)[0] == Lb.ERR_SHAPE
    assert _c_logpdf(bj, tabs, nl, None, None, y, None, batch=-1)[0] == Lb.ERR_SHAPE
    assert _c_logpdf(bj, tabs, 0, None, None, y, None)[0] == Lb.ERR_SHAPE
    assert _c_logpdf(bj, (None, tabs[1], tabs[2]), nl, None, None, y, None)[0] == Lb.ERR_ARG
    assert _c_logpdf(bj, tabs, nl, None, None, None, None, dim=dim, batch=N)[0] == Lb.ERR_ARG
    assert _c_logpdf(bj, tabs, nl, None, None, y, None, dt=77)[0] == Lb.ERR_ARG
    assert _launches(bj) == n0


# ------------------------------------------------------------------ the generic path on other transforms, against central differences
def _fd_check(name, got, f, h=1e-5):
    """Central difference of the objective f(±h) in Float64 (truncation ~h², rounding ~1e-16·|f|/h ~ 1e-10 of the objective's terms)
    against one entry `got` of a gradient tensor whose max-norm is `scale`: 1e-6 of max(|difference|, scale), the flat Float64 bar."""
    got, scale = got
    d = (f(+h) - f(-h)) / (2 * h)
    err = abs(got - d) / max(abs(d), scale)
    print(f"central difference {name}: function {got:.12g}, difference {d:.12g}, error {err:.3g} of its scale")
    assert err <= 1e-6, f"{name}: {got} vs {d}"


def _base_lp(x, mu, sigma):
    w = (x - mu.reshape(-1, 1)) / sigma.reshape(-1, 1)
    return -0.5 * (w * w).sum(axis=0) - np.log(sigma).sum() - 0.5 * x.shape[0] * math.log(2 * math.pi)


def _entry(t, idx):
    t = host(t).reshape(-1) if t.dim() != 2 else host(t)
    return float(t[idx]), float(np.abs(t).max())


def test_generic_elementwise_chain_with_a_diagonal_base(bj, orc):
    """exp ∘ Shift(m) ∘ Scale(s): the inverse is inverse(Scale(s)) ∘ Shift(−m) ∘ log, whose stages own the parameters −m and s."""
    dim, N = 5, 9
    r = rng(6000)
    m, s = 0.3 * r.normal(size=dim), np.exp(0.2 * r.normal(size=dim))
    mu, sigma = 0.2 * r.normal(size=dim), np.exp(0.3 * r.normal(size=dim))
    Y = np.asfortranarray(np.exp(0.5 * r.normal(size=(dim, N))))
    c = r.normal(size=N)
    T = lambda a: torch.tensor(a).cuda()
    ms, ss, mus, sgs = T(m), T(s), T(mu), T(sigma)
    td = bj.transformed(bj.MvNormal(mus, sgs), bj.elementwise(bj.exp) @ bj.Shift(ms) @ bj.Scale(ss))

    def obj(m=m, s=s, mu=mu, sigma=sigma, Y=Y):
        tot = 0.0
        for n in range(N):                                            # the oracle's chain returns one log-det per call: column by column
            x, l = orc.chain([(orc.OP_LOG, None, None), (orc.OP_SHIFT, -m, None), (orc.OP_SCALE_INV, s, None)], np.asfortranarray(Y[:, n:n + 1]))
            tot += c[n] * (_base_lp(np.asarray(x, np.float64), mu, sigma)[0] + float(l))
        return tot

    lp, yb, g = bj.logpdf_vjp_params(td, dev(Y), T(c))
    close(host(lp), host(bj.logpdf(td, dev(Y))), np.float64, scale=dim, what="chain lp vs bj.logpdf")
    st = g["transform"]["stages"]
    assert st[0] is None and len(st) == 3

    def bump(a, i, h):
        b = a.copy()
        b.reshape(-1)[i] += h
        return b

    gs = _entry(st[1], 2)
    _fd_check("Shift parameter (−m)[2]", gs, lambda h: obj(m=bump(m, 2, -h)))
    _fd_check("Scale parameter s[1]", _entry(st[2], 1), lambda h: obj(s=bump(s, 1, h)))
    _fd_check("base mu[3]", _entry(g["base"]["mu"], 3), lambda h: obj(mu=bump(mu, 3, h)))
    _fd_check("base sigma[0]", _entry(g["base"]["sigma"], 0), lambda h: obj(sigma=bump(sigma, 0, h)))
    _fd_check("y[1, 4]", (float(host(yb)[1, 4]), float(np.abs(host(yb)[:, 4]).max())), lambda h: obj(Y=np.asfortranarray(Y + h * (np.arange(dim * N).reshape(N, dim).T == 4 * dim + 1))))


def _planar_draw(r, dim, nl):
    w = r.normal(size=(dim, nl)) / math.sqrt(dim)
    u = 0.1 * r.normal(size=(dim, nl)) / math.sqrt(dim)
    b = r.normal(size=nl)
    return w, u, b


def _planar_inverse(orc, w, u, b, Y, check=False):
    x = np.asfortranarray(Y)
    ell = np.zeros(Y.shape[1])
    for k in range(w.shape[1] - 1, -1, -1):
        x, l = orc.planar(w[:, k], u[:, k], b[k:k + 1], x, inverse=True)
        x = np.asfortranarray(x)
        if check:                                                     # 1 + wᵀû·sech² of the layer at its pre-image stays above 0.5
            assert orc.planar(w[:, k], u[:, k], b[k:k + 1], x)[1].min() > math.log(0.5)
        ell = ell + l
    return x, ell


def test_generic_two_planar_layers(bj, orc):
    dim, nl, N = 6, 2, 9
    r = rng(6100)
    w, u, b = _planar_draw(r, dim, nl)
    mu, sigma = 0.2 * r.normal(size=dim), np.exp(0.3 * r.normal(size=dim))
    Y = np.asfortranarray(r.normal(size=(dim, N)))
    c = r.normal(size=N)
    _planar_inverse(orc, w, u, b, Y, check=True)
    T = lambda a: torch.tensor(np.ascontiguousarray(a)).cuda()
    ps = [bj.PlanarLayer(T(w[:, k]), T(u[:, k]), T(b[k:k + 1])) for k in range(nl)]
    td = bj.transformed(bj.MvNormal(T(mu), T(sigma)), ps[1] @ ps[0])

    def obj(w=w, u=u, b=b, mu=mu, sigma=sigma):
        x, ell = _planar_inverse(orc, w, u, b, Y)
        return float((c * (_base_lp(x, mu, sigma) + ell)).sum())

    lp, yb, g = bj.logpdf_vjp_params(td, dev(Y), T(c))
    close(host(lp), host(bj.logpdf(td, dev(Y))), np.float64, scale=nl + dim, what="planar lp vs bj.logpdf")
    st = g["transform"]["stages"]                                      # stage j of the inverse is inverse(layer nl-1-j)
    assert len(st) == nl

    def bump(a, idx, h):
        q = a.copy()
        q[idx] += h
        return q

    for k in range(nl):
        sk = st[nl - 1 - k]
        _fd_check(f"planar w[2, {k}]", _entry(sk["w"].reshape(-1), 2), lambda h: obj(w=bump(w, (2, k), h)))
        _fd_check(f"planar u[3, {k}]", _entry(sk["u"].reshape(-1), 3), lambda h: obj(u=bump(u, (3, k), h)))
        _fd_check(f"planar b[{k}]", _entry(sk["b"].reshape(-1), 0), lambda h: obj(b=bump(b, k, h)))
    _fd_check("base mu[1]", _entry(g["base"]["mu"], 1), lambda h: obj(mu=bump(mu, 1, h)))
    _fd_check("base sigma[4]", _entry(g["base"]["sigma"], 4), lambda h: obj(sigma=bump(sigma, 4, h)))


def test_generic_planar_after_two_radial_layers(bj, orc):
    """Planar ∘ Radial ∘ Radial: the plan of the inverse is [inverse(Planar), inverse(run of two)] — not the fused pass."""
    dim, N = 6, 9
    r = rng(6200)
    w, u, b = _planar_draw(r, dim, 1)
    al, be, z0 = _params(r, dim, 2, np.float64)
    mu, sigma = 0.2 * r.normal(size=dim), np.exp(0.3 * r.normal(size=dim))
    Y = r.normal(size=(dim, N))
    Y[0] += 2.0
    Y = np.asfortranarray(Y)
    c = r.normal(size=N)
    _planar_inverse(orc, w, u, b, Y, check=True)
    T = lambda a: torch.tensor(np.ascontiguousarray(a)).cuda()
    rs = _layers(bj, al, be, z0)
    pl = bj.PlanarLayer(T(w[:, 0]), T(u[:, 0]), T(b[0:1]))
    td = bj.transformed(bj.MvNormal(T(mu), T(sigma)), pl @ rs[1] @ rs[0])
    assert [type(s).__name__ for s in bj.interface._td_inverse(td)._plan()[0]] == ["Inverse", "Inverse"]

    def obj(w=w, u=u, b=b, al=al, be=be, z0=z0, mu=mu, sigma=sigma):
        x, ell = _planar_inverse(orc, w, u, b, Y)
        for k in (1, 0):
            x, l = orc.radial(al[k], be[k], np.ascontiguousarray(z0[:, k]), np.asfortranarray(x), True)
            ell = ell + l
        return float((c * (_base_lp(np.asarray(x), mu, sigma) + ell)).sum())

    lp, yb, g = bj.logpdf_vjp_params(td, dev(Y), T(c))
    close(host(lp), host(bj.logpdf(td, dev(Y))), np.float64, scale=3 + dim, what="planar, radial, radial lp vs bj.logpdf")
    st = g["transform"]["stages"]                                      # inverse(Planar), inverse(R2), inverse(R1)
    assert len(st) == 3 and set(st[0]) == {"w", "u", "b"} and set(st[1]) == set(st[2]) == {"alpha_", "beta", "z_0"}

    def bump(a, idx, h):
        q = a.copy()
        q[idx] += h
        return q

    _fd_check("planar w[2]", _entry(st[0]["w"].reshape(-1), 2), lambda h: obj(w=bump(w, (2, 0), h)))
    _fd_check("planar u[3]", _entry(st[0]["u"].reshape(-1), 3), lambda h: obj(u=bump(u, (3, 0), h)))
    _fd_check("planar b", _entry(st[0]["b"].reshape(-1), 0), lambda h: obj(b=bump(b, 0, h)))
    for k in range(2):
        sk = st[2 - k]
        _fd_check(f"radial alpha_[{k}]", _entry(sk["alpha_"].reshape(-1), 0), lambda h: obj(al=bump(al, k, h)))
        _fd_check(f"radial beta[{k}]", _entry(sk["beta"].reshape(-1), 0), lambda h: obj(be=bump(be, k, h)))
        _fd_check(f"radial z_0[4, {k}]", _entry(sk["z_0"].reshape(-1), 4), lambda h: obj(z0=bump(z0, (4, k), h)))
    _fd_check("base mu[1]", _entry(g["base"]["mu"], 1), lambda h: obj(mu=bump(mu, 1, h)))
    _fd_check("base sigma[4]", _entry(g["base"]["sigma"], 4), lambda h: obj(sigma=bump(sigma, 4, h)))


def test_full_covariance_base_is_refused(bj):
    dim = 4
    flow = bj.RadialLayer(torch.zeros(1).cuda(), torch.zeros(1).cuda(), torch.zeros(dim).cuda())
    td = bj.transformed(bj.MvNormal(torch.zeros(dim), cov=torch.eye(dim)), flow)
    with pytest.raises(NotImplementedError):
        bj.logpdf_vjp_params(td, torch.zeros(dim, 3, device="cuda"))
