"""The fused log-density pass for runs of PlanarLayers (include/bjx_planar_logpdf.h: bjx_planar_logpdf_vjp_params) and its routing in
`bj.logpdf_vjp_params`, against Float64 numpy (tests/_planar_logpdf_grad_ref.py, pinned against central differences by
tests/test_host_planar_logpdf_grad.py): the oracle's inverse map layer by layer for x and ℓ, the closed forms for lp, x̄, μ̄, σ̄,
`orc.planar_inv_vjp` for ȳ and `orc.planar_param_vjp(x, −ȳ, −c)` for the layers.

Bars: `flat_close` (1e-3 Float32, 1e-6 Float64, flat) — ȳ per sample, with `cond=planar_inverse_amp(…)` as the existing inverse-Planar
pullback tests pass it; every parameter tensor (one layer's w̄, ū or b̄) per tensor on its own max-norm; μ̄ and σ̄ per tensor with
`term_scale` = the max-norm of their summands; lp with `close` at scale n_layers + dim.  Nothing else widens a bar.

Draws: w ~ N/√dim, u ~ 0.1·N/√dim, b ~ N, y ~ N, c ~ N, μ ~ 0.2·N, σ = exp(0.3·N) (`_planar_draw`'s scale of tests/test_gpu_logpdf_grad.py:
every layer determinant >= 0.65, stacks of at most 12 layers).

Shapes, one per branch of the launcher: the one-wave register tile (Float32 whole packs on aligned bases: 24 rows G = 8; 64 x 3 G = 16
with the layers padded to 4 and a second block holding one column; 128 x 8 G = 32; two layer groups with padding at 128 x 9 — where an
incomplete x would show — and 40 x 12), the column tile's minimum (8 rows Float32, 4 Float64), a
partial last pack (35 rows), one pack per thread on 64 … 256 threads (36, 333 rows), more than one pack per thread (1 500, 2 048 rows), base
pointers one element past a 16-byte boundary, and batches at which every block walks more than one tile."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _planar_logpdf_grad_ref import ref_planar_logpdf_grad  # noqa: E402
from _tol import flat_close, planar_inverse_amp  # noqa: E402
from test_gpu_parity import bj, close, dev, host, rng  # noqa: E402,F401  (fixtures / helpers)
from test_gpu_radial_stack_params import _launches, _p  # noqa: E402

F32, F64 = np.float32, np.float64
SHAPES = [(24, 2, 70, (F32,)), (64, 3, 257, (F32,)), (128, 8, 130, (F32,)), (128, 9, 67, (F32,)), (40, 12, 70, (F32,)),
          (8, 2, 37, (F32,)), (4, 2, 37, (F64,)), (36, 3, 67, (F32, F64)), (35, 3, 67, (F32, F64)), (333, 2, 9, (F32, F64)),
          (1500, 2, 5, (F32,)), (2048, 2, 5, (F32, F64))]
CASES = [(d, nl, N, dt) for (d, nl, N, dts) in SHAPES for dt in dts]
IDS = [f"{d}x{nl}x{N}-{np.dtype(dt).name}" for d, nl, N, dt in CASES]
BASES = ["standard", "standard-with-bars", "diagonal", "diagonal-no-bars"]
OUTS = ("lp", "y_bar", "w_bar", "u_bar", "b_bar", "mu_bar", "sigma_bar")


def _draw(seed, dim, nl, N, dt):
    r = rng(seed)
    w = (r.normal(size=(dim, nl)) / math.sqrt(dim)).astype(dt)
    u = (0.1 * r.normal(size=(dim, nl)) / math.sqrt(dim)).astype(dt)
    b = r.normal(size=nl).astype(dt)
    Y = np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    c = r.normal(size=N).astype(dt)
    mu = (0.2 * r.normal(size=dim)).astype(dt)
    sigma = np.exp(0.3 * r.normal(size=dim)).astype(dt)
    return dict(w=w, u=u, b=b, Y=Y, c=c, mu=mu, sigma=sigma)


def _ref(orc, d, diagonal, c="own"):
    dt = d["Y"].dtype
    ref = ref_planar_logpdf_grad(orc, d["w"], d["u"], d["b"], d["mu"] if diagonal else None, d["sigma"] if diagonal else None, d["Y"],
                                 d["c"] if isinstance(c, str) else c)
    ref["cond"] = planar_inverse_amp(orc, d["w"].astype(F64), d["u"].astype(F64), d["b"].astype(F64), ref["x"], dt)
    return ref


def _tables(d):
    """Layer-major device tables (w, u, b) as bjx_planar takes them."""
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (d["w"].T.reshape(-1), d["u"].T.reshape(-1), d["b"]))


def _off_by_one(a):
    """The (dim, N) array on a device base one element past a 16-byte boundary, column-major."""
    dim, N = a.shape
    buf = torch.empty(dim * N + 1, dtype=torch.from_numpy(a[:1, :1].copy()).dtype, device="cuda")
    y = buf[1:].view(N, dim).T
    y.copy_(dev(a))
    assert y.data_ptr() % 16 == a.dtype.itemsize
    return y


def _c_entry(bj, tabs, nl, mu, sigma, y, c, dim=None, batch=None, dt=None, lp=True, y_bar=True, layers=True, base=True, two_of_three=False, work="own"):
    """bjx_planar_logpdf_vjp_params -> (status, dict of the outputs asked for: device tensors pre-filled with 7)."""
    I = bj.interface
    tt = tabs[1]
    ctx = I.context(tt.device)
    dim = y.shape[0] if dim is None else dim
    batch = y.shape[1] if batch is None else batch
    nb, nd, nn = max(batch, 0), max(dim, 0), max(nl, 1)
    full = lambda *s: torch.full(s, 7.0, dtype=tt.dtype, device="cuda")
    o = dict(lp=full(nb) if lp else None, y_bar=torch.full((nb, nd), 7.0, dtype=tt.dtype, device="cuda").T if y_bar else None,
             w_bar=full(nn * nd) if layers else None, u_bar=full(nn * nd) if layers else None, b_bar=full(nn) if layers else None,
             mu_bar=full(nd) if base else None, sigma_bar=full(nd) if base else None)
    if work == "own":                                                  # the header's formula (bjx_planar_logpdf_work_elems)
        n, up4 = 0, lambda k: (k + 3) // 4 * 4
        if layers or base:
            n = (up4(2 * nn * nb) if layers else 0) + up4(nd * nb) + (up4(nd * nb) if layers and not y_bar else 0) + (up4(nb) if layers and c is None else 0)
        work = torch.empty(n, dtype=tt.dtype, device="cuda") if n else None
    rc = bj._lib.load().bjx_planar_logpdf_vjp_params(ctx.h, I._dt(tt) if dt is None else dt, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl, _p(mu), _p(sigma), _p(y), _p(c),
                                                     _p(o["lp"]), _p(o["y_bar"]), _p(o["w_bar"]), _p(o["u_bar"]), None if two_of_three else _p(o["b_bar"]),
                                                     _p(o["mu_bar"]), _p(o["sigma_bar"]), _p(work), dim, batch)
    return rc, o


def _check(o, ref, dt, what, nl, dim):
    """Every output present in `o` against the reference at the bars of the module docstring; returns the worst gradient error."""
    worst = 0.0
    if o.get("lp") is not None:
        close(host(o["lp"]), ref["lp"], dt, scale=nl + dim, what=what + " lp")
    if o.get("y_bar") is not None:
        worst = max(worst, flat_close(host(o["y_bar"]).reshape(ref["y_bar"].shape), ref["y_bar"], dt, what + " y_bar", cond=ref["cond"]))
    if o.get("w_bar") is not None:
        gw, gu, gb = host(o["w_bar"]).reshape(nl, dim).T, host(o["u_bar"]).reshape(nl, dim).T, host(o["b_bar"])
        for k in range(nl):
            worst = max(worst, flat_close(gw[:, k], ref["w_bar"][:, k], dt, f"{what} w_bar[{k}]", per="tensor"),
                        flat_close(gu[:, k], ref["u_bar"][:, k], dt, f"{what} u_bar[{k}]", per="tensor"),
                        flat_close(gb[k:k + 1], ref["b_bar"][k:k + 1], dt, f"{what} b_bar[{k}]", per="tensor"))
    if o.get("mu_bar") is not None:
        worst = max(worst, flat_close(host(o["mu_bar"]), ref["mu_bar"], dt, what + " mu_bar", per="tensor", term_scale=ref["t_mu"]),
                    flat_close(host(o["sigma_bar"]), ref["sigma_bar"], dt, what + " sigma_bar", per="tensor", term_scale=ref["t_sigma"]))
    return worst


def _devs(d, y=None):
    return (dev(d["Y"]) if y is None else y, torch.from_numpy(d["c"]).cuda(), torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda())


@pytest.fixture(scope="module")
def refs(orc):
    """Per case: the draw and the reference for the standard and the diagonal base — computed once, never written to."""
    out = {}
    for i, case in enumerate(CASES):
        dim, nl, N, dt = case
        d = _draw(7000 + i, dim, nl, N, dt)
        d["standard"] = _ref(orc, d, False)
        d["diagonal"] = _ref(orc, d, True)
        out[case] = d
    return out


# ------------------------------------------------------------------ every form of the pass, every base variant (the C entry)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_reference(bj, refs, case):
    dim, nl, N, dt = case
    d = refs[case]
    tabs = _tables(d)
    yd, cd, mud, sgd = _devs(d)
    for base in BASES:
        diag = base.startswith("diagonal")                            # standard-with-bars: mu = sigma = NULL, mu_bar and sigma_bar asked for
        rc, o = _c_entry(bj, tabs, nl, mud if diag else None, sgd if diag else None, yd, cd, base=base in ("diagonal", "standard-with-bars"))
        assert rc == 0
        what = f"planar logpdf {IDS[CASES.index(case)]} base={base}"
        worst = _check(o, d["diagonal" if diag else "standard"], dt, what, nl, dim)
        print(f"{what}: worst gradient error {worst:.3g} of its scale")


@pytest.mark.parametrize("dim,nl,N,dt", [(36, 3, 37, F32), (36, 3, 37, F64), (128, 8, 130, F32)])
def test_element_aligned_base_pointer(bj, orc, dim, nl, N, dt):
    """y (and ȳ) on a base one element past a 16-byte boundary; 128 x 8 Float32 is the register tile's own shape, which such a base takes
    off that tile."""
    d = _draw(7100 + dim, dim, nl, N, dt)
    tabs = _tables(d)
    y = _off_by_one(d["Y"])
    _, cd, mud, sgd = _devs(d, y)
    rc, o = _c_entry(bj, tabs, nl, mud, sgd, y, cd)
    assert rc == 0
    _check(o, _ref(orc, d, True), dt, f"planar logpdf element-aligned {dim}x{nl} {np.dtype(dt).name}", nl, dim)


@pytest.mark.parametrize("dim,dt", [(36, F64), (64, F32)])
def test_blocks_walk_many_tiles_and_repeat_bits(bj, orc, dim, dt):
    """The pass's grid is capped at num_cu·2048/NT blocks of C columns (NT = 64 here; C = 16 Float64, 8 Float32): a batch of one full round of
    tiles, three more tiles and a partial one — blocks walk a second tile, the last of them a partial one (the smallest batch that does).  The reference's values, and the same bits in
    EVERY output from a second call (fixed-order sums, no atomics)."""
    nl = 3
    C_ = 16 if dt == F64 else 8
    cap = torch.cuda.get_device_properties(0).multi_processor_count * (2048 // 64)
    N = cap * C_ + 3 * C_ + 5
    d = _draw(7200 + dim, dim, nl, N, dt)
    tabs = _tables(d)
    args = (bj, tabs, nl) + tuple(_devs(d)[k] for k in (2, 3, 0, 1))
    rc, o = _c_entry(*args)
    assert rc == 0
    _check(o, _ref(orc, d, True), dt, f"planar logpdf many tiles dim={dim} N={N} {np.dtype(dt).name}", nl, dim)
    rc, o2 = _c_entry(*args)
    assert rc == 0
    for k in OUTS:
        assert torch.equal(o[k], o2[k]), f"{k} differs between two identical calls"


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("dim,nl,N", [(36, 3, 67), (128, 9, 67)])
def test_repeat_call_bits_small(bj, dim, nl, N, dt):
    d = _draw(7250 + dim, dim, nl, N, dt)
    tabs = _tables(d)
    args = (bj, tabs, nl) + tuple(_devs(d)[k] for k in (2, 3, 0, 1))
    (rc, o), (rc2, o2) = _c_entry(*args), _c_entry(*args)
    assert rc == 0 and rc2 == 0
    for k in OUTS:
        assert torch.equal(o[k], o2[k]), f"{k} differs between two identical calls"


# ------------------------------------------------------------------ optional outputs and edges of the C entry
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("dim,nl,N", [(36, 3, 67), (128, 8, 70)])
def test_optional_outputs(bj, orc, dim, nl, N, dt):
    """y_bar = NULL (ȳ then lives in `work`) leaves every other output bit-identical; lp_bar = NULL is c = 1; with nothing summed over the
    batch asked for, work = NULL and the pass is the only hot launch; two of the three layer cotangents is an argument error."""
    d = _draw(7400 + dim, dim, nl, N, dt)
    tabs = _tables(d)
    yd, cd, mud, sgd = _devs(d)
    rc, full = _c_entry(bj, tabs, nl, mud, sgd, yd, cd)
    assert rc == 0
    rc, o = _c_entry(bj, tabs, nl, mud, sgd, yd, cd, y_bar=False)
    assert rc == 0
    for k in OUTS:
        if k != "y_bar":
            assert torch.equal(o[k], full[k]), f"{k} changes when y_bar is not written"
    rc, o = _c_entry(bj, tabs, nl, mud, sgd, yd, cd, layers=False)
    assert rc == 0
    for k in ("lp", "y_bar", "mu_bar", "sigma_bar"):
        assert torch.equal(o[k], full[k]), f"{k} changes when the layer cotangents are not written"
    rc, o = _c_entry(bj, tabs, nl, mud, sgd, yd, cd, layers=False, base=False, work=None)
    assert rc == 0
    assert torch.equal(o["y_bar"], full["y_bar"]) and torch.equal(o["lp"], full["lp"])
    (rc, _), _, k = bj.kernel_timed(lambda: _c_entry(bj, tabs, nl, mud, sgd, yd, cd, layers=False, base=False, work=None))
    assert rc == 0 and k == 1, f"the pass alone took {k} hot launches"
    ones = torch.ones(N, dtype=yd.dtype, device="cuda")
    (rc, a), (rc2, b) = _c_entry(bj, tabs, nl, mud, sgd, yd, None), _c_entry(bj, tabs, nl, mud, sgd, yd, ones)
    assert rc == 0 and rc2 == 0
    for k in OUTS:
        assert torch.equal(a[k], b[k]), f"{k}: lp_bar = NULL is not c = 1"
    _check(a, _ref(orc, d, True, c=None), dt, f"planar logpdf lp_bar=NULL {dim}x{nl} {np.dtype(dt).name}", nl, dim)
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_entry(bj, tabs, nl, mud, sgd, yd, cd, two_of_three=True)[0] == bj._lib.ERR_ARG
    assert _c_entry(bj, tabs, nl, mud, sgd, yd, cd, work=None)[0] == bj._lib.ERR_ARG              # summed outputs without work
    assert _launches(bj) == n0


@pytest.mark.parametrize("dt", [F32, F64])
def test_empty_batch_writes_zeros_and_launches_nothing(bj, dt):
    dim, nl = 36, 3
    d = _draw(7500, dim, nl, 1, dt)
    tabs = _tables(d)
    torch.cuda.synchronize()
    n0 = _launches(bj)
    rc, o = _c_entry(bj, tabs, nl, None, None, None, None, dim=dim, batch=0)
    assert rc == 0 and _launches(bj) == n0
    torch.cuda.synchronize()
    for k in ("w_bar", "u_bar", "b_bar", "mu_bar", "sigma_bar"):
        assert float(o[k].abs().max()) == 0.0, k


def test_argument_checks_launch_nothing(bj):
    dim, nl, N, dt = 36, 2, 5, F32
    d = _draw(7600, dim, nl, N, dt)
    tabs = _tables(d)
    y = dev(d["Y"])
    Lb = bj._lib
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_entry(bj, tabs, nl, None, None, y, None, dim=0)[0] == Lb.ERR_SHAPE
    assert _c_entry(bj, tabs, nl, None, None, y, None, batch=-1)[0] == Lb.ERR_SHAPE
    assert _c_entry(bj, tabs, 0, None, None, y, None)[0] == Lb.ERR_SHAPE
    assert _c_entry(bj, (None, tabs[1], tabs[2]), nl, None, None, y, None)[0] == Lb.ERR_ARG
    assert _c_entry(bj, tabs, nl, None, None, None, None, dim=dim, batch=N)[0] == Lb.ERR_ARG
    assert _c_entry(bj, tabs, nl, None, None, y, None, dt=77)[0] == Lb.ERR_ARG
    assert _launches(bj) == n0


# ------------------------------------------------------------------ the public function
def _layers(bj, d):
    mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return [bj.PlanarLayer(mk(d["w"][:, k]), mk(d["u"][:, k]), mk(d["b"][k:k + 1])) for k in range(d["w"].shape[1])]


def _td(bj, d, diagonal, flow=None):
    if flow is None:
        ls = _layers(bj, d)
        flow = ls[0]
        for l in ls[1:]:
            flow = l @ flow
    base = bj.MvNormal(torch.from_numpy(d["mu"]).cuda(), torch.from_numpy(d["sigma"]).cuda()) if diagonal else bj.MvNormal(len(d["mu"]))
    return bj.transformed(base, flow)


def _run_of(bj, td):
    ib = bj.interface._td_inverse(td)
    run = (ib._plan()[0][0] if isinstance(ib, bj.interface.ComposedFunction) else ib).orig
    assert isinstance(run, bj.PlanarLayer)
    return run


def _force_generic(run, tdt, dim):
    """Fill the run's memory of refusals so that `logpdf_vjp_params` takes the generic path."""
    run._refused.update({("logpdf", tdt, dim, False), ("logpdf", tdt, dim, True)})


def _public_as_outputs(lp, yb, grads, nl, dim):
    """The public function's results in the layout `_check` reads (stage j of inverse(run) is inverse(layer nl-1-j))."""
    o = dict(lp=lp, y_bar=yb)
    if grads:
        g = grads["transform"]
        if "stages" in g:
            st = g["stages"][::-1]
            W, U, B = (torch.stack([s[n].reshape(-1) for s in st]).reshape(-1) for n in ("w", "u", "b"))
        else:
            W, U, B = g["w"].reshape(dim, nl).T.reshape(-1), g["u"].reshape(dim, nl).T.reshape(-1), g["b"].reshape(-1)
        o.update(w_bar=W, u_bar=U, b_bar=B)
        if "mu" in grads["base"]:
            o.update(mu_bar=grads["base"]["mu"], sigma_bar=grads["base"]["sigma"])
    return o


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("diagonal", [False, True])
@pytest.mark.parametrize("dim,nl,N", [(36, 3, 130), (128, 8, 70)])
def test_public_function(bj, orc, dim, nl, N, diagonal, dt):
    d = _draw(7700 + dim, dim, nl, N, dt)
    td = _td(bj, d, diagonal)
    yd, cd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda()
    what = f"public dim={dim} L={nl} {np.dtype(dt).name} diagonal={diagonal}"
    ref = _ref(orc, d, diagonal)
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    _check(_public_as_outputs(lp, yb, g, nl, dim), ref, dt, what, nl, dim)
    close(host(lp), host(bj.logpdf(td, yd)), dt, scale=nl + dim, what=what + " lp vs bj.logpdf")
    _, _, kf = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    run = _run_of(bj, td)
    assert not run._refused
    # keys, shapes and order of vjp_params(inverse(flow), …)
    _, gv = bj.vjp_params(bj.inverse(td.transform), yd, dev(ref["x_bar"].astype(dt)), cd)
    assert set(g) == {"transform", "base"} and set(g["base"]) == ({"mu", "sigma"} if diagonal else set())
    assert list(g["transform"]) == ["stages"] and len(g["transform"]["stages"]) == len(gv["stages"]) == nl
    for j in range(nl):
        a, b = g["transform"]["stages"][j], gv["stages"][j]
        assert list(a) == list(b) == ["w", "u", "b"]
        for name in a:
            assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype
            flat_close(host(a[name]).reshape(-1), host(b[name]).reshape(-1), dt, f"{what} stage {j} {name} vs vjp_params", per="tensor")
    # params=False: only the pass (after the two table gathers); want_y_bar=False
    (lp3, yb3, g3), _, k3 = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd, params=False))
    assert g3 == {} and torch.equal(yb3, yb) and torch.equal(lp3, lp)
    assert k3 <= 3, f"params=False took {k3} hot launches"
    lp4, yb4, g4 = bj.logpdf_vjp_params(td, yd, cd, want_y_bar=False)
    assert yb4 is None and torch.equal(lp4, lp)
    o4 = _public_as_outputs(lp4, None, g4, nl, dim)
    for k, v in _public_as_outputs(lp, None, g, nl, dim).items():
        assert v is None or torch.equal(v, o4[k]), f"{k} changes with want_y_bar=False"
    # vector input
    lpv, ybv, gvv = bj.logpdf_vjp_params(td, yd[:, 0].contiguous(), float(d["c"][0]))
    assert ybv.shape == (dim,)
    close(host(lpv).reshape(-1), ref["lp"][:1], dt, scale=nl + dim, what=what + " vector lp")
    flat_close(host(ybv).reshape(dim, 1), ref["y_bar"][:, :1], dt, what + " vector y_bar", cond=ref["cond"][:1])
    # the generic path, forced: the same answers at the flat bar, through more launches
    _force_generic(run, yd.dtype, dim)
    lp2, yb2, g2 = bj.logpdf_vjp_params(td, yd, cd)
    _, _, kg = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    print(f"{what}: hot launches fused {kf}, generic {kg}, params=False {k3}")
    assert kf < kg
    o, o2 = _public_as_outputs(lp, yb, g, nl, dim), _public_as_outputs(lp2, yb2, g2, nl, dim)
    _check(o2, ref, dt, what + " generic", nl, dim)
    close(host(lp), host(lp2), dt, scale=nl + dim, what=what + " fused vs generic lp")
    flat_close(host(yb), host(yb2), dt, what + " fused vs generic y_bar", cond=ref["cond"])
    for name in ("w_bar", "u_bar"):
        for k in range(nl):
            flat_close(host(o[name])[k * dim:(k + 1) * dim], host(o2[name])[k * dim:(k + 1) * dim], dt, f"{what} fused vs generic {name}[{k}]", per="tensor")
    for k in range(nl):
        flat_close(host(o["b_bar"])[k:k + 1], host(o2["b_bar"])[k:k + 1], dt, f"{what} fused vs generic b_bar[{k}]", per="tensor")
    if diagonal:
        flat_close(host(o["mu_bar"]), host(o2["mu_bar"]), dt, what + " fused vs generic mu_bar", per="tensor", term_scale=ref["t_mu"])
        flat_close(host(o["sigma_bar"]), host(o2["sigma_bar"]), dt, what + " fused vs generic sigma_bar", per="tensor", term_scale=ref["t_sigma"])


@pytest.mark.parametrize("dt", [F32, F64])
def test_lp_bar_variants(bj, orc, dt):
    """None (= 1), a Python number, a (batch,) tensor, and all zeros: ȳ and every gradient are then EXACTLY zero and lp is still right."""
    dim, nl, N = 36, 3, 67
    d = _draw(7800, dim, nl, N, dt)
    td = _td(bj, d, True)
    yd = dev(d["Y"])
    for name, arg, cref in (("None", None, None), ("number", 0.7, np.full(N, 0.7)), ("tensor", torch.from_numpy(d["c"]).cuda(), d["c"])):
        lp, yb, g = bj.logpdf_vjp_params(td, yd, arg)
        _check(_public_as_outputs(lp, yb, g, nl, dim), _ref(orc, d, True, c=cref), dt, f"lp_bar={name} {np.dtype(dt).name}", nl, dim)
    assert not _run_of(bj, td)._refused
    for zero in (0.0, torch.zeros(N, dtype=yd.dtype, device="cuda")):
        lp, yb, g = bj.logpdf_vjp_params(td, yd, zero)
        o = _public_as_outputs(lp, yb, g, nl, dim)
        close(host(lp), _ref(orc, d, True)["lp"], dt, scale=nl + dim, what="lp with a zero cotangent")
        for k in OUTS[1:]:
            assert float(o[k].abs().max()) == 0.0, f"{k} is not exactly zero for a zero cotangent"


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("form", ["layer", "matrix", "stack"])
def test_single_planar_layer_and_matrix_layer(bj, orc, form, dt):
    """One PlanarLayer, a PlanarLayer with (dim, n_layers) matrices and PlanarLayer.stack: the layer's own dictionary in the shapes
    vjp_params(inverse(layer), …) gives, fused in fewer hot launches than the generic path."""
    dim, N = 36, 67
    nl = 1 if form == "layer" else 3
    d = _draw(7900 + nl, dim, nl, N, dt)
    mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if form == "layer":
        flow = bj.PlanarLayer(mk(d["w"][:, 0]), mk(d["u"][:, 0]), mk(d["b"]))
    elif form == "matrix":
        flow = bj.PlanarLayer(mk(d["w"]), mk(d["u"]), mk(d["b"]))
    else:
        flow = bj.PlanarLayer.stack(_layers(bj, d))
    td = _td(bj, d, True, flow)
    yd, cd = dev(d["Y"]), torch.from_numpy(d["c"]).cuda()
    ref = _ref(orc, d, True)
    what = f"{form} {np.dtype(dt).name}"
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    _, _, kf = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    assert list(g["transform"]) == ["w", "u", "b"]
    _check(_public_as_outputs(lp, yb, g, nl, dim), ref, dt, what, nl, dim)
    run = _run_of(bj, td)
    assert run is flow and not run._refused
    _force_generic(run, yd.dtype, dim)
    lp2, yb2, g2 = bj.logpdf_vjp_params(td, yd, cd)
    _, _, kg = bj.kernel_timed(lambda: bj.logpdf_vjp_params(td, yd, cd))
    print(f"{what}: hot launches fused {kf}, generic {kg}")
    assert kf < kg
    for name in ("w", "u", "b"):
        assert g["transform"][name].shape == g2["transform"][name].shape, name
    _check(_public_as_outputs(lp2, yb2, g2, nl, dim), ref, dt, what + " generic", nl, dim)


@pytest.mark.parametrize("dt", [F32, F64])
def test_refused_height_goes_through_the_generic_path(bj, orc, dt):
    """2 rows: BJX_ERR_UNSUPPORTED from the C entry with nothing launched; the public function remembers it and still returns the
    reference's values."""
    dim, nl, N = 2, 3, 70
    d = _draw(8000, dim, nl, N, dt)
    tabs = _tables(d)
    yd, cd, mud, sgd = _devs(d)
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_entry(bj, tabs, nl, mud, sgd, yd, cd)[0] == bj._lib.ERR_UNSUPPORTED
    assert _c_entry(bj, tabs, nl, None, None, yd, cd, layers=False, base=False, work=None)[0] == bj._lib.ERR_UNSUPPORTED
    assert _launches(bj) == n0
    td = _td(bj, d, True)
    lp, yb, g = bj.logpdf_vjp_params(td, yd, cd)
    _check(_public_as_outputs(lp, yb, g, nl, dim), _ref(orc, d, True), dt, f"refused height, generic {np.dtype(dt).name}", nl, dim)
    assert ("logpdf", yd.dtype, dim, True) in _run_of(bj, td)._refused
