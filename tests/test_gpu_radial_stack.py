"""A run of RadialLayers in ONE launch (include/bjx_radial_stack.h: bjx_radial_stack / bjx_radial_stack_vjp; `_RadialRun` and the
composition planner in bijectors.jl_amd/interface.py) against the oracle composed here: `orc.radial` layer after layer in Float64
for the map and its inverse; for the pullback a forward sweep that keeps every layer's input, then `orc.radial_vjp` from the last
layer back with the same ℓ̄.  Bars: `close` (scale = n_layers on the log-det) for the maps, the flat 1e-3 / 1e-6 of `flat_close`
for the pullbacks.  Inputs are drawn away from z = z₀ (the pullbacks divide by r = ‖z − z₀‖).

Shapes: the smallest at which each path can go wrong — group form on whole packs (a ragged last block, more than one block, more
than one pack per lane), on partial packs (35 rows) and on scalar packs (an element-aligned base), the lane-per-column form (one
column past a 64-column tile, direct short columns, tiled ones), n_layers = 1 against bjx_radial, 17 layers, and the first height
the register kernels refuse."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, close, dev, host, rng, sum_close  # noqa: E402,F401  (fixtures / helpers)

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


def _layers(bj, al, be, z0, on_device=True):
    mk = (lambda a: torch.tensor(a).cuda()) if on_device else torch.tensor
    return [bj.RadialLayer(mk(al[k:k + 1]), mk(be[k:k + 1]), mk(np.ascontiguousarray(z0[:, k]))) for k in range(len(al))]


def _compose(ls):
    f = ls[0]
    for l in ls[1:]:
        f = l @ f
    return f


def _ref_map(orc, al, be, z0, X, inverse=False):
    """(out, ladj, [input of every applied layer]) in Float64; inverse: the last layer's inverse first."""
    x = np.asfortranarray(np.asarray(X, np.float64))
    nl = len(al)
    ladj = np.zeros(x.shape[1])
    inputs = []
    for k in (range(nl - 1, -1, -1) if inverse else range(nl)):
        inputs.append(x)
        x, l = orc.radial(np.float64(al[k]), np.float64(be[k]), z0[:, k].astype(np.float64), x, inverse)
        x = np.asfortranarray(x)
        ladj = ladj + l
    return x, ladj, inputs


def _ref_vjp(orc, al, be, z0, X, G, lbar, inverse=False):
    nl = len(al)
    _, _, inputs = _ref_map(orc, al, be, z0, X, inverse)
    order = list(range(nl - 1, -1, -1) if inverse else range(nl))
    g = np.asarray(G, np.float64)
    for k, xin in zip(reversed(order), reversed(inputs)):
        g = orc.radial_vjp(np.float64(al[k]), np.float64(be[k]), z0[:, k].astype(np.float64), xin, g, None if lbar is None else np.asarray(lbar, np.float64), inverse=inverse)
    return g


@pytest.fixture(scope="module")
def refs(orc):
    """Per case: parameters, points and the oracle's results, computed once and shared by the tests (never written to)."""
    out = {}
    for i, (dim, nl, N, dt) in enumerate(CASES):
        r = rng(1000 + i)
        al, be, z0 = _params(r, dim, nl, dt)
        Z = _points(r, dim, N, dt)
        G = np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
        lbar = r.normal(size=N).astype(dt)
        Y, l, _ = _ref_map(orc, al, be, z0, Z)
        Yd = np.asfortranarray(Y.astype(dt))                   # the inverse is evaluated at the rounded image
        Zi, li, _ = _ref_map(orc, al, be, z0, Yd, inverse=True)
        out[(dim, nl, N, dt)] = dict(al=al, be=be, z0=z0, Z=Z, G=G, lbar=lbar, Y=Y, l=l, Yd=Yd, Zi=Zi, li=li,
                                     vf=_ref_vjp(orc, al, be, z0, Z, G, lbar), vi=_ref_vjp(orc, al, be, z0, Yd, G, lbar, inverse=True))
    return out


# ------------------------------------------------------------------ the C entries, called directly
def _tables(al, be, z0):
    return torch.tensor(al).cuda(), torch.tensor(be).cuda(), torch.tensor(np.ascontiguousarray(z0.T).reshape(-1)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _c_stack(bj, inverse, tabs, nl, x, y, ps=None, s=None, flags=0, dim=None, batch=None, dt=None):
    I = bj.interface
    ctx = I.context(x.device if x is not None else tabs[0].device)
    dim = x.shape[0] if dim is None else dim
    batch = x.shape[1] if batch is None else batch
    return bj._lib.load().bjx_radial_stack(ctx.h, I._dt(tabs[0]) if dt is None else dt, int(inverse), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl, _p(x), _p(y),
                                           _p(ps), _p(s), dim, batch, flags)


def _c_stack_vjp(bj, inverse, tabs, nl, x, g, lb, xb, dim=None, batch=None, dt=None):
    I = bj.interface
    ctx = I.context(tabs[0].device)
    dim = x.shape[0] if dim is None else dim
    batch = x.shape[1] if batch is None else batch
    return bj._lib.load().bjx_radial_stack_vjp(ctx.h, I._dt(tabs[0]) if dt is None else dt, int(inverse), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), nl, _p(x), _p(g),
                                               _p(lb), _p(xb), dim, batch)


def _launches(bj):
    return int(bj._lib.load().bjx_launch_count())


# ------------------------------------------------------------------ every path against the oracle
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_map_matches_oracle(bj, refs, case, inverse):
    dim, nl, N, dt = case
    c = refs[case]
    run = bj.interface._RadialRun(_layers(bj, c["al"], c["be"], c["z0"]))
    b = bj.inverse(run) if inverse else run
    Xd = dev(c["Yd"] if inverse else c["Z"])
    bj.with_logabsdet_jacobian(b, Xd, per_sample=True)
    (y, l), _, k = bj.kernel_timed(lambda: bj.with_logabsdet_jacobian(b, Xd, per_sample=True))
    assert k == 1, f"{nl} fused RadialLayers took {k} hot launches"
    close(host(y), c["Zi"] if inverse else c["Y"], dt, what=f"radial stack {case} inverse={inverse}")
    close(host(l), c["li"] if inverse else c["l"], dt, scale=nl, what="radial stack ladj")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pullback_matches_oracle(bj, orc, refs, case, inverse):
    dim, nl, N, dt = case
    c = refs[case]
    run = bj.interface._RadialRun(_layers(bj, c["al"], c["be"], c["z0"]))
    b = bj.inverse(run) if inverse else run
    Xd, Gd, lb = dev(c["Yd"] if inverse else c["Z"]), dev(c["G"]), torch.from_numpy(c["lbar"]).cuda()
    bj.vjp(b, Xd, Gd, lb)
    xb, _, k = bj.kernel_timed(lambda: bj.vjp(b, Xd, Gd, lb))
    assert k == 1
    worst = flat_close(host(xb), c["vi"] if inverse else c["vf"], dt, f"radial stack vjp {IDS[CASES.index(case)]} inverse={inverse}")
    print(f"radial stack vjp {case} inverse={inverse}: worst error {worst:.3g} of the column's scale")
    # no log-det cotangent
    ref0 = _ref_vjp(orc, c["al"], c["be"], c["z0"], c["Yd"] if inverse else c["Z"], c["G"], None, inverse)
    flat_close(host(bj.vjp(b, Xd, Gd)), ref0, dt, "radial stack vjp, no ladj_bar")


def test_scalar_packs_on_an_element_aligned_base(bj, orc):
    """Group form with V = 1: 8 Float32 rows whose base is one element past a 16-byte boundary (map and pullback)."""
    dim, nl, N, dt = 8, 3, 37, np.float32
    r = rng(1100)
    al, be, z0 = _params(r, dim, nl, dt)
    Z, G = _points(r, dim, N, dt), np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = r.normal(size=N).astype(dt)
    tabs = _tables(al, be, z0)

    def off(a):                                           # (dim, N) column-major view that starts 4 bytes into its buffer
        buf = torch.empty(dim * N + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(N, dim).T
        if a is not None:
            v.copy_(dev(a))
        assert v.data_ptr() % 16 == 4
        return v
    x, y, g, xb = off(Z), off(None), off(G), off(None)
    ps = torch.empty(N, dtype=torch.float32, device="cuda")
    for inverse in (False, True):
        assert _c_stack(bj, inverse, tabs, nl, x, y, ps) == 0
        Y, l, _ = _ref_map(orc, al, be, z0, Z, inverse)
        close(host(y), Y, dt, what="V = 1 map")
        close(host(ps), l, dt, scale=nl, what="V = 1 ladj")
        assert _c_stack_vjp(bj, inverse, tabs, nl, x, g, torch.from_numpy(lbar).cuda(), xb) == 0
        flat_close(host(xb), _ref_vjp(orc, al, be, z0, Z, G, lbar, inverse), dt, f"radial stack vjp V = 1 inverse={inverse}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 67), (10, 70), (2, 65)])
def test_one_layer_through_the_c_entry_is_bjx_radial(bj, dim, N, dt):
    """n_layers = 1 is served, and is the single-layer kernels' result (same arithmetic, same order): tolerance asserted, bit
    equality printed."""
    r = rng(1200 + dim)
    al, be, z0 = _params(r, dim, 1, dt)
    Z, G = _points(r, dim, N, dt), np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = torch.from_numpy(r.normal(size=N).astype(dt)).cuda()
    layer = _layers(bj, al, be, z0)[0]
    tabs = _tables(al, be, z0)
    Xd, Gd = dev(Z), dev(G)
    for inverse in (False, True):
        b = bj.inverse(layer) if inverse else layer
        y1, l1 = bj.with_logabsdet_jacobian(b, Xd, per_sample=True)
        y = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
        ps = torch.empty(N, dtype=Xd.dtype, device="cuda")
        assert _c_stack(bj, inverse, tabs, 1, Xd, y, ps) == 0
        print(f"dim {dim} {np.dtype(dt).name} inverse={inverse}: map bits equal {torch.equal(y, y1)}, ladj bits equal {torch.equal(ps, l1)}")
        close(host(y), host(y1), dt, what="stack of one vs bjx_radial")
        close(host(ps), host(l1), dt, what="stack of one vs bjx_radial: ladj")
        v1 = bj.vjp(b, Xd, Gd, lbar)
        xb = torch.empty((N, dim), dtype=Xd.dtype, device="cuda").T
        assert _c_stack_vjp(bj, inverse, tabs, 1, Xd, Gd, lbar, xb) == 0
        print(f"dim {dim} {np.dtype(dt).name} inverse={inverse}: pullback bits equal {torch.equal(xb, v1)}")
        flat_close(host(xb), host(v1), dt, f"stack of one vs bjx_radial_vjp dim={dim} inverse={inverse}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 67), (10, 70)])
def test_seventeen_layers(bj, orc, dim, N, dt):
    """Served (1 launch) or refused and evaluated layer by layer (17): either way the oracle's values."""
    nl = 17
    r = rng(1300 + dim)
    al, be, z0 = _params(r, dim, nl, dt)
    Z, G = _points(r, dim, N, dt), np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = r.normal(size=N).astype(dt)
    flow = _compose(_layers(bj, al, be, z0))
    (y, l), _, k = bj.kernel_timed(lambda: bj.with_logabsdet_jacobian(flow, dev(Z), per_sample=True))
    assert k in (1, nl)
    Y, lr, _ = _ref_map(orc, al, be, z0, Z)
    close(host(y), Y, dt, what="17 layers")
    close(host(l), lr, dt, scale=nl, what="17 layers ladj")
    xb, _, kv = bj.kernel_timed(lambda: bj.vjp(flow, dev(Z), dev(G), torch.from_numpy(lbar).cuda()))
    assert kv in (1, 2 * nl - 1)
    flat_close(host(xb), _ref_vjp(orc, al, be, z0, Z, G, lbar), dt, f"17 layers vjp dim={dim}")


# ------------------------------------------------------------------ the planner reaches the fused entries
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,N", [(64, 513), (10, 100)])
def test_composed_radial_flow_is_one_fused_launch(bj, orc, dim, N, dt):
    nl = 3
    r = rng(1400 + dim)
    al, be, z0 = _params(r, dim, nl, dt)
    ls = _layers(bj, al, be, z0)
    flow = _compose(ls)
    run = bj.interface._RadialRun(ls)
    Z, G = _points(r, dim, N, dt), np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    Zd, Gd, lb = dev(Z), dev(G), torch.from_numpy(r.normal(size=N).astype(dt)).cuda()
    bj.with_logabsdet_jacobian(flow, Zd)
    (y, l), _, k = bj.kernel_timed(lambda: bj.with_logabsdet_jacobian(flow, Zd))
    assert k == 1, f"{nl} composed RadialLayers took {k} hot launches"
    yr, lr = bj.with_logabsdet_jacobian(run, Zd)
    assert torch.equal(y, yr) and torch.equal(l, lr)                             # same kernel, same tables: same bits
    Y, l_ref, _ = _ref_map(orc, al, be, z0, Z)
    close(host(y), Y, dt, what="composed radial fwd")
    close(host(l), l_ref, dt, scale=nl, what="composed radial ladj")
    y2, _, k2 = bj.kernel_timed(lambda: bj.transform(flow, Zd))
    assert k2 == 1 and torch.equal(y2, y)
    inv = bj.inverse(flow)
    assert isinstance(inv, bj.ComposedFunction)
    bj.with_logabsdet_jacobian(inv, y)
    (zb, lbk), _, k3 = bj.kernel_timed(lambda: bj.with_logabsdet_jacobian(inv, y))
    assert k3 == 1
    zs, ls_ = bj.with_logabsdet_jacobian(bj.inverse(run), y)
    assert torch.equal(zb, zs) and torch.equal(lbk, ls_)
    Zi, li, _ = _ref_map(orc, al, be, z0, host(y), inverse=True)
    close(host(zb), Zi, dt, what="composed radial inverse")
    close(host(lbk), li, dt, scale=nl, what="composed radial inverse ladj")
    bj.vjp(flow, Zd, Gd, lb)
    xb, _, k4 = bj.kernel_timed(lambda: bj.vjp(flow, Zd, Gd, lb))
    assert k4 == 1
    assert torch.equal(xb, bj.vjp(run, Zd, Gd, lb))
    flat_close(host(xb), _ref_vjp(orc, al, be, z0, Z, G, host(lb)), dt, f"composed radial vjp dim={dim}")
    yb, _, k5 = bj.kernel_timed(lambda: bj.vjp(inv, y, Gd, lb))
    assert k5 == 1
    flat_close(host(yb), _ref_vjp(orc, al, be, z0, host(y), G, host(lb), inverse=True), dt, f"composed radial inverse vjp dim={dim}")
    # logpdf of a transformed distribution: the generic path evaluates the inverse run in one hot launch
    td = bj.transformed(bj.MvNormal(dim), flow)
    bj.logpdf(td, y)
    lp, _, k6 = bj.kernel_timed(lambda: bj.logpdf(td, y))
    assert k6 <= 2, f"logpdf took {k6} hot launches"                             # the fused inverse run (+ the base density's chain), not one per layer
    ref_lp = -0.5 * (Zi ** 2).sum(axis=0) - 0.5 * dim * math.log(2 * math.pi) + li
    close(host(lp), ref_lp, dt, scale=nl + dim, what="logpdf through the fused inverse")


def test_mixed_flows_split_where_they_must(bj, orc):
    r = rng(1500)
    dim, N, dt = 10, 333, np.float64
    al, be, z0 = _params(r, dim, 2, dt)
    rs = _layers(bj, al, be, z0)
    w = (r.normal(size=(dim, 2)) / math.sqrt(dim)).astype(dt)
    u = (r.normal(size=(dim, 2)) / math.sqrt(dim)).astype(dt)
    pb = r.normal(size=2).astype(dt)
    ps = [bj.PlanarLayer(torch.tensor(np.ascontiguousarray(w[:, k])).cuda(), torch.tensor(np.ascontiguousarray(u[:, k])).cuda(), torch.tensor(pb[k:k + 1]).cuda()) for k in range(2)]
    Z = _points(r, dim, N, dt)
    flow = ps[1] @ ps[0] @ rs[1] @ rs[0]                   # Planar ∘ Planar ∘ Radial ∘ Radial
    bj.with_logabsdet_jacobian(flow, dev(Z))
    (y, l), _, k = bj.kernel_timed(lambda: bj.with_logabsdet_jacobian(flow, dev(Z)))
    assert k == 2
    Y1, l1, _ = _ref_map(orc, al, be, z0, Z)
    Y2, l2 = orc.planar(w, u, pb, Y1)
    close(host(y), Y2, dt, what="2 radial then 2 planar")
    close(host(l), l1 + l2, dt, scale=4, what="ladj")
    # a Shift between two radial layers splits the run; the chain still evaluates
    flow2 = rs[1] @ bj.Shift(0.25) @ rs[0]
    assert [type(st).__name__ for st in flow2._plan()[0]] == ["RadialLayer", "Shift", "RadialLayer"]
    y3, l3 = bj.with_logabsdet_jacobian(flow2, dev(Z), per_sample=True)
    Ya, la = orc.radial(al[0], be[0], z0[:, 0], Z)
    Yb, lb_ = orc.radial(al[1], be[1], z0[:, 1], np.asfortranarray(Ya + 0.25))
    close(host(y3), Yb, dt, what="radial shift radial")
    close(host(l3), la + lb_, dt, scale=2, what="ladj")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(128, 8, 130), (10, 3, 100), (64, 2, 513)])
def test_round_trip(bj, dim, nl, N, dt):
    r = rng(1600 + dim)
    al, be, z0 = _params(r, dim, nl, dt)
    flow = _compose(_layers(bj, al, be, z0))
    Z = _points(r, dim, N, dt)
    back = bj.transform(bj.inverse(flow), bj.transform(flow, dev(Z)))
    np.testing.assert_allclose(host(back), Z, rtol=1e-3 if dt == np.float32 else 1e-6, atol=(2e-3 if dt == np.float32 else 2e-8))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 67), (10, 3, 70)])
def test_aliasing_gives_the_same_bits(bj, dim, nl, N, dt):
    r = rng(1700 + dim)
    al, be, z0 = _params(r, dim, nl, dt)
    tabs = _tables(al, be, z0)
    Z, G = _points(r, dim, N, dt), np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = torch.from_numpy(r.normal(size=N).astype(dt)).cuda()
    for inverse in (False, True):
        x, y = dev(Z), torch.empty((N, dim), dtype=dev(Z).dtype, device="cuda").T
        assert _c_stack(bj, inverse, tabs, nl, x, y) == 0
        xa = dev(Z)
        assert _c_stack(bj, inverse, tabs, nl, xa, xa) == 0                      # out == in
        assert torch.equal(xa, y)
        g, xb = dev(G), torch.empty((N, dim), dtype=dev(G).dtype, device="cuda").T
        assert _c_stack_vjp(bj, inverse, tabs, nl, x, g, lbar, xb) == 0
        ga = dev(G)
        assert _c_stack_vjp(bj, inverse, tabs, nl, x, ga, lbar, ga) == 0        # in_bar == out_bar
        assert torch.equal(ga, xb)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim,nl,N", [(64, 3, 1030), (10, 3, 4100)])
def test_log_det_sum_accumulate_and_empty_batch(bj, dim, nl, N, dt):
    r = rng(1800 + dim)
    al, be, z0 = _params(r, dim, nl, dt)
    tabs = _tables(al, be, z0)
    x = dev(_points(r, dim, N, dt))
    y = torch.empty((N, dim), dtype=x.dtype, device="cuda").T
    ps = torch.empty(N, dtype=x.dtype, device="cuda")
    s = torch.empty(1, dtype=torch.float64, device="cuda")
    assert _c_stack(bj, False, tabs, nl, x, y, ps, s) == 0
    sum_close(float(s), float(host(ps).astype(np.float64).sum()), dt, N, what="ladj_sum vs Σ ladj_ps")
    s2 = torch.empty(1, dtype=torch.float64, device="cuda")
    assert _c_stack(bj, False, tabs, nl, x, y, None, s2) == 0
    assert torch.equal(s, s2)                                                    # fixed-order reduction: repeated calls give the same bits
    ps0, s0 = ps.clone(), float(s)
    assert _c_stack(bj, False, tabs, nl, x, y, ps, s, flags=bj._lib.BJX_ACCUMULATE) == 0
    np.testing.assert_allclose(host(ps), 2 * host(ps0), rtol=1e-6)
    assert abs(float(s) - 2 * s0) <= 1e-12 * abs(s0) + 1e-12
    # an empty batch: the sum is zeroed, nothing is launched
    s.fill_(7.0)
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_stack(bj, False, tabs, nl, None, None, None, s, dim=dim, batch=0) == 0
    assert _c_stack_vjp(bj, False, tabs, nl, None, None, None, None, dim=dim, batch=0) == 0
    assert _launches(bj) == n0 and float(s) == 0.0


def test_run_follows_parameter_updates(bj):
    """The gathered tables are rebuilt when a layer's parameter changes in place (an optimiser step), when an attribute is
    re-assigned, and when a host-resident parameter is re-uploaded."""
    r = rng(1900)
    dim, nl, N, dt = 32, 4, 257, np.float32
    for on_device in (True, False):
        al, be, z0 = _params(r, dim, nl, dt)
        ls = _layers(bj, al, be, z0, on_device=on_device)
        flow = _compose(ls)
        Zd = dev(_points(r, dim, N, dt))
        y0, l0 = bj.with_logabsdet_jacobian(flow, Zd)
        with torch.no_grad():
            ls[2].z_0.mul_(0.5)
            ls[0].beta.add_(0.125)
        y1, l1 = bj.with_logabsdet_jacobian(flow, Zd)
        assert not torch.equal(y0, y1)
        fresh = _compose([bj.RadialLayer(l.alpha_.clone(), l.beta.clone(), l.z_0.clone()) for l in ls])
        y2, l2 = bj.with_logabsdet_jacobian(fresh, Zd)
        assert torch.equal(y1, y2) and torch.equal(l1, l2)
        ls[1].z_0 = ls[1].z_0 + 0.25                                            # a re-assigned attribute
        y3, l3 = bj.with_logabsdet_jacobian(flow, Zd)
        assert not torch.equal(y3, y1)
        fresh = _compose([bj.RadialLayer(l.alpha_.clone(), l.beta.clone(), l.z_0.clone()) for l in ls])
        y4, l4 = bj.with_logabsdet_jacobian(fresh, Zd)
        assert torch.equal(y3, y4) and torch.equal(l3, l4)


def test_refused_height_falls_back_to_the_layers(bj, orc):
    """2 049 Float32 rows: 513 packs, more than 64 lanes x 8 packs — the first height the register kernels' geometry (flow_cfg,
    bjx_flow.hip) refuses.  The run is evaluated layer by layer (2 launches, oracle values); the C entries answer
    BJX_ERR_UNSUPPORTED and launch nothing."""
    dim, nl, N, dt = 2049, 2, 3, np.float32
    r = rng(2000)
    al, be, z0 = _params(r, dim, nl, dt)
    Z, G = _points(r, dim, N, dt), np.asfortranarray(r.normal(size=(dim, N)).astype(dt))
    lbar = r.normal(size=N).astype(dt)
    flow = _compose(_layers(bj, al, be, z0))
    bj.with_logabsdet_jacobian(flow, dev(Z), per_sample=True)
    (y, l), _, k = bj.kernel_timed(lambda: bj.with_logabsdet_jacobian(flow, dev(Z), per_sample=True))
    assert k == 2
    Y, lr, _ = _ref_map(orc, al, be, z0, Z)
    close(host(y), Y, dt, what="fallback map")
    close(host(l), lr, dt, scale=nl, what="fallback ladj")
    flat_close(host(bj.vjp(flow, dev(Z), dev(G), torch.from_numpy(lbar).cuda())), _ref_vjp(orc, al, be, z0, Z, G, lbar), dt, "fallback vjp")
    tabs = _tables(al, be, z0)
    x = dev(Z)
    y2 = torch.empty((N, dim), dtype=x.dtype, device="cuda").T
    torch.cuda.synchronize()
    n0 = _launches(bj)
    U = bj._lib.ERR_UNSUPPORTED
    assert _c_stack(bj, False, tabs, nl, x, y2) == U and _c_stack(bj, True, tabs, nl, x, y2) == U
    assert _c_stack_vjp(bj, False, tabs, nl, x, dev(G), None, y2) == U
    assert _launches(bj) == n0


def test_argument_checks_launch_nothing(bj):
    dim, nl, N, dt = 8, 2, 5, np.float32
    r = rng(2100)
    al, be, z0 = _params(r, dim, nl, dt)
    tabs = _tables(al, be, z0)
    x = dev(_points(r, dim, N, dt))
    y = torch.empty((N, dim), dtype=x.dtype, device="cuda").T
    L = bj._lib
    torch.cuda.synchronize()
    n0 = _launches(bj)
    assert _c_stack(bj, False, tabs, 0, x, y) == L.ERR_SHAPE and _c_stack(bj, False, tabs, -1, x, y) == L.ERR_SHAPE
    assert _c_stack(bj, False, tabs, nl, x, y, dim=0) == L.ERR_SHAPE
    assert _c_stack_vjp(bj, False, tabs, 0, x, x, None, y) == L.ERR_SHAPE and _c_stack_vjp(bj, False, tabs, nl, x, x, None, y, dim=0) == L.ERR_SHAPE
    assert _c_stack(bj, False, (None, tabs[1], tabs[2]), nl, x, y, dt=L.BJX_F32) == L.ERR_ARG
    assert _c_stack(bj, False, (tabs[0], tabs[1], None), nl, x, y) == L.ERR_ARG
    assert _c_stack(bj, False, tabs, nl, x, None) == L.ERR_ARG and _c_stack(bj, False, tabs, nl, None, y, dim=dim, batch=N) == L.ERR_ARG
    assert _c_stack_vjp(bj, False, tabs, nl, x, None, None, y) == L.ERR_ARG and _c_stack_vjp(bj, False, tabs, nl, x, x, None, None) == L.ERR_ARG
    assert _c_stack(bj, False, tabs, nl, x, y, dt=77) == L.ERR_ARG and _c_stack_vjp(bj, False, tabs, nl, x, x, None, y, dt=77) == L.ERR_ARG
    assert _launches(bj) == n0


@pytest.mark.parametrize("dt", DTYPES)
def test_vjp_params_of_a_composition_with_a_radial_run_is_per_layer(bj, dt):
    """`vjp_params` is not fused: a composition with a radial run returns what the layers' own rules give one after another
    (the chain rule by hand, same launches: the same bits)."""
    r = rng(2200)
    dim, nl, N = 12, 3, 70
    al, be, z0 = _params(r, dim, nl, dt)
    ls = _layers(bj, al, be, z0)
    flow = _compose(ls) @ bj.Shift(0.5)                     # Shift, then the run of three
    Zd = dev(_points(r, dim, N, dt))
    Gd = dev(np.asfortranarray(r.normal(size=(dim, N)).astype(dt)))
    lb = torch.from_numpy(r.normal(size=N).astype(dt)).cuda()
    assert [type(s).__name__ for s in flow._plan()[0]] == ["Shift", "_RadialRun"]
    xb, gr = bj.vjp_params(flow, Zd, Gd, lb)
    assert len(gr["stages"]) == 4
    stages = [bj.Shift(0.5)] + ls
    inputs = [Zd]
    for st in stages[:-1]:
        inputs.append(bj.transform(st, inputs[-1]))
    g, by_hand = Gd, [None] * 4
    for i in (3, 2, 1):
        g, by_hand[i] = bj.vjp_params(stages[i], inputs[i], g, lb)
    for i in (1, 2, 3):
        for name in ("alpha_", "beta", "z_0"):
            assert gr["stages"][i][name].shape == by_hand[i][name].shape
            flat_close(host(gr["stages"][i][name]), host(by_hand[i][name]), dt, f"vjp_params stage {i} {name}", per="tensor")
    flat_close(host(xb), host(bj.vjp(bj.Shift(0.5), Zd, g, lb)), dt, "vjp_params input cotangent")
