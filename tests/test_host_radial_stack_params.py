"""Host side of the fused parameter pullback of a RadialLayer run (include/bjx_radial_stack_params.h, `_RadialRun._vjp_params`), no
GPU: the header's prototype is the ctypes signature of bijectors.jl_amd/_lib.py, argument by argument; `_vjp_params_composed` hands
radial runs of either direction to the run and maps its per-layer dictionaries back onto `_stages()`; and a numpy Float64 emulation
of the kernel's two sweeps — the primal sweep that keeps one or two scalars per layer, the reverse sweep that REWINDS the column,
takes z̄₀ₖ from ḡ − ḡ′ and the inverse run's dot product from the closed form (gain·dg − kl·r²)/(a + c·r²) — agrees with the oracle
composed layer by layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _radial_params_ref import ref_run_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_radial_stack_params.h")
ENTRIES = ["bjx_radial_stack_vjp_params"]

_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


@pytest.fixture(scope="module")
def bj():
    import bijectors_amd

    return bijectors_amd


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_RADIAL_STACK_PARAMS
    assert list(table) == ENTRIES
    for ret, name, args in protos:
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.fullmatch(r"(.*?[\w*])\s*(\w+)?", a)
            ty = m.group(1) if m.group(2) and not a.endswith("*") else a
            types.append(_CTYPES[ty.replace(" *", "*")])
        res, argtypes = table[name]
        assert res is C.c_int and ret == "int"
        assert argtypes == types, f"{name}: header {types} vs _lib.py {argtypes}"
    # the sibling header, its table and bjx.h are as they were
    assert list(bj._lib.SIGNATURES_RADIAL_STACK) == ["bjx_radial_stack", "bjx_radial_stack_vjp"]
    assert "radial_stack" not in open(os.path.join(ROOT, "include", "bjx.h")).read()


def _rad(bj, k, dim=3):
    import torch

    return bj.RadialLayer(torch.full((1,), 0.1 * k), torch.full((1,), -0.2 * k), torch.full((dim,), float(k)))


def test_composition_hands_radial_runs_to_the_run_and_maps_the_layers_back(bj, monkeypatch):
    """The planned stages (not the unfused list) drive `_vjp_params_composed`: a run is ONE call of `_RadialRun._vjp_params` with its
    direction, and layer k's dictionary lands on stage lo + k (inverse run: hi − 1 − k)."""
    import torch

    I = bj.interface
    rs = [_rad(bj, k) for k in range(4)]
    calls = []

    def fake(self, x, out_bar, ladj_bar, inv):
        calls.append((list(self.layers), inv))
        return out_bar, [{"layer": l} for l in self.layers]

    monkeypatch.setattr(I._RadialRun, "_vjp_params", fake)
    monkeypatch.setattr(I, "transform", lambda st, x: x)
    x = torch.zeros(3, 2)
    flow = rs[2] @ rs[1] @ rs[0]
    xb, gr = bj.vjp_params(flow, x, x)
    assert calls == [(rs[0:3], False)] and [d["layer"] for d in gr["stages"]] == rs[0:3]
    calls.clear()
    xb, gr = bj.vjp_params(bj.inverse(flow), x, x)                   # stages: inv(r2), inv(r1), inv(r0); the run is r0, r1, r2
    assert calls == [(rs[0:3], True)] and [d["layer"] for d in gr["stages"]] == [rs[2], rs[1], rs[0]]
    assert [s.orig for s in bj.inverse(flow)._stages()] == [rs[2], rs[1], rs[0]]
    calls.clear()
    two_dirs = bj.inverse(rs[3]) @ bj.inverse(rs[2]) @ rs[1] @ rs[0]  # a forward run, then an inverse one (of r3 ∘ r2 reversed)
    xb, gr = bj.vjp_params(two_dirs, x, x)
    assert calls == [([rs[3], rs[2]], True), (rs[0:2], False)]        # pulled back from the last stage
    assert [d["layer"] for d in gr["stages"]] == [rs[0], rs[1], rs[2], rs[3]]
    # the run itself: dictionaries in application order
    calls.clear()
    run = I._RadialRun(rs[0:3])
    assert [d["layer"] for d in bj.vjp_params(run, x, x)[1]["stages"]] == rs[0:3]
    assert [d["layer"] for d in bj.vjp_params(bj.inverse(run), x, x)[1]["stages"]] == [rs[2], rs[1], rs[0]]
    # the layer-by-layer plan is still there for the fallback
    st, sp = I._radial_runs_unfused(flow)
    assert st == rs[0:3] and sp == [(0, 1), (1, 2), (2, 3)]


def _emulate(al, be, z0, X, G, lbar, inverse):
    """The two sweeps of radial_stack_params_kernel in numpy Float64, all columns at once."""
    dim, N = X.shape
    nl = len(al)
    sp = lambda v: np.logaddexp(0.0, v)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    alpha, apb = sp(al), sp(be)
    bh = apb - alpha
    lb = np.zeros(N) if lbar is None else lbar
    z, g = X.copy(), G.copy()
    stash = [None] * nl
    for li in range(nl):                                              # primal sweep: the last layer is not applied
        l = nl - 1 - li if inverse else li
        Z0 = z0[:, l:l + 1]
        dl = z - Z0
        ss = (dl * dl).sum(axis=0)
        if not inverse:
            rr = np.sqrt(ss)
            stash[l] = (rr,)
            if li + 1 < nl:
                z = z + bh[l] / (alpha[l] + rr) * dl
        else:
            gam = np.sqrt(ss)
            aa = apb[l] - gam
            r0 = (np.sqrt(aa * aa + 4 * alpha[l] * gam) - aa) / 2
            gain = (alpha[l] + r0) / (apb[l] + r0)
            stash[l] = (gain, gam)
            if li + 1 < nl:
                z = Z0 + gain * dl
    ab, bb, zb = np.zeros(nl), np.zeros(nl), np.zeros((dim, nl))
    for li in range(nl - 1, -1, -1):                                  # reverse sweep
        l = nl - 1 - li if inverse else li
        Z0 = z0[:, l:l + 1]
        if not inverse:
            rr, gain = stash[l][0], 1.0
        else:
            gain = stash[l][0]
            rr = gain * stash[l][1]
        h = 1.0 / (alpha[l] + rr)
        a = 1.0 + bh[l] * h
        c = -bh[l] * h * h / rr
        lr = (dim - 1) * (-bh[l] * h * h) / a + (-2.0 * bh[l] * h * h + 2.0 * bh[l] * h ** 3 * rr) / (1.0 + bh[l] * h - bh[l] * h * h * rr)
        kl = lb * lr / rr
        if li + 1 < nl:                                               # rewind the column to this layer's input
            z = Z0 + (z - Z0) * (1.0 / a if not inverse else 1.0 / gain)
        dl = z - Z0
        dg = (dl * g).sum(axis=0)
        if not inverse:
            ca, cd, dgx, lbx = a, c * dg + kl, dg, lb
        else:
            dv = gain * dg - kl * rr * rr
            ca, cd = 1.0 / a, gain * (-kl / a - c * dv / (a * (a + c * rr * rr)))
            dgx, lbx = -(dv / (a + c * rr * rr)), -lb                 # −δ_preᵀḡ′ without a second reduction
        gn = ca * g + cd * dl
        zb[:, l] = (g - gn).sum(axis=1)
        D = a - bh[l] * h * h * rr
        gb = h * dgx + lbx * ((dim - 1) * h / a + (h - h * h * rr) / D)
        ga = -h * h * (bh[l] * dgx + lbx * ((dim - 1) * bh[l] / a + (bh[l] - 2.0 * bh[l] * h * rr) / D))
        ab[l] = sig(al[l]) * (ga.sum() - gb.sum())
        bb[l] = sig(be[l]) * gb.sum()
        g = gn
    return g, ab, bb, zb


@pytest.mark.parametrize("with_lbar", [True, False])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dim,nl,N", [(2, 4, 33), (7, 1, 20), (12, 5, 50), (35, 3, 17)])
def test_numpy_emulation_of_both_sweeps_matches_the_oracle(orc, dim, nl, N, inverse, with_lbar):
    r = np.random.default_rng(100 * dim + nl)
    al, be = 0.5 * r.normal(size=nl), r.normal(size=nl)
    z0 = 0.3 * r.normal(size=(dim, nl))
    X = r.normal(size=(dim, N))
    X[0] += 2.0
    X = np.asfortranarray(X)
    G = np.asfortranarray(r.normal(size=(dim, N)))
    lbar = r.normal(size=N) if with_lbar else None
    xb, ab, bb, zb, _ = ref_run_params(orc, al, be, z0, X, G, lbar, inverse)
    exb, eab, ebb, ezb = _emulate(al, be, z0, X, G, lbar, inverse)
    for got, ref, what in ((exb, xb, "x_bar"), (eab, ab, "alpha_bar"), (ebb, bb, "beta_bar"), (ezb, zb, "z0_bar")):
        err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300)
        assert err <= 1e-10, f"{what}: {err:.3g} of the reference's max-norm (dim {dim}, {nl} layers, inverse={inverse})"
