"""Host side of `logpdf_vjp_params` and of the fused log-density pass for RadialLayer runs (include/bjx_radial_stack_logpdf.h), no GPU:
the header's prototype is the ctypes signature of bijectors.jl_amd/_lib.py, argument by argument; the Float64 reference the GPU tests
use (tests/_logpdf_grad_ref.py) agrees with central differences of Σ c·lp taken through the oracle's MAPS for every parameter and for
y — the yardstick is pinned before any GPU run —; and a numpy Float64 emulation of the kernel's order of operations (the full primal
sweep, whitening, the generated seed, the reverse sweep that rewinds from x by 1/γₖ, the μ̄ / σ̄ rows) agrees with that reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _logpdf_grad_ref import objective, ref_logpdf_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_radial_stack_logpdf.h")
ENTRIES = ["bjx_radial_stack_logpdf_vjp_params"]

_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


@pytest.fixture(scope="module")
def bj():
    import bijectors_amd

    return bijectors_amd


def test_header_prototype_matches_the_ctypes_signature(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_RADIAL_STACK_LOGPDF
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
    # the sibling headers' tables and bjx.h are as they were; the function is exported like logpdf
    assert list(bj._lib.SIGNATURES_RADIAL_STACK_PARAMS) == ["bjx_radial_stack_vjp_params"]
    assert "radial_stack" not in open(os.path.join(ROOT, "include", "bjx.h")).read()
    assert "logpdf_vjp_params" in bj.__all__ and callable(bj.logpdf_vjp_params)


def test_bases_out_of_scope_raise(bj):
    import torch

    flow = bj.RadialLayer(torch.zeros(1), torch.zeros(1), torch.zeros(3))
    y = torch.zeros(3, 2)
    with pytest.raises(NotImplementedError, match="full-covariance"):
        bj.logpdf_vjp_params(bj.transformed(bj.MvNormal(torch.zeros(3), cov=torch.eye(3)), flow), y)
    with pytest.raises(NotImplementedError, match="MvNormal"):
        bj.logpdf_vjp_params(bj.transformed(bj.TorchBase(torch.distributions.Normal(torch.zeros(3), torch.ones(3))), flow), y)


def test_base_parameters_of_the_wrong_length_raise_before_any_kernel(bj):
    """The kernels read `dim` entries of μ and σ: a one-element ("isotropic") or otherwise short σ, or a long one, is a DimensionMismatch
    on a RadialLayer flow (the fused pass) as on any other transform (the generic path) — raised before the input is even looked at."""
    import torch

    r1 = bj.RadialLayer(torch.zeros(1), torch.zeros(1), torch.zeros(3))
    r2 = bj.RadialLayer(torch.ones(1), torch.zeros(1), torch.ones(3))
    y = torch.zeros(3, 2)
    for flow in (r1, r2 @ r1, bj.Shift(0.5)):
        for sigma in (torch.ones(1), torch.ones(2), torch.ones(4)):
            with pytest.raises(ValueError, match="DimensionMismatch: base parameter sigma"):
                bj.logpdf_vjp_params(bj.transformed(bj.MvNormal(torch.zeros(3), sigma), flow), y)
        with pytest.raises(ValueError, match="DimensionMismatch"):
            bj.logpdf_vjp_params(bj.transformed(bj.MvNormal(torch.zeros(3), torch.ones(3)), flow), torch.zeros(4, 2))


def _draw(dim, nl, N, seed, diagonal=True):
    r = np.random.default_rng(seed)
    al, be = 0.5 * r.normal(size=nl), r.normal(size=nl)
    z0 = 0.3 * r.normal(size=(dim, nl))
    Y = r.normal(size=(dim, N))
    Y[0] += 2.0
    mu = 0.2 * r.normal(size=dim) if diagonal else None
    sigma = np.exp(0.3 * r.normal(size=dim)) if diagonal else None
    return al, be, z0, mu, sigma, np.asfortranarray(Y), r.normal(size=N)


@pytest.mark.parametrize("dim,nl,N", [(6, 3, 5), (2, 1, 7)])
def test_reference_is_the_central_difference_of_the_objective(orc, dim, nl, N):
    """d/dθ Σ c·lp through the oracle's inverse map and its log-det alone, central differences with step h = 1e-5 in Float64:
    truncation ~h²·|f‴|/6 ~ 1e-11, rounding ~1e-16·|Σ c·lp|/h ~ 1e-10 of the objective's terms.  Bar: 1e-6 of max(|derivative|,
    max |summand|) for every parameter entry (α_, β, every z₀ row of every layer, every μ and σ row) and, for y, 1e-6 of the column's
    max-norm — the flat Float64 bar of the GPU tests on the same scales."""
    al, be, z0, mu, sigma, Y, c = _draw(dim, nl, N, 50 + dim)
    ref = ref_logpdf_grad(orc, al, be, z0, mu, sigma, Y, c)
    h = 1e-5
    ta, tb, tz = ref["terms"]

    def fd(name, idx):
        vals = []
        for sgn in (+1.0, -1.0):
            p = dict(al=al.copy(), be=be.copy(), z0=z0.copy(), mu=mu.copy(), sigma=sigma.copy(), Y=Y.copy())
            p[name][idx] += sgn * h
            vals.append(objective(orc, p["al"], p["be"], p["z0"], p["mu"], p["sigma"], p["Y"], c))
        return (vals[0] - vals[1]) / (2 * h)

    worst = 0.0
    for k in range(nl):
        checks = [("al", k, ref["alpha_bar"][k], ta[k]), ("be", k, ref["beta_bar"][k], tb[k])] + [("z0", (i, k), ref["z0_bar"][i, k], tz[k]) for i in range(dim)]
        for name, idx, got, term in checks:
            d = fd(name, idx)
            err = abs(got - d) / max(abs(d), term)
            worst = max(worst, err)
            assert err <= 1e-6, f"{name}{idx}: reference {got} vs central difference {d}"
    for i in range(dim):
        for name, got, term in (("mu", ref["mu_bar"][i], ref["t_mu"]), ("sigma", ref["sigma_bar"][i], ref["t_sigma"])):
            d = fd(name, i)
            err = abs(got - d) / max(abs(d), term)
            worst = max(worst, err)
            assert err <= 1e-6, f"{name}[{i}]: reference {got} vs central difference {d}"
    for n in range(N):
        scale = np.abs(ref["y_bar"][:, n]).max()
        for i in range(dim):
            d = fd("Y", (i, n))
            err = abs(ref["y_bar"][i, n] - d) / scale
            worst = max(worst, err)
            assert err <= 1e-6, f"y_bar[{i},{n}]: reference {ref['y_bar'][i, n]} vs central difference {d}"
    print(f"dim {dim}, {nl} layers: worst error of the reference against central differences {worst:.3g} of its scale")


def _emulate(al, be, z0, mu, sigma, Y, c):
    """rsp_group_body / rsp_walk_body with LP = true in numpy Float64, all columns at once."""
    dim, N = Y.shape
    nl = len(al)
    sp = lambda v: np.logaddexp(0.0, v)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    alpha, apb = sp(al), sp(be)
    bh = apb - alpha
    m = np.zeros((dim, 1)) if mu is None else mu.reshape(-1, 1)
    s = np.ones((dim, 1)) if sigma is None else sigma.reshape(-1, 1)
    z = Y.copy()
    stash = [None] * nl
    ldet = np.zeros(N)
    for li in range(nl):                                              # primal sweep: EVERY layer is applied, the log-det is summed
        l = nl - 1 - li
        Z0 = z0[:, l:l + 1]
        dl = z - Z0
        gam = np.sqrt((dl * dl).sum(axis=0))
        aa = apb[l] - gam
        r0 = (np.sqrt(aa * aa + 4 * alpha[l] * gam) - aa) / 2
        gain = (alpha[l] + r0) / (apb[l] + r0)
        stash[l] = (gain, gam)
        rf = gain * gam
        h = 1.0 / (alpha[l] + rf)
        ldet -= (dim - 1) * np.log(1.0 + bh[l] * h) + np.log(1.0 + bh[l] * h - bh[l] * h * h * rf)
        z = Z0 + gain * dl
    w = (z - m) / s                                                   # whitening at x, the density, the seed
    cst = np.log(s).sum() + 0.5 * dim * np.log(2.0 * np.pi)
    lp = -0.5 * (w * w).sum(axis=0) - cst + ldet
    g = -c * w / s
    mu_bar = (-g).sum(axis=1)
    sigma_bar = (-g * w - c / s).sum(axis=1)
    ab, bb, zb = np.zeros(nl), np.zeros(nl), np.zeros((dim, nl))
    for li in range(nl - 1, -1, -1):                                  # reverse sweep: rewind from x by 1/γₖ, every layer
        l = nl - 1 - li
        Z0 = z0[:, l:l + 1]
        gain = stash[l][0]
        rr = gain * stash[l][1]
        h = 1.0 / (alpha[l] + rr)
        a = 1.0 + bh[l] * h
        cc = -bh[l] * h * h / rr
        lr = (dim - 1) * (-bh[l] * h * h) / a + (-2.0 * bh[l] * h * h + 2.0 * bh[l] * h ** 3 * rr) / (1.0 + bh[l] * h - bh[l] * h * h * rr)
        kl = c * lr / rr
        z = Z0 + (z - Z0) * (1.0 / gain)
        dl = z - Z0
        dg = (dl * g).sum(axis=0)
        dv = gain * dg - kl * rr * rr
        ca, cd = 1.0 / a, gain * (-kl / a - cc * dv / (a * (a + cc * rr * rr)))
        dgx, lbx = -(dv / (a + cc * rr * rr)), -c
        gn = ca * g + cd * dl
        zb[:, l] = (g - gn).sum(axis=1)
        D = a - bh[l] * h * h * rr
        gb = h * dgx + lbx * ((dim - 1) * h / a + (h - h * h * rr) / D)
        ga = -h * h * (bh[l] * dgx + lbx * ((dim - 1) * bh[l] / a + (bh[l] - 2.0 * bh[l] * h * rr) / D))
        ab[l] = sig(al[l]) * (ga.sum() - gb.sum())
        bb[l] = sig(be[l]) * gb.sum()
        g = gn
    return dict(lp=lp, y_bar=g, alpha_bar=ab, beta_bar=bb, z0_bar=zb, mu_bar=mu_bar, sigma_bar=sigma_bar)


@pytest.mark.parametrize("diagonal", [True, False])
@pytest.mark.parametrize("dim,nl,N", [(6, 3, 33), (2, 1, 20), (12, 5, 50), (35, 3, 17)])
def test_numpy_emulation_of_the_kernels_order_matches_the_reference(orc, dim, nl, N, diagonal):
    al, be, z0, mu, sigma, Y, c = _draw(dim, nl, N, 100 * dim + nl, diagonal)
    ref = ref_logpdf_grad(orc, al, be, z0, mu, sigma, Y, c)
    emu = _emulate(al, be, z0, mu, sigma, Y, c)
    for what in ("lp", "y_bar", "alpha_bar", "beta_bar", "z0_bar", "mu_bar", "sigma_bar"):
        err = np.abs(emu[what] - ref[what]).max() / (np.abs(ref[what]).max() + 1e-300)
        assert err <= 1e-12, f"{what}: {err:.3g} of the reference's max-norm (dim {dim}, {nl} layers)"
    # all-zero cotangent: every gradient vanishes exactly, the density does not change
    zero = _emulate(al, be, z0, mu, sigma, Y, np.zeros(N))
    assert np.array_equal(zero["lp"], emu["lp"])
    assert all(not np.any(zero[k]) for k in ("y_bar", "alpha_bar", "beta_bar", "z0_bar", "mu_bar", "sigma_bar"))
