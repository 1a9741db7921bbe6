"""The numpy reference the GPU suite of bjx_scale_matrix_chain rests on (tests/_scale_matrix_chain_ref.py), checked on the CPU against the
project's oracle: `oracle.chain` for the chain and its log-det, `oracle.mvnormal_full_logpdf` for the density term — to 1e-12 — and
finite on every input the GPU suite draws.  No GPU, no torch."""
import math

import numpy as np
import pytest

import _scale_matrix_chain_ref as R

BAR = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want) / (np.abs(want) + 1.0)
    assert err.max() <= BAR, f"{what}: {err.max():.3g}"


@pytest.mark.parametrize("dim", [2, 6, 12, 64])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_chain_and_log_det_match_the_oracle(orc, name, dim):
    batch = 7
    ops, x = R.family(name, dim, batch, np.float64)
    cx, l = R.chain_ref(ops, x)
    y_orc, l_total = orc.chain(ops, x)
    _close(cx, y_orc, f"{name} c(x)")
    if not any(k in (R.OP_SCALE, R.OP_SCALE_INV) and np.ndim(p) for k, p, _ in ops):
        _close(l.sum(), l_total, f"{name} Σ log-det")       # (a per-row Scale on a MATRIX: the reference, and the oracle with it, counts Σ log|a_i| once, scale.jl:31-32)
    for n in range(batch):       # a vector input: the log-det of that column alone
        y1, l1 = orc.chain(ops, x[:, n].copy())
        _close(cx[:, n], y1, f"{name} column {n}")
        _close(l[n], l1, f"{name} log-det of column {n}")


@pytest.mark.parametrize("dim", [2, 6, 12, 64])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_values_log_det_and_density_match_the_oracle(orc, name, dim):
    """out and ladj of ref() from the oracle's chain and numpy's factorisations; the density flag with a Cholesky factor in the inverse
    direction is the oracle's full-covariance normal density of c(x) plus the chain's log-det (transformed_distribution.jl:165-169)."""
    batch = 5
    ops, x = R.family(name, dim, batch, np.float64)
    cx = np.asfortranarray(orc.chain(ops, x)[0])
    lc = np.array([float(orc.chain(ops, x[:, n].copy())[1]) for n in range(batch)])
    a = R.matrix(dim, np.float64)
    lad = np.linalg.slogdet(a)[1]
    out, ladj = R.ref(a, ops, x, 0, False)
    _close(out, a @ cx, f"{name} a c(x)")
    _close(ladj, lc + lad, f"{name} forward log-det")
    out, ladj = R.ref(a, ops, x, 1, False)
    _close(a @ out, cx, f"{name} a (a \\ c(x))")
    _close(ladj, lc - lad, f"{name} inverse log-det")
    # the density: cov = L Lᵀ with L exactly the factor the oracle recomputes
    r = R.rng_for("cov", dim)
    A = r.normal(size=(dim, dim)) / math.sqrt(dim)
    cov = A @ A.T + 0.3 * np.eye(dim)
    Lc = np.linalg.cholesky(cov)
    out, ladj = R.ref(Lc, ops, x, 1, True)
    _close(ladj, orc.mvnormal_full_logpdf(cx, np.zeros(dim), cov) + lc, f"{name} logpdf")
    _close(out, np.linalg.solve(Lc, cx), f"{name} whitened values")
    # forward with the density flag: log N(a c(x); 0, I) + log-det, with I as the covariance
    out, ladj = R.ref(a, ops, x, 0, True)
    _close(ladj, orc.mvnormal_full_logpdf(a @ cx, np.zeros(dim), np.eye(dim)) + lc + lad, f"{name} forward density")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_reference_is_finite_on_every_input_of_the_gpu_suite(dt):
    for dim in R.dims_of(dt):
        mats = [(R.matrix(dim, dt), 0), (R.matrix(dim, dt), 1), (R.matrix(dim, dt, "cholesky"), 1)]
        for name in R.FAMILIES:
            for batch in R.batches_of(dt, dim):
                ops, x = R.family(name, dim, batch, dt)
                assert x.dtype == np.dtype(dt) and x.shape == (dim, batch)
                if any(k == R.OP_LOG for k, _, _ in ops):
                    assert (x > 0).all(), "a log would see a non-positive argument"
                for a, inverse in mats:
                    out, ladj = R.ref(a, ops, x, inverse, True)
                    assert np.isfinite(out).all() and np.isfinite(ladj).all(), (name, dim, batch, inverse)
                    # nothing overflows in the call's own type either
                    assert np.isfinite(out.astype(dt)).all() and np.isfinite(ladj.astype(dt)).all(), (name, dim, batch, inverse)


def test_reduction_paths_cover_the_kernel_branches():
    """The dims of the suite reach every way the kernel reduces a column's log-det (csrc/bjx_matrix.hip: colred / DPP / LDS atomics / Gc == 1)."""
    f32 = {d: R.reduction_path(np.float32, d) for d in R.F32_DIMS}
    f64 = {d: R.reduction_path(np.float64, d) for d in R.F64_DIMS}
    assert f32[4] == "Gc1" and f64[2] == "Gc1" and f32[64] == "dpp"
    assert [d for d, p in f32.items() if p == "lds_atomics"] == [12, 24, 48, 80, 96, 112]
    assert [d for d, p in f64.items() if p == "lds_atomics"] == [6, 10, 50, 96, 112]
    assert [d for d, p in f32.items() if p == "shuffle"] == [8, 16, 32, 128]
    assert [d for d, p in f64.items() if p == "shuffle"] == [4, 16, 32, 64]
