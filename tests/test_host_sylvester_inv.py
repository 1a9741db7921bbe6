"""Host side of the inverse of the shared Sylvester layer (include/bjx_sylvester_inv.h, `SylvesterLayer(..., orthonormal=True)`), no GPU:
the Float64 reference of tests/_sylvester_inv_ref.py is held to an independent evaluation — the forward reference applied to its z gives
y back, its ȳ satisfies Jᵀȳ = z̄ − c∇ℓ through the forward reference's `in_bar`, and central differences of φ = ⟨z̄, z(y; θ)⟩ − c·ℓ(z; θ) over
a DENSE Newton solve of the forward forms (a perturbed Q is not orthonormal, so the back-substitution is not what is differenced) hold in
every input and every parameter entry; the companion header is plain C99 and C++ and its prototypes are the ctypes signatures argument by
argument; the built library exports both entries; the host class keeps the inverse opt-in."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _sylvester_inv_ref import RefInv, inv_draws, near_singular
from _sylvester_ref import RefShared, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_sylvester_inv.h")
ENTRIES = ["bjx_sylvester_inv", "bjx_sylvester_inv_vjp"]
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_sylvester_inv.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, const void*, int, const void*, void*, void*, double*, int64_t, int64_t,
           uint32_t) = bjx_sylvester_inv;
  int (*g)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, const void*, int, const void*, const void*, const void*, void*, void*,
           int64_t, int64_t) = bjx_sylvester_inv_vjp;
  return (f != NULL && g != NULL && BJX_SYLVESTER_MAX_UNITS == 16 && BJX_VERSION == 100) ? 0 : 1;
}
"""

CASES = [(dim, M) for dim in (1, 2, 3, 5, 8) for M in (1, 2, 3) if M <= dim]


@pytest.fixture(scope="module")
def bj():
    import bijectors_amd

    return bijectors_amd


# ------------------------------------------------------------------ the reference
def _nan_low(R, Rt):
    low = np.tril(np.ones(R.shape), -1) > 0
    Rn, Rtn = R.copy(), Rt.copy()
    Rn[low], Rtn[low] = np.nan, np.nan
    return Rn, Rtn


@pytest.mark.parametrize("dim,M", CASES)
def test_reference_inverts_the_forward_reference_and_transposes_its_jacobian(dim, M):
    """With NaN below both diagonals: forward(z) = y and ladj = −ℓ(z) to 1e-12 of the column's scale; the forward pullback of (ȳ, c) at z
    is Jᵀȳ + c∇ℓ, so it must give z̄ back."""
    N = 9
    Q, R, Rt, b, z, y, zb, c = inv_draws(seed("sylvester-inv-host", dim, M), dim, M, N, np.float64)
    Rn, Rtn = _nan_low(R, Rt)
    ref = RefInv(Q, Rn, Rtn, b, y, zb, c)
    for k in ("out", "ladj", "in_bar"):
        assert np.isfinite(getattr(ref, k)).all(), k
    assert np.abs(ref.d).min() >= 0.19
    fwd = ref.fwd                                            # RefShared at ref.out with the cotangents (ȳ, c)
    scale = np.maximum(1.0, np.abs(y).max(axis=0))
    assert (np.abs(fwd.out - y).max(axis=0) <= 1e-12 * scale).all(), np.abs(fwd.out - y).max()
    assert np.abs(ref.out - z).max() <= 1e-12 * max(1.0, np.abs(z).max())
    assert np.abs(fwd.ladj + ref.ladj).max() <= 1e-12 * max(1.0, np.abs(ref.ladj).max())
    assert np.abs(fwd.in_bar - zb).max() <= 1e-11 * max(1.0, np.abs(zb).max()), np.abs(fwd.in_bar - zb).max()
    low = np.tril(np.ones((M, M)), -1) > 0
    for t in ref.summed(N)[1:3]:
        assert not t[low].any()


def _dense_inverse(Q, R, Rt, b, y, z0):
    """z with z + Q·triu(R)·tanh(triu(R̃)·Qᵀz + b) = y by Newton's iteration on the dense Jacobian, for ANY Q, column by column."""
    U, Ut = np.triu(R), np.triu(Rt)
    z = z0.copy()
    for n in range(y.shape[1]):
        zn = z[:, n]
        for _ in range(60):
            a = np.tanh(Ut @ (Q.T @ zn) + b)
            f = zn + Q @ (U @ a) - y[:, n]
            J = np.eye(len(zn)) + Q @ U @ np.diag(1.0 - a * a) @ Ut @ Q.T
            step = np.linalg.solve(J, f)
            zn = zn - step
            if np.abs(step).max() <= 1e-15 * max(1.0, np.abs(zn).max()):
                break
        z[:, n] = zn
    return z


def _phi(Q, R, Rt, b, y, zb, c, z0):
    z = _dense_inverse(Q, R, Rt, b, y, z0)
    a = np.tanh(np.triu(Rt) @ (Q.T @ z) + b[:, None])
    ladj = np.log(np.abs(1.0 + (1.0 - a * a) * (np.diag(R) * np.diag(Rt))[:, None])).sum(axis=0)
    return float((zb * z).sum() - c @ ladj)


@pytest.mark.parametrize("dim,M", CASES)
def test_reference_matches_central_differences_over_a_dense_solve(dim, M):
    """φ = Σ_n ⟨z̄_n, z_n(y; θ)⟩ − c_n·ℓ(z_n; θ) with z from the dense Newton solve of the forward forms, differenced (h = 1e-5: truncation
    ~h² and rounding ~eps/h are both ~1e-10 per column, and 1/min|d| <= 5.3 by the draws) in every entry of y and of every parameter (Q a
    free parameter of the forms), at 1e-6 of the term scale."""
    h, N = 1e-5, 4
    Q, R, Rt, b, z, y, zb, c = inv_draws(seed("sylvester-inv-forms", dim, M), dim, M, N, np.float64)
    Rn, Rtn = _nan_low(R, Rt)
    ref = RefInv(Q, Rn, Rtn, b, y, zb, c)
    ts = ref.term_scale(N)
    P = [Q.copy(), R.copy(), Rt.copy(), b.copy(), y.copy()]
    for name, k, want, scale in (("q", 0, ref.summed(N)[0], ts), ("r", 1, ref.summed(N)[1], ts), ("r_tilde", 2, ref.summed(N)[2], ts), ("b", 3, ref.summed(N)[3], ts),
                                 ("y", 4, ref.in_bar, max(ts, np.abs(ref.in_bar).max()))):
        for idx in np.ndindex(P[k].shape):
            if k in (1, 2) and idx[0] > idx[1]:
                continue
            keep = P[k][idx]
            P[k][idx] = keep + h
            hi = _phi(*P, zb, c, ref.out)
            P[k][idx] = keep - h
            lo = _phi(*P, zb, c, ref.out)
            P[k][idx] = keep
            err = abs((hi - lo) / (2 * h) - want[idx]) / scale
            assert err <= 1e-6, f"dim={dim} M={M} {name}{idx}: {err:.3g} of the term scale"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_near_singular_recipe_reaches_small_determinants_and_the_reference_still_inverts(dt):
    for dim, M in ((8, 3), (64, 16)):
        Q, R, Rt, b, z, y, zb, c = near_singular(seed("sylvester-inv-singular", np.dtype(dt).name, dim), dim, M, 64, dt)
        ref = RefInv(Q, R, Rt, b, y, zb, c)
        assert R[0, 0] * Rt[0, 0] > -1.0
        assert 2e-4 <= np.abs(ref.d).min() <= 4e-3, np.abs(ref.d).min()
        tol = 1e-3 if dt == np.float32 else 1e-6       # Q rounded to Float32 is orthonormal to ~1e-7 only
        assert (np.abs(ref.fwd.out - y).max(axis=0) <= 1e-3 * tol * np.abs(y).max(axis=0)).all()


# ------------------------------------------------------------------ the header and the library
@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_as_c99_and_as_cxx(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc, "gcc and g++ are part of the image"
    std, ext = ("-std=c99", "c") if lang == "c" else ("-std=c++11", "cpp")
    src = tmp_path / f"sylvester_inv.{ext}"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, std, *WARN, "-c", str(src), "-o", str(tmp_path / "sylvester_inv.o")])      # both prototypes pinned, not linked
    assert "sylvester_inv" not in open(os.path.join(ROOT, "include", "bjx.h")).read()                    # bjx.h does not mention the companion header
    sib = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bjx_sylvester.h")).read(), flags=re.S)
    assert "sylvester_inv" not in sib                                                                     # bjx_sylvester.h names it in a comment only


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_SYLVESTER_INV
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


def test_built_library_exports_both_entries(bj):
    assert os.path.exists(bj._lib.LIB_PATH), f"{bj._lib.LIB_PATH} is not built"
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


# ------------------------------------------------------------------ the host class
def test_inverse_is_opt_in_and_the_defect_is_reported(bj):
    torch = pytest.importorskip("torch")
    dim, M = 4, 2
    args = (torch.randn(dim, M), torch.randn(M, M), torch.randn(M, M), torch.randn(M))
    plain = bj.SylvesterLayer(*args)
    assert plain.orthonormal is False
    x = torch.randn(8, dim).T
    for call in (lambda: bj.transform(bj.inverse(plain), x), lambda: bj.vjp(bj.inverse(plain), x, x), lambda: bj.vjp_params(bj.inverse(plain), x, x)):
        with pytest.raises(NotImplementedError, match="inverse map is not built") as info:
            call()
        assert "orthonormal=True" in str(info.value)
    layer = bj.SylvesterLayer(*args, orthonormal=True)
    assert layer.orthonormal is True and bj.SylvesterLayer(*args, orthonormal=1).orthonormal is True
    assert (layer.dim, layer.n_units) == (dim, M)
    assert bj.isinvertible(layer) and not bj.isclosedform(bj.inverse(layer))
    # the defect: 0 for an identity block, 3 for the same block scaled by 2, Float64 whatever the parameter's dtype
    eye = torch.eye(dim, dtype=torch.float32)[:, :M]
    one = lambda q: bj.SylvesterLayer(q, *args[1:], orthonormal=True)
    assert one(eye).orthonormality_defect() == 0.0
    assert one(2.0 * eye).orthonormality_defect() == 3.0
    assert isinstance(one(eye).orthonormality_defect(), float)
    qr = torch.linalg.qr(torch.randn(dim, M, dtype=torch.float64))[0]
    assert one(qr).orthonormality_defect() <= 1e-14 and 1e-9 <= one(qr.float()).orthonormality_defect() <= 1e-6
    assert bj.SylvesterLayer(torch.tensor([0.6, 0.8]), torch.randn(1), torch.randn(1), torch.randn(1), orthonormal=True).orthonormality_defect() <= 1e-7
    # wrong shapes are refused as before, whatever the keyword says
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.SylvesterLayer(torch.randn(dim, M, 3), *args[1:], orthonormal=True)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.SylvesterLayer(args[0], torch.randn(M, M + 1), *args[2:], orthonormal=True)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.SylvesterLayer(*args[:3], torch.randn(M + 1), orthonormal=True)
    with pytest.raises(ValueError, match="above dim 2"):
        bj.SylvesterLayer(torch.randn(2, 3), torch.randn(3, 3), torch.randn(3, 3), torch.randn(3), orthonormal=True)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._tables(torch.empty(0, dtype=torch.float32), dim + 1)
