"""Host side of the amortised Sylvester layer (include/bjx_sylvester_cols.h, `AmortizedSylvesterLayer`), no GPU: the companion header
is plain C99 and C++; its prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py argument by argument; a built library
exports both entries; the Float64 reference of tests/_sylvester_cols_ref.py is held to an independent evaluation — the forms written
unit by unit with plain loops, the dense central-difference Jacobian of the map and numpy's slogdet of it, and central differences of
⟨ȳ, y⟩ + ℓ̄·ladj in every parameter and input — at dim 1, 2, 3, 5, 8 and M 1, 2, 3 with M <= dim, with NaNs in the strict lower
triangles of R and R̃; the two fixed columns of every draw behave as stated; the host class passes a permuted network output and four
slices of one head with their column strides and no copy, copies anything else once, and refuses wrong shapes and sizes with a
ValueError and the inverse with a NotImplementedError."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _sylvester_cols_ref import RefAll, draws, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_sylvester_cols.h")
ENTRIES = ["bjx_sylvester_cols", "bjx_sylvester_cols_vjp"]
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_sylvester_cols.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, const void*, int64_t, int64_t, int64_t, int64_t, int, const void*, void*, void*,
           double*, int64_t, int64_t, uint32_t) = bjx_sylvester_cols;
  int (*g)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, const void*, int64_t, int64_t, int64_t, int64_t, int, const void*, const void*,
           const void*, void*, void*, void*, void*, void*, int64_t, int64_t) = bjx_sylvester_cols_vjp;
  return (f != NULL && g != NULL && BJX_SYLVESTER_COLS_MAX_UNITS == 16 && BJX_VERSION == 100) ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def bj():
    import bijectors_amd

    return bijectors_amd


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_as_c99_and_as_cxx(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    assert cc, "gcc and g++ are part of the image"
    std, ext = ("-std=c99", "c") if lang == "c" else ("-std=c++11", "cpp")
    src = tmp_path / f"sylvester_cols.{ext}"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, std, *WARN, "-c", str(src), "-o", str(tmp_path / "sylvester_cols.o")])      # both prototypes pinned, not linked
    only = tmp_path / f"only.{ext}"
    only.write_text('#include "bjx_sylvester_cols.h"\nint main(void) { return BJX_SYLVESTER_COLS_MAX_UNITS == 16 ? 0 : 1; }\n')
    subprocess.check_call([cc, std, *WARN, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_SYLVESTER_COLS
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
    assert bj._lib.BJX_SYLVESTER_COLS_MAX_UNITS == int(re.search(r"#define BJX_SYLVESTER_COLS_MAX_UNITS (\d+)", text).group(1))
    assert "sylvester" not in open(os.path.join(ROOT, "include", "bjx.h")).read()      # bjx.h itself is untouched by the companion header


def test_built_library_exports_both_entries(bj):
    assert set(ENTRIES) <= set(bj._lib.SIGNATURES_SYLVESTER_COLS)
    if not os.path.exists(bj._lib.LIB_PATH):
        return                                          # nothing built here: the GPU suite loads the library (load() checks every export)
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


# ------------------------------------------------------------------ the reference against an independent evaluation
def _forms(Q, R, Rt, b, z):
    """(y, ladj) of ONE column, unit by unit with plain loops: only R[i, j], R̃[i, j] with i <= j are touched."""
    dim, M = Q.shape
    s = [sum(Q[r, m] * z[r] for r in range(dim)) for m in range(M)]
    a = [np.tanh(sum(Rt[i, j] * s[j] for j in range(i, M)) + b[i]) for i in range(M)]
    p = [sum(R[i, j] * a[j] for j in range(i, M)) for i in range(M)]
    y = np.array([z[r] + sum(Q[r, m] * p[m] for m in range(M)) for r in range(dim)])
    ladj = sum(np.log(abs(1.0 + (1.0 - a[m] ** 2) * Rt[m, m] * R[m, m])) for m in range(M))
    return y, ladj


def _phi(Q, R, Rt, b, z, g, lb):
    y, ladj = _forms(Q, R, Rt, b, z)
    return float(g @ y + lb * ladj)


CASES = [(dim, M) for dim in (1, 2, 3, 5, 8) for M in (1, 2, 3) if M <= dim]


@pytest.mark.parametrize("dim,M", CASES)
def test_reference_matches_the_jacobian_and_central_differences(dim, M):
    """Values against the plain loops to 1e-13; log-det against slogdet of the central-difference Jacobian of the loops to 1e-7 (h = 1e-5:
    each entry carries ~h²·|y‴| + eps/h ~ 1e-10, and 1/min|d| <= 5 by the draws); every cotangent against central differences of
    ⟨ȳ, y⟩ + ℓ̄·ladj (Q perturbed as a free parameter: the log-det is then the FORM, not the Jacobian's) at 1e-6 of the column's term
    scale.  The strict lower triangles hold NaN in the reference's inputs and are left out of the differences: never read."""
    h, N = 1e-5, 3
    Q, R, Rt, b, z, g, lb = draws(seed("forms", dim, M), dim, M, N, np.float64)
    low = np.tril(np.ones((M, M)), -1) > 0
    Rn, Rtn = R.copy(), Rt.copy()
    Rn[low], Rtn[low] = np.nan, np.nan
    ref = RefAll(Q, Rn, Rtn, b, z, g, lb)
    for k in ("out", "ladj", "in_bar", "qb", "rb", "rtb", "bb", "scale"):
        assert np.isfinite(getattr(ref, k)).all(), k
    assert not ref.rb[low].any() and not ref.rtb[low].any()                # exact zeros below the diagonal
    for n in range(N):
        what = f"dim={dim} M={M} column {n}"
        P = [Q[:, :, n].copy(), R[:, :, n].copy(), Rt[:, :, n].copy(), b[:, n].copy(), z[:, n].copy()]
        y, ladj = _forms(*P)
        assert np.abs(ref.out[:, n] - y).max() <= 1e-13 * max(1.0, np.abs(y).max()), what
        assert abs(ref.ladj[n] - ladj) <= 1e-13 * max(1.0, abs(ladj)), what
        assert np.abs(Q[:, :, n].T @ Q[:, :, n] - np.eye(M)).max() <= 1e-14, what
        J = np.empty((dim, dim))
        for c in range(dim):
            e = np.zeros(dim)
            e[c] = h
            J[:, c] = (_forms(*P[:4], P[4] + e)[0] - _forms(*P[:4], P[4] - e)[0]) / (2 * h)
        assert abs(np.linalg.slogdet(J)[1] - ref.ladj[n]) <= 1e-7, f"{what}: log-det {ref.ladj[n]} vs slogdet {np.linalg.slogdet(J)[1]}"
        for name, k, want in (("q", 0, ref.qb[:, :, n]), ("r", 1, ref.rb[:, :, n]), ("r_tilde", 2, ref.rtb[:, :, n]), ("b", 3, ref.bb[:, n]),
                              ("z", 4, ref.in_bar[:, n])):
            for idx in np.ndindex(P[k].shape):
                if k in (1, 2) and idx[0] > idx[1]:
                    continue
                keep = P[k][idx]
                P[k][idx] = keep + h
                hi = _phi(*P, g[:, n], lb[n])
                P[k][idx] = keep - h
                lo = _phi(*P, g[:, n], lb[n])
                P[k][idx] = keep
                err = abs((hi - lo) / (2 * h) - want[idx]) / max(ref.scale[n], np.abs(ref.in_bar[:, n]).max())
                assert err <= 1e-6, f"{what} {name}{idx}: {err:.3g} of the column's term scale"


def test_the_two_fixed_columns_behave_as_stated():
    """Column 0 (R = 0): the identity, log-det exactly 0, Q̄ = z s̄ᵀ, R̃̄ = 0 = b̄ (nothing downstream of t reaches an output).
    Column 1: R_00·R̃_00 = −3 with d_0 < 0 and |d_0| >= 0.2; over the whole recipe min|d| stays away from 0."""
    dmin = np.inf
    for dim, M in [(1, 1), (2, 1), (5, 3), (9, 4), (16, 16), (65, 5), (1024, 16)]:
        N = 6
        Q, R, Rt, b, z, g, lb = draws(seed("fixed", dim, M), dim, M, N, np.float64)
        ref = RefAll(Q, R, Rt, b, z, g, lb)
        assert not R[:, :, 0].any() and np.array_equal(ref.out[:, 0], z[:, 0]) and ref.ladj[0] == 0.0
        assert np.array_equal(ref.in_bar[:, 0], g[:, 0]) and not ref.rtb[:, :, 0].any() and not ref.bb[:, 0].any()
        s = Q[:, :, 0].T @ z[:, 0]
        assert np.array_equal(ref.qb[:, :, 0], np.zeros((dim, M)))           # s̄ = R̃ᵀt̄ with t̄ = 0, p = 0
        a = np.tanh(np.triu(Rt[:, :, 0]) @ s + b[:, 0])
        want = np.triu(np.outer(Q[:, :, 0].T @ g[:, 0], a)) + np.diag(lb[0] * (1.0 - a * a) * np.diag(Rt[:, :, 0]))      # d = 1 at R = 0
        assert np.allclose(ref.rb[:, :, 0], want, rtol=0, atol=1e-13)
        assert R[0, 0, 1] * Rt[0, 0, 1] == -3.0
        assert ref.d[0, 1] < 0 and abs(ref.d[0, 1]) >= 0.2, (dim, M, ref.d[0, 1])
        dmin = min(dmin, np.abs(ref.d).min())
    assert dmin >= 0.2, dmin


# ------------------------------------------------------------------ the host class
def test_host_class_passes_laid_out_tensors_without_a_copy(bj):
    torch = pytest.importorskip("torch")
    dim, M, N = 6, 3, 10
    like = torch.empty(0, dtype=torch.float32)
    # network outputs (batch, M, dim), (batch, M, M), (batch, M) seen column-major per column
    nq, nr, nrt, nb = torch.randn(N, M, dim), torch.randn(N, M, M), torch.randn(N, M, M), torch.randn(N, M)
    layer = bj.AmortizedSylvesterLayer(nq.permute(2, 1, 0), nr.permute(2, 1, 0), nrt.permute(2, 1, 0), nb.T)
    pq, pr, prt, pb, lq, lr, lrt, lb = layer._col_params(like, dim, N)
    assert (pq.data_ptr(), pr.data_ptr(), prt.data_ptr(), pb.data_ptr()) == (nq.data_ptr(), nr.data_ptr(), nrt.data_ptr(), nb.data_ptr())
    assert (lq, lr, lrt, lb) == (dim * M, M * M, M * M, M)
    # one head [dim·M + 2M² + M (+ padding), batch] sliced four ways: the column stride is the head's
    rows = dim * M + 2 * M * M + M + 5
    head = torch.randn(N, rows)
    o1, o2, o3 = dim * M, dim * M + M * M, dim * M + 2 * M * M
    hq = head[:, :o1].view(N, M, dim).permute(2, 1, 0)
    hr = head[:, o1:o2].view(N, M, M).permute(2, 1, 0)
    hrt = head[:, o2:o3].view(N, M, M).permute(2, 1, 0)
    hb = head[:, o3:o3 + M].T
    layer = bj.AmortizedSylvesterLayer(hq, hr, hrt, hb)
    pq, pr, prt, pb, lq, lr, lrt, lb = layer._col_params(like, dim, N)
    es, p0 = head.element_size(), head.data_ptr()
    assert (pq.data_ptr(), pr.data_ptr(), prt.data_ptr(), pb.data_ptr()) == (p0, p0 + o1 * es, p0 + o2 * es, p0 + o3 * es)
    assert (lq, lr, lrt, lb) == (rows, rows, rows, rows)
    # anything else is made so once: contiguous tensors have the batch fastest
    cq, cr, cb = torch.randn(dim, M, N), torch.randn(M, M, N), torch.randn(M, N)
    layer = bj.AmortizedSylvesterLayer(cq, cr, cr.clone(), cb)
    pq, pr, prt, pb, lq, lr, lrt, lb = layer._col_params(like, dim, N)
    assert pq.data_ptr() != cq.data_ptr() and pq.stride() == (1, dim, dim * M) and torch.equal(pq, cq) and lq == dim * M
    assert pr.data_ptr() != cr.data_ptr() and pr.stride() == (1, M, M * M) and torch.equal(pr, cr) and (lr, lrt) == (M * M, M * M)
    assert pb.data_ptr() != cb.data_ptr() and pb.stride() == (1, M) and torch.equal(pb, cb) and lb == M
    # M = 1 given as (dim, batch) and three (batch,) vectors: slices of one head [dim + 3, batch] pass as they are
    head1 = torch.randn(N, dim + 3)
    layer = bj.AmortizedSylvesterLayer(head1[:, :dim].T, head1[:, dim], head1[:, dim + 1], head1[:, dim + 2])
    pq, pr, prt, pb, lq, lr, lrt, lb = layer._col_params(like, dim, N)
    assert layer.n_units == 1 and pq.shape == (dim, 1, N) and pr.shape == (1, 1, N) and pb.shape == (1, N)
    p0 = head1.data_ptr()
    assert (pq.data_ptr(), pr.data_ptr(), prt.data_ptr(), pb.data_ptr()) == (p0, p0 + dim * es, p0 + (dim + 1) * es, p0 + (dim + 2) * es)
    assert (lq, lr, lrt, lb) == (dim + 3,) * 4


def test_host_class_is_a_bijector_of_its_own_and_refuses_wrong_shapes_and_the_inverse(bj):
    torch = pytest.importorskip("torch")
    I = bj.interface
    dim, M, N = 4, 2, 8

    def make(dim=dim, M=M, N=N):
        return bj.AmortizedSylvesterLayer(torch.randn(dim, M, N), torch.randn(M, M, N), torch.randn(M, M, N), torch.randn(M, N))

    layer = make()
    assert "AmortizedSylvesterLayer" in bj.__all__ and isinstance(layer, bj.Bijector)
    # the planner keeps it as a stage of its own: a stack is l_K @ … @ l_1
    st, spans = (layer @ make() @ bj.Shift(1.0))._plan()
    assert [type(s).__name__ for s in st] == ["Shift", "AmortizedSylvesterLayer", "AmortizedSylvesterLayer"] and spans == [(0, 1), (1, 2), (2, 3)]
    assert bj.isinvertible(layer) and not bj.isclosedform(bj.inverse(layer))
    assert I._has_own_params(layer) and "AmortizedSylvesterLayer" in I._PARAM_STAGES
    like = torch.empty(0, dtype=torch.float32)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._col_params(like, dim + 1, N)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._col_params(like, dim, N + 1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedSylvesterLayer(torch.randn(dim), torch.randn(N), torch.randn(N), torch.randn(N))
    q = torch.randn(dim, M, N)
    for r, rt, b in ((torch.randn(M, M + 1, N), torch.randn(M, M, N), torch.randn(M, N)), (torch.randn(M, M, N), torch.randn(M, M, N + 1), torch.randn(M, N)),
                     (torch.randn(M, M, N), torch.randn(M, M, N), torch.randn(M + 1, N)), (torch.randn(N), torch.randn(M, M, N), torch.randn(M, N)),
                     (torch.randn(M, M, N), torch.randn(M, M, N), torch.randn(N))):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            bj.AmortizedSylvesterLayer(q, r, rt, b)
    for units in (0, 17):
        with pytest.raises(ValueError, match="16"):
            bj.AmortizedSylvesterLayer(torch.randn(32, units, N), torch.randn(units, units, N), torch.randn(units, units, N), torch.randn(units, N))
    with pytest.raises(ValueError, match="above dim 2"):
        make(dim=2, M=3)
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        big = bj.AmortizedSylvesterLayer(torch.randn(lim + 1, 1), torch.randn(1), torch.randn(1), torch.randn(1))
        with pytest.raises(ValueError, match=str(lim)):
            big._col_params(torch.empty(0, dtype=dt), lim + 1, 1)
        ok = bj.AmortizedSylvesterLayer(torch.randn(lim, 1), torch.randn(1), torch.randn(1), torch.randn(1))
        ok._col_params(torch.empty(0, dtype=dt), lim, 1)
    # the inverse is not built: applied to data it says so, and with it the log-density of a transformed distribution
    x = torch.randn(N, dim).T
    inv = bj.inverse(layer)
    for call in (lambda: bj.transform(inv, x), lambda: bj.with_logabsdet_jacobian(inv, x), lambda: bj.vjp(inv, x, x), lambda: bj.vjp_params(inv, x, x),
                 lambda: bj.logpdf(bj.transformed(bj.MvNormal(dim), layer), x)):       # (logpdf_vjp_params looks at the device first: the GPU suite)
        with pytest.raises(NotImplementedError, match="inverse map is not built"):
            call()
