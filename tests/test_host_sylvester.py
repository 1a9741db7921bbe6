"""Host side of the shared Sylvester layer (include/bjx_sylvester.h, `SylvesterLayer`), no GPU: the companion header is plain C99 and
C++; its prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py argument by argument and its LDS rule is the host's; the
cross-compiled library exports both entries; the Float64 reference of tests/_sylvester_ref.py is the batch sum of the per-column
sibling's reference on expanded parameters and agrees with central differences of Σ_n(⟨ȳ_n, y_n⟩ + ℓ̄_n·ladj_n) in every shared
parameter and every input at dim 1 … 8, M 1 … 3, with NaN below both diagonals and with the negative-determinant recipe; no draw of
this file or of the GPU test comes nearer to d = 0 than 0.2; the host class is public, a parameter stage, refuses wrong shapes and
sizes and does not build the inverse."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _sylvester_cols_ref import RefAll
from _sylvester_ref import Draw, RefShared, draws, gpu_draws, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_sylvester.h")
ENTRIES = ["bjx_sylvester", "bjx_sylvester_vjp_params"]
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_sylvester.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, const void*, int, const void*, void*, void*, double*, int64_t, int64_t,
           uint32_t) = bjx_sylvester;
  int (*g)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, const void*, int, const void*, const void*, const void*, void*, void*, void*,
           void*, void*, int64_t, int64_t) = bjx_sylvester_vjp_params;
  return (f != NULL && g != NULL && BJX_SYLVESTER_MAX_UNITS == 16 && BJX_SYLVESTER_LDS_BYTES(64, 16) <= BJX_SYLVESTER_LDS_BUDGET &&
          BJX_SYLVESTER_LDS_BYTES(128, 14) > BJX_SYLVESTER_LDS_BUDGET && BJX_VERSION == 100) ? 0 : 1;
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
    src = tmp_path / f"sylvester.{ext}"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, std, *WARN, "-c", str(src), "-o", str(tmp_path / "sylvester.o")])      # both prototypes pinned, not linked
    only = tmp_path / f"only.{ext}"
    only.write_text('#include "bjx_sylvester.h"\nint main(void) { return BJX_SYLVESTER_LDS_BYTES(1024, 1) <= BJX_SYLVESTER_LDS_BUDGET ? 0 : 1; }\n')
    subprocess.check_call([cc, std, *WARN, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])
    assert "sylvester.h" not in open(os.path.join(ROOT, "include", "bjx.h")).read()        # bjx.h does not mention the companion header


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_SYLVESTER
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
    assert bj._lib.BJX_SYLVESTER_MAX_UNITS == int(re.search(r"#define BJX_SYLVESTER_MAX_UNITS (\d+)", text).group(1))
    assert bj._lib.BJX_SYLVESTER_LDS_BUDGET == int(re.search(r"#define BJX_SYLVESTER_LDS_BUDGET (\d+)", text).group(1))


def test_lds_rule_of_the_host_is_the_headers(bj, tmp_path):
    """`_lib.sylvester_lds_bytes` against the header's macro evaluated by the C compiler over a grid of (dim, M); the largest M that fits
    at dim 64, 128, 256, 512 and 1 024 is 16, 13, 7, 3 and 1."""
    cases = [(d, m) for d in (1, 2, 3, 16, 64, 65, 128, 129, 256, 257, 512, 1024) for m in range(1, 17) if m <= d]
    body = "".join(f'  printf("%lu\\n", (unsigned long)BJX_SYLVESTER_LDS_BYTES({d}, {m}));\n' for d, m in cases)
    src = tmp_path / "lds.c"
    src.write_text('#include "bjx_sylvester.h"\n#include <stdio.h>\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call([shutil.which("gcc"), "-std=c99", *WARN, str(src), "-o", str(tmp_path / "lds")])
    got = [int(s) for s in subprocess.check_output([str(tmp_path / "lds")]).split()]
    assert got == [bj._lib.sylvester_lds_bytes(d, m) for d, m in cases]
    for dim, most in ((64, 16), (128, 13), (256, 7), (512, 3), (1024, 1)):
        fits = [m for m in range(1, 17) if bj._lib.sylvester_lds_bytes(dim, m) <= bj._lib.BJX_SYLVESTER_LDS_BUDGET]
        assert fits == list(range(1, most + 1)), (dim, fits)


def test_cross_compiled_library_exports_both_entries(bj):
    assert os.path.exists(bj._lib.LIB_PATH), f"{bj._lib.LIB_PATH} is not built"
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


# ------------------------------------------------------------------ the reference
def _expanded(Q, R, Rt, b, N):
    return np.repeat(Q[:, :, None], N, axis=2), np.repeat(R[:, :, None], N, axis=2), np.repeat(Rt[:, :, None], N, axis=2), np.repeat(b[:, None], N, axis=1)


def test_summed_reference_is_the_batch_sum_of_the_per_column_reference():
    """The parameters expanded to N columns through the per-column sibling's reference: values, ladj and x̄ are equal column by column,
    the summands are its per-column cotangents and `summed(N)` is their batch sum, to 1e-13 of the term scale."""
    for dim, M, N, negdet in ((1, 1, 5, False), (2, 2, 9, False), (5, 3, 33, False), (8, 3, 14, True), (16, 16, 20, False), (65, 5, 7, True)):
        Q, R, Rt, b, z, g, lb = draws(seed("shared-vs-cols", dim, M, negdet), dim, M, N, np.float64, negdet)
        S = RefShared(Q, R, Rt, b, z, g, lb)
        P = RefAll(*_expanded(Q, R, Rt, b, N), z, g, lb)
        what = f"dim={dim} M={M} N={N} negdet={negdet}"
        for k in ("out", "ladj", "in_bar"):
            got, ref = getattr(S, k), getattr(P, k)
            assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), (what, k)
        ts = S.term_scale(N)
        assert ts == P.scale.max() or abs(ts - P.scale.max()) <= 1e-13 * ts, what
        for cols, tot, ref in ((S.qb_cols, S.qb, P.qb), (S.rb_cols, S.rb, P.rb), (S.rtb_cols, S.rtb, P.rtb), (S.bb_cols, S.bb, P.bb)):
            assert np.abs(cols - ref).max() <= 1e-13 * ts, what
            assert np.abs(tot - ref.sum(axis=-1)).max() <= 1e-13 * ts, what
        for got, ref in zip(S.summed(N), (P.qb, P.rb, P.rtb, P.bb)):
            assert np.abs(got - ref.sum(axis=-1)).max() <= 1e-13 * ts, what
        n = N // 2
        for got, ref in zip(S.summed(n), (P.qb, P.rb, P.rtb, P.bb)):
            assert np.abs(got - ref[..., :n].sum(axis=-1)).max() <= 1e-13 * ts, what
        assert S.term_scale(n) == P.scale[:n].max() or abs(S.term_scale(n) - P.scale[:n].max()) <= 1e-13 * ts, what


def _forms(Q, R, Rt, b, z):
    """The layer on all columns in plain loops over the upper triangles alone."""
    dim, M = Q.shape
    N = z.shape[1]
    y, ladj = np.empty((dim, N)), np.empty(N)
    for n in range(N):
        s = [sum(Q[r, m] * z[r, n] for r in range(dim)) for m in range(M)]
        a = [np.tanh(sum(Rt[i, j] * s[j] for j in range(i, M)) + b[i]) for i in range(M)]
        p = [sum(R[i, j] * a[j] for j in range(i, M)) for i in range(M)]
        y[:, n] = [z[r, n] + sum(Q[r, m] * p[m] for m in range(M)) for r in range(dim)]
        ladj[n] = sum(np.log(abs(1.0 + (1.0 - a[m] ** 2) * Rt[m, m] * R[m, m])) for m in range(M))
    return y, ladj


def _phi(Q, R, Rt, b, z, g, lb):
    y, ladj = _forms(Q, R, Rt, b, z)
    return float((g * y).sum() + lb @ ladj)


CASES = [(dim, M, negdet) for dim in range(1, 9) for M in (1, 2, 3) if M <= dim for negdet in (False, True)]


@pytest.mark.parametrize("dim,M,negdet", CASES)
def test_reference_matches_central_differences_in_every_parameter_and_input(dim, M, negdet):
    """Σ_n(⟨ȳ_n, y_n⟩ + ℓ̄_n·ladj_n) through plain loops, differenced (h = 1e-5: truncation ~h² and rounding ~eps/h are both ~1e-10 per
    column, and 1/min|d| <= 5 by the draws) in every shared parameter (Q as a free parameter: the log-det is then the FORM) and every
    input, at 1e-6 of the term scale.  The strict lower triangles hold NaN in the reference's inputs and are left out of the differences."""
    h, N = 1e-5, 8
    Q, R, Rt, b, z, g, lb = draws(seed("shared-forms", dim, M, negdet), dim, M, N, np.float64, negdet)
    low = np.tril(np.ones((M, M)), -1) > 0
    Rn, Rtn = R.copy(), Rt.copy()
    Rn[low], Rtn[low] = np.nan, np.nan
    ref = RefShared(Q, Rn, Rtn, b, z, g, lb)
    what = f"dim={dim} M={M} negdet={negdet}"
    for k in ("out", "ladj", "in_bar", "qb", "rb", "rtb", "bb", "scale_cols"):
        assert np.isfinite(getattr(ref, k)).all(), (what, k)
    assert not ref.rb[low].any() and not ref.rtb[low].any() and not ref.rb_cols[low].any() and not ref.rtb_cols[low].any()
    assert np.abs(ref.d).min() >= 0.2, (what, np.abs(ref.d).min())
    if negdet:
        assert (ref.d[0] <= -1.5).any() and (ref.d[0] >= 0.7).any() and ((ref.d[0] <= -1.5) | (ref.d[0] >= 0.7)).all(), (what, ref.d[0])
    y, ladj = _forms(Q, R, Rt, b, z)
    assert np.abs(ref.out - y).max() <= 1e-13 * max(1.0, np.abs(y).max()) and np.abs(ref.ladj - ladj).max() <= 1e-13 * max(1.0, np.abs(ladj).max()), what
    ts = ref.term_scale(N)
    P = [Q.copy(), R.copy(), Rt.copy(), b.copy(), z.copy()]
    for name, k, want, scale in (("q", 0, ref.qb, ts), ("r", 1, ref.rb, ts), ("r_tilde", 2, ref.rtb, ts), ("b", 3, ref.bb, ts),
                                 ("z", 4, ref.in_bar, max(ts, np.abs(ref.in_bar).max()))):
        for idx in np.ndindex(P[k].shape):
            if k in (1, 2) and idx[0] > idx[1]:
                continue
            keep = P[k][idx]
            P[k][idx] = keep + h
            hi = _phi(*P, g, lb)
            P[k][idx] = keep - h
            lo = _phi(*P, g, lb)
            P[k][idx] = keep
            err = abs((hi - lo) / (2 * h) - want[idx]) / scale
            assert err <= 1e-6, f"{what} {name}{idx}: {err:.3g} of the term scale"


def test_no_draw_of_the_host_or_the_gpu_test_comes_near_a_zero_determinant():
    """min|d| >= 0.2 over every draw of tests/test_gpu_zz_sylvester_shared.py (`gpu_draws`); the negative-determinant draws hold columns of
    both signs of d_0."""
    dmin = np.inf
    for dt, dim, M, N, key, negdet in gpu_draws():
        D = Draw(dt, dim, M, N, key, negdet)
        here = np.abs(D.ref.d).min()
        assert here >= 0.2, (np.dtype(dt).name, dim, M, N, key, here)
        if negdet:
            assert (D.ref.d[0] <= -1.5).any() and (D.ref.d[0] >= 0.7).any(), key
        dmin = min(dmin, here)
    assert dmin >= 0.2


# ------------------------------------------------------------------ the host class
def test_host_class_is_public_a_parameter_stage_and_refuses_wrong_shapes_and_the_inverse(bj):
    torch = pytest.importorskip("torch")
    I = bj.interface
    dim, M = 4, 2

    def make(dim=dim, M=M):
        return bj.SylvesterLayer(torch.randn(dim, M), torch.randn(M, M), torch.randn(M, M), torch.randn(M))

    layer = make()
    assert "SylvesterLayer" in bj.__all__ and isinstance(layer, bj.Bijector)
    assert (layer.dim, layer.n_units) == (dim, M)
    assert bj.isinvertible(layer) and not bj.isclosedform(bj.inverse(layer))
    assert I._has_own_params(layer) and I._has_own_params(bj.inverse(layer)) and "SylvesterLayer" in I._PARAM_STAGES
    assert layer._key() == layer._key() and len(layer._key()) == 4
    # a stage of its own between other stages; two of them are not merged
    planar = bj.PlanarLayer(torch.randn(dim), torch.randn(dim), torch.randn(1))
    st, spans = (bj.Shift(1.0) @ layer @ planar)._plan()
    assert [type(s).__name__ for s in st][1:] == ["SylvesterLayer", "Shift"] and spans[1:] == [(1, 2), (2, 3)]
    st, _ = (layer @ make())._plan()
    assert [type(s).__name__ for s in st] == ["SylvesterLayer", "SylvesterLayer"]
    # the M = 1 shorthand
    for r in (torch.randn(()), torch.randn(1), torch.randn(1, 1)):
        one = bj.SylvesterLayer(torch.randn(dim), r, r.clone(), r.clone().reshape(-1)[0] if r.dim() == 0 else r.reshape(-1))
        assert (one.dim, one.n_units) == (dim, 1)
        q, rr, rt, b = one._tables(torch.empty(0, dtype=torch.float32), dim)
        assert q.shape == (dim,) and rr.shape == (1, 1) and rt.shape == (1, 1) and b.shape == (1,)
    # dense column-major tables
    q, rr, rt, b = layer._tables(torch.empty(0, dtype=torch.float64), dim)
    assert q.shape == (dim, M) and q.stride() == (1, dim) and rr.stride() == (1, M) and rt.stride() == (1, M) and b.is_contiguous() and q.dtype == torch.float64
    assert torch.equal(q, layer.q.double()) and torch.equal(rr, layer.r.double())
    # wrong shapes
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.SylvesterLayer(torch.randn(dim, M, 3), torch.randn(M, M), torch.randn(M, M), torch.randn(M))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.SylvesterLayer(torch.tensor(1.0), torch.randn(1), torch.randn(1), torch.randn(1))
    q = torch.randn(dim, M)
    for r, rt, b in ((torch.randn(M, M + 1), torch.randn(M, M), torch.randn(M)), (torch.randn(M, M), torch.randn(M + 1, M), torch.randn(M)),
                     (torch.randn(M, M), torch.randn(M, M), torch.randn(M + 1)), (torch.randn(M), torch.randn(M, M), torch.randn(M)),
                     (torch.randn(M, M), torch.randn(M, M), torch.randn(M, 1))):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            bj.SylvesterLayer(q, r, rt, b)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.SylvesterLayer(torch.randn(dim), torch.randn(2), torch.randn(1), torch.randn(1))
    for units in (0, 17):
        with pytest.raises(ValueError, match="16"):
            bj.SylvesterLayer(torch.randn(32, units), torch.randn(units, units), torch.randn(units, units), torch.randn(units))
    with pytest.raises(ValueError, match="above dim 2"):
        make(dim=2, M=3)
    like = torch.empty(0, dtype=torch.float32)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._tables(like, dim + 1)
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        big = bj.SylvesterLayer(torch.randn(lim + 1), torch.randn(1), torch.randn(1), torch.randn(1))
        with pytest.raises(ValueError, match=str(lim)):
            big._tables(torch.empty(0, dtype=dt), lim + 1)
        bj.SylvesterLayer(torch.randn(lim), torch.randn(1), torch.randn(1), torch.randn(1))._tables(torch.empty(0, dtype=dt), lim)
    # the inverse is not built: applied to data it says so, and with it the log-density of a transformed distribution
    x = torch.randn(8, dim).T
    inv = bj.inverse(layer)
    for call in (lambda: bj.transform(inv, x), lambda: bj.with_logabsdet_jacobian(inv, x), lambda: bj.vjp(inv, x, x), lambda: bj.vjp_params(inv, x, x),
                 lambda: bj.logpdf(bj.transformed(bj.MvNormal(dim), layer), x)):
        with pytest.raises(NotImplementedError, match="inverse map is not built"):
            call()
