"""Host side of the amortised Householder flow (include/bjx_householder_cols.h, `AmortizedHouseholderFlow`), no GPU: the companion
header is plain C99 and C++; its prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py argument by argument; a built
library exports both entries; the Float64 reference of tests/_householder_cols_ref.py is held to an independent evaluation — the
dense matrix A = H_{L−1}⋯H_0 diag(eˢ) built explicitly, numpy's slogdet, and central differences of ⟨ȳ, out⟩ + ℓ̄·ladj in every
parameter — at dim 1, 2, 3, 5, 8, L 1, 2, 3, all four head combinations and both directions; the degenerate column (v_0 == 0) is the
identity at that layer with v̄_0 exactly 0 and the rest of its stack unaffected; the host class passes a permuted network output and
three slices of one head with their column strides and no copy, copies anything else once, returns cotangents in the constructor's
shapes, and refuses wrong shapes and sizes with a ValueError."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _householder_cols_ref import HEADS, RefAll, draws, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_householder_cols.h")
ENTRIES = ["bjx_householder_cols", "bjx_householder_cols_vjp"]
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_householder_cols.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, int, const void*, const void*, const void*, int64_t, int64_t, int64_t, int, const void*, void*, void*, double*,
           int64_t, int64_t, uint32_t) = bjx_householder_cols;
  int (*g)(bjx_ctx*, bjx_dtype, int, const void*, const void*, const void*, int64_t, int64_t, int64_t, int, const void*, const void*, const void*,
           void*, void*, void*, void*, int64_t, int64_t) = bjx_householder_cols_vjp;
  return (f != NULL && g != NULL && BJX_HOUSEHOLDER_COLS_MAX_LAYERS == 64 && BJX_VERSION == 100) ? 0 : 1;
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
    src = tmp_path / f"householder_cols.{ext}"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, std, *WARN, "-c", str(src), "-o", str(tmp_path / "householder_cols.o")])      # both prototypes pinned, not linked
    only = tmp_path / f"only.{ext}"
    only.write_text('#include "bjx_householder_cols.h"\nint main(void) { return BJX_HOUSEHOLDER_COLS_MAX_LAYERS == 64 ? 0 : 1; }\n')
    subprocess.check_call([cc, std, *WARN, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_HOUSEHOLDER_COLS
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
    assert bj._lib.BJX_HOUSEHOLDER_COLS_MAX_LAYERS == int(re.search(r"#define BJX_HOUSEHOLDER_COLS_MAX_LAYERS (\d+)", text).group(1))
    assert "householder" not in open(os.path.join(ROOT, "include", "bjx.h")).read()      # bjx.h itself is untouched by the companion header


def test_built_library_exports_both_entries(bj):
    assert set(ENTRIES) <= set(bj._lib.SIGNATURES_HOUSEHOLDER_COLS)
    if not os.path.exists(bj._lib.LIB_PATH):
        return                                          # nothing built here: the GPU suite loads the library (load() checks every export)
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


# ------------------------------------------------------------------ the reference against an independent evaluation
def _dense(v, s, n):
    """A = H_{L−1}⋯H_0 diag(eˢ) of column n as an explicit (dim, dim) matrix (H = I − 2vvᵀ/vᵀv; the identity at v == 0)."""
    dim, L, _ = v.shape
    A = np.eye(dim) if s is None else np.diag(np.exp(s[:, n]))
    for k in range(L):
        vk = v[:, k, n]
        ss = vk @ vk
        H = np.eye(dim) if ss == 0 else np.eye(dim) - 2.0 * np.outer(vk, vk) / ss
        A = H @ A
    return A


def _phi(v, s, m, xn, gn, lbn, n, inverse):
    """⟨ȳ, out⟩ + ℓ̄·ladj of column n through the dense matrix and slogdet alone."""
    A = _dense(v, s, n)
    mn = 0.0 if m is None else m[:, n]
    if not inverse:
        out, ladj = A @ xn + mn, np.linalg.slogdet(A)[1]
    else:
        out, ladj = np.linalg.solve(A, xn - mn), -np.linalg.slogdet(A)[1]
    return float(gn @ out + lbn * ladj)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("head", HEADS)
def test_reference_matches_dense_matrices_and_central_differences(head, inverse):
    """out = A x + m (inverse: A⁻¹(y − m)), in_bar = Aᵀȳ (A⁻ᵀx̄) and ladj = ±log|det A| to 1e-12; every parameter cotangent against central
    differences (h = 1e-5: truncation ~ h² and rounding ~ eps/h are both ~1e-10) of the dense evaluation at 1e-6 of the column's term
    scale.  Column 0 is the degenerate one: its first layer is left out of the differences (t jumps from 0 to 2/‖v‖² there, the flow is
    not differentiable in v_0 at 0) and held to exactly 0 instead."""
    h = 1e-5
    for dim in (1, 2, 3, 5, 8):
        for L in (1, 2, 3):
            N = 3
            v, s, m, x, g, lb = draws(seed("dense", dim, L, head, inverse), dim, L, N, np.float64, head)
            R = RefAll(v, s, m, x, g, lb, inverse)
            assert (R.sb is None) == (s is None) and (R.mb is None) == (m is None)
            for n in range(N):
                A = _dense(v, s, n)
                mn = 0.0 if m is None else m[:, n]
                what = f"dim={dim} L={L} head={head} inverse={inverse} column {n}"
                if not inverse:
                    out, inb, ladj = A @ x[:, n] + mn, A.T @ g[:, n], np.linalg.slogdet(A)[1]
                else:
                    out, inb, ladj = np.linalg.solve(A, x[:, n] - mn), np.linalg.solve(A.T, g[:, n]), -np.linalg.slogdet(A)[1]
                assert np.abs(R.out[:, n] - out).max() <= 1e-12 * max(1.0, np.abs(out).max()), what
                assert np.abs(R.in_bar[:, n] - inb).max() <= 1e-12 * max(1.0, np.abs(inb).max()), what
                assert abs(R.ladj[n] - ladj) <= 1e-12 * max(1.0, abs(ladj)), what
                if s is None:
                    assert R.ladj[n] == 0.0
                params = [("v", v, R.vb)] + ([("log_scale", s, R.sb)] if s is not None else []) + ([("shift", m, R.mb)] if m is not None else [])
                for name, p, ref in params:
                    for idx in np.ndindex(p[..., n].shape):
                        if name == "v" and n == 0 and idx[1] == 0:
                            assert ref[..., n][idx] == 0.0, what
                            continue
                        keep = p[..., n][idx]
                        p[..., n][idx] = keep + h
                        hi = _phi(v, s, m, x[:, n], g[:, n], lb[n], n, inverse)
                        p[..., n][idx] = keep - h
                        lo = _phi(v, s, m, x[:, n], g[:, n], lb[n], n, inverse)
                        p[..., n][idx] = keep
                        err = abs((hi - lo) / (2 * h) - ref[..., n][idx]) / R.scale[n]
                        assert err <= 1e-6, f"{what} {name}{idx}: {err:.3g} of the column's term scale"


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_degenerate_layer_is_the_identity_and_leaves_the_rest_alone(inverse):
    """Column 0 has v_0 == 0: with that layer REMOVED from the stack the values, the log-det, the input cotangent and the cotangents of
    every other parameter are the same numbers (bit for bit: the layer adds 0·v), and v̄_0 is exactly 0."""
    dim, L, N = 5, 3, 4
    v, s, m, x, g, lb = draws(seed("degenerate", inverse), dim, L, N, np.float64)
    assert (v[:, 0, 0] == 0).all() and (v[:, 0, 1:] != 0).any()
    R = RefAll(v, s, m, x, g, lb, inverse)
    S = RefAll(v[:, 1:, :1], s[:, :1], m[:, :1], x[:, :1], g[:, :1], lb[:1], inverse)
    assert (R.vb[:, 0, 0] == 0).all()
    for k in ("out", "ladj", "in_bar", "sb", "mb"):
        assert np.array_equal(getattr(R, k)[..., :1], getattr(S, k)), k
    assert np.array_equal(R.vb[:, 1:, :1], S.vb)
    assert (R.vb[:, 0, 1:] != 0).any()


# ------------------------------------------------------------------ the host class
def test_host_class_passes_laid_out_tensors_without_a_copy(bj):
    torch = pytest.importorskip("torch")
    dim, L, N = 6, 3, 10
    like = torch.empty(0, dtype=torch.float32)
    # a network output (batch, L, dim) seen as (dim, L, batch); (batch, dim) seen as (dim, batch)
    net_v, net_s, net_m = torch.randn(N, L, dim), torch.randn(N, dim), torch.randn(N, dim)
    flow = bj.AmortizedHouseholderFlow(net_v.permute(2, 1, 0), net_s.T, net_m.T)
    pv, ps, pm, lv, ls, lm = flow._col_params(like, dim, N)
    assert (pv.data_ptr(), ps.data_ptr(), pm.data_ptr()) == (net_v.data_ptr(), net_s.data_ptr(), net_m.data_ptr())
    assert (lv, ls, lm) == (dim * L, dim, dim)
    # one head [dim·L + 2·dim (+ padding), batch] sliced three ways: the column stride is the head's
    rows = dim * L + 2 * dim + 5
    head = torch.randn(N, rows)
    hv = head[:, :dim * L].view(N, L, dim).permute(2, 1, 0)
    hs = head[:, dim * L:dim * L + dim].T
    hm = head[:, dim * L + dim:dim * L + 2 * dim].T
    flow = bj.AmortizedHouseholderFlow(hv, hs, hm)
    pv, ps, pm, lv, ls, lm = flow._col_params(like, dim, N)
    es = head.element_size()
    assert (pv.data_ptr(), ps.data_ptr(), pm.data_ptr()) == (head.data_ptr(), head.data_ptr() + dim * L * es, head.data_ptr() + (dim * L + dim) * es)
    assert (lv, ls, lm) == (rows, rows, rows)
    # absent parameters: None and a stride of 0
    flow = bj.AmortizedHouseholderFlow(hv, shift=hm)
    pv, ps, pm, lv, ls, lm = flow._col_params(like, dim, N)
    assert ps is None and ls == 0 and pm.data_ptr() == hm.data_ptr() and lm == rows
    flow = bj.AmortizedHouseholderFlow(hv)
    assert flow._col_params(like, dim, N)[1:3] == [None, None]
    # anything else is made so once: a contiguous (dim, L, batch) tensor has the batch fastest
    cv, cs = torch.randn(dim, L, N), torch.randn(dim, N)
    flow = bj.AmortizedHouseholderFlow(cv, cs, cs.clone())
    pv, ps, pm, lv, ls, lm = flow._col_params(like, dim, N)
    assert pv.data_ptr() != cv.data_ptr() and pv.stride() == (1, dim, dim * L) and torch.equal(pv, cv) and lv == dim * L
    assert ps.data_ptr() != cs.data_ptr() and ps.stride() == (1, dim) and torch.equal(ps, cs) and (ls, lm) == (dim, dim)
    # one layer given as (dim, batch)
    v2 = torch.randn(N, dim).T
    flow = bj.AmortizedHouseholderFlow(v2)
    pv, ps, pm, lv, ls, lm = flow._col_params(like, dim, N)
    assert flow.n_layers == 1 and pv.data_ptr() == v2.data_ptr() and pv.shape == (dim, 1, N) and lv == dim


def test_host_class_is_a_bijector_of_its_own_and_refuses_wrong_shapes(bj):
    torch = pytest.importorskip("torch")
    I = bj.interface
    dim, N = 4, 8
    flow = bj.AmortizedHouseholderFlow(torch.randn(dim, 2, N), torch.randn(dim, N), torch.randn(dim, N))
    assert "AmortizedHouseholderFlow" in bj.__all__ and isinstance(flow, bj.Bijector)
    # the planner keeps it as a stage of its own
    st, spans = (flow @ flow @ bj.Shift(1.0))._plan()
    assert [type(s).__name__ for s in st] == ["Shift", "AmortizedHouseholderFlow", "AmortizedHouseholderFlow"] and spans == [(0, 1), (1, 2), (2, 3)]
    rad = bj.RadialLayer(torch.randn(1), torch.randn(1), torch.randn(dim))
    st, _ = (rad @ flow @ rad)._plan()
    assert [type(s).__name__ for s in st] == ["RadialLayer", "AmortizedHouseholderFlow", "RadialLayer"]
    assert bj.isclosedform(bj.inverse(flow)) and bj.isinvertible(flow)
    assert I._has_own_params(flow) and I._has_own_params(bj.inverse(flow)) and "AmortizedHouseholderFlow" in I._PARAM_STAGES
    like = torch.empty(0, dtype=torch.float32)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        flow._col_params(like, dim + 1, N)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        flow._col_params(like, dim, N + 1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedHouseholderFlow(torch.randn(dim))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedHouseholderFlow(torch.randn(dim, 2, N), torch.randn(dim + 1, N))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedHouseholderFlow(torch.randn(dim, 2, N), None, torch.randn(dim, N + 1))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedHouseholderFlow(torch.randn(dim, 2, N), torch.randn(dim, 2, N))
    for nl in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.AmortizedHouseholderFlow(torch.randn(dim, nl, N))
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        big = bj.AmortizedHouseholderFlow(torch.randn(lim + 1, 1))
        with pytest.raises(ValueError, match=str(lim)):
            big._col_params(torch.empty(0, dtype=dt), lim + 1, 1)
        ok = bj.AmortizedHouseholderFlow(torch.randn(lim, 1))
        ok._col_params(torch.empty(0, dtype=dt), lim, 1)
