"""Host side of the amortised planar flow (include/bjx_planar_cols.h, `AmortizedPlanarLayer`), no GPU: the companion header is
plain C99; its prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py argument by argument; a built library exports both
entries; the Float64 reference of tests/_planar_cols_ref.py (the oracle column by column) has per-column parameter cotangents that
agree with central differences of `orc.planar`; the host class passes a permuted network output and a slice of one head with their
column strides and no copy, copies anything else once, and refuses wrong shapes and sizes with a ValueError."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _planar_cols_ref import draws, joint_scale, ref_param_vjp, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_planar_cols.h")
ENTRIES = ["bjx_planar_cols", "bjx_planar_cols_vjp"]
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_planar_cols.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, int, const void*, const void*, const void*, int64_t, int64_t, int64_t, int, const void*, void*, void*, double*,
           int64_t, int64_t, uint32_t) = bjx_planar_cols;
  int (*g)(bjx_ctx*, bjx_dtype, int, const void*, const void*, const void*, int64_t, int64_t, int64_t, int, const void*, const void*, const void*,
           void*, void*, void*, void*, int64_t, int64_t) = bjx_planar_cols_vjp;
  return (f != NULL && g != NULL && BJX_PLANAR_COLS_MAX_LAYERS == 64 && BJX_VERSION == 100) ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def bj():
    import bijectors_amd

    return bijectors_amd


def test_header_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = tmp_path / "planar_cols.c"
    src.write_text(PROGRAM)
    subprocess.check_call([gcc, *CFLAGS, "-c", str(src), "-o", str(tmp_path / "planar_cols.o")])
    only = tmp_path / "only.c"
    only.write_text('#include "bjx_planar_cols.h"\nint main(void) { return BJX_PLANAR_COLS_MAX_LAYERS == 64 ? 0 : 1; }\n')
    subprocess.check_call([gcc, *CFLAGS, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_PLANAR_COLS
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
    assert bj._lib.BJX_PLANAR_COLS_MAX_LAYERS == int(re.search(r"#define BJX_PLANAR_COLS_MAX_LAYERS (\d+)", text).group(1))
    assert "planar_cols" not in open(os.path.join(ROOT, "include", "bjx.h")).read()      # bjx.h itself is untouched by the companion header


def test_built_library_exports_both_entries(bj):
    assert set(ENTRIES) <= set(bj._lib.SIGNATURES_PLANAR_COLS)
    if not os.path.exists(bj._lib.LIB_PATH):
        return                                          # nothing built here: the GPU suite loads the library (load() checks every export)
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


@pytest.mark.parametrize("dim", [3, 7])
@pytest.mark.parametrize("L", [1, 3])
def test_reference_parameter_cotangents_match_central_differences(orc, dim, L):
    """φ(w, u, b) = ⟨ȳ, f(x)⟩ + ℓ̄·logabsdetjac of one column through `orc.planar` in Float64; its central differences (h = 1e-5:
    truncation ~ h² and rounding ~ eps/h are both ~1e-10) against the reference's closed forms, to 1e-6 of the column's joint scale."""
    N = 4
    w, u, b, x, g, lb = draws(seed("fd", dim, L), dim, L, N, np.float64)
    wb, ub, bb = ref_param_vjp(orc, w, u, b, x, g, lb)
    scale = joint_scale(wb, ub, bb)
    h = 1e-5

    def phi(w_, u_, b_, n):
        y, l = orc.planar(w_, u_, b_, np.asfortranarray(x[:, n:n + 1]))
        return float(np.sum(g[:, n] * np.asarray(y)[:, 0]) + lb[n] * np.asarray(l)[0])

    for n in range(N):
        base = [w[:, :, n].copy(), u[:, :, n].copy(), b[:, n].copy()]
        for which, ref in ((0, wb[:, :, n]), (1, ub[:, :, n]), (2, bb[:, n])):
            fd = np.empty_like(ref)
            for idx in np.ndindex(ref.shape):
                hi, lo = [a.copy() for a in base], [a.copy() for a in base]
                hi[which][idx] += h
                lo[which][idx] -= h
                fd[idx] = (phi(*hi, n) - phi(*lo, n)) / (2 * h)
            err = np.abs(fd - ref).max() / scale[n]
            assert err <= 1e-6, f"dim={dim} L={L} column {n} parameter {'wub'[which]}: {err:.3g} of the column's scale"


def test_host_class_passes_laid_out_tensors_without_a_copy(bj):
    torch = pytest.importorskip("torch")
    dim, L, N = 6, 3, 10
    like = torch.empty(0, dtype=torch.float32)
    # a network output (batch, L, dim) seen as (dim, L, batch)
    net_w, net_u = torch.randn(N, L, dim), torch.randn(N, L, dim)
    net_b = torch.randn(N, L)
    layer = bj.AmortizedPlanarLayer(net_w.permute(2, 1, 0), net_u.permute(2, 1, 0), net_b.T)
    pw, pu, pb, lw, lu, lb = layer._col_params(like, dim, N)
    assert (pw.data_ptr(), pu.data_ptr(), pb.data_ptr()) == (net_w.data_ptr(), net_u.data_ptr(), net_b.data_ptr())
    assert (lw, lu, lb) == (dim * L, dim * L, L)
    # one head [2·dim·L + L (+ padding), batch] sliced three ways: the column stride is the head's
    rows = 2 * dim * L + L + 5
    head = torch.randn(N, rows)
    hw = head[:, :dim * L].view(N, L, dim).permute(2, 1, 0)
    hu = head[:, dim * L:2 * dim * L].view(N, L, dim).permute(2, 1, 0)
    hb = head[:, 2 * dim * L:2 * dim * L + L].T
    layer = bj.AmortizedPlanarLayer(hw, hu, hb)
    pw, pu, pb, lw, lu, lb = layer._col_params(like, dim, N)
    es = head.element_size()
    assert (pw.data_ptr(), pu.data_ptr(), pb.data_ptr()) == (head.data_ptr(), head.data_ptr() + dim * L * es, head.data_ptr() + 2 * dim * L * es)
    assert (lw, lu, lb) == (rows, rows, rows)
    # anything else is made so once: a contiguous (dim, L, batch) tensor has the batch fastest
    cw = torch.randn(dim, L, N)
    layer = bj.AmortizedPlanarLayer(cw, cw.clone(), torch.randn(L, N))
    pw, pu, pb, lw, lu, lb = layer._col_params(like, dim, N)
    assert pw.data_ptr() != cw.data_ptr() and pw.stride() == (1, dim, dim * L) and torch.equal(pw, cw) and (lw, lb) == (dim * L, L)
    assert pb.stride(0) == 1 and torch.equal(pb, layer.b)
    # one layer given as (dim, batch) / (batch,)
    w2 = torch.randn(N, dim).T
    b1 = torch.randn(N)
    layer = bj.AmortizedPlanarLayer(w2, w2.clone(), b1)
    pw, pu, pb, lw, lu, lb = layer._col_params(like, dim, N)
    assert layer.n_layers == 1 and pw.data_ptr() == w2.data_ptr() and pb.data_ptr() == b1.data_ptr() and (lw, lb) == (dim, 1)


def test_host_class_is_a_bijector_of_its_own_and_refuses_wrong_shapes(bj):
    torch = pytest.importorskip("torch")
    I = bj.interface
    dim, N = 4, 8
    layer = bj.AmortizedPlanarLayer(torch.randn(dim, 2, N), torch.randn(dim, 2, N), torch.randn(2, N))
    assert "AmortizedPlanarLayer" in bj.__all__ and isinstance(layer, bj.Bijector) and not isinstance(layer, bj.PlanarLayer)
    assert I._planar_kind(layer) == 0 and I._planar_kind(bj.inverse(layer)) == 0
    st, spans = (layer @ layer @ bj.Shift(1.0))._plan()
    assert [type(s).__name__ for s in st] == ["Shift", "AmortizedPlanarLayer", "AmortizedPlanarLayer"] and spans == [(0, 1), (1, 2), (2, 3)]
    assert not bj.isclosedform(bj.inverse(layer)) and bj.isinvertible(layer)
    like = torch.empty(0, dtype=torch.float32)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._col_params(like, dim + 1, N)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._col_params(like, dim, N + 1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedPlanarLayer(torch.randn(dim, 2, N), torch.randn(dim, 3, N), torch.randn(2, N))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedPlanarLayer(torch.randn(dim, 2, N), torch.randn(dim, 2, N), torch.randn(N))
    for nl in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.AmortizedPlanarLayer(torch.randn(dim, nl, N), torch.randn(dim, nl, N), torch.randn(nl, N))
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        big = bj.AmortizedPlanarLayer(torch.randn(lim + 1, 1), torch.randn(lim + 1, 1), torch.randn(1))
        with pytest.raises(ValueError, match=str(lim)):
            big._col_params(torch.empty(0, dtype=dt), lim + 1, 1)
        ok = bj.AmortizedPlanarLayer(torch.randn(lim, 1), torch.randn(lim, 1), torch.randn(1))
        ok._col_params(torch.empty(0, dtype=dt), lim, 1)
