"""Host side of the amortised radial flow (include/bjx_radial_cols.h, `AmortizedRadialLayer`), no GPU: the companion header is
plain C99 and C++; its prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py argument by argument; a built library
exports both entries; the Float64 reference of tests/_radial_cols_ref.py (the oracle column by column) has per-column parameter
cotangents that agree with central differences of `orc.radial` alone, in both directions, and that sum to the batch-summed reference
of a run (tests/_radial_params_ref.py) when every column has the same parameters; the host class passes a permuted network output
and three slices of one head with their column strides and no copy, copies anything else once, and refuses wrong shapes and sizes
with a ValueError."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _radial_cols_ref import RefAll, VecAll, draws, seed
from _radial_params_ref import ref_run_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_radial_cols.h")
ENTRIES = ["bjx_radial_cols", "bjx_radial_cols_vjp"]
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_radial_cols.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, int, const void*, const void*, const void*, int64_t, int64_t, int64_t, int, const void*, void*, void*, double*,
           int64_t, int64_t, uint32_t) = bjx_radial_cols;
  int (*g)(bjx_ctx*, bjx_dtype, int, const void*, const void*, const void*, int64_t, int64_t, int64_t, int, const void*, const void*, const void*,
           void*, void*, void*, void*, int64_t, int64_t) = bjx_radial_cols_vjp;
  return (f != NULL && g != NULL && BJX_RADIAL_COLS_MAX_LAYERS == 64 && BJX_VERSION == 100) ? 0 : 1;
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
    src = tmp_path / f"radial_cols.{ext}"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, std, *WARN, "-c", str(src), "-o", str(tmp_path / "radial_cols.o")])      # both prototypes pinned, not linked
    only = tmp_path / f"only.{ext}"
    only.write_text('#include "bjx_radial_cols.h"\nint main(void) { return BJX_RADIAL_COLS_MAX_LAYERS == 64 ? 0 : 1; }\n')
    subprocess.check_call([cc, std, *WARN, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_RADIAL_COLS
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
    assert bj._lib.BJX_RADIAL_COLS_MAX_LAYERS == int(re.search(r"#define BJX_RADIAL_COLS_MAX_LAYERS (\d+)", text).group(1))
    assert "radial_cols" not in open(os.path.join(ROOT, "include", "bjx.h")).read()      # bjx.h itself is untouched by the companion header


def test_built_library_exports_both_entries(bj):
    assert set(ENTRIES) <= set(bj._lib.SIGNATURES_RADIAL_COLS)
    if not os.path.exists(bj._lib.LIB_PATH):
        return                                          # nothing built here: the GPU suite loads the library (load() checks every export)
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_reference_parameter_cotangents_match_central_differences(orc, inverse):
    """φ(α_, β, z₀) = ⟨ȳ, f(x)⟩ + ℓ̄·logabsdetjac of one column through `orc.radial` ALONE (layer by layer, no closed-form derivative),
    Float64, dim 3, L 2; its central differences (h = 1e-5: truncation ~ h² and rounding ~ eps/h are both ~1e-10) in every parameter
    of two columns against the reference's closed forms, to 1e-6 of the column's joint scale.  Columns 1 and 2: column 0 sits on the
    kink r = 0 of the first layer, where the central difference is not the derivative."""
    dim, L, N = 3, 2, 3
    al, be, z0, x, g, lb = draws(seed("fd", inverse), dim, L, N, np.float64)
    R = RefAll(orc, al, be, z0, x, g, lb, inverse)
    h = 1e-5

    def phi(al_, be_, z0_, n):
        cur, ladj = np.asfortranarray(x[:, n:n + 1]), 0.0
        for k in (range(L - 1, -1, -1) if inverse else range(L)):
            cur, l = orc.radial(al_[k], be_[k], np.ascontiguousarray(z0_[:, k]), cur, inverse)
            cur = np.asfortranarray(cur)
            ladj += float(l[0])
        return float(np.sum(g[:, n] * cur[:, 0]) + lb[n] * ladj)

    for n in (1, 2):
        base = [al[:, n].copy(), be[:, n].copy(), z0[:, :, n].copy()]
        for which, ref in ((0, R.ab[:, n]), (1, R.bb[:, n]), (2, R.zb[:, :, n])):
            fd = np.empty_like(ref)
            for idx in np.ndindex(ref.shape):
                hi, lo = [a.copy() for a in base], [a.copy() for a in base]
                hi[which][idx] += h
                lo[which][idx] -= h
                fd[idx] = (phi(*hi, n) - phi(*lo, n)) / (2 * h)
            err = np.abs(fd - ref).max() / R.scale[n]
            assert err <= 1e-6, f"inverse={inverse} column {n} parameter {('alpha_', 'beta', 'z_0')[which]}: {err:.3g} of the column's scale"


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_same_parameters_in_every_column_sum_to_the_run_reference(orc, inverse):
    """With one (α_, β, z₀) repeated in every column the per-column cotangents, summed over the batch, are the batch-summed cotangents of a
    run of RadialLayers (`_radial_params_ref.ref_run_params`), and x̄ is its x̄: 1e-12 of the largest entry.  The vectorised restatement
    (`VecAll`, the reference of the grid-stride GPU test) is held to the column-by-column reference on the same draw."""
    dim, L, N = 4, 3, 12
    al, be, z0, x, g, lb = draws(seed("run", inverse), dim, L, N, np.float64)
    al, be, z0 = (np.repeat(a[..., 1:2], N, axis=-1) for a in (al, be, z0))
    R = RefAll(orc, al, be, z0, x, g, lb, inverse)
    xb, ab, bb, zb, _ = ref_run_params(orc, al[:, 0], be[:, 0], z0[:, :, 0], x, g, lb, inverse=inverse)
    for got, ref, what in ((R.in_bar, xb, "x̄"), (R.ab.sum(axis=-1), ab, "ᾱ_"), (R.bb.sum(axis=-1), bb, "β̄"), (R.zb.sum(axis=-1), zb, "z̄₀")):
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what
    V = VecAll(al, be, z0, x, g, lb, inverse)
    for k in ("out", "ladj", "in_bar", "ab", "bb", "zb"):
        assert np.abs(getattr(V, k) - getattr(R, k)).max() <= 1e-12 * max(1.0, np.abs(getattr(R, k)).max()), k


def test_forward_reference_carries_the_cotangent_radial_vjp_returns(orc):
    """The forward reference reads the carried cotangent off radial_param_vjp's z̄₀ = ȳ − radial_vjp(…); layer by layer with the direct
    `orc.radial_vjp` call instead it is the same x̄ to 1e-14 of each column's largest entry (dim 1 and 5, L 8)."""
    for dim in (1, 5):
        L, N = 8, 6
        al, be, z0, x, g, lb = draws(seed("carry", dim), dim, L, N, np.float64)
        R = RefAll(orc, al, be, z0, x, g, lb)
        for n in range(N):
            cur, states = np.asfortranarray(x[:, n:n + 1]), []
            for k in range(L):
                states.append(cur)
                cur = np.asfortranarray(orc.radial(al[k, n], be[k, n], np.ascontiguousarray(z0[:, k, n]), cur)[0])
            gn = g[:, n:n + 1]
            for k in range(L - 1, -1, -1):
                gn = orc.radial_vjp(al[k, n], be[k, n], np.ascontiguousarray(z0[:, k, n]), states[k], gn, lb[n:n + 1])
            assert np.abs(gn[:, 0] - R.in_bar[:, n]).max() <= 1e-14 * max(1.0, np.abs(gn).max()), (dim, n)


def test_host_class_passes_laid_out_tensors_without_a_copy(bj):
    torch = pytest.importorskip("torch")
    dim, L, N = 6, 3, 10
    like = torch.empty(0, dtype=torch.float32)
    # a network output (batch, L, dim) seen as (dim, L, batch)
    net_z, net_a, net_b = torch.randn(N, L, dim), torch.randn(N, L), torch.randn(N, L)
    layer = bj.AmortizedRadialLayer(net_a.T, net_b.T, net_z.permute(2, 1, 0))
    pa, pb, pz, la, lb, lz = layer._col_params(like, dim, N)
    assert (pa.data_ptr(), pb.data_ptr(), pz.data_ptr()) == (net_a.data_ptr(), net_b.data_ptr(), net_z.data_ptr())
    assert (la, lb, lz) == (L, L, dim * L)
    # one head [dim·L + 2L (+ padding), batch] sliced three ways: the column stride is the head's
    rows = dim * L + 2 * L + 5
    head = torch.randn(N, rows)
    hz = head[:, :dim * L].view(N, L, dim).permute(2, 1, 0)
    ha = head[:, dim * L:dim * L + L].T
    hb = head[:, dim * L + L:dim * L + 2 * L].T
    layer = bj.AmortizedRadialLayer(ha, hb, hz)
    pa, pb, pz, la, lb, lz = layer._col_params(like, dim, N)
    es = head.element_size()
    assert (pz.data_ptr(), pa.data_ptr(), pb.data_ptr()) == (head.data_ptr(), head.data_ptr() + dim * L * es, head.data_ptr() + (dim * L + L) * es)
    assert (la, lb, lz) == (rows, rows, rows)
    # anything else is made so once: a contiguous (dim, L, batch) tensor has the batch fastest
    cz, ca = torch.randn(dim, L, N), torch.randn(L, N)
    layer = bj.AmortizedRadialLayer(ca, ca.clone(), cz)
    pa, pb, pz, la, lb, lz = layer._col_params(like, dim, N)
    assert pz.data_ptr() != cz.data_ptr() and pz.stride() == (1, dim, dim * L) and torch.equal(pz, cz) and (la, lz) == (L, dim * L)
    assert pa.data_ptr() != ca.data_ptr() and pa.stride(0) == 1 and torch.equal(pa, ca)
    # one layer given as (dim, batch) / (batch,)
    z2, a1 = torch.randn(N, dim).T, torch.randn(N)
    layer = bj.AmortizedRadialLayer(a1, a1.clone(), z2)
    pa, pb, pz, la, lb, lz = layer._col_params(like, dim, N)
    assert layer.n_layers == 1 and pz.data_ptr() == z2.data_ptr() and pa.data_ptr() == a1.data_ptr() and (la, lz) == (1, dim)


def test_host_class_is_a_bijector_of_its_own_and_refuses_wrong_shapes(bj):
    torch = pytest.importorskip("torch")
    I = bj.interface
    dim, N = 4, 8
    layer = bj.AmortizedRadialLayer(torch.randn(2, N), torch.randn(2, N), torch.randn(dim, 2, N))
    assert "AmortizedRadialLayer" in bj.__all__ and isinstance(layer, bj.Bijector) and not isinstance(layer, bj.RadialLayer)
    assert I._radial_kind(layer) == 0 and I._radial_kind(bj.inverse(layer)) == 0
    # the planner keeps it as a stage of its own, also between RadialLayers that would otherwise fuse into one run
    st, spans = (layer @ layer @ bj.Shift(1.0))._plan()
    assert [type(s).__name__ for s in st] == ["Shift", "AmortizedRadialLayer", "AmortizedRadialLayer"] and spans == [(0, 1), (1, 2), (2, 3)]
    rad = bj.RadialLayer(torch.randn(1), torch.randn(1), torch.randn(dim))
    st, _ = (rad @ layer @ rad)._plan()
    assert [type(s).__name__ for s in st] == ["RadialLayer", "AmortizedRadialLayer", "RadialLayer"]
    assert bj.isclosedform(bj.inverse(layer)) and bj.isinvertible(layer)
    assert I._has_own_params(layer) and I._has_own_params(bj.inverse(layer)) and "AmortizedRadialLayer" in I._PARAM_STAGES
    like = torch.empty(0, dtype=torch.float32)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._col_params(like, dim + 1, N)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._col_params(like, dim, N + 1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedRadialLayer(torch.randn(3, N), torch.randn(2, N), torch.randn(dim, 2, N))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedRadialLayer(torch.randn(2, N), torch.randn(N), torch.randn(dim, 2, N))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedRadialLayer(torch.randn(N), torch.randn(N), torch.randn(dim))
    for nl in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.AmortizedRadialLayer(torch.randn(nl, N), torch.randn(nl, N), torch.randn(dim, nl, N))
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        big = bj.AmortizedRadialLayer(torch.randn(1), torch.randn(1), torch.randn(lim + 1, 1))
        with pytest.raises(ValueError, match=str(lim)):
            big._col_params(torch.empty(0, dtype=dt), lim + 1, 1)
        ok = bj.AmortizedRadialLayer(torch.randn(1), torch.randn(1), torch.randn(lim, 1))
        ok._col_params(torch.empty(0, dtype=dt), lim, 1)
