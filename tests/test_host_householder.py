"""Host side of the shared Householder layer (include/bjx_householder.h, `HouseholderLayer`), no GPU and no built library: the
companion header is plain C99 and C++; its prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py argument by argument and
its LDS rule is the host's; the Float64 reference of tests/_householder_ref.py is held to an independent evaluation — the dense
product of I − t v vᵀ built explicitly, numpy's slogdet, and central differences of Σ_n⟨ȳ_n, out_n⟩ in every entry of V — at dim 1 … 8,
L 1 … 3 and both directions; v̄_k is orthogonal to v_k; a zero v_k is the identity with v̄_k exactly 0; the summed reference is the
batch sum of the per-column sibling's reference on expanded parameters; the host class refuses wrong shapes and sizes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _householder_cols_ref import RefAll
from _householder_ref import RefShared, apply, draws, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_householder.h")
ENTRIES = ["bjx_householder", "bjx_householder_vjp_params"]
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_householder.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, int, const void*, int, const void*, void*, void*, double*, int64_t, int64_t, uint32_t) = bjx_householder;
  int (*g)(bjx_ctx*, bjx_dtype, int, const void*, int, const void*, const void*, const void*, void*, void*, int64_t, int64_t) =
      bjx_householder_vjp_params;
  return (f != NULL && g != NULL && BJX_HOUSEHOLDER_MAX_LAYERS == 64 && BJX_HOUSEHOLDER_LDS_BYTES(64, 31) <= BJX_HOUSEHOLDER_LDS_BUDGET &&
          BJX_HOUSEHOLDER_LDS_BYTES(64, 32) > BJX_HOUSEHOLDER_LDS_BUDGET && BJX_VERSION == 100) ? 0 : 1;
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
    src = tmp_path / f"householder.{ext}"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, std, *WARN, "-c", str(src), "-o", str(tmp_path / "householder.o")])      # both prototypes pinned, not linked
    only = tmp_path / f"only.{ext}"
    only.write_text('#include "bjx_householder.h"\nint main(void) { return BJX_HOUSEHOLDER_LDS_BYTES(1024, 1) <= BJX_HOUSEHOLDER_LDS_BUDGET ? 0 : 1; }\n')
    subprocess.check_call([cc, std, *WARN, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_HOUSEHOLDER
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
    assert bj._lib.BJX_HOUSEHOLDER_MAX_LAYERS == int(re.search(r"#define BJX_HOUSEHOLDER_MAX_LAYERS (\d+)", text).group(1))
    assert bj._lib.BJX_HOUSEHOLDER_LDS_BUDGET == int(re.search(r"#define BJX_HOUSEHOLDER_LDS_BUDGET (\d+)", text).group(1))
    assert "householder" not in open(os.path.join(ROOT, "include", "bjx.h")).read()      # bjx.h itself is untouched by the companion header


def test_lds_rule_of_the_host_is_the_headers(bj, tmp_path):
    """`_lib.householder_lds_bytes` against the header's macro evaluated by the C compiler, at the boundaries the GPU test walks."""
    cases = [(64, 31), (64, 32), (1024, 1), (1024, 2), (512, 3), (512, 4), (1, 64), (3, 64)]
    body = "".join(f'  printf("%lu\\n", (unsigned long)BJX_HOUSEHOLDER_LDS_BYTES({d}, {l}));\n' for d, l in cases)
    src = tmp_path / "lds.c"
    src.write_text('#include "bjx_householder.h"\n#include <stdio.h>\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call([shutil.which("gcc"), "-std=c99", *WARN, str(src), "-o", str(tmp_path / "lds")])
    got = [int(s) for s in subprocess.check_output([str(tmp_path / "lds")]).split()]
    assert got == [bj._lib.householder_lds_bytes(d, l) for d, l in cases]
    fits = [b <= bj._lib.BJX_HOUSEHOLDER_LDS_BUDGET for b in got]
    assert fits == [True, False, True, False, True, False, True, True]


def test_built_library_exports_both_entries(bj):
    assert set(ENTRIES) <= set(bj._lib.SIGNATURES_HOUSEHOLDER)
    if not os.path.exists(bj._lib.LIB_PATH):
        return                                          # nothing built here: the GPU suite loads the library (load() checks every export)
    lib = C.CDLL(bj._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{bj._lib.LIB_PATH} does not export {name}"


# ------------------------------------------------------------------ the reference against an independent evaluation
def _dense(V):
    """U = H_{L−1}⋯H_0 as an explicit (dim, dim) matrix (H = I − 2vvᵀ/vᵀv; the identity at v == 0)."""
    dim, L = V.shape
    U = np.eye(dim)
    for k in range(L):
        vk = V[:, k]
        ss = vk @ vk
        U = (np.eye(dim) if ss == 0 else np.eye(dim) - 2.0 * np.outer(vk, vk) / ss) @ U
    return U


def _phi(V, x, g, inverse):
    """Σ_n ⟨ȳ_n, out_n⟩ through the dense matrix alone."""
    U = _dense(V)
    return float((g * (np.linalg.solve(U, x) if inverse else U @ x)).sum())


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_reference_matches_dense_matrices_slogdet_and_central_differences(inverse):
    """out = U x (inverse: U⁻¹y) and in_bar = Uᵀȳ (U⁻ᵀx̄) to 1e-12, slogdet(U) == 0 to 1e-12 and the reference's log-det exactly 0; every
    entry of v̄ against central differences (h = 1e-5: truncation ~ h² and rounding ~ eps/h are both ~1e-10) of the dense evaluation at
    1e-6 of the layer's term scale; the sums are the sums of their summands; v̄_kᵀv_k = 0 (the map depends on the direction of v_k only)."""
    h = 1e-5
    for dim in range(1, 9):
        for L in (1, 2, 3):
            N = 7
            V, x, g = draws(seed("shared-dense", dim, L, inverse), dim, L, N, np.float64)
            R = RefShared(V, x, g, inverse)
            what = f"dim={dim} L={L} inverse={inverse}"
            U = _dense(V)
            out, inb = (np.linalg.solve(U, x), np.linalg.solve(U.T, g)) if inverse else (U @ x, U.T @ g)
            assert np.abs(R.out - out).max() <= 1e-12 * max(1.0, np.abs(out).max()), what
            assert np.abs(R.in_bar - inb).max() <= 1e-12 * max(1.0, np.abs(inb).max()), what
            assert np.array_equal(R.out, apply(V, x, inverse)) and np.array_equal(R.in_bar, apply(V, g, not inverse)), what
            sign, logdet = np.linalg.slogdet(U)
            assert abs(logdet) <= 1e-12 and abs(sign) == 1.0 and not R.ladj.any() and R.ladj.shape == (N,), what
            assert np.abs(R.vb - R.vb_cols.sum(axis=2)).max() <= 1e-13 * max(1.0, R.term_scale.max()), what
            for k in range(L):
                assert abs(R.vb[:, k] @ V[:, k]) <= 1e-12 * R.term_scale[k] * np.abs(V[:, k]).sum(), f"{what}: v̄_{k} is not orthogonal to v_{k}"
                for r in range(dim):
                    keep = V[r, k]
                    V[r, k] = keep + h
                    hi = _phi(V, x, g, inverse)
                    V[r, k] = keep - h
                    lo = _phi(V, x, g, inverse)
                    V[r, k] = keep
                    err = abs((hi - lo) / (2 * h) - R.vb[r, k]) / R.term_scale[k]
                    assert err <= 1e-6, f"{what} v[{r}, {k}]: {err:.3g} of the layer's term scale"


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_a_zero_layer_is_the_identity_and_leaves_the_rest_alone(inverse):
    """v_1 == 0: with that layer REMOVED from the stack the values, the input cotangent and the cotangents of the other layers are the
    same numbers (bit for bit: the layer adds 0·v), and v̄_1 is exactly 0."""
    dim, L, N = 5, 3, 6
    V, x, g = draws(seed("shared-zero", inverse), dim, L, N, np.float64)
    V[:, 1] = 0.0
    R = RefShared(V, x, g, inverse)
    S = RefShared(V[:, [0, 2]], x, g, inverse)
    assert not R.vb[:, 1].any() and not R.vb_cols[:, 1].any() and R.term_scale[1] == 0.0
    assert np.array_equal(R.out, S.out) and np.array_equal(R.in_bar, S.in_bar) and np.array_equal(R.vb[:, [0, 2]], S.vb)
    assert R.vb[:, 0].any() and R.vb[:, 2].any()


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_summed_reference_is_the_batch_sum_of_the_per_column_reference(inverse):
    """The parameters expanded to (dim, L, N) through the per-column sibling's reference: values and input cotangents are the same, and
    its per-column v̄ summed over the batch is v̄ of the shared layer, to 1e-13 of the term scale."""
    for dim, L, N in ((1, 1, 5), (2, 3, 9), (5, 2, 33), (8, 3, 7), (16, 8, 20)):
        V, x, g = draws(seed("shared-cols", dim, L, inverse), dim, L, N, np.float64)
        R = RefShared(V, x, g, inverse)
        P = RefAll(np.repeat(V[:, :, None], N, axis=2), None, None, x, g, None, inverse)
        what = f"dim={dim} L={L} N={N} inverse={inverse}"
        assert np.abs(R.out - P.out).max() <= 1e-13 * np.abs(P.out).max() and np.abs(R.in_bar - P.in_bar).max() <= 1e-13 * np.abs(P.in_bar).max(), what
        assert not P.ladj.any(), what
        assert np.abs(R.vb_cols - P.vb).max() <= 1e-13 * R.term_scale.max(), what
        for k in range(L):
            assert np.abs(R.vb[:, k] - P.vb[:, k].sum(axis=1)).max() <= 1e-13 * N * R.term_scale[k], what


# ------------------------------------------------------------------ the host class
def test_host_class_is_public_a_parameter_stage_and_refuses_wrong_shapes(bj):
    torch = pytest.importorskip("torch")
    I = bj.interface
    dim = 4
    layer = bj.HouseholderLayer(torch.randn(dim, 3))
    one = bj.HouseholderLayer(torch.randn(dim))
    assert "HouseholderLayer" in bj.__all__ and isinstance(layer, bj.Bijector)
    assert (layer.dim, layer.n_layers, one.dim, one.n_layers) == (dim, 3, dim, 1)
    assert bj.isclosedform(bj.inverse(layer)) and bj.isinvertible(layer)
    assert I._has_own_params(layer) and I._has_own_params(bj.inverse(layer)) and "HouseholderLayer" in I._PARAM_STAGES
    # a stage of its own between other stages; two of them are not merged (one object already holds a whole stack)
    planar = bj.PlanarLayer(torch.randn(dim), torch.randn(dim), torch.randn(1))
    st, spans = (bj.Shift(1.0) @ layer @ planar)._plan()
    assert [type(s).__name__ for s in st][1:] == ["HouseholderLayer", "Shift"] and spans[1:] == [(1, 2), (2, 3)]
    st, _ = (layer @ one)._plan()
    assert [type(s).__name__ for s in st] == ["HouseholderLayer", "HouseholderLayer"]
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.HouseholderLayer(torch.randn(dim, 2, 5))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.HouseholderLayer(torch.tensor(1.0))
    for nl in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.HouseholderLayer(torch.randn(dim, nl))
    like = torch.empty(0, dtype=torch.float32)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        layer._table(like, dim + 1)
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        with pytest.raises(ValueError, match=str(lim)):
            bj.HouseholderLayer(torch.randn(lim + 1))._table(torch.empty(0, dtype=dt), lim + 1)
        t = bj.HouseholderLayer(torch.randn(lim, 2, dtype=dt))._table(torch.empty(0, dtype=dt), lim)
        assert t.shape == (lim, 2) and t.stride() == (1, lim)              # dense T[dim, n_layers], layer k at v + k*dim
    assert one._table(like, dim).shape == (dim,)
