"""Host side of the fused log-density pass for PlanarLayer runs (include/bjx_planar_logpdf.h), no GPU: the Float64 reference the GPU
tests use (tests/_planar_logpdf_grad_ref.py: the oracle's inverse map, `planar_inv_vjp` for ȳ, `planar_param_vjp` at x with (−ȳ, −c)
for the layers) agrees with central differences of Σ c·lp taken through the oracle's MAPS alone, for entries of w, u, b, μ, σ and y —
the yardstick is pinned before any GPU run; the identity the entry relies on (the forward parameter pullback is jointly linear:
θ̄(−ȳ, −c) = −θ̄(ȳ, c) with the per-layer scalar negated) holds in the oracle; the header is a C99 header and bijectors.jl_amd/_lib.py
names exactly its entry."""
import ast
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _planar_logpdf_grad_ref import objective, ref_planar_logpdf_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_planar_logpdf.h")
LIB = os.path.join(ROOT, "bijectors.jl_amd", "libbjx_hip.so")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
ENTRIES = ["bjx_planar_logpdf_vjp_params"]

PROGRAM = r"""
#include "bjx_planar_logpdf.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, const void*, const void*, const void*, int, const void*, const void*, const void*, const void*, void*, void*,
           void*, void*, void*, void*, void*, void*, int64_t, int64_t) = bjx_planar_logpdf_vjp_params;
  /* the tables and x; + ȳ without y_bar; + ones without lp_bar; only x for the base rows alone; nothing when nothing is summed */
  return (f != NULL && bjx_planar_logpdf_work_elems(8, 128, 10, 1, 1, 1, 1) == 2 * 8 * 10 + 128 * 10 &&
          bjx_planar_logpdf_work_elems(8, 128, 10, 1, 0, 0, 0) == 2 * 8 * 10 + 2 * 128 * 10 + 12 &&
          bjx_planar_logpdf_work_elems(8, 128, 10, 0, 1, 0, 0) == 128 * 10 && bjx_planar_logpdf_work_elems(8, 128, 10, 0, 0, 0, 0) == 0 &&
          bjx_planar_logpdf_work_elems(3, 35, 5, 1, 1, 0, 0) == 32 + 176 + 176 + 8 &&
          BJX_VERSION == 100) ? 0 : 1;
}
"""


def test_header_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = tmp_path / "planar_logpdf.c"
    src.write_text(PROGRAM)
    subprocess.check_call([gcc, *CFLAGS, "-c", str(src), "-o", str(tmp_path / "planar_logpdf.o")])
    only = tmp_path / "only.c"
    only.write_text(PROGRAM.replace("(f != NULL && ", "(").replace("= bjx_planar_logpdf_vjp_params;", "= NULL; (void)f;"))
    subprocess.check_call([gcc, *CFLAGS, str(only), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])


def test_header_declares_exactly_the_bound_entry():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"\bint\s+(bjx_\w+)\s*\(", text) == ENTRIES
    tree = ast.parse(open(os.path.join(ROOT, "bijectors.jl_amd", "_lib.py")).read())
    table = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "SIGNATURES_PLANAR_LOGPDF")
    assert [k.value for k in table.keys] == ENTRIES
    # 20 arguments: ctx, dtype, three tables, n_layers, twelve pointers, dim, batch — as the prototype
    proto = re.search(r"\bint\s+bjx_planar_logpdf_vjp_params\s*\(([^)]*)\)\s*;", text).group(1)
    kinds = ["i64" if "int64_t" in a else ("i" if re.search(r"\b(int|bjx_dtype)\b", a) else "p") for a in proto.split(",")]
    args = [ast.unparse(e) for e in table.values[0].elts[1].elts]
    assert [{"_vp": "p", "_i": "i", "_i64": "i64"}[a] for a in args] == kinds
    assert "planar_logpdf" not in open(os.path.join(ROOT, "include", "bjx.h")).read()


def test_built_library_exports_the_entry():
    if not os.path.exists(LIB):
        return                                          # nothing built here: build() checks the same through _lib.load()
    nm = shutil.which("nm")
    assert nm, "binutils is part of the image"
    out = subprocess.check_output([nm, "-D", "--defined-only", LIB], text=True)
    assert ENTRIES[0] in {line.split()[-1] for line in out.splitlines() if line.strip()}, f"{LIB} does not export {ENTRIES[0]}"


def _draw(dim, nl, N, seed):
    r = np.random.default_rng(seed)
    w = r.normal(size=(dim, nl)) / np.sqrt(dim)
    u = 0.1 * r.normal(size=(dim, nl)) / np.sqrt(dim)
    b = r.normal(size=nl)
    mu, sigma = 0.2 * r.normal(size=dim), np.exp(0.3 * r.normal(size=dim))
    return w, u, b, mu, sigma, np.asfortranarray(r.normal(size=(dim, N))), r.normal(size=N)


@pytest.mark.parametrize("dim,nl,N", [(6, 2, 5), (8, 3, 4), (3, 3, 6)])
def test_reference_is_the_central_difference_of_the_objective(orc, dim, nl, N):
    """d/dθ Σ c·lp through the oracle's inverse map and its log-det alone, central differences with step h = 1e-5 in Float64 (truncation
    ~h², rounding ~1e-16·|Σ c·lp|/h ~ 1e-10 of the objective's terms).  Bar: 1e-6 of max(|difference|, the tensor's max-norm) — one
    layer's w̄, ū or b̄; μ̄; σ̄; a column of ȳ — the rule of `_fd_check` in tests/test_gpu_logpdf_grad.py."""
    w, u, b, mu, sigma, Y, c = _draw(dim, nl, N, 70 + dim)
    ref = ref_planar_logpdf_grad(orc, w, u, b, mu, sigma, Y, c)
    h = 1e-5

    def fd(name, idx):
        vals = []
        for sgn in (+1.0, -1.0):
            p = dict(w=w.copy(), u=u.copy(), b=b.copy(), mu=mu.copy(), sigma=sigma.copy(), Y=Y.copy())
            p[name][idx] += sgn * h
            vals.append(objective(orc, p["w"], p["u"], p["b"], p["mu"], p["sigma"], p["Y"], c))
        return (vals[0] - vals[1]) / (2 * h)

    worst = 0.0
    checks = []
    for k in range(nl):
        checks += [("w", (i, k), ref["w_bar"][i, k], np.abs(ref["w_bar"][:, k]).max()) for i in range(dim)]
        checks += [("u", (i, k), ref["u_bar"][i, k], np.abs(ref["u_bar"][:, k]).max()) for i in range(dim)]
        checks.append(("b", k, ref["b_bar"][k], abs(ref["b_bar"][k])))
    checks += [("mu", i, ref["mu_bar"][i], np.abs(ref["mu_bar"]).max()) for i in range(dim)]
    checks += [("sigma", i, ref["sigma_bar"][i], np.abs(ref["sigma_bar"]).max()) for i in range(dim)]
    checks += [("Y", (i, n), ref["y_bar"][i, n], np.abs(ref["y_bar"][:, n]).max()) for n in range(N) for i in range(dim)]
    for name, idx, got, scale in checks:
        d = fd(name, idx)
        err = abs(got - d) / max(abs(d), scale)
        worst = max(worst, err)
        assert err <= 1e-6, f"{name}{idx}: reference {got} vs central difference {d} ({err:.3g} of its scale)"
    print(f"dim {dim}, {nl} layers: worst error of the reference against central differences {worst:.3g} of its scale")


def test_parameter_pullback_is_jointly_linear_with_the_scalar_negated(orc):
    """What the entry does instead of writing −ȳ: the forward parameter pullback at x with (−ȳ, −c) is minus the one with (ȳ, c) —
    `planar_param_vjp` recomputes its per-layer scalar from its arguments, so it flips sign with them — to rounding."""
    w, u, b, mu, sigma, Y, c = _draw(6, 4, 6, 91)
    ref = ref_planar_logpdf_grad(orc, w, u, b, mu, sigma, Y, c)
    pos = orc.planar_param_vjp(w, u, b, ref["x"], ref["y_bar"], c)
    for got, name in zip(pos, ("w_bar", "u_bar", "b_bar")):
        err = np.abs(-np.asarray(got).reshape(ref[name].shape) - ref[name]).max() / np.abs(ref[name]).max()
        assert err <= 1e-15 * 64, f"{name}: {err:.3g}"


def test_zero_cotangent_gives_zero_gradients_in_the_reference(orc):
    w, u, b, mu, sigma, Y, c = _draw(5, 3, 4, 92)
    ref, zero = ref_planar_logpdf_grad(orc, w, u, b, mu, sigma, Y, c), ref_planar_logpdf_grad(orc, w, u, b, mu, sigma, Y, np.zeros(4))
    assert np.array_equal(ref["lp"], zero["lp"])
    assert all(not np.any(zero[k]) for k in ("y_bar", "w_bar", "u_bar", "b_bar", "mu_bar", "sigma_bar"))
