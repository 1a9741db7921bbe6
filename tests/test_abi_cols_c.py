"""include/bjx_cols.h (the per-column spline entries, companion of bjx.h) is a C header: a plain C99 program that includes it compiles
with -std=c99 -pedantic -Werror, as tests/test_abi_c.py checks for bjx.h.

Dispatch coverage of the same entries (CPU only, no GPU module imported): every specialised bin count K of `launch_fwd` /
`launch_vjp` in bijectors.jl_amd/csrc/bjx_spline_cols.hip is run by the GPU tests in both directions, and so is at least one
streaming K (the `default:` arm) below and above each of them, so a new `case` arm cannot ship untested.  The test files are
read as text: the forward K's are those of test_gpu_spline_cols.py's SHAPES, the pullback K's test_gpu_spline_cols_edges.py's
VJP_CASES (K_VJP in both forms)."""
import ast
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]

PROGRAM = r"""
#include "bjx_cols.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, int, int, const int32_t*, int64_t, const void*, const void*, const void*, int64_t, int64_t, int64_t, int,
           double, const void*, void*, void*, double*, int64_t, int64_t, uint32_t) = bjx_rqs_cols;
  int (*g)(bjx_ctx*, bjx_dtype, int, int, const int32_t*, int64_t, const void*, const void*, const void*, int64_t, int64_t, int64_t, int,
           double, const void*, const void*, const void*, void*, void*, void*, void*, int64_t, int64_t) = bjx_rqs_cols_vjp;
  return (f != NULL && g != NULL && BJX_COLS_KNOTS == 0 && BJX_COLS_RAW == 1 && BJX_COLS_MAX_BINS == 64 && BJX_VERSION == 100) ? 0 : 1;
}
"""


def test_cols_header_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = tmp_path / "cols.c"
    src.write_text(PROGRAM)
    subprocess.check_call([gcc, *CFLAGS, "-c", str(src), "-o", str(tmp_path / "cols.o")])
    only = tmp_path / "only_cols.c"
    only.write_text('#include "bjx_cols.h"\nint main(void) { return BJX_COLS_RAW == 1 ? 0 : 1; }\n')
    subprocess.check_call([gcc, *CFLAGS, str(only), "-o", str(tmp_path / "only_cols")])
    subprocess.check_call([str(tmp_path / "only_cols")])


SPLINE_COLS = os.path.join(ROOT, "bijectors.jl_amd", "csrc", "bjx_spline_cols.hip")
TESTS = os.path.dirname(os.path.abspath(__file__))


def _arms(fn):
    """The `case N:` labels of the switch of the host function `fn` (launch_fwd / launch_vjp); it must also have a default arm."""
    src = open(SPLINE_COLS).read()
    m = re.search(r"void\s+" + fn + r"\s*\(.*?\{(.*?)#undef", src, re.S)
    assert m, f"{fn} not found in {SPLINE_COLS}"
    assert "default:" in m.group(1), f"{fn}: no streaming (default) arm"
    return sorted(int(k) for k in re.findall(r"case\s+(\d+)\s*:", m.group(1)))


def _module(name):
    return ast.parse(open(os.path.join(TESTS, name)).read())


def _assigned(tree, name):
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return node.value
    raise AssertionError(f"{name} is not assigned at module level")


def _parametrized(tree, fn):
    """{argnames: argvalues node} of the @pytest.mark.parametrize decorators of the test function `fn`."""
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == fn:
            return {ast.literal_eval(d.args[0]): d.args[1] for d in node.decorator_list
                    if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize"}
    raise AssertionError(f"{fn} not found")


def _covers(arms, ks, what):
    streaming = [k for k in set(ks) if k not in arms]
    for a in arms:
        assert a in ks, f"{what}: the specialised K = {a} is never run (tested K: {sorted(set(ks))})"
        assert any(k < a for k in streaming), f"{what}: no streaming K below the specialised K = {a} (tested K: {sorted(set(ks))})"
        assert any(k > a for k in streaming), f"{what}: no streaming K above the specialised K = {a} (tested K: {sorted(set(ks))})"


def test_every_forward_arm_is_run_by_the_value_test():
    arms = _arms("launch_fwd")
    assert arms, "launch_fwd has no specialised arm"
    tree = _module("test_gpu_spline_cols.py")
    p = _parametrized(tree, "test_per_column_spline_matches_oracle")
    assert isinstance(p.get("shape"), ast.Name) and p["shape"].id == "SHAPES"
    assert sorted(ast.literal_eval(p["form"])) == ["knots", "raw"] and sorted(ast.literal_eval(p["inverse"])) == [False, True]
    _covers(arms, [K for _, K, _ in ast.literal_eval(_assigned(tree, "SHAPES"))], "bjx_rqs_cols")


def test_every_pullback_arm_is_run_by_the_instantiation_test():
    arms = _arms("launch_vjp")
    assert arms, "launch_vjp has no specialised arm"
    tree = _module("test_gpu_spline_cols_edges.py")
    p = _parametrized(tree, "test_every_pullback_instantiation_matches_oracle")
    assert isinstance(p.get("K,form"), ast.Name) and p["K,form"].id == "VJP_CASES"
    assert sorted(ast.literal_eval(p["inverse"])) == [False, True]
    cases = _assigned(tree, "VJP_CASES")                       # [(K, form) for K in K_VJP for form in (...) if not (K == 1 and ...)]
    assert isinstance(cases, ast.ListComp) and ast.unparse(cases.generators[0].iter) == "K_VJP"
    assert ast.literal_eval(cases.generators[1].iter) == ("knots", "raw")
    ifs = [ast.unparse(c) for g in cases.generators for c in g.ifs]
    assert ifs in ([], ["not (K == 1 and form == 'knots')"]), f"VJP_CASES drops more than the knot form at K = 1: {ifs}"
    _covers(arms, ast.literal_eval(_assigned(tree, "K_VJP")), "bjx_rqs_cols_vjp")
