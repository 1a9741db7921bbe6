"""include/bjx_coupling.h (Coupling with a per-sample elementwise-chain law, companion of bjx.h) is a C header: a plain C99
program that includes it compiles with -std=c99 -pedantic -Werror, as tests/test_abi_cols_c.py checks for bjx_cols.h.

Also CPU only (no GPU module imported): the built library, when there is one, exports both entries; the ctypes table of
bijectors.jl_amd/_lib.py names exactly the header's entries; and the parameter table of tests/test_gpu_coupling_chain.py (LAWS,
read as text) takes every parameter slot of every op from each of its three sources — host scalar, per-row vector, per-sample
array — and holds every op kind the kernel serves, so that a source or an op cannot ship untested."""
import ast
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
HEADER = os.path.join(ROOT, "include", "bjx_coupling.h")
KERNELS = os.path.join(ROOT, "bijectors.jl_amd", "csrc", "bjx_coupling_chain.hip")
LIB = os.path.join(ROOT, "bijectors.jl_amd", "libbjx_hip.so")
ENTRIES = ["bjx_coupling_chain", "bjx_coupling_chain_vjp"]

PROGRAM = r"""
#include "bjx_coupling.h"
#include <stddef.h>

int main(void) {
  int (*f)(bjx_ctx*, bjx_dtype, int, const int32_t*, int64_t, const bjx_op*, int, const void* const*, const int64_t*, const void*, void*, void*,
           double*, int64_t, int64_t, uint32_t) = bjx_coupling_chain;
  int (*g)(bjx_ctx*, bjx_dtype, int, const int32_t*, int64_t, const bjx_op*, int, const void* const*, const int64_t*, const void*, const void*,
           const void*, void*, void* const*, int64_t, int64_t) = bjx_coupling_chain_vjp;
  bjx_op ops[BJX_COUPLING_MAX_OPS];
  ops[0].kind = BJX_OP_AFFINE;
  return (f != NULL && g != NULL && BJX_COUPLING_MAX_OPS == 4 && BJX_COUPLING_MAX_OPS == BJX_MAX_SEG_OPS && ops[0].kind == 32 &&
          (int)BJX_OP_AFFINE > (int)BJX_OP_STDNORMAL_LOGPDF && BJX_VERSION == 100) ? 0 : 1;
}
"""


def test_coupling_header_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = tmp_path / "coupling.c"
    src.write_text(PROGRAM)
    subprocess.check_call([gcc, *CFLAGS, "-c", str(src), "-o", str(tmp_path / "coupling.o")])
    only = tmp_path / "only_coupling.c"
    only.write_text('#include "bjx_coupling.h"\nint main(void) { return BJX_OP_AFFINE == 32 ? 0 : 1; }\n')
    subprocess.check_call([gcc, *CFLAGS, str(only), "-o", str(tmp_path / "only_coupling")])
    subprocess.check_call([str(tmp_path / "only_coupling")])


def test_header_declares_exactly_the_bound_entries():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\bint\s+(bjx_\w+)\s*\(", text)
    assert declared == ENTRIES
    tree = ast.parse(open(os.path.join(ROOT, "bijectors.jl_amd", "_lib.py")).read())
    table = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "SIGNATURES_COUPLING")
    assert [k.value for k in table.keys] == ENTRIES
    consts = {n.targets[0].id: ast.literal_eval(n.value) for n in tree.body
              if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") in ("OP_AFFINE", "BJX_COUPLING_MAX_OPS")}
    assert consts == {"OP_AFFINE": 32, "BJX_COUPLING_MAX_OPS": 4}


def test_built_library_exports_the_entries():
    if not os.path.exists(LIB):
        return                                          # nothing built here: build() checks the same through _lib.load()
    nm = shutil.which("nm")
    assert nm, "binutils is part of the image"
    out = subprocess.check_output([nm, "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRIES:
        assert name in exported, f"{LIB} does not export {name}"


# op of the test table -> (kernel kind, number of parameters)
OPS = {"id": ("CK_ID", 0), "exp": ("CK_EXP", 0), "log": ("CK_LOG", 0), "flip": ("CK_FLIP", 0), "shift": ("CK_SHIFT", 1), "scale": ("CK_SCALE", 1),
       "scale_inv": ("CK_SCALE_INV", 1), "leaky": ("CK_LEAKY", 1), "logit": ("CK_LOGIT", 2), "logit_inv": ("CK_LOGIT_INV", 2), "affine": ("CK_AFFINE", 2)}


def _laws():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_coupling_chain.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "LAWS":
            return tree, ast.literal_eval(node.value)
    raise AssertionError("LAWS is not assigned at module level")


def test_gpu_parameter_table_takes_every_source_and_every_op():
    tree, laws = _laws()
    # the ABI kinds the host side maps onto a kernel kind (kind_info in bjx_coupling_chain.hip): each is in the table
    src = open(KERNELS).read()
    served = set(re.findall(r"case\s+BJX_OP_\w+:\s*return\s*\{(CK_\w+),", src))
    assert served == {ck for ck, _ in OPS.values()}, f"kind_info serves {sorted(served)}"
    seen_ops = {op for law in laws.values() for op, _, _ in law}
    assert seen_ops == set(OPS), f"ops never run: {sorted(set(OPS) - seen_ops)}; unknown: {sorted(seen_ops - set(OPS))}"
    by_source = {}
    for name, law in laws.items():
        assert 1 <= len(law) <= 4
        for op, s0, s1 in law:
            for j, s in enumerate((s0, s1)):
                assert (s is not None) == (j < OPS[op][1]), f"{name}: {op} parameter {j} source {s!r}"
                if s is not None:
                    assert s in ("s", "r", "c")
                    by_source.setdefault(s, set()).add((op, j))
    assert set(by_source) == {"s", "r", "c"}, "every source kind — host scalar, per-row vector, per-sample array — is exercised"
    for op, (_, n_par) in OPS.items():
        for j in range(n_par):
            assert (op, j) in by_source["c"], f"{op} parameter {j} is never per-sample"
    # ... within ONE chain too
    assert any({s for _, s0, s1 in law for s in (s0, s1) if s} == {"s", "r", "c"} for law in laws.values()), "no law mixes the three sources"
    # the table is what the value test and the pullback test run, in both directions and dtypes
    for fn in ("test_every_op_and_chain_matches_oracle", "test_pullback_matches_oracle_closed_forms"):
        node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == fn)
        par = {ast.literal_eval(d.args[0]): ast.unparse(d.args[1]) for d in node.decorator_list if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize"}
        assert par["name"] == "sorted(LAWS)" and par["inverse"] == "[False, True]" and par["dt"] == "[np.float32, np.float64]", par
