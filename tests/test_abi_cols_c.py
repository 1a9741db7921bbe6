"""include/bjx_cols.h (the per-column spline entries, companion of bjx.h) is a C header: a plain C99 program that includes it compiles
with -std=c99 -pedantic -Werror, as tests/test_abi_c.py checks for bjx.h."""
import os
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
