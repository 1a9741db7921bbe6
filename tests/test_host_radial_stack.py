"""Host side of the fused RadialLayer run (include/bjx_radial_stack.h, `_RadialRun`), no GPU: the composition planner groups
maximal runs of >= 2 RadialLayer stages (inverse runs: the inverse of the REVERSED run), leaves single radial stages and runs of
mixed direction alone, and maps the planned stages back onto `_stages()`; the parameter pullback of a composition sees the single
layers again; the header's prototypes are the ctypes signatures of bijectors.jl_amd/_lib.py, argument by argument."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bjx_radial_stack.h")
ENTRIES = ["bjx_radial_stack", "bjx_radial_stack_vjp"]


@pytest.fixture(scope="module")
def bj():
    import bijectors_amd

    return bijectors_amd


def _rad(bj, k, dim=3):
    import torch

    return bj.RadialLayer(torch.full((1,), 0.1 * k), torch.full((1,), -0.2 * k), torch.full((dim,), float(k)))


def test_planner_groups_radial_runs(bj):
    import torch

    I = bj.interface
    rs = [_rad(bj, k) for k in range(6)]
    pl = [bj.PlanarLayer(torch.full((3,), float(k)), torch.ones(3), torch.zeros(1)) for k in range(2)]
    # application order: r0, r1, r2, Shift, r3, p0, p1, r4, r5
    flow = rs[5] @ rs[4] @ pl[1] @ pl[0] @ rs[3] @ bj.Shift(1.0) @ rs[2] @ rs[1] @ rs[0]
    st, spans = flow._plan()
    assert [type(x).__name__ for x in st] == ["_RadialRun", "Shift", "RadialLayer", "_PlanarRun", "_RadialRun"]
    assert spans == [(0, 3), (3, 4), (4, 5), (5, 7), (7, 9)]
    assert st[0].layers == rs[0:3] and st[0].n_layers == 3 and st[4].layers == rs[4:6]
    assert st[2] is rs[3]                                                                 # a single radial stage stays itself
    assert flow._plan() is flow._plan()
    # the inverse flow: inv(r5), inv(r4), inv(p1), inv(p0), inv(r3), Shift(-1), inv(r2), inv(r1), inv(r0)
    sti, spi = bj.inverse(flow)._plan()
    assert [type(x).__name__ for x in sti] == ["Inverse", "Inverse", "Inverse", "Shift", "Inverse"]
    assert spi == [(0, 2), (2, 4), (4, 5), (5, 6), (6, 9)]
    assert isinstance(sti[0].orig, I._RadialRun) and sti[0].orig.layers == [rs[4], rs[5]]  # the forward run applies r4 then r5
    assert isinstance(sti[1].orig, I._PlanarRun) and sti[2].orig is rs[3]
    assert isinstance(sti[4].orig, I._RadialRun) and sti[4].orig.layers == rs[0:3]
    # a lone layer, and a run whose stages point in different directions, are left alone
    assert (rs[1] @ bj.Shift(0.5))._plan()[0][1] is rs[1]
    mixed = bj.inverse(rs[2]) @ rs[1] @ bj.inverse(rs[0])
    stm, spm = mixed._plan()
    assert spm == [(0, 1), (1, 2), (2, 3)] and stm[1] is rs[1] and stm[0].orig is rs[0] and stm[2].orig is rs[2]
    two_dirs = bj.inverse(rs[3]) @ bj.inverse(rs[2]) @ rs[1] @ rs[0]
    st2, sp2 = two_dirs._plan()
    assert sp2 == [(0, 2), (2, 4)] and st2[0].layers == rs[0:2] and st2[1].orig.layers == [rs[3], rs[2]]
    assert I._planned([rs[0], rs[1]])[0][0] == I._RadialRun(rs[0:2])                       # `==` through the layers' keys
    with pytest.raises(TypeError):
        I._RadialRun([rs[0], pl[0]])


def test_parameter_pullback_plan_sees_single_radial_layers(bj):
    """`vjp_params` of a composition is not fused for radial runs: its stage list is the plan with every `_RadialRun` put back as
    its layers (planar runs stay merged), spans one stage wide."""
    import torch

    I = bj.interface
    rs = [_rad(bj, k) for k in range(3)]
    pl = [bj.PlanarLayer(torch.full((3,), float(k)), torch.ones(3), torch.zeros(1)) for k in range(2)]
    flow = pl[1] @ pl[0] @ rs[2] @ rs[1] @ rs[0]
    st, sp = I._radial_runs_unfused(flow)
    assert st[:3] == rs and isinstance(st[3], I._PlanarRun) and sp == [(0, 1), (1, 2), (2, 3), (3, 5)]
    sti, spi = I._radial_runs_unfused(bj.inverse(flow))
    assert [s.orig for s in sti[1:]] == [rs[2], rs[1], rs[0]] and spi == [(0, 2), (2, 3), (3, 4), (4, 5)]


_CTYPES = {"bjx_ctx*": C.c_void_p, "bjx_dtype": C.c_int, "int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p,
           "double*": C.c_void_p, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


def test_header_prototypes_match_the_ctypes_signatures(bj):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(int)\s+(bjx_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [p[1] for p in protos] == ENTRIES
    table = bj._lib.SIGNATURES_RADIAL_STACK
    assert list(table) == ENTRIES
    for ret, name, args in protos:
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.fullmatch(r"(.*?[\w*])\s*(\w+)?", a)
            ty = m.group(1) if m.group(2) and not a.endswith("*") else a          # "bjx_ctx*" (unnamed) or "const void* alpha_"
            types.append(_CTYPES[ty.replace(" *", "*")])
        res, argtypes = table[name]
        assert res is C.c_int and ret == "int"
        assert argtypes == types, f"{name}: header {types} vs _lib.py {argtypes}"
    # bjx.h itself is untouched by the companion header
    assert "radial_stack" not in open(os.path.join(ROOT, "include", "bjx.h")).read()
