"""The dispatch restatement, references, draws and tables of tests/test_gpu_seq_abi.py (tests/_seq_ref.py), checked on the CPU:
  * edges — RANGES is exactly what a scan of `form` over 1 … 11 000 rows gives, so every lo / hi in it is the edge of the form written
    next to it (`form` changes at that height and not one row before it), no family or (G, NP) the dispatchers can choose is left
    out, and H = 2 of quad_stream_kernel is never reached with the default switches;
  * every alignment, leading-dimension, loop-trip and alias shape of the GPU file reaches the instantiation its section is about;
  * references — ordered_ref / simplex_ref agree with oracle.ordered / oracle.simplex in Float64 (ε = eps(Float64)) to 1e-12 of a
    column's scale;
  * headroom — on every draw the GPU file compares with a reference, the oracle's own Float32 path stays within a tenth of the flat
    bar of the Float64 reference evaluated with ε = eps(Float32); the figures are printed.  A draw that breaks this is changed, never
    the bar.  Transforms and the Ordered pullback; oracle.simplex_vjp computes in Float64 whatever it is given, and its inputs are the
    transforms' draws, whose stick remainder is asserted to stay >= 0.499.
No GPU, no torch."""
import numpy as np
import pytest

import _seq_ref as R

TENTH = 0.1 * 1e-3          # a tenth of the flat Float32 bar of tests/_tol.py
COMBOS = sorted(R.RANGES)
COMBO_IDS = [f"{e}-{d}-{'inverse' if i else 'forward'}" for e, d, i in COMBOS]


def _scan(entry, dtname, inverse):
    rows, prev = [], None
    for K in range(1, R.SCAN_MAX + 1):
        k = R.key(R.form(entry, dtname, inverse, K, 3))
        if k != prev:
            rows.append([K, K, k])
            prev = k
        else:
            rows[-1][1] = K
    return [tuple(r) for r in rows]


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("entry,dtname,inverse", COMBOS, ids=COMBO_IDS)
def test_every_table_height_is_the_edge_of_the_form_written_next_to_it(entry, dtname, inverse):
    rows = R.RANGES[(entry, dtname, inverse)]
    assert _scan(entry, dtname, inverse) == list(rows)
    for lo, hi, k in rows:                                        # said again, row by row: the form changes AT lo and AFTER hi
        assert R.key(R.form(entry, dtname, inverse, lo, 3)) == k == R.key(R.form(entry, dtname, inverse, hi, 3))
        assert lo == 1 or R.key(R.form(entry, dtname, inverse, lo - 1, 3)) != k
        assert hi == R.SCAN_MAX or R.key(R.form(entry, dtname, inverse, hi + 1, 3)) != k
    hs = R.form_heights(entry, dtname, inverse)
    assert all(R.form(entry, dtname, inverse, K, 3).family not in ("none", "refused") for K in hs)
    assert {k[0] for _, _, k in rows} - {"refused"} == {R.form(entry, dtname, inverse, K, 3).family for K in hs}
    assert {k for _, _, k in rows if k[0] != "refused"} == {R.key(R.form(entry, dtname, inverse, K, 3)) for K in hs}     # every (G, NP), both TABLE
    # the batch never changes the family, and nsteps stays 1 at the edge batches
    for K in hs:
        fm = R.form(entry, dtname, inverse, K, 3)
        for b in R.edge_batches(fm):
            fb = R.form(entry, dtname, inverse, K, b)
            assert R.key(fb) == R.key(fm) and fb.get("nsteps", 1) == 1


def test_the_forms_the_issue_names():
    f = R.form
    assert all(f(e, d, i, K, 3).get("H", 1) == 1 for e in R.TRANSFORMS for d in R.DTS for i in R.DIRS for K in range(1, 300))      # H = 2: never by default
    # the tall kernels: smallest G, a middle G, the largest, both sides of the hole
    assert [f("ordered", "float32", False, K, 3).get("G") for K in (65, 500, 1024, 1025, 1228, 1229, 2017, 2048, 2049)] == [3, 16, 32, None, None, 39, 64, 64, None]
    assert [f("ordered", "float64", False, K, 3).get("G") for K in (65, 250, 497, 512, 513)] == [5, 16, 32, 32, None]
    assert [f("simplex", "float32", True, K, 3).get("G") for K in (128, 129, 161, 481, 512, 513)] == [4, 5, 6, 16, 16, None]
    assert f("simplex", "float32", True, 128, 3).family == "quad" and f("simplex", "float64", True, 300, 3).family == "chunk"
    assert [f("simplex_vjp", "float64", True, K, 3).get("G") for K in (65, 512, 513, 614, 615, 1009, 1024, 1025)] == [5, 32, None, None, 39, 64, 64, None]
    assert [f("simplex_vjp", "float32", True, K, 3).family for K in (2048, 2049)] == ["tall_vjp", "chunk_vjp"]
    # TABLE = false one row in, both types, transform and pullback
    for d, kt, kv in (("float32", 10242, 10241), ("float64", 5122, 5121)):
        for i in R.DIRS:
            assert f("simplex", d, i, kt - 1, 3)["TABLE"] and not f("simplex", d, i, kt, 3)["TABLE"]
            assert f("simplex_vjp", d, i, kv - 1, 3)["TABLE"] and not f("simplex_vjp", d, i, kv, 3)["TABLE"]
            assert kt in R.form_heights("simplex", d, i) and kt - 1 in R.form_heights("simplex", d, i)
            assert kv in R.form_heights("simplex_vjp", d, i) and kv + 1 in R.form_heights("simplex_vjp", d, i)
    # the chunk walkers at rows mod C in {C − 1, 0, 1}
    for d in ("float32", "float64"):
        for e, i in (("ordered", False), ("ordered", True), ("simplex", False), ("simplex", True)):
            fms = [f(e, d, i, K, 3) for K in R.form_heights(e, d, i)]
            C = 256 // np.dtype(d).itemsize
            got = {max(R.rows_io(e, K, i)) % C for K, fm in zip(R.form_heights(e, d, i), fms) if fm.family == "chunk"}
            assert got >= {C - 1, 0, 1}, (e, d, i, got)
        for i in R.DIRS:
            CH = 128 // np.dtype(d).itemsize
            got = {K % CH for K in R.form_heights("simplex_vjp", d, i) if f("simplex_vjp", d, i, K, 3).family == "chunk_vjp"}
            assert got >= {CH - 1, 0, 1}, (d, i, got)
    # the Ordered pullback stream: packs = 2, 3, 33, 64, 65, 129, 257, 512 and one row into a new pack after each
    for d, V in (("float32", 4), ("float64", 2)):
        hs = R.form_heights("ordered_vjp", d, False)
        packs = {(K + V - 1) // V for K in hs if f("ordered_vjp", d, False, K, 3).family == "ordered_stream"}
        assert packs >= {33, 64, 65, 129, 257, 512} | ({3} if V == 4 else {5}) and 2 not in packs, (d, sorted(packs))    # up to 8 rows (2 | 4 packs): the tiny kernel's
        assert {K for K in hs if K % V == 1} >= ({9, 257, 513, 1025} if V == 4 else {9, 65, 129, 257, 513})
        assert (2047 if V == 4 else 1023) in hs and 2 * V * 256 in hs
    for d, K in (("float32", 8), ("float64", 4)):                                                   # ... except where it steps aside: in_bar == in
        assert K in R.ALIAS_IN_KS[("ordered_vjp", d)] and f("ordered_vjp", d, False, K, 3, alias="in")["G"] == 2


@pytest.mark.parametrize("dtname", ["float32", "float64"])
def test_alignment_shapes_reach_the_element_forms(dtname):
    V = R.vw(dtname)
    seen = set()
    for entry in ("ordered", "simplex", "ordered_vjp", "simplex_vjp"):
        for inverse in R.DIRS:
            for K in R.align_ks(entry, dtname):
                f0 = R.form(entry, dtname, inverse, K, 3)
                for off in R.OFFSETS[dtname]:
                    for oi, oo, ob in R.offset_patterns(entry, off):
                        fm = R.form(entry, dtname, inverse, K, 3, off_in=oi, off_out=oo, off_bar=ob)
                        assert fm.family not in ("refused", "none")
                        ri, ro = R.rows_io(entry, K, inverse)
                        seen.add((fm.family, fm.get("V"), fm.get("VIN"), fm.get("VOUT"), fm.get("VK"), fm.get("VK1"), fm.get("partial", 0) > 0, ri % V == 0, ro % V == 0, f0.family))
    fams = {s[0] for s in seen}
    assert fams >= {"tiny", "wave", "tall", "chunk", "tiny_vjp", "ordered_stream", "ordered_tall", "simplex_lane", "tall_vjp", "chunk_vjp"}
    assert any(s[0] == "wave" and s[1] == 1 and s[7] and s[8] for s in seen)                       # seq_wave_kernel<T, Op, 1> at a whole-pack height
    assert any(s[0] == "wave" and s[1] == 1 and s[9] == "quad" for s in seen)                      # where an aligned call takes the quad frames
    assert any(s[0] == "chunk" and s[1] == 1 and s[7] and s[8] for s in seen)                      # seq_chunk_kernel<T, Op, 1, *>
    assert any(s[0] == "tall" and s[2] is False and s[7] for s in seen) and any(s[0] == "tall" and s[3] is False and s[8] for s in seen)
    assert any(s[0] == "tall" and s[2] is True and s[3] is False and s[8] for s in seen)           # one side only
    assert any(s[0] == "tall_vjp" and s[4] is False and s[5] is False for s in seen)
    assert any(s[0] == "ordered_tall" and s[1] == 1 for s in seen) and any(s[0] == "simplex_lane" and s[1] == 1 and s[9] == "simplex_stream" for s in seen)
    assert any(s[0] == "simplex_lane" and s[1] == 1 and s[9] == "simplex_lane" for s in seen)
    assert any(s[0] == "ordered_stream" and s[6] for s in seen)                                    # the partial last pack on an unaligned base
    assert R.form("ordered_vjp", dtname, False, R.ORDERED_TALL_TRIP_K[dtname], 3)["V"] == V


@pytest.mark.parametrize("dtname", ["float32", "float64"])
def test_leading_dimension_shapes_reach_both_walkers_and_the_ragged_pack_branch(dtname):
    V = R.vw(dtname)
    seen = set()
    for kind in R.TRANSFORMS:
        for K in R.LD_KS[(kind, dtname)]:
            for inverse in R.DIRS:
                ri, ro = R.rows_io(kind, K, inverse)
                for li, lo in R.ld_variants(dtname, ri, ro):
                    assert (li, lo) != (ri, ro) and li >= ri and lo >= ro
                    fm = R.form(kind + "_ld", dtname, inverse, K, R.LD_BATCH, ld_in=li, ld_out=lo)
                    assert fm.family in ("wave", "chunk")
                    seen.add((kind, fm.family, fm["V"], fm.get("ld_in"), fm.get("ld_out"), fm.get("ragged_in"), fm.get("ragged_out")))
        ks = R.LD_KS[(kind, dtname)]
        fams = [R.form(kind + "_ld", dtname, False, K, R.LD_BATCH, ld_in=K + 8, ld_out=K + 8).family for K in ks]
        i = fams.index("chunk")
        assert fams[i - 1] == "wave" and ks[i] == ks[i - 1] + 1                                    # the last height before `chunk_min`, the first after
    for kind in R.TRANSFORMS:
        assert {s[1:5] for s in seen if s[0] == kind and s[1] == "wave"} == {("wave", V, True, False), ("wave", V, False, True), ("wave", 1, True, True)}
        assert {s[2] for s in seen if s[0] == kind and s[1] == "chunk"} == {V, 1}
    assert ("simplex", "chunk", V, None, None, True, False) in seen and ("simplex", "chunk", V, None, None, False, True) in seen      # V = VW, !full_in / !full_out
    assert R.LD_BATCH > 64 and R.LD_BATCH % 64 != 0


def test_trip_shapes_take_two_and_three_steps_with_a_ragged_last_set():
    for entry, dtname, inverse, K in R.TRIPS + [R.TRIP3]:
        n = 3 if (entry, dtname, inverse, K) == R.TRIP3 else 2
        f0 = R.form(entry, dtname, inverse, K, 3)
        assert f0.family in ("tall", "tall_vjp") and f0["CPS"] >= 2                                # a ragged set needs more than one column a set
        b = R.trip_batch(f0["CPS"], n)
        fm = R.form(entry, dtname, inverse, K, b)
        sets = -(-b // fm["CPS"])
        assert fm["nsteps"] == n and sets == n * 4096 + 2 and b % fm["CPS"] == 1                   # the last wave: a full set, then one column
        assert b * K * np.dtype(dtname).itemsize <= 70e6
        assert np.gcd(R.TRIP_D, fm["CPS"]) == 1
    got = {(e, d, i) for e, d, i, _ in R.TRIPS}
    assert got == {(e, d, i) for e in ("ordered", "simplex", "simplex_vjp") for d in ("float32", "float64") for i in R.DIRS} - {("simplex", "float64", True)}
    for key3 in got:                                                                               # a whole-pack aligned height and an odd one, each
        ks = [K for e, d, i, K in R.TRIPS if (e, d, i) == key3]
        assert len(ks) == 2 and ks[0] % 2 != ks[1] % 2
    for d in ("float32", "float64"):
        assert R.form("ordered_vjp", d, False, R.ORDERED_TALL_TRIP_K[d], 2049) == R.Form(family="ordered_tall", V=R.vw(d), group=1)
    idx = R.tiled_index(R.TRIP_D, 100)
    assert np.array_equal(idx[:R.TRIP_D], np.arange(R.TRIP_D)) and np.array_equal(idx[R.TRIP_D:], idx[:100 - R.TRIP_D])


def test_alias_shapes_reach_the_kernels_the_dispatchers_step_aside_to():
    for d, V in (("float32", 4), ("float64", 2)):
        fams = [R.form("ordered_vjp", d, False, K, 3, alias="in").family for K in R.ALIAS_IN_KS[("ordered_vjp", d)]]
        assert fams[0] == "ordered_lane" and fams.count("ordered_column") == 2 and "ordered_stream" in fams and "tiny_vjp" not in fams and "ordered_tall" not in fams
        assert [R.form("ordered_vjp", d, False, K, 3).family for K in R.ALIAS_IN_KS[("ordered_vjp", d)][:2]] == ["tiny_vjp"] * 2
        for i in R.DIRS:
            fams = {R.form("simplex_vjp", d, i, K, 3, alias="in").family for K in R.ALIAS_IN_KS[("simplex_vjp", d)]}
            assert fams == {"simplex_lane", "simplex_stream", "tall_vjp", "chunk_vjp"}
            assert all(R.form("simplex_vjp", d, i, K, 3, alias="out_bar") == R.Form(family="refused", code=R.ERR_ARG) for K in R.ALIAS_IN_KS[("simplex_vjp", d)])
            assert R.form("simplex_vjp", d, i, 5, 0, alias="out_bar").family == "none"
        served, refused = R.ALIAS_OUT_BAR_SERVED[d], R.ALIAS_OUT_BAR_REFUSED[d]
        assert refused == served[-1] + 1 == 512 * V + 1
        assert [R.form("ordered_vjp", d, True, K, 3, alias="out_bar").family for K in served] == ["tiny_vjp", "tiny_vjp"] + ["ordered_stream"] * 3
        assert R.form("ordered_vjp", d, True, refused, 3, alias="out_bar") == R.Form(family="refused", code=R.ERR_ARG)
        assert R.form("ordered_vjp", d, True, refused, 3).family == "ordered_tall"


def test_refusals_of_the_descriptor_range():
    for d in ("float32", "float64"):
        ld = R.LD_REFUSED[d]
        assert 64 * ld * np.dtype(d).itemsize == 1 << 31
        for i in R.DIRS:
            assert R.form("ordered_ld", d, i, 300, 2, ld_in=ld, ld_out=ld) == R.Form(family="refused", code=R.ERR_UNSUPPORTED)
            assert R.form("ordered_ld", d, i, 300, 2, ld_in=ld - 1, ld_out=ld - 1).family == "chunk"
            assert R.form("simplex_vjp", d, i, ld, 1) == R.Form(family="refused", code=R.ERR_UNSUPPORTED)
            assert R.form("simplex_vjp", d, i, ld - 1, 1).family == "chunk_vjp"
        assert R.form("ordered_ld", d, False, 300, 2, ld_in=299, ld_out=300)["code"] == R.ERR_SHAPE
    assert R.form("simplex", "float32", False, 1, 3)["code"] == R.ERR_SHAPE and R.form("ordered", "float32", False, 0, 3)["code"] == R.ERR_SHAPE
    assert R.form("ordered", "float32", False, 5, -1)["code"] == R.ERR_SHAPE and R.form("ordered", "float32", False, 5, 0).family == "none"


# ------------------------------------------------------------------ references
def _col_err(got, ref, floor=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref).max(axis=0) / (np.abs(ref).max(axis=0) + floor + np.finfo(np.float64).tiny)).max())


@pytest.mark.parametrize("K", [2, 3, 8, 17, 64, 129, 513, 1100])
def test_numpy_references_agree_with_the_oracle_in_float64(orc, K):
    e64 = R.eps_of("float64")
    for kind in R.TRANSFORMS:
        for inverse in R.DIRS:
            if kind == "ordered" and K < 2:
                continue
            a = R.draw(kind, "float64", inverse, K, 9)
            out, ladj, floor = R.ordered_ref(a, inverse) if kind == "ordered" else R.simplex_ref(a, inverse, e64)
            o_out, o_ladj = (orc.ordered if kind == "ordered" else orc.simplex)(a, inverse=inverse)
            assert _col_err(out, o_out) <= 1e-12, (kind, inverse, K)
            assert (np.abs(ladj - o_ladj) <= 1e-12 * (np.abs(o_ladj) + floor * np.sqrt(K))).all(), (kind, inverse, K)
            assert floor.shape == ladj.shape == (9,) and (floor >= 0).all()


# ------------------------------------------------------------------ headroom
def _draw_list(dtname):
    """(kind, inverse, K, batch) of every transform draw the GPU file compares with the reference"""
    out = set()
    for kind in R.TRANSFORMS:
        for inverse in R.DIRS:
            for K in R.form_heights(kind, dtname, inverse):
                out.add((kind, inverse, K, max(R.edge_batches(R.form(kind, dtname, inverse, K, 3)))))
            for K in R.align_ks(kind, dtname):
                fm = R.form(kind, dtname, inverse, K, 3)
                if fm.family != "refused":
                    out.add((kind, inverse, K, fm["group"] + 1))
            for K in R.LD_KS[(kind, dtname)]:
                out.add((kind, inverse, K, R.LD_BATCH))
            out.add((kind, inverse, 12, 3))                                                        # the call after a refusal
    for entry, d, inverse, K in R.TRIPS + [R.TRIP3]:
        if d == dtname and entry in R.TRANSFORMS:
            out.add((entry, inverse, K, R.TRIP_D))
    out |= {("ordered", inverse, 300, 2) for inverse in R.DIRS}                                    # the served neighbour of the 2 GiB refusal
    return sorted(out)


def _ordered_vjp_draw_list(dtname):
    """(inverse, K, batch) of every Ordered pullback draw the GPU file compares with the oracle"""
    out = set()
    for inverse in R.DIRS:
        f = lambda K, **kw: R.form("ordered_vjp", dtname, inverse, K, 3, **kw)
        out |= {(inverse, K, max(R.edge_batches(f(K)))) for K in R.form_heights("ordered_vjp", dtname, inverse)}
        out |= {(inverse, K, f(K)["group"] + 1) for K in R.align_ks("ordered_vjp", dtname)}
        out |= {(inverse, K, f(K, alias="in")["group"] + 1) for K in R.ALIAS_IN_KS[("ordered_vjp", dtname)]}
        out |= {(inverse, K, f(K, alias="out_bar")["group"] + 1) for K in R.ALIAS_OUT_BAR_SERVED[dtname]}
        out |= {(inverse, R.ALIAS_OUT_BAR_REFUSED[dtname], 3), (inverse, 12, 3), (inverse, R.ORDERED_TALL_TRIP_K[dtname], R.TRIP_D)}
    return sorted(out)


@pytest.mark.parametrize("kind", R.TRANSFORMS)
def test_float32_oracle_stays_within_a_tenth_of_the_bar_of_the_float64_reference(orc, kind):
    """every Float32 draw: values on the column's max-norm, the log-det on |ref| + floor (the bar the GPU file uses)"""
    worst = {}
    for k, inverse, K, batch in _draw_list("float32"):
        if k != kind:
            continue
        a = R.draw(kind, "float32", inverse, K, batch)
        out, ladj, floor = R.ref(kind, "float32", inverse, K, batch)
        o_out, o_ladj = (orc.ordered if kind == "ordered" else orc.simplex)(a, inverse=inverse)
        assert o_out.dtype == np.float32
        e_v = _col_err(o_out, out)
        e_l = float((np.abs(np.asarray(o_ladj, np.float64) - ladj) / (np.abs(ladj) + floor + np.finfo(np.float64).tiny)).max())
        assert e_v <= TENTH and e_l <= TENTH, f"{kind} inverse={inverse} K={K}: Float32 oracle {e_v:.3g} (values) {e_l:.3g} (log-det) off the Float64 reference"
        if kind == "simplex":
            x = np.asarray(out if inverse else a, np.float64)
            assert (1.0 - np.cumsum(x[:-1], axis=0)).min() >= 0.499, (inverse, K)                 # the stick remainder stays large
        w = worst.setdefault(inverse, [0.0, 0.0, 0, 0])
        if e_v > w[0]:
            w[0], w[2] = e_v, K
        if e_l > w[1]:
            w[1], w[3] = e_l, K
    for inverse, (ev, el, kv, kl) in sorted(worst.items()):
        print(f"Float32 oracle vs Float64 reference, {kind} {'inverse' if inverse else 'forward'}: values {ev:.2e} (K = {kv}), log-det {el:.2e} (K = {kl}); a tenth of the bar is {TENTH:.0e}")


def test_float32_oracle_of_the_ordered_pullback_stays_within_a_tenth_of_the_bar(orc):
    worst = {}
    for inverse, K, b in _ordered_vjp_draw_list("float32"):
        a = R.draw("ordered", "float32", inverse, K, b)
        g, l = R.draw_bar("ordered", "float32", inverse, K, b)
        got = orc.ordered_vjp(a, g, l, inverse=inverse)
        assert got.dtype == np.float32
        e = _col_err(got, R.ref_vjp("ordered", "float32", inverse, K, b))
        assert e <= TENTH, f"ordered_vjp inverse={inverse} K={K}: {e:.3g}"
        worst[inverse] = max(worst.get(inverse, 0.0), e)
    print("Float32 oracle vs Float64 oracle, Ordered pullback, worst (forward, inverse):", {k: f"{v:.2e}" for k, v in worst.items()})
