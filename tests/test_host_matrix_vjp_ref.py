"""The inputs, references and tables of tests/test_gpu_matrix_vjp_abi.py (tests/_matrix_vjp_ref.py), checked on the CPU:
  * every row of FORM_EDGES, STAGING and the trip / alias lists reaches the form written next to it, K lo and K hi of a FORM_EDGES row
    are the smallest and largest K that do, and no family, (GS, KMAX, NT) or width the dispatchers can choose is left out;
  * the tiled generator's index map is right and TRIP_D is coprime to every samples-per-block;
  * `second_trip_batch` exceeds cus · blocks_per_cu · samples_per_block for EVERY blocks_per_cu a CU of 32 waves can hold, at 128, 256
    and 304 CUs, and leaves the ragged tail it promises;
  * the draws measure the kernel, not the data: the oracle's own Float32 evaluation of the INVERSE pullback stays within a tenth of the
    flat bar (1e-4 of the sample's max-norm) of its Float64 evaluation on every table draw; the FORWARD pullback (whose oracle computes
    in Float64 whatever it is given) moves by at most 1e-4 of the sample's max-norm under three random symmetric 1-ulp(Float32) relative
    perturbations of X — the method of test_gpu_parity.test_matrix_bijectors_match_oracle.  A draw that breaks either is redrawn with
    another seed (_matrix_vjp_ref.RESEED); the bar is never widened.
No GPU, no torch."""
import math

import numpy as np
import pytest

import _matrix_vjp_ref as R

TENTH = 0.1 * 1e-3          # a tenth of the flat Float32 bar of tests/_tol.py
CUS = (128, 256, 304)


def _sample_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    n = ref.shape[-1]
    return float((np.abs(got - ref).reshape(-1, n).max(axis=0) / (np.abs(ref).reshape(-1, n).max(axis=0) + np.finfo(np.float64).tiny)).max())


def _table_draws(dt, kinds=R.KINDS):
    """(kind, K, batch) of every draw the GPU file compares with the oracle in `dt`"""
    out = []
    for kind in kinds:
        for K in sorted(set(R.EDGE_KS) | set(R.STAGING_KS) | set(R.ALIAS_KS)):
            for inverse in (True, False):
                fm = R.form(kind, K, dt, inverse)
                if fm[0] != "none":
                    out += [(kind, K, max(R.edge_batches(fm))), (kind, K, R.samples_per_block(fm) + 1)]
        out.append((kind, 12, 3))
        if kind in R.TRIP_KINDS:
            out += [(kind, K, R.TRIP_D) for K in R.TRIP_KS + (R.ALIAS_TRIP_K,)]
    if "pd_vec" in kinds:
        out.append(("pd_vec", R.MEM_K, R.TRIP_D))
    return sorted(set(out))


# ------------------------------------------------------------------ the dispatch tables
@pytest.mark.parametrize("dt", R.DTS, ids=lambda d: d.name)
def test_every_form_edge_row_reaches_its_form_and_is_the_edge_of_it(dt):
    scan = range(1, R.K_REFUSED + 1)
    for inverse in (True, False):
        rows = R.FORM_EDGES[(dt, inverse)]
        for kind in R.KINDS:
            forms = {K: R.form(kind, K, dt, inverse) for K in scan}
            for (lo, hi), family, geom in rows:
                ks = [K for K in scan if forms[K][:2] == (family, geom)]
                if kind == "vec_corr" and inverse and lo == 1:
                    assert forms[1] == ("none", None, 0) and ks[0] == 2
                    ks = [1] + ks
                assert (ks[0], ks[-1]) == (lo, hi), (kind, inverse, family, geom, ks[0], ks[-1])
            assert forms[R.K_REFUSED][0] == "refused" and forms[R.K_MAX_SERVED][0] == "mem"
            assert {f[:2] for f in forms.values()} - {("none", None), ("refused", None)} == {(fam, g) for _, fam, g in rows}     # nothing left out
        assert {k for lohi, _, _ in rows for k in lohi} - {1024} == set(R.EDGE_KS) - {2, 3}         # (2, 3: the issue's list, inside the first form)
    # what the issue's K-range table calls "MFMA (16, 12)" and "(32, 24)" is the group kernel in the forward direction, by default
    assert R.form("pd", 9, dt, False)[0] == "grp" and R.form("pd", 24, dt, False)[0] == "grp"
    assert R.form("pd", 13, dt, False)[0] == ("mfma_fwd" if dt == R.F32 else "grp")
    assert R.form("pd", 49, R.F64, True)[1] == (64, 64, 128) and R.form("pd", 48, R.F64, True)[1] == (64, 48, 256) and R.form("pd", 49, R.F32, True)[1] == (64, 64, 256)


def test_every_staging_row_reaches_its_width_with_the_offset_on_each_pointer_and_on_all():
    seen = set()
    for dt, dirs, ks, kinds, off, family, width in R.STAGING:
        assert off == 0 or off in R.STAGING_OFFSETS[dt]
        for inverse in dirs:
            for K in ks:
                assert K in R.STAGING_KS
                for kind in kinds:
                    for offs in (((0, 0, 0),) if off == 0 else R.offset_patterns(off)):
                        fm = R.form(kind, K, dt, bool(inverse), *offs)
                        assert (fm[0], fm[2]) == (family, width), (dt.name, inverse, K, kind, offs, fm)
                        seen.add((dt, bool(inverse), K, kind, off))
    # every (dtype, direction, K, kind, offset) of the staging test has a row
    want = {(dt, inv, K, kind, off) for dt in R.DTS for inv in (True, False) for K in R.STAGING_KS for kind in R.KINDS for off in (0,) + R.STAGING_OFFSETS[dt]}
    assert seen == want, sorted(want - seen)[:5]
    # every width a dispatcher can choose is in the table: V = pack / 1 of the lane kernel, VWT = pack / 2 / 1, VEC true / false —
    # also at a K that is a whole number of packs, where only an unaligned or 8-byte-aligned base reaches the narrow ones
    got = {(dt, fam, w) for dt, _, _, _, _, fam, w in R.STAGING}
    assert got >= {(R.F32, "lane", 4), (R.F32, "lane", 1), (R.F64, "lane", 2), (R.F64, "lane", 1), (R.F32, "mfma_inv", 4), (R.F32, "mfma_inv", 2),
                   (R.F32, "mfma_inv", 1), (R.F64, "mfma_inv", 2), (R.F64, "mfma_inv", 1), (R.F32, "mfma_fwd", 4), (R.F32, "mfma_fwd", 1),
                   (R.F64, "mfma_fwd", 2), (R.F64, "mfma_fwd", 1), (R.F32, "grp", 1), (R.F64, "grp", 1)}
    for K in (16, 64):
        assert R.form("pd", K, R.F32, True, 2, 0, 0)[2] == 2 and R.form("pd", K, R.F32, True, 0, 0, 1)[2] == 1 and R.form("pd", K, R.F32, False, 0, 1, 0)[2] == 1
    # a scan: the table's widths are all the widths there are
    for dt in R.DTS:
        for inverse in (True, False):
            ws = {(R.form(kind, K, dt, inverse, o, 0, 0)[0], R.form(kind, K, dt, inverse, o, 0, 0)[2]) for kind in R.KINDS for K in range(2, 65) for o in (0, 1, 2)}
            assert ws == {(fam, w) for d, dirs, _, _, _, fam, w in R.STAGING if d == dt and int(inverse) in dirs}, (dt.name, inverse)


def test_trip_and_alias_shapes_reach_one_form_each_at_its_smallest_k():
    for dt in R.DTS:
        for inverse in (True, False):
            geoms = [R.form("pd", K, dt, inverse)[:2] for K in R.TRIP_KS]
            assert len(set(geoms)) == len(R.TRIP_KS)
            assert set(geoms) == {(fam, g) for _, fam, g in R.FORM_EDGES[(dt, inverse)] if fam != "mem"}
            assert sorted(R.TRIP_KS) == sorted(max(lo, 2) for (lo, _), fam, _ in R.FORM_EDGES[(dt, inverse)] if fam != "mem")
        assert {R.form("pd", K, dt, True)[0] for K in R.ALIAS_KS} == {"lane", "mfma_inv", "mem"}
        assert {R.form("pd", K, dt, False)[0] for K in R.ALIAS_KS} == {"lane", "grp", "mfma_fwd", "mem"}
        assert R.form("pd", R.ALIAS_TRIP_K, dt, True)[0] == "mfma_inv" and R.form("pd", R.ALIAS_TRIP_K, dt, False)[0] == "grp"
    assert R.form("pd_vec", R.MEM_K, R.F32, True)[0] == R.form("pd_vec", R.MEM_K, R.F32, False)[0] == "mem"


def test_edge_batches_name_the_edges_of_a_block():
    assert R.edge_batches(("lane", (1, 4, 64), 4)) == (1, 63, 64, 65, 129)
    assert R.edge_batches(("mfma_inv", (16, 12, 256), 4)) == (1, 15, 16, 17)
    assert R.edge_batches(("grp", (32, 24, 256), 1)) == (1, 7, 8, 9)
    assert R.edge_batches(("mfma_fwd", (64, 48, 256), 4)) == (1, 3, 4, 5)
    assert R.edge_batches(("mfma_inv", (64, 64, 128), 2)) == (1, 2, 3)
    assert R.edge_batches(("mem", (1, 0, 64), 1)) == (1, 63, 65)


# ------------------------------------------------------------------ the tiled batch and the trip sizes
def test_tiled_index_map_and_reference():
    for D, batch in ((37, 37), (37, 38), (37, 8197), (5, 3), (64, 1000)):
        idx = R.tiled_index(D, batch)
        assert idx.shape == (batch,) and idx.dtype == np.int64 and idx.min() == 0 and idx.max() == min(D, batch) - 1
        assert np.array_equal(idx[:min(D, batch)], np.arange(min(D, batch))) and np.array_equal(idx[D:], idx[:max(batch - D, 0)])
    a, g, l, idx = R.tiled("vec_corr", "float64", 5, 7, 23, True)
    assert a.shape == (10, 7) and g.shape == (5, 5, 7) and l.shape == (7,) and idx.shape == (23,)
    full = R.ref_vjp("vec_corr", a[:, idx], g[:, :, idx], l[idx], True)
    assert np.array_equal(full, R.ref("vec_corr", "float64", 5, 7, True)[:, idx])          # the reference of the tiled batch is the tiled reference
    # coprime to every samples-per-block: a distinct sample visits every slot of a block
    spbs = {R.samples_per_block(R.form("pd", K, dt, inv)) for K in R.TRIP_KS for dt in R.DTS for inv in (True, False)}
    assert spbs == {64, 16, 8, 4, 2} and all(math.gcd(R.TRIP_D, s) == 1 for s in spbs)
    for s in spbs:
        assert {(i % s, int(d)) for i, d in enumerate(R.tiled_index(R.TRIP_D, R.TRIP_D * s))} == {(a_, b_) for a_ in range(s) for b_ in range(R.TRIP_D)}


@pytest.mark.parametrize("cus", CUS)
def test_second_trip_batch_exceeds_every_possible_residency(cus):
    for dt in R.DTS:
        for inverse in (True, False):
            for K in R.TRIP_KS:
                fm = R.form("pd", K, dt, inverse)
                family, geom, _ = fm
                b = R.second_trip_batch(fm, cus)
                spb = R.samples_per_block(fm)
                if family == "lane":
                    cap = 32 * cus                                       # matrix_vjp_impl: 32 tiles a CU, whatever is resident
                    assert b > 2 * cap * 64 and (b - 2 * cap * 64) == 65          # a third trip of two blocks, the last with one sample
                    continue
                GS, _, NT = geom
                for per_cu in range(1, 32 * 64 // NT + 1):                        # 32 waves a CU: no more blocks of NT threads can be resident
                    assert b > cus * per_cu * spb, (K, dt.name, inverse, per_cu)
                assert 2048 % NT == 0 and b - cus * (2048 // NT) * spb == spb + 1       # one full block more, and one sample
                assert (b % spb) == 1 and (b - 1) // spb >= 1
    for dt in R.DTS:
        fm = R.form("pd_vec", R.MEM_K, dt, True)
        b = R.second_trip_batch(fm, cus, R.MEM_K, dt)
        blocks = R.mem_blocks_cap(R.MEM_K, dt, cus)
        assert b == blocks * 64 + 1 and blocks * 64 * 2 * R.MEM_K * R.MEM_K * dt.itemsize <= R.MEM_WS_BYTES and blocks <= 16 * cus
    assert R.mem_blocks_cap(65, R.F32, 256) == 248 and R.mem_blocks_cap(65, R.F64, 256) == 124 and R.mem_blocks_cap(1024, R.F64, 256) == 1
    assert R.second_trip_batch(R.form("pd", 9, R.F32, True), 256) == 32785 and R.second_trip_batch(R.form("pd", 49, R.F64, True), 256) == 8195
    assert R.second_trip_batch(R.form("pd", 2, R.F32, True), 256) == 1048641


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dt", R.DTS, ids=lambda d: d.name)
def test_every_input_and_reference_is_finite_and_the_unread_triangle_is_zero(orc, dt, kind):
    for kind, K, batch in _table_draws(dt, (kind,)):
        d = R.draw(kind, dt.name, K, batch)
        assert all(a.dtype == dt and np.isfinite(a).all() for a in d.values()), (kind, K)
        n_in, n_out = R.sizes(kind, K, True)
        assert d["y"].size == (n_in if kind in R.PACKED else K * K) * batch and d["X"].shape == (K, K, batch) and d["ybar"].shape == d["y"].shape
        for inverse in (True, False):
            for with_l in (True, False):
                out = R.ref(kind, dt.name, K, batch, inverse, with_l)
                assert out.dtype == np.float64 and np.isfinite(out).all() and out.shape == (d["y"].shape if inverse else d["X"].shape), (kind, K, inverse)
                if not inverse and K > 1:
                    assert (out[R.unread_triangle(kind, K)] == 0).all(), (kind, K)


def test_float32_oracle_of_the_inverse_pullback_is_within_a_tenth_of_the_bar(orc):
    worst = {}
    for kind, K, batch in _table_draws(R.F32):
        a, g, l = R.operands(kind, "float32", K, batch, True)
        if a.size == 0:
            continue
        g32 = orc.matrix_bijector_vjp(kind, a, g, l, inverse=True)
        assert g32.dtype == np.float32
        e = _sample_err(g32, R.ref(kind, "float32", K, batch, True))
        assert e <= TENTH, f"{kind} K={K}: the Float32 oracle is {e:.3g} of the sample's scale off the Float64 one (a tenth of the bar: {TENTH:g})"
        worst[kind] = max(worst.get(kind, 0.0), e)
    print("Float32 oracle vs Float64 oracle, inverse pullback, worst per kind:", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("kind", R.KINDS)
def test_forward_pullback_moves_less_than_a_tenth_of_the_bar_under_a_one_ulp_perturbation(orc, kind):
    """the forward oracle computes in Float64 whatever it is given, so the conditioning of a draw is measured on the data: three random
    symmetric relative perturbations of X of one Float32 ulp"""
    a, g, l = R.operands("pd", "float32", 4, 5, False)
    assert orc.matrix_bijector_vjp("pd", a, g, l, inverse=False).dtype == np.float64
    eps = float(np.finfo(np.float32).eps)
    worst = {}
    for kind, K, batch in _table_draws(R.F32, (kind,)):
        X, g, l = R.operands(kind, "float32", K, batch, False)
        base = R.ref(kind, "float32", K, batch, False)
        r = R.rng_for("perturb", kind, K, batch)
        X64 = R.f64(X)
        e = 0.0
        for _ in range(3):
            P = 1.0 + eps * r.uniform(-1.0, 1.0, size=X64.shape)
            P = 0.5 * (P + P.transpose(1, 0, 2))
            e = max(e, _sample_err(R.ref_vjp(kind, X64 * P, g, l, False), base))
        assert e <= TENTH, f"{kind} K={K} batch={batch}: the forward pullback moves by {e:.3g} of the sample's scale under a 1-ulp perturbation of X: redraw (RESEED)"
        worst[kind] = max(worst.get(kind, 0.0), e)
    print("forward pullback under 1-ulp(Float32) perturbations of X, worst per kind:", {k: f"{v:.2e}" for k, v in worst.items()})
