"""The pullbacks of the four matrix-variate bijectors — bjx_vec_corr_vjp, bjx_corr_vjp, bjx_pd_vjp, bjx_pd_vec_vjp of include/bjx.h —
through the C ABI at every kernel form, staging width and loop trip that their dispatchers (matrix_vjp_impl in csrc/bjx_matrix_vjp.hip,
bjx_matrix_vjp_grp, bjx_matrix_inv_vjp_mfma / mf_kind / mf_launch, bjx_matrix_fwd_vjp_mfma / fw_kind / fw_launch) choose among, against
the Float64 oracle on the dt-rounded inputs (tests/_matrix_vjp_ref.py: draws, reference, `form`, the tables;
tests/test_host_matrix_vjp_ref.py checks on the CPU that every table row reaches the form written next to it and that the draws
measure the kernel, not their own conditioning).  Default tuning switches only; no subprocess, no environment variable.

Which shape reaches which instantiation (all four kinds; SPB = samples per block):
  K = 1 … 4 | 5 … 8     matrix_lane_vjp_kernel<T, KMAX = 4 | 8, KIND, INV, V>, both directions; V = pack aligned, 1 with any pointer offset;
                        SPB = 64.  (K = 1 of VecCorr: inverse has nothing to differentiate, forward takes out_bar = NULL.)
  K = 9 … 64, inverse   matrix_inv_vjp_mfma_kernel<T, GS, KMAX, KIND, VWT, NT>: (GS, KMAX) = (16, 12) at 9 … 12, (16, 16) at 13 … 16,
                        (32, 24) at 17 … 24, (32, 32) at 25 … 32, (64, 48) at 33 … 48, (64, 64) at 49 … 64; NT = 256, Float64 (64, 64): 128;
                        SPB = NT / GS = 16, 16, 8, 8, 4, 4 | 2.  VWT = pack with K and the free length whole packs and 16-byte bases
                        (K = 16, 24, 32, 48, 64; 12 for the dense kinds), 2 (Float32: even K and free length, 8-byte bases — K = 12 packed
                        kinds, K = 10, 14 dense kinds, every pack K with an offset of 2), else 1.
  K = 9 … 64, forward   matrix_fwd_vjp_mfma_kernel<T, GS, KMAX, KIND, VEC, NT> at K = 13 … 16 (Float32 only) and 25 … 64, the same
                        (GS, KMAX, NT); VEC where VWT would be a pack.  matrix_grp_vjp_kernel<T, GS, KMAX, KIND, false> — by DEFAULT, not
                        only behind a switch — at K = 9 … 12 and 17 … 24 (Float64: 9 … 24): 256 threads, one element per lane, no loop.
  K = 65 … 1024         matrix_mem_vjp_kernel<T, KIND, INV> (K = 65 here); 1025: BJX_ERR_UNSUPPORTED.
Tests: (a) test_form_edges_and_batch_edges — K = 1, 2, 3, 4 | 5, 8 | 9, 12 | 13, 16 | 17, 24 | 25, 32 | 33, 48 | 49, 64 | 65 at batches
1, 63, 64, 65, 129 (lane), 1, SPB − 1, SPB, SPB + 1 (group forms), 1, 63, 65 (K = 65), with ladj_bar, with NULL and with zeros (the
bits of NULL); (b) test_staging_width_… — offsets of 1, 2 (Float64: 1) elements on each pointer alone and on all three at K = 4, 8,
10, 12, 14, 16, 24, 32, 48, 64: the width asserted with `form`, the bits of the aligned call; (c) test_second_trip_… — one case per form
at its smallest K (2, 5, 9, 13, 17, 25, 33, 49), vec_corr and pd, `second_trip_batch` samples tiled on the device from 37 distinct
ones, and the workspace kernel at K = 65, pd_vec, Float32 with 248·64 + 1 samples (measured alone on the MI355X: 0.54 s inverse,
0.24 s forward, so it stays); (d) test_a_sample_gives_the_same_bits_… — alone and at every index of SPB + 1; (e) test_in_bar_may_alias_in
— K = 4, 12, 32, 64, 65, and the trip batch at K = 12; (f) batch = 0, K = 1 of VecCorr, K = 0, batch = −1, NULL pointers, a bad dtype,
K = 1025 and an ordinary call after it.

What every comparison asserts: in_bar is a view into a marker-filled buffer one sample longer (one marker element in front when
offset), all markers intact; every call is made twice and gives identical bits; `_tol.flat_close(per="sample")`, the flat 1e-3 / 1e-6
of the sample's max-norm with no growth factor; forward results exactly zero on the triangle the reference does not read.  Bitwise
equality — offset forms with the aligned call, a sample at every index, in_bar == in with the out-of-place call, every later copy of
a tiled sample with its first — holds at EVERY form: staging changes addresses, not arithmetic, in all five kernels.

Worst measured |got − ref| / scale (MI355X, 256 CUs, from the error log that tests/_tol.py writes; the bar is 1e-3 | 1e-6), Float32 | Float64:
  lane      inverse 6.7e-5 | 6.4e-14 (offset forms 6.1e-7 | 1.3e-15, the million-sample trips 1.4e-6 | 2.0e-14)
            forward 3.3e-5 | 3.3e-13 (offset 2.0e-5 | 3.3e-13, trips 3.5e-6 | 3.2e-15)
  mfma_inv  inverse 9.5e-7 | 1.2e-15 (offset, VWT = 2 and 1 included, 9.5e-7 | 1.2e-15, trips 6.3e-7 | 1.2e-15)
  mfma_fwd  forward 1.2e-4 | 2.1e-13 (offset, VEC = false, 4.8e-5 | 1.6e-13, trips 7.5e-5 | 1.2e-13); by K: 16 2.4e-5, 25 6.1e-5,
            32 1.2e-4, 33 7.5e-5, 48 3.8e-5, 49 2.7e-5, 64 9.8e-5
  grp       forward 9.0e-5 | 9.9e-14 (offset 3.2e-5 | 9.0e-14, trips 3.5e-5 | 2.0e-13)
  mem K=65  inverse 1.0e-6 | 2.2e-15, forward 8.3e-5 | 1.6e-13, trips (Float32) 4.6e-7 / 2.6e-5 — first measurements of this kernel;
            the Float32 forward pullback at 65 rows sits where the 64-row MFMA form does, no `grow=` needed
No defect found.  The whole file: 326 tests, 25 s on the MI355X, no test above 1.2 s (K = 65: the oracle's Python loops)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _matrix_vjp_ref as R  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, host  # noqa: E402,F401

MARK = 7.25
DT_IDS = [dt.name for dt in R.DTS]
DIRS = (True, False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dir(inverse):
    return "inverse" if inverse else "forward"


def _name(fm):
    family, geom, width = fm
    return f"{family}{geom} w={width}".replace(" ", "", 2)


class _Guard:
    """`per`·batch elements behind `off` marker elements, one more sample (at least one element) of markers behind them"""

    def __init__(self, c, per, batch, off=0):
        self.n, self.off = per * batch, off
        self.buf = torch.full((off + self.n + max(per, 1),), MARK, dtype=c.tdt, device="cuda")
        self.view = self.buf[off:]

    def intact(self, written=True):
        return bool((self.buf[:self.off] == MARK).all()) and bool((self.buf[self.off + (self.n if written else 0):] == MARK).all())


class _Call:
    def __init__(self, bj, dt):
        self.L = bj._lib
        self.lib = self.L.load()
        self.ctx = bj.context()
        self.dt = np.dtype(dt)
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dtc = self.L.BJX_F32 if self.dt == np.float32 else self.L.BJX_F64
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count

    def fn(self, kind):
        return getattr(self.lib, f"bjx_{kind}_vjp")

    def flat(self, a):
        """a column-major array -> its elements in memory order on the device (None for an array without elements)"""
        a = np.asarray(a, self.dt)
        return torch.from_numpy(np.array(a.reshape(-1, order="F"))).cuda() if a.size else None

    def at(self, flat, off=0):
        """a flat device tensor -> the same elements `off` elements into a marker-filled buffer (16-byte aligned base + off elements)"""
        if flat is None:
            return None
        buf = torch.full((flat.numel() + off,), MARK, dtype=self.tdt, device="cuda")
        buf[off:] = flat
        return buf[off:]

    def run(self, kind, inverse, a, g, l, K, batch, offs=(0, 0, 0), alias=False, twice=True, what=""):
        """bjx_<kind>_vjp on flat device tensors (`g`, `l` may be None), twice by default (identical bits), guards checked
        -> in_bar, flat on the device.  `alias`: in_bar == in (the input is copied behind the guard's markers first)."""
        n_in, _ = R.sizes(kind, K, inverse)
        a_d, g_d = (None if alias else self.at(a, offs[0])), self.at(g, offs[1])
        runs = []
        for _ in range(2 if twice else 1):
            o = _Guard(self, n_in, batch, offs[2])
            if alias:
                o.view[:o.n] = a
            rc = self.fn(kind)(self.ctx.h, self.dtc, int(inverse), _p(o.view if alias else a_d), _p(g_d), _p(l), _p(o.view), K, batch)
            self.L.check(self.ctx.h, rc, f"bjx_{kind}_vjp")
            runs.append(o)
        torch.cuda.synchronize()
        if twice:
            assert torch.equal(runs[0].buf, runs[1].buf), f"{what}: in_bar not repeatable"
        assert runs[0].intact(), f"{what}: wrote outside in_bar"
        return runs[0].view[:runs[0].n]

    def shape(self, kind, K, batch, inverse):
        return (R.free_len(kind, K), batch) if inverse and kind in R.PACKED else (K, K, batch)

    def np(self, flat, kind, K, batch, inverse):
        return host(flat).reshape(self.shape(kind, K, batch, inverse), order="F")


def _first(a, b):
    """the first b samples of a column-major operand"""
    return np.asfortranarray(a[..., :b])


def _check_forward_zero(got, kind, K, what):
    if K > 1:
        assert (got[R.unread_triangle(kind, K)] == 0).all(), f"{what}: the triangle the reference does not read is not exactly zero"


# ------------------------------------------------------------------ a. form edges, every pointer aligned
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("K", R.EDGE_KS)
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_form_edges_and_batch_edges(bj, dt, K, kind):
    """K lo and K hi of every form at the batches of `edge_batches`; with `ladj_bar`, with NULL, and with zeros (the bits of NULL).  The
    operands of a smaller batch are the first samples of the largest one: one reference per (kind, K, direction)."""
    c = _Call(bj, dt)
    for inverse in DIRS:
        fm = R.form(kind, K, dt, inverse)
        if fm[0] == "none":
            continue
        bs = R.edge_batches(fm)
        a, g, l = R.operands(kind, dt.name, K, bs[-1], inverse)
        ref_l, ref_0 = R.ref(kind, dt.name, K, bs[-1], inverse), R.ref(kind, dt.name, K, bs[-1], inverse, False)
        for b in bs:
            what = f"matrix_vjp_abi edges {_name(fm)} {kind} {_dir(inverse)} {dt.name} K={K} batch={b}"
            a_d, g_d, l_d = c.flat(_first(a, b)), c.flat(_first(g, b)), c.flat(l[:b])
            got = c.np(c.run(kind, inverse, a_d, g_d, l_d, K, b, what=what), kind, K, b, inverse)
            flat_close(got, ref_l[..., :b], c.dt, what, per="sample")
            r0 = c.run(kind, inverse, a_d, g_d, None, K, b, what=f"{what} ladj_bar=NULL")
            got0 = c.np(r0, kind, K, b, inverse)
            flat_close(got0, ref_0[..., :b], c.dt, f"{what} ladj_bar=NULL", per="sample")
            rz = c.run(kind, inverse, a_d, g_d, torch.zeros(b, dtype=c.tdt, device="cuda"), K, b, what=f"{what} ladj_bar=0")
            assert torch.equal(rz, r0), f"{what}: ladj_bar = NULL does not give the bits of a ladj_bar of zeros"
            if not inverse:
                _check_forward_zero(got, kind, K, what)
                _check_forward_zero(got0, kind, K, what)


# ------------------------------------------------------------------ b. staging widths
STAGING_CASES = [(dt, inv, K, off) for dt in R.DTS for inv in DIRS for K in R.STAGING_KS for off in R.STAGING_OFFSETS[dt]]


def _staging_row(dt, inverse, K, kind, off):
    rows = [(fam, w) for d, dirs, ks, kinds, o, fam, w in R.STAGING if d == dt and int(inverse) in dirs and K in ks and kind in kinds and o == off]
    assert len(rows) == 1, (dt, inverse, K, kind, off, rows)
    return rows[0]


@pytest.mark.parametrize("dt,inverse,K,off", STAGING_CASES, ids=[f"{dt.name}-{_dir(inv)}-{K}-off{off}" for dt, inv, K, off in STAGING_CASES])
def test_staging_width_changes_addresses_not_arithmetic(bj, dt, inverse, K, off):
    """`off` elements on `in`, on `out_bar`, on `in_bar` alone and on all three: the width R.STAGING names (asserted with R.form), the bits
    of the aligned call of the same data, and the oracle within the bar.  One block plus one sample (a full tile plus one at K <= 8)."""
    c = _Call(bj, dt)
    for kind in R.KINDS:
        fm0 = R.form(kind, K, dt, inverse)
        assert (fm0[0], fm0[2]) == _staging_row(dt, inverse, K, kind, 0)
        b = R.samples_per_block(fm0) + 1
        a, g, l = R.operands(kind, dt.name, K, b, inverse)
        a_d, g_d, l_d = c.flat(a), c.flat(g), c.flat(l)
        ref = R.ref(kind, dt.name, K, b, inverse)
        what = f"matrix_vjp_abi staging {_name(fm0)} {kind} {_dir(inverse)} {dt.name} K={K} batch={b}"
        r0 = c.run(kind, inverse, a_d, g_d, l_d, K, b, what=what)
        flat_close(c.np(r0, kind, K, b, inverse), ref, c.dt, what, per="sample")
        for offs in R.offset_patterns(off):
            fm = R.form(kind, K, dt, inverse, *offs)
            assert (fm[0], fm[2]) == _staging_row(dt, inverse, K, kind, off) and fm[1] == fm0[1], (kind, offs, fm)
            w2 = f"matrix_vjp_abi staging {_name(fm)} {kind} {_dir(inverse)} {dt.name} K={K} batch={b} offsets={offs}"
            r = c.run(kind, inverse, a_d, g_d, l_d, K, b, offs=offs, what=w2)
            flat_close(c.np(r, kind, K, b, inverse), ref, c.dt, w2, per="sample")
            assert torch.equal(r, r0), f"{w2}: not the bits of the aligned call ({_name(fm0)})"


# ------------------------------------------------------------------ c. the second trip of every persistent loop
def _trip(c, kind, K, inverse, batch, fm, alias=False, tag="trips"):
    """a batch tiled on the device from R.TRIP_D distinct samples: the first copies against the oracle, every later copy the bits of its
    first copy, guards intact, two calls identical"""
    D = R.TRIP_D
    a, g, l, idx = R.tiled(kind, c.dt.name, K, D, batch, inverse)
    n_in, n_out = R.sizes(kind, K, inverse)
    idx_d = torch.from_numpy(idx).cuda()
    tile = lambda x, n: c.flat(x).view(D, n).index_select(0, idx_d).reshape(-1)
    what = f"matrix_vjp_abi {tag} {_name(fm)} {kind} {_dir(inverse)} {c.dt.name} K={K} batch={batch}"
    r = c.run(kind, inverse, tile(a, n_in), tile(g, n_out), tile(l, 1), K, batch, alias=alias, what=what).view(batch, n_in)
    flat_close(c.np(r[:D].reshape(-1), kind, K, D, inverse), R.ref(kind, c.dt.name, K, D, inverse), c.dt, what, per="sample")
    same = (r == r[:D].index_select(0, idx_d)).all(dim=1)
    assert bool(same.all()), f"{what}: sample {int((~same).nonzero()[0])} (+{int((~same).sum()) - 1} more) differs from the first copy of its data"
    return r


@pytest.mark.parametrize("inverse", DIRS, ids=_dir)
@pytest.mark.parametrize("kind", R.TRIP_KINDS)
@pytest.mark.parametrize("K", R.TRIP_KS)
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_second_trip_of_the_persistent_loop(bj, dt, K, kind, inverse):
    """R.second_trip_batch: more samples than cus · (2048 / NT) blocks hold — a bound from 32 waves a CU, not from the library — plus one
    block and one sample (lane kernel: twice its grid cap plus 65).  The group kernel (forward, K = 9, 17; Float64 also 13) has no loop:
    the same batch is a grid of that many blocks."""
    c = _Call(bj, dt)
    fm = R.form(kind, K, dt, inverse)
    _trip(c, kind, K, inverse, R.second_trip_batch(fm, c.cus), fm)


@pytest.mark.parametrize("inverse", DIRS, ids=_dir)
def test_second_trip_of_the_workspace_kernel(bj, inverse):
    """matrix_mem_vjp_kernel at K = 65, pd_vec, Float32: blocks·64 + 1 samples, blocks = min(512 MiB / (2·K²·4·64), 16·cus) = 248 at 256
    CUs — lane 0 of block 0 takes a second trip on the same slice of the workspace."""
    c = _Call(bj, R.F32)
    fm = R.form("pd_vec", R.MEM_K, R.F32, inverse)
    assert fm[0] == "mem"
    _trip(c, "pd_vec", R.MEM_K, inverse, R.second_trip_batch(fm, c.cus, R.MEM_K, R.F32), fm)


# ------------------------------------------------------------------ d. position independence
POSITION_KS = tuple(K for K in R.EDGE_KS if K not in (1, 3))


@pytest.mark.parametrize("K", POSITION_KS)
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_a_sample_gives_the_same_bits_alone_and_at_every_index_of_a_block_plus_one(bj, dt, K):
    """sample 0 alone, and in place of sample j (which takes its place) of a batch of samples-per-block + 1 of other data, for every j:
    LDS of neighbouring groups that overlapped, or an MFMA block that read a neighbour's rows, would change its bits.  (Workspace
    kernel, 50 ms a launch: j = 0, 63, 64 — the first and the last lane of block 0, and block 1.)"""
    c = _Call(bj, dt)
    for kind in R.KINDS:
        for inverse in DIRS:
            fm = R.form(kind, K, dt, inverse)
            B = R.samples_per_block(fm) + 1
            n_in, n_out = R.sizes(kind, K, inverse)
            a, g, l = (c.flat(x) for x in R.operands(kind, dt.name, K, B, inverse))
            a, g, l = a.view(B, n_in), g.view(B, n_out), l.view(B, 1)
            what = f"matrix_vjp_abi position {_name(fm)} {kind} {_dir(inverse)} {dt.name} K={K}"
            r0 = c.run(kind, inverse, a[:1].reshape(-1), g[:1].reshape(-1), l[:1].reshape(-1), K, 1, twice=False, what=what)
            for j in ((0, 63, 64) if fm[0] == "mem" else range(B)):
                perm = torch.arange(B, device="cuda")
                perm[0], perm[j] = j, 0
                r = c.run(kind, inverse, a[perm].reshape(-1), g[perm].reshape(-1), l[perm].reshape(-1), K, B, twice=False, what=what)
                assert torch.equal(r.view(B, n_in)[j], r0), f"{what}: the result of a sample differs at index {j} of a batch of {B}"


# ------------------------------------------------------------------ e. in_bar == in
@pytest.mark.parametrize("K", R.ALIAS_KS)
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_in_bar_may_alias_in(bj, dt, K):
    """include/bjx.h: "in_bar may alias in".  The same pointer for both: the bits of the out-of-place call, at one block plus one sample
    (every family, both directions) and, at K = 12, at the trip batch (the prefetch of the next sample reads `in` while the current
    one is written to in_bar)."""
    c = _Call(bj, dt)
    for kind in R.KINDS:
        for inverse in DIRS:
            fm = R.form(kind, K, dt, inverse)
            b = R.samples_per_block(fm) + 1
            a, g, l = (c.flat(x) for x in R.operands(kind, dt.name, K, b, inverse))
            what = f"matrix_vjp_abi alias {_name(fm)} {kind} {_dir(inverse)} {dt.name} K={K} batch={b}"
            r0 = c.run(kind, inverse, a, g, l, K, b, what=what)
            flat_close(c.np(r0, kind, K, b, inverse), R.ref(kind, dt.name, K, b, inverse), c.dt, what, per="sample")
            ra = c.run(kind, inverse, a, g, l, K, b, alias=True, what=f"{what} in_bar == in")
            assert torch.equal(ra, r0), f"{what}: in_bar == in does not give the bits of the out-of-place call"
            if K == R.ALIAS_TRIP_K and kind in R.TRIP_KINDS:
                batch = R.second_trip_batch(fm, c.cus)
                assert torch.equal(_trip(c, kind, K, inverse, batch, fm, alias=True, tag="alias-trips"), _trip(c, kind, K, inverse, batch, fm, tag="alias-trips"))


# ------------------------------------------------------------------ f. edges of the contract
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_empty_batch_and_vec_corr_of_one_row(bj, orc, dt):
    c = _Call(bj, dt)
    for kind in R.KINDS:
        for inverse in (0, 1):
            assert c.fn(kind)(c.ctx.h, c.dtc, inverse, None, None, None, None, 12, 0) == 0
            o = _Guard(c, 144, 3)
            a, g, l = (c.flat(x) for x in R.operands(kind, dt.name, 12, 3, bool(inverse)))
            assert c.fn(kind)(c.ctx.h, c.dtc, inverse, _p(a), _p(g), _p(l), _p(o.view), 12, 0) == 0
            torch.cuda.synchronize()
            assert o.intact(False), f"{kind} {inverse}: batch = 0 wrote"
    # VecCorr, K = 1: no free parameter
    for batch in (1, 5):
        o = _Guard(c, 1, batch)
        n0 = c.lib.bjx_launch_count()
        assert c.fn("vec_corr")(c.ctx.h, c.dtc, 1, None, None, None, None, 1, batch) == 0
        assert c.fn("vec_corr")(c.ctx.h, c.dtc, 1, None, _p(c.at(torch.ones(batch, dtype=c.tdt, device="cuda"))), None, _p(o.view), 1, batch) == 0
        torch.cuda.synchronize()
        assert o.intact(False) and c.lib.bjx_launch_count() == n0, "inverse VecCorr at K = 1 touched something"
        X = np.ones((1, 1, batch), c.dt)
        lb = R.rng_for("k1", dt.name, batch).normal(size=batch).astype(c.dt)
        for l in (None, lb):
            want = orc.matrix_bijector_vjp("vec_corr", R.f64(X), np.zeros((0, batch)), None if l is None else l.astype(np.float64), inverse=False)
            got = c.run("vec_corr", False, c.flat(X), None, None if l is None else c.flat(l), 1, batch, what=f"vec_corr forward K=1 batch={batch} out_bar=NULL")
            assert np.array_equal(c.np(got, "vec_corr", 1, batch, False), want)


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_refusals_write_nothing_and_leave_the_context_usable(bj, dt):
    c = _Call(bj, dt)
    K, batch = 12, 3
    for kind in R.KINDS:
        for inverse in (0, 1):
            a, g, l = (c.at(c.flat(x)) for x in R.operands(kind, dt.name, K, batch, bool(inverse)))
            o = _Guard(c, K * K, batch)
            f = c.fn(kind)
            n0 = c.lib.bjx_launch_count()
            assert f(c.ctx.h, c.dtc, inverse, _p(a), _p(g), _p(l), _p(o.view), 0, batch) == c.L.ERR_SHAPE
            assert f(c.ctx.h, c.dtc, inverse, _p(a), _p(g), _p(l), _p(o.view), K, -1) == c.L.ERR_SHAPE
            assert f(c.ctx.h, c.dtc, inverse, None, _p(g), _p(l), _p(o.view), K, batch) == c.L.ERR_ARG
            assert f(c.ctx.h, c.dtc, inverse, _p(a), None, _p(l), _p(o.view), K, batch) == c.L.ERR_ARG
            assert f(c.ctx.h, c.dtc, inverse, _p(a), _p(g), _p(l), None, K, batch) == c.L.ERR_ARG
            assert f(c.ctx.h, 7, inverse, _p(a), _p(g), _p(l), _p(o.view), K, batch) == c.L.ERR_ARG
            assert f(None, c.dtc, inverse, _p(a), _p(g), _p(l), _p(o.view), K, batch) == c.L.ERR_ARG
            assert f(c.ctx.h, c.dtc, inverse, _p(a), _p(g), _p(l), _p(o.view), R.K_REFUSED, 1) == c.L.ERR_UNSUPPORTED      # refused before anything is read
            assert str(R.K_REFUSED) in c.lib.bjx_last_error(c.ctx.h).decode()
            torch.cuda.synchronize()
            assert o.intact(False) and c.lib.bjx_launch_count() == n0, f"{kind} {inverse}: a refused call launched or wrote"
            # the context is still usable: one ordinary call
            what = f"matrix_vjp_abi after-refusal {kind} {_dir(inverse)} {dt.name} K={K} batch={batch}"
            got = c.run(kind, bool(inverse), *(c.flat(x) for x in R.operands(kind, dt.name, K, batch, bool(inverse))), K, batch, what=what)
            flat_close(c.np(got, kind, K, batch, bool(inverse)), R.ref(kind, dt.name, K, batch, bool(inverse)), c.dt, what, per="sample")
