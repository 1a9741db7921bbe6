"""bjx_ordered, bjx_simplex, bjx_ordered_ld, bjx_simplex_ld, bjx_ordered_vjp and bjx_simplex_vjp of include/bjx.h through the C ABI at
every kernel form, alignment, leading dimension and loop trip that their dispatchers choose among — ordered_impl, simplex_impl,
launch_quad_stream, launch_seq, launch_seq_chunk, ordered_vjp_impl, simplex_vjp_impl, launch_simplex_vjp_stream (csrc/bjx_seq.hip),
bjx_seq_tiny, bjx_seq_tiny_vjp (csrc/bjx_tiny.hip), bjx_tall_stream, bjx_tall_simplex_vjp (csrc/bjx_tall.hip) — against Float64 numpy
references of ordered.jl:36-80 and simplex.jl:47-138 and the oracle's pullbacks, ε = eps of the type (tests/_seq_ref.py: `form`,
draws, references, tables; tests/test_host_seq_ref.py proves on the CPU that every shape below reaches the form named next to it).
Default tuning switches only; no subprocess, no environment variable.

Which shape reaches which instantiation (Float32 | Float64; contiguous, 16-byte aligned unless said; VW = 4 | 2):
  transforms      K = 1 (Simplex 2) … 8     seq_tiny_kernel<T, Op, KI, KO>, 256 columns a block
                  K = 16 n | 8 n, n <= 8    quad_stream_kernel<T, VW, NP = n, Op, 1, 4, H = 1>, G = 4 (Simplex inverse: G = 2 at K = 8 n | 4 n
                                            for n = 2, 3, 4, 5, 7, 8, G = 4 at 48, 80 … 128 | 24, 40 … 64); 4·64/G columns a block.  H = 2 is
                                            not reachable with the default switches (the strip never exceeds 9 KiB at G >= 2)
                  65 … 2 048 | 65 … 512     tall_stream_kernel<T, Op, VIN, VOUT> (Simplex inverse: 129 … 512 | never), G = ceil(rows / 32 | 16),
                                            CPS = 64/G columns a set; not 1 025 … 1 228 (eff < 0.6).  VIN / VOUT false with an odd height
                                            or an offset base (K = 256, 257 offset by one element)
                  the other heights         seq_wave_kernel<T, Op, V> up to 63 rows (Simplex inverse: 127 | 97; with a leading dimension
                                            199 | 99, Simplex 195 | 97 — the last before `chunk_min`), V = 1 with an offset base or with
                                            both sides strided; beyond, seq_chunk_kernel<T, Op, V, TABLE>, C = 64 | 32 rows a chunk, V = VW
                                            only with aligned bases and whole-pack leading dimensions (its ragged-last-pack branch:
                                            bjx_simplex_ld, K = 196, 200, 201 | 98, 100, 101), TABLE = false from K = 10 242 | 5 122
  bjx_ordered_vjp 1 … 8                     ordered_vjp_tiny_kernel; with in_bar == in ordered_vjp_kernel<T, V, INV> (1 … 7 | 1 … 3 rows)
                  9 … 2 048 | 9 … 1 024     ordered_vjp_stream_kernel<T, VW, R, INV>: (G, R) = (4, 1) … (64, 1), (64, 2), (64, 4), (64, 8);
                                            (256/G)·UC columns a block; a partial last pack at K mod VW != 0 (K = 63 on an offset base)
                  beyond                    ordered_vjp_tall_kernel<T, V, INV> (V = 1 at 2 052 | 1 026 rows on an offset base); with
                                            in_bar == in ordered_vjp_column_kernel
  bjx_simplex_vjp 2 … 8                     simplex_vjp_tiny_kernel
                  16 n | 8 n (inverse 8 n | 4 n at G = 2, n = 2 … 8; 80 … 128 | 40 … 64 at G = 4)   simplex_vjp_stream_kernel<T, VW, NP, G, INV>
                  65 … 2 048 | 65 … 1 024   tall_simplex_vjp_kernel<T, INV, VK, VK1>; not 1 025 … 1 228 | 513 … 614
                  the other heights <= 64   simplex_vjp_kernel<T, V, INV> (V = 1 on an offset base — also at K = 32 | 16, which the stream
                                            kernel refuses unaligned)
                  the hole and beyond       simplex_vjp_chunk_kernel<T, INV, TABLE>, TABLE = false from K = 10 241 | 5 121
Tests: (a) test_transform_forms / test_pullback_forms — R.form_heights: lo and hi of every row of R.RANGES plus the tall kernels'
smallest, middle and largest G, the chunk walkers at rows mod C = C − 1, 0, 1, TABLE = false one row in; batches 1, group − 1, group,
group + 1; the flags (ladj_ps alone, ladj_sum alone, both, neither, BJX_ACCUMULATE on both, out = NULL) and ladj_bar given | NULL |
zeros at the largest batch; (b) test_*_offset_bases — R.ALIGN_KS, one (Float32: and two) elements on each pointer alone and on all;
(c) test_leading_dimensions — R.LD_KS x R.ld_variants at 67 columns; (d) test_*_trip* — R.TRIPS, R.TRIP3, 8·CUs + 1 columns of
ordered_vjp_tall_kernel; (e) test_*_position — a column alone and at every index of group + 1; (f) test_alias_* ; (g) test_refusals_*.

What every comparison asserts: outputs are views into marker-filled buffers one column longer (one marker element in front when
offset; with a leading dimension the rows between `rows` and `ld` of every column are markers), all markers intact; every call is
made twice and gives identical bits; values pass `_tol.flat_close(per="sample")` at the flat 1e-3 | 1e-6 of the column's max-norm
(no floor: at K = 2, where ½·Dirichlet is one point, the forward draw is (½·U(0.1, 0.9), the rest)); per-column log-dets
per="element" with floor = the largest |term| of the column's sum (an Ordered log-det is Σy and can cancel); ladj_sum `sum_close`
against the Float64 sum.  No `cond=` bar, no column left out: the draws keep the stick remainder >= 0.5.

Bitwise equality.  Offset bases and leading dimensions change addresses, not arithmetic: a call that stays in its kernel family has the
bits of the aligned | contiguous call.  Two families legitimately differ and only meet the bar: (1) an offset that moves the call to
ANOTHER family (quad frames -> wave kernel, Simplex stream -> lane kernel: other code for log and logistic); (2) the forward direction
of ordered_vjp_tall_kernel, whose suffix sum is per pack, then per wave: V = 1 associates the same terms differently than V = VW.
Strided Ordered calls are compared with each other (the contiguous call at those heights is the tall kernel's).  Position: the Float32
Simplex inverse (TSimplexInv, QSimplexInv) chooses WAVE-WIDE between the fast rounds and the NaN-exact ones, and the tall Simplex
pullback between the affine scan and the clamped rounds; on these draws (finite, no clamped row) every call makes the same choice, so
the bits are asserted there too.

Worst measured |got − ref| / scale (MI355X, 256 CUs, from the error log that tests/_tol.py writes; the bar is 1e-3 | 1e-6), Float32 | Float64,
the worse of the two directions, every section of this file:
  transforms  tiny   values 6.8e-7 | 9.5e-16, log-det 2.4e-7 | 3.7e-16      quad   values 5.2e-7 | 5.0e-16, log-det 1.8e-6 | 8.2e-16
              wave   values 5.1e-7 | 5.9e-16, log-det 1.8e-6 | 1.8e-15      tall   values 1.1e-6 | 4.7e-16, log-det 6.3e-6 | 1.7e-15
              chunk  values 2.3e-6 | 5.0e-16, log-det 2.1e-5 | 6.3e-15 (Ordered inverse at 2 112 rows: Σ of 2 111 logs in the walker's order)
  Ordered pullback   tiny 3.4e-7 | 1.3e-15, lane (in_bar == in) 1.9e-7 | 4.6e-16, stream 5.9e-7 | 3.1e-15, tall 3.7e-7 | 4.1e-15,
                     column (in_bar == in) 3.1e-6 | 5.5e-15
  Simplex pullback   tiny 2.5e-6 | 2.5e-15, lane 5.7e-7 | 1.0e-15, stream 5.5e-7 | 8.7e-16, tall 1.1e-6 | 8.7e-16, chunk 7.3e-6 | 9.3e-16
Nothing is within a factor of 40 of the bar.  Found: the aliasing contract (test_alias_in_bar_is_out_bar); no arithmetic defect.
The whole file: 65 tests — one per entry, type and direction (and span of heights), each walking its table inside, `what` naming the
case that fails — 7 543 comparisons with a reference, 18.3 s on the MI355X, no test above 1.6 s."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _seq_ref as R  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, host, sum_close  # noqa: E402,F401

MARK = 7.25
ACC = 1                     # BJX_ACCUMULATE
DT_IDS = [dt.name for dt in R.DTS]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dir(inverse):
    return "inverse" if inverse else "forward"


class _Guard:
    """`batch` columns of `rows` rows at leading dimension `ld`, behind `off` marker elements, one more column of markers behind them"""

    def __init__(self, c, rows, batch, off=0, ld=0):
        self.rows, self.ld, self.batch, self.off = rows, ld or rows, batch, off
        self.n = self.ld * batch
        self.buf = torch.full((off + self.n + max(self.ld, 1),), MARK, dtype=c.tdt, device="cuda")
        self.view = self.buf[off:]

    def cols(self):
        return self.view[:self.n].view(self.batch, self.ld)

    def data(self):
        """(batch, rows), the written part"""
        return self.cols()[:, :self.rows]

    def intact(self, written=True):
        ok = bool((self.buf[:self.off] == MARK).all()) and bool((self.view[self.n:] == MARK).all())
        if not written:
            return ok and bool((self.view[:self.n] == MARK).all())
        return ok and bool((self.cols()[:, self.rows:] == MARK).all())


class _Res:
    out = ps = sum = out_t = ps_t = None


class _Call:
    def __init__(self, bj, dt):
        self.L = bj._lib
        self.lib = self.L.load()
        self.ctx = bj.context()
        self.dt = np.dtype(dt)
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dtc = self.L.BJX_F32 if self.dt == np.float32 else self.L.BJX_F64
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count

    def dev(self, a):
        """(rows, batch) column-major numpy, or a (batch, rows) device tensor -> (batch, rows) device tensor"""
        if isinstance(a, torch.Tensor):
            return a
        return torch.from_numpy(np.array(np.asarray(a, self.dt).T, order="C")).cuda()

    def place(self, a, off=0, ld=0):
        """(batch, rows) device tensor -> the same columns `off` elements into a marker-filled buffer, at leading dimension ld"""
        batch, rows = a.shape
        ld = ld or rows
        buf = torch.full((off + ld * batch + (ld - rows),), MARK, dtype=self.tdt, device="cuda")
        buf[off:off + ld * batch].view(batch, ld)[:, :rows] = a
        return buf[off:]

    def transform(self, kind, inverse, x, K, batch, out=True, ps=True, sm=True, flags=0, off_in=0, off_out=0, ld_in=0, ld_out=0, pre_ps=None, pre_sum=None,
                  twice=True, what=""):
        """bjx_<kind> (bjx_<kind>_ld with a leading dimension) twice (identical bits), guards checked -> _Res"""
        ri, ro = R.rows_io(kind, K, inverse)
        x_d = self.place(self.dev(x), off_in, ld_in)
        use_ld = bool(ld_in or ld_out)
        fn = getattr(self.lib, f"bjx_{kind}_ld" if use_ld else f"bjx_{kind}")
        runs = []
        for _ in range(2 if twice else 1):
            o = _Guard(self, ro, batch, off_out, ld_out) if out else None
            p = _Guard(self, 1, batch) if ps else None
            s = torch.full((3,), MARK, dtype=torch.float64, device="cuda") if sm else None
            if pre_ps is not None:
                p.view[:batch] = pre_ps
            if pre_sum is not None:
                s[1] = pre_sum
            ptrs = (_p(p.view) if ps else None, _p(s[1:]) if sm else None)
            if use_ld:
                rc = fn(self.ctx.h, self.dtc, int(inverse), _p(x_d), ld_in or ri, _p(o.view), ld_out or ro, *ptrs, K, batch, flags)
            else:
                rc = fn(self.ctx.h, self.dtc, int(inverse), _p(x_d), _p(o.view) if out else None, *ptrs, K, batch, flags)
            self.L.check(self.ctx.h, rc, fn.__name__)
            runs.append((o, p, s))
        torch.cuda.synchronize()
        (o, p, s), (o2, p2, s2) = runs[0], runs[-1]
        r = _Res()
        if out:
            assert torch.equal(o.buf, o2.buf), f"{what}: out not repeatable"
            assert o.intact(), f"{what}: wrote outside out"
            r.out_t = o.data()
        if ps:
            assert torch.equal(p.buf, p2.buf), f"{what}: ladj_ps not repeatable"
            assert p.intact(), f"{what}: wrote outside ladj_ps"
            r.ps_t = p.view[:batch]
        if sm:
            assert torch.equal(s, s2), f"{what}: ladj_sum not repeatable"
            sh = host(s)
            assert sh[0] == MARK and sh[2] == MARK, f"{what}: wrote next to ladj_sum"
            r.sum = float(sh[1])
        return r

    def vjp(self, kind, inverse, a, g, l, K, batch, offs=(0, 0, 0), alias=None, twice=True, what=""):
        """bjx_<kind>_vjp on (batch, rows) device tensors / numpy (`l` may be None), offs = (in, in_bar, out_bar) -> in_bar (batch, rows_in).
        alias "in": in_bar == in; "out_bar": in_bar == out_bar (Ordered only: the same shape)"""
        ri, ro = R.rows_io(kind, K, inverse)
        a, g = self.dev(a), self.dev(g)
        l_d = None if l is None else (l if isinstance(l, torch.Tensor) else torch.from_numpy(np.array(l, self.dt)).cuda())
        a_d, g_d = self.place(a, offs[0]), self.place(g, offs[2])
        fn = getattr(self.lib, f"bjx_{kind}_vjp")
        runs = []
        for _ in range(2 if twice else 1):
            o = _Guard(self, ri, batch, offs[1])
            if alias == "in":
                o.data()[:] = a
            elif alias == "out_bar":
                o.data()[:] = g
            rc = fn(self.ctx.h, self.dtc, int(inverse), _p(o.view) if alias == "in" else _p(a_d), _p(o.view) if alias == "out_bar" else _p(g_d), _p(l_d), _p(o.view), K, batch)
            self.L.check(self.ctx.h, rc, fn.__name__)
            runs.append(o)
        torch.cuda.synchronize()
        assert torch.equal(runs[0].buf, runs[-1].buf), f"{what}: in_bar not repeatable"
        assert runs[0].intact(), f"{what}: wrote outside in_bar"
        return runs[0].data()


def _np(t):
    """(batch, rows) device tensor -> (rows, batch) numpy"""
    return host(t).T


def _check(c, r, ref, kind, inverse, K, batch, what):
    """a transform's result against (out, ladj, floor) of the first `batch` reference columns"""
    out, ladj, floor = (np.asarray(v)[..., :batch] for v in ref)
    if r.out_t is not None:
        flat_close(_np(r.out_t), out, c.dt, f"{what} values", per="sample")
    if r.ps_t is not None:
        flat_close(host(r.ps_t), ladj, c.dt, f"{what} ladj_ps", per="element", floor=floor)
    if r.sum is not None:
        sum_close(r.sum, ladj.sum(), c.dt.type, max(K - 1, 1) * batch, f"{what} ladj_sum")


SPANS = {"to-2113-rows": (1, 2113), "taller": (2114, 1 << 30)}


def _span_heights(entry, dt, inverse, span):
    lo, hi = SPANS[span]
    return [K for K in R.form_heights(entry, dt.name, inverse) if lo <= K <= hi]


def _cases(entries):
    """one test per (entry, type, direction, span of heights): the heights are walked inside the test, `what` names the one that fails"""
    return [(entry, dt, inverse, span) for entry in entries for dt in R.DTS for inverse in R.DIRS for span in SPANS if _span_heights(entry, dt, inverse, span)]


def _ids(cases):
    return [f"{e}-{dt.name}-{_dir(i)}-{span}" for e, dt, i, span in cases]


# ------------------------------------------------------------------ a. forms
TRANSFORM_CASES = _cases(R.TRANSFORMS)
PULLBACK_CASES = _cases(("ordered_vjp", "simplex_vjp"))


@pytest.mark.parametrize("kind,dt,inverse,span", TRANSFORM_CASES, ids=_ids(TRANSFORM_CASES))
def test_transform_forms(bj, kind, dt, inverse, span):
    """lo and hi of every form: batches 1, group − 1, group, group + 1 with both log-det outputs; at the largest batch ladj_ps alone,
    ladj_sum alone, neither (the LADJ = false ops of the Simplex), BJX_ACCUMULATE on both and, for the Simplex forward, out = NULL — the
    bits of the call with both wherever the output exists.  The columns of a smaller batch are the first of the largest one."""
    c = _Call(bj, dt)
    for K in _span_heights(kind, dt, inverse, span):
        _transform_forms_at(c, kind, dt, inverse, K)


def _transform_forms_at(c, kind, dt, inverse, K):
    fm = R.form(kind, dt, inverse, K, 3)
    bs = R.edge_batches(fm)
    B = bs[-1]
    x = c.dev(R.draw(kind, dt.name, inverse, K, B))
    ref = R.ref(kind, dt.name, inverse, K, B)
    for b in bs:
        what = f"seq_abi forms {fm!r} {kind} {_dir(inverse)} {dt.name} K={K} batch={b}"
        r = c.transform(kind, inverse, x[:b], K, b, what=what)
        _check(c, r, ref, kind, inverse, K, b, what)
    what = f"seq_abi flags {fm!r} {kind} {_dir(inverse)} {dt.name} K={K} batch={B}"
    r_ps = c.transform(kind, inverse, x, K, B, sm=False, what=f"{what} ladj_ps alone")
    r_sm = c.transform(kind, inverse, x, K, B, ps=False, what=f"{what} ladj_sum alone")
    r_no = c.transform(kind, inverse, x, K, B, ps=False, sm=False, what=f"{what} neither")
    for rr, tag in ((r_ps, "ladj_ps alone"), (r_sm, "ladj_sum alone")):
        _check(c, rr, ref, kind, inverse, K, B, f"{what} {tag}")
        assert torch.equal(rr.out_t, r.out_t), f"{what} {tag}: out differs from the call with both"
    assert torch.equal(r_ps.ps_t, r.ps_t) and r_sm.sum == r.sum, f"{what}: a log-det output depends on the other one"
    _check(c, r_no, ref, kind, inverse, K, B, f"{what} neither")
    if kind == "ordered":
        assert torch.equal(r_no.out_t, r.out_t), f"{what}: out without log-det outputs differs"
    pre_ps = torch.from_numpy(R.rng_for("pre", kind, dt.name, K).normal(size=B).astype(dt)).cuda()
    r_acc = c.transform(kind, inverse, x, K, B, flags=ACC, pre_ps=pre_ps, pre_sum=-2.5, what=f"{what} accumulate")
    assert torch.equal(r_acc.out_t, r.out_t), f"{what}: out with BJX_ACCUMULATE differs"
    # old + value, one rounding (the kernels may contract the value's last multiply into the add): on the scale of the larger term
    flat_close(host(r_acc.ps_t), host(pre_ps).astype(np.float64) + ref[1], c.dt, f"{what} accumulated ladj_ps", per="element", floor=ref[2] + np.abs(host(pre_ps)))
    sum_close(r_acc.sum, -2.5 + ref[1].sum(), dt.type, max(K - 1, 1) * B, f"{what} accumulated ladj_sum")
    if kind == "simplex" and not inverse:
        r_null = c.transform(kind, inverse, x, K, B, out=False, what=f"{what} out=NULL")
        assert torch.equal(r_null.ps_t, r.ps_t) and r_null.sum == r.sum, f"{what}: the log-det without `out` differs"


@pytest.mark.parametrize("entry,dt,inverse,span", PULLBACK_CASES, ids=_ids(PULLBACK_CASES))
def test_pullback_forms(bj, entry, dt, inverse, span):
    """lo and hi of every form at batches 1, group − 1, group, group + 1 with ladj_bar; NULL and zeros at the largest (the same bits)"""
    c = _Call(bj, dt)
    for K in _span_heights(entry, dt, inverse, span):
        _pullback_forms_at(c, entry, dt, inverse, K)


def _pullback_forms_at(c, entry, dt, inverse, K):
    kind = entry.split("_")[0]
    fm = R.form(entry, dt, inverse, K, 3)
    bs = R.edge_batches(fm)
    B = bs[-1]
    a = c.dev(R.draw(kind, dt.name, inverse, K, B))
    g_np, l_np = R.draw_bar(kind, dt.name, inverse, K, B)
    g, l = c.dev(g_np), torch.from_numpy(np.array(l_np)).cuda()
    ref = R.ref_vjp(kind, dt.name, inverse, K, B)
    for b in bs:
        what = f"seq_abi forms {fm!r} {entry} {_dir(inverse)} {dt.name} K={K} batch={b}"
        flat_close(_np(c.vjp(kind, inverse, a[:b], g[:b], l[:b], K, b, what=what)), ref[:, :b], c.dt, what, per="sample")
    what = f"seq_abi forms {fm!r} {entry} {_dir(inverse)} {dt.name} K={K} batch={B} ladj_bar=NULL"
    r0 = c.vjp(kind, inverse, a, g, None, K, B, what=what)
    flat_close(_np(r0), R.ref_vjp(kind, dt.name, inverse, K, B, False), c.dt, what, per="sample")
    rz = c.vjp(kind, inverse, a, g, torch.zeros(B, dtype=c.tdt, device="cuda"), K, B, what=what)
    assert torch.equal(rz, r0), f"{what}: not the bits of a ladj_bar of zeros"


# ------------------------------------------------------------------ b. offset bases
PULLBACKS = ("ordered_vjp", "simplex_vjp")
ALIGN_T = [(kind, dt) for kind in R.TRANSFORMS for dt in R.DTS]
ALIGN_V = [(entry, dt) for entry in PULLBACKS for dt in R.DTS]


def ED_IDS(cases):
    return [f"{e}-{dt.name}" for e, dt in cases]


def _same_arithmetic(f0, fm, inverse):
    if fm.family != f0.family:
        return False                                       # another kernel family (quad -> wave, stream -> lane): the bar only
    return not (fm.family == "ordered_tall" and not inverse and fm["V"] != f0["V"])     # pack-wise suffix sums: another association


@pytest.mark.parametrize("kind,dt", ALIGN_T, ids=ED_IDS(ALIGN_T))
def test_transforms_on_offset_bases(bj, kind, dt):
    """R.ALIGN_KS x R.OFFSETS: `off` elements on `in` alone, on `out` alone and on both: the instantiation `form` names, the bar, and —
    in the same kernel family — the bits of the aligned call (module docstring: where the bits may differ)"""
    c = _Call(bj, dt)
    for K in R.align_ks(kind, dt.name):
        for off in R.OFFSETS[dt.name]:
            _transform_offsets_at(c, kind, dt, K, off)


def _transform_offsets_at(c, kind, dt, K, off):
    for inverse in R.DIRS:
        f0 = R.form(kind, dt, inverse, K, 3)
        if f0.family == "refused":
            continue
        B = f0["group"] + 1
        x = c.dev(R.draw(kind, dt.name, inverse, K, B))
        ref = R.ref(kind, dt.name, inverse, K, B)
        what = f"seq_abi align {f0!r} {kind} {_dir(inverse)} {dt.name} K={K} batch={B}"
        r0 = c.transform(kind, inverse, x, K, B, what=what)
        _check(c, r0, ref, kind, inverse, K, B, what)
        for oi, oo, _ in R.offset_patterns(kind, off):
            fm = R.form(kind, dt, inverse, K, B, off_in=oi, off_out=oo)
            w2 = f"seq_abi align {fm!r} {kind} {_dir(inverse)} {dt.name} K={K} batch={B} offsets=({oi},{oo})"
            r = c.transform(kind, inverse, x, K, B, off_in=oi, off_out=oo, what=w2)
            _check(c, r, ref, kind, inverse, K, B, w2)
            if _same_arithmetic(f0, fm, inverse):
                assert torch.equal(r.out_t, r0.out_t) and torch.equal(r.ps_t, r0.ps_t) and r.sum == r0.sum, f"{w2}: not the bits of the aligned call ({f0!r})"


@pytest.mark.parametrize("entry,dt", ALIGN_V, ids=ED_IDS(ALIGN_V))
def test_pullbacks_on_offset_bases(bj, entry, dt):
    """R.ALIGN_KS x R.OFFSETS: `off` elements on `in`, `in_bar`, `out_bar` alone and on all three"""
    c = _Call(bj, dt)
    for K in R.align_ks(entry, dt.name):
        for off in R.OFFSETS[dt.name]:
            _pullback_offsets_at(c, entry, dt, K, off)


def _pullback_offsets_at(c, entry, dt, K, off):
    kind = entry.split("_")[0]
    for inverse in R.DIRS:
        f0 = R.form(entry, dt, inverse, K, 3)
        B = f0["group"] + 1
        a, (g, l) = R.draw(kind, dt.name, inverse, K, B), R.draw_bar(kind, dt.name, inverse, K, B)
        a, g = c.dev(a), c.dev(g)
        ref = R.ref_vjp(kind, dt.name, inverse, K, B)
        what = f"seq_abi align {f0!r} {entry} {_dir(inverse)} {dt.name} K={K} batch={B}"
        r0 = c.vjp(kind, inverse, a, g, l, K, B, what=what)
        flat_close(_np(r0), ref, c.dt, what, per="sample")
        for oi, oo, ob in R.offset_patterns(entry, off):
            fm = R.form(entry, dt, inverse, K, B, off_in=oi, off_out=oo, off_bar=ob)
            w2 = f"seq_abi align {fm!r} {entry} {_dir(inverse)} {dt.name} K={K} batch={B} offsets=({oi},{oo},{ob})"
            r = c.vjp(kind, inverse, a, g, l, K, B, offs=(oi, oo, ob), what=w2)
            flat_close(_np(r), ref, c.dt, w2, per="sample")
            if _same_arithmetic(f0, fm, inverse):
                assert torch.equal(r, r0), f"{w2}: not the bits of the aligned call ({f0!r})"


# ------------------------------------------------------------------ c. leading dimensions
@pytest.mark.parametrize("kind,dt", ALIGN_T, ids=ED_IDS(ALIGN_T))
def test_leading_dimensions(bj, kind, dt):
    """bjx_<kind>_ld with only `in` strided, only `out`, both; whole-pack and odd leading dimensions; 67 columns (a full wave and a
    ragged one).  The bar, the rows between `rows` and `ld` untouched, and one set of bits for every variant — the contiguous call's
    where that call runs the same family (the Simplex inverse; Ordered and the Simplex forward run the tall kernel there)."""
    c = _Call(bj, dt)
    for K in R.LD_KS[(kind, dt.name)]:
        _leading_dimensions_at(c, kind, dt, K)


def _leading_dimensions_at(c, kind, dt, K):
    B = R.LD_BATCH
    for inverse in R.DIRS:
        ri, ro = R.rows_io(kind, K, inverse)
        x = c.dev(R.draw(kind, dt.name, inverse, K, B))
        ref = R.ref(kind, dt.name, inverse, K, B)
        f0 = R.form(kind, dt, inverse, K, B)
        what = f"seq_abi ld {f0!r} {kind} {_dir(inverse)} {dt.name} K={K} batch={B}"
        r0 = c.transform(kind, inverse, x, K, B, what=what)
        _check(c, r0, ref, kind, inverse, K, B, what)
        first = None
        for li, lo in R.ld_variants(dt, ri, ro):
            fm = R.form(kind + "_ld", dt, inverse, K, B, ld_in=li, ld_out=lo)
            w2 = f"seq_abi ld {fm!r} {kind} {_dir(inverse)} {dt.name} K={K} batch={B} ld=({li},{lo})"
            r = c.transform(kind, inverse, x, K, B, ld_in=li, ld_out=lo, what=w2)
            _check(c, r, ref, kind, inverse, K, B, w2)
            base = r0 if fm.family == f0.family else first
            if base is not None:
                assert torch.equal(r.out_t, base.out_t) and torch.equal(r.ps_t, base.ps_t) and r.sum == base.sum, f"{w2}: the bits depend on the leading dimensions"
            first = first or r


# ------------------------------------------------------------------ d. loop trips
def _tile(c, a, idx_d):
    return c.dev(a).index_select(0, idx_d)


def _later_copies_equal(t, D, idx_d, what):
    same = (t == t[:D].index_select(0, idx_d)).reshape(t.shape[0], -1).all(dim=1)
    assert bool(same.all()), f"{what}: column {int((~same).nonzero()[0])} (+{int((~same).sum()) - 1} more) differs from the first copy of its data"


def _trip(c, entry, inverse, K, nsteps):
    D = R.TRIP_D
    dn = c.dt.name
    kind = entry.split("_")[0]
    f0 = R.form(entry, dn, inverse, K, 3)
    batch = R.trip_batch(f0["CPS"], nsteps)
    fm = R.form(entry, dn, inverse, K, batch)
    assert fm["nsteps"] == nsteps
    idx_d = torch.from_numpy(R.tiled_index(D, batch)).cuda()
    what = f"seq_abi trips {fm!r} {entry} {_dir(inverse)} {dn} K={K} batch={batch}"
    x = _tile(c, R.draw(kind, dn, inverse, K, D), idx_d)
    if entry in R.TRANSFORMS:
        r = c.transform(kind, inverse, x, K, batch, what=what)
        out, ladj, floor = R.ref(kind, dn, inverse, K, D)
        flat_close(_np(r.out_t[:D]), out, c.dt, f"{what} values", per="sample")
        flat_close(host(r.ps_t[:D]), ladj, c.dt, f"{what} ladj_ps", per="element", floor=floor)
        sum_close(r.sum, float(ladj[R.tiled_index(D, batch)].sum()), c.dt.type, (K - 1) * batch, f"{what} ladj_sum")
        _later_copies_equal(r.out_t, D, idx_d, f"{what} values")
        _later_copies_equal(r.ps_t, D, idx_d, f"{what} ladj_ps")
        return
    g, l = R.draw_bar(kind, dn, inverse, K, D)
    r = c.vjp(kind, inverse, x, _tile(c, g, idx_d), torch.from_numpy(np.array(l)).cuda().index_select(0, idx_d), K, batch, what=what)
    flat_close(_np(r[:D]), R.ref_vjp(kind, dn, inverse, K, D), c.dt, what, per="sample")
    _later_copies_equal(r, D, idx_d, what)


TRIP_GROUPS = sorted({(e, d) for e, d, _, _ in R.TRIPS})


@pytest.mark.parametrize("entry,dtname", TRIP_GROUPS, ids=[f"{e}-{d}" for e, d in TRIP_GROUPS])
def test_second_step_of_the_tall_kernels(bj, entry, dtname):
    """8 192·CPS + CPS + 1 columns, tiled on the device from 37 distinct ones: nsteps = 2, the last wave walks a full set and then a ragged
    one (the strip keeps the previous step's values where the ragged set writes nothing).  The first copies against the reference,
    every later copy the bits of its first."""
    c = _Call(bj, dtname)
    for e, d, inverse, K in R.TRIPS:
        if (e, d) == (entry, dtname):
            _trip(c, entry, inverse, K, 2)


def test_third_step_of_the_tall_kernel(bj):
    entry, dtname, inverse, K = R.TRIP3
    _trip(_Call(bj, dtname), entry, inverse, K, 3)


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_second_column_of_a_block_of_the_tall_ordered_pullback(bj, dt):
    """ordered_vjp_tall_kernel: a grid of at most 8·CUs blocks, one column a trip — 8·CUs + 1 columns give block 0 a second column
    (the forward's carry and wave sums start again)"""
    c = _Call(bj, dt)
    for inverse in R.DIRS:
        _ordered_tall_trip(c, dt, inverse)


def _ordered_tall_trip(c, dt, inverse):
    K, D = R.ORDERED_TALL_TRIP_K[dt.name], R.TRIP_D
    batch = 8 * c.cus + 1
    fm = R.form("ordered_vjp", dt, inverse, K, batch)
    assert fm.family == "ordered_tall" and fm["V"] == R.vw(dt)
    idx_d = torch.from_numpy(R.tiled_index(D, batch)).cuda()
    g, l = R.draw_bar("ordered", dt.name, inverse, K, D)
    what = f"seq_abi trips {fm!r} ordered_vjp {_dir(inverse)} {dt.name} K={K} batch={batch}"
    r = c.vjp("ordered", inverse, _tile(c, R.draw("ordered", dt.name, inverse, K, D), idx_d), _tile(c, g, idx_d),
              torch.from_numpy(np.array(l)).cuda().index_select(0, idx_d), K, batch, what=what)
    flat_close(_np(r[:D]), R.ref_vjp("ordered", dt.name, inverse, K, D), c.dt, what, per="sample")
    _later_copies_equal(r, D, idx_d, what)


# ------------------------------------------------------------------ e. position independence
POS_CASES = ALIGN_T + ALIGN_V


@pytest.mark.parametrize("entry,dt", POS_CASES, ids=ED_IDS(POS_CASES))
def test_a_column_gives_the_same_bits_alone_and_at_every_index_of_a_group_plus_one(bj, entry, dt):
    """column 0 alone, and in place of column j (which takes its place) of group + 1 columns of other data, for every j (groups of
    256: every j below 70 and from 190 on — every wave of the block, both blocks), at the heights of R.ALIGN_KS (one or two per
    family).  Module docstring: the wave-wide choices."""
    c = _Call(bj, dt)
    for K in R.align_ks(entry, dt.name):
        _position_at(c, entry, dt, K)


def _position_at(c, entry, dt, K):
    kind = entry.split("_")[0]
    for inverse in R.DIRS:
        fm = R.form(entry, dt, inverse, K, 3)
        if fm.family == "refused":
            continue
        B = fm["group"] + 1
        js = range(B) if B <= 130 else [j for j in range(B) if j < 70 or j >= 190]
        x = c.dev(R.draw(kind, dt.name, inverse, K, B))
        what = f"seq_abi position {fm!r} {entry} {_dir(inverse)} {dt.name} K={K}"
        if entry in R.TRANSFORMS:
            r0 = c.transform(kind, inverse, x[:1], K, 1, twice=False, what=what)
        else:
            g_np, l_np = R.draw_bar(kind, dt.name, inverse, K, B)
            g, l = c.dev(g_np), torch.from_numpy(np.array(l_np)).cuda()
            r0 = c.vjp(kind, inverse, x[:1], g[:1], l[:1], K, 1, twice=False, what=what)
        for j in js:
            perm = torch.arange(B, device="cuda")
            perm[0], perm[j] = j, 0
            if entry in R.TRANSFORMS:
                r = c.transform(kind, inverse, x[perm], K, B, twice=False, what=what)
                assert torch.equal(r.out_t[j], r0.out_t[0]) and torch.equal(r.ps_t[j], r0.ps_t[0]), f"{what}: the result of a column differs at index {j} of {B}"
            else:
                r = c.vjp(kind, inverse, x[perm], g[perm], l[perm], K, B, twice=False, what=what)
                assert torch.equal(r[j], r0[0]), f"{what}: the result of a column differs at index {j} of {B}"


# ------------------------------------------------------------------ f. aliasing
@pytest.mark.parametrize("entry,dt", ALIGN_V, ids=ED_IDS(ALIGN_V))
def test_alias_in_bar_is_in(bj, entry, dt):
    """include/bjx.h: in_bar may alias `in`.  Every kernel of both families loads all it needs of a column (and of the columns its wave
    or block shares a run with) before its first store, except ordered_vjp_tall_kernel, which walks from the column's end and reads the
    row behind a tile after that tile is written.  The dispatchers step aside from that kernel and from the two tiny kernels — to
    ordered_vjp_kernel, simplex_vjp_kernel / the stream kernel, and ordered_vjp_column_kernel — and nothing else reaches
    ordered_vjp_kernel and ordered_vjp_column_kernel by default, so this test is also their forms test: batches 1, group − 1, group,
    group + 1, an offset of one (Float32: and two) elements on the shared pointer, on out_bar and on both (ordered_vjp_kernel<T, 1, *>),
    and a column alone and at every index of group + 1.  The bits of the out-of-place call wherever that call runs the same family;
    the bar everywhere.  Heights: R.ALIAS_IN_KS.
    `__restrict__`: every pullback kernel declares in, out_bar and in_bar `__restrict__`, and the header now allows two of them to be one
    pointer.  That is harmless in the kernels an alias reaches: a thread (lane kernels, stream kernels: a wave, through LDS behind a
    barrier) stores only addresses it has loaded itself, and every stored value depends on those loads, so no load can be moved behind
    the store that overwrites it whatever the compiler may assume about the pointers.  The same holds for ordered_vjp_tiny_kernel with
    in_bar == out_bar (test_alias_in_bar_is_out_bar): the column is loaded whole into registers before the one store."""
    c = _Call(bj, dt)
    for K in R.ALIAS_IN_KS[(entry, dt.name)]:
        _alias_in_at(c, entry, dt, K)


ALIAS_ONLY = ("ordered_lane", "ordered_column")          # families that only in_bar == in reaches


def _alias_in_at(c, entry, dt, K):
    kind = entry.split("_")[0]
    for inverse in R.DIRS:
        f0, fm = R.form(entry, dt, inverse, K, 3), R.form(entry, dt, inverse, K, 3, alias="in")
        bs = R.edge_batches(fm) if fm.family in ALIAS_ONLY else (fm["group"] + 1,)
        B = bs[-1]
        a, (g, l) = c.dev(R.draw(kind, dt.name, inverse, K, B)), R.draw_bar(kind, dt.name, inverse, K, B)
        g, l = c.dev(g), torch.from_numpy(np.array(l)).cuda()
        ref = R.ref_vjp(kind, dt.name, inverse, K, B)
        for b in bs:
            what = f"seq_abi alias {fm!r} {entry} {_dir(inverse)} {dt.name} K={K} batch={b} in_bar == in"
            ra = c.vjp(kind, inverse, a[:b], g[:b], l[:b], K, b, alias="in", what=what)
            flat_close(_np(ra), ref[:, :b], c.dt, what, per="sample")
            if fm.family == f0.family:
                assert torch.equal(ra, c.vjp(kind, inverse, a[:b], g[:b], l[:b], K, b, what=what)), f"{what}: not the bits of the out-of-place call"
        if fm.family not in ALIAS_ONLY:
            continue
        for off in R.OFFSETS[dt.name]:                   # in and in_bar are one pointer: one offset for both
            for oi, ob in ((off, 0), (0, off), (off, off)):
                fo = R.form(entry, dt, inverse, K, B, off_in=oi, off_bar=ob, alias="in")
                assert fo.family == fm.family and fo.get("V", 1) == 1
                w2 = f"seq_abi alias {fo!r} {entry} {_dir(inverse)} {dt.name} K={K} batch={B} in_bar == in offsets=({oi},{oi},{ob})"
                ro = c.vjp(kind, inverse, a, g, l, K, B, offs=(oi, oi, ob), alias="in", what=w2)
                flat_close(_np(ro), ref, c.dt, w2, per="sample")
                assert torch.equal(ro, ra), f"{w2}: not the bits of the aligned call"
        what = f"seq_abi alias-position {fm!r} {entry} {_dir(inverse)} {dt.name} K={K}"
        r1 = c.vjp(kind, inverse, a[:1], g[:1], l[:1], K, 1, alias="in", twice=False, what=what)
        for j in (range(B) if B <= 130 else [j for j in range(B) if j < 70 or j >= 190]):
            perm = torch.arange(B, device="cuda")
            perm[0], perm[j] = j, 0
            r = c.vjp(kind, inverse, a[perm], g[perm], l[perm], K, B, alias="in", twice=False, what=what)
            assert torch.equal(r[j], r1[0]), f"{what}: the result of a column differs at index {j} of {B}"


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_alias_in_bar_is_out_bar(bj, dt):
    """bjx_ordered_vjp serves in_bar == out_bar up to 2 048 | 1 024 rows (tiny and stream kernels: a lane's own packs, loaded before they are
    stored) with the bits of the out-of-place call, and refuses it beyond (ordered_vjp_tall_kernel reads the cotangent of the row
    behind a pack, which another lane or an earlier tile has overwritten).  bjx_simplex_vjp refuses it at every height: in_bar and
    out_bar differ by a row a column, so column c of the one lies over columns c − 1 and c of the other, which another lane, wave or
    block may not have read.  A refusal is BJX_ERR_ARG before any launch, in_bar (= out_bar) untouched."""
    c = _Call(bj, dt)
    for inverse in R.DIRS:
        for K in R.ALIAS_OUT_BAR_SERVED[dt.name]:
            fm = R.form("ordered_vjp", dt, inverse, K, 3, alias="out_bar")
            B = fm["group"] + 1
            a, (g, l) = R.draw("ordered", dt.name, inverse, K, B), R.draw_bar("ordered", dt.name, inverse, K, B)
            what = f"seq_abi alias {fm!r} ordered_vjp {_dir(inverse)} {dt.name} K={K} batch={B} in_bar == out_bar"
            r0 = c.vjp("ordered", inverse, a, g, l, K, B, what=what)
            ra = c.vjp("ordered", inverse, a, g, l, K, B, alias="out_bar", what=what)
            flat_close(_np(ra), R.ref_vjp("ordered", dt.name, inverse, K, B), c.dt, what, per="sample")
            assert torch.equal(ra, r0), f"{what}: not the bits of the out-of-place call"
        # refused
        todo = [("ordered", R.ALIAS_OUT_BAR_REFUSED[dt.name])] + [("simplex", K) for K in R.ALIAS_IN_KS[("simplex_vjp", dt.name)]]
        for kind, K in todo:
            B = 3
            ri, ro = R.rows_io(kind, K, inverse)
            a = c.place(c.dev(R.draw(kind, dt.name, inverse, K, B)))
            g_np, l_np = R.draw_bar(kind, dt.name, inverse, K, B)
            l = torch.from_numpy(np.array(l_np)).cuda()
            o = _Guard(c, max(ri, ro), B)                                  # room for either shape
            flat = o.view[:ro * B]
            flat[:] = c.dev(g_np).reshape(-1)
            before = o.buf.clone()
            n0 = c.lib.bjx_launch_count()
            rc = getattr(c.lib, f"bjx_{kind}_vjp")(c.ctx.h, c.dtc, int(inverse), _p(a), _p(o.view), _p(l), _p(o.view), K, B)
            torch.cuda.synchronize()
            assert rc == c.L.ERR_ARG, f"bjx_{kind}_vjp {_dir(inverse)} K={K}: in_bar == out_bar returned {rc}"
            assert b"alias" in c.lib.bjx_last_error(c.ctx.h)
            assert c.lib.bjx_launch_count() == n0 and torch.equal(o.buf, before), f"bjx_{kind}_vjp K={K}: a refused call launched or wrote"
            assert getattr(c.lib, f"bjx_{kind}_vjp")(c.ctx.h, c.dtc, int(inverse), _p(a), _p(o.view), _p(l), _p(o.view), K, 0) == 0       # an empty batch touches nothing
            what = f"seq_abi after-refusal {kind}_vjp {_dir(inverse)} {dt.name} K={K}"
            flat_close(_np(c.vjp(kind, inverse, R.draw(kind, dt.name, inverse, K, B), g_np, l_np, K, B, what=what)), R.ref_vjp(kind, dt.name, inverse, K, B), c.dt, what, per="sample")


# ------------------------------------------------------------------ g. refusals
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_refusals_of_the_transforms(bj, dt):
    """batch = 0 (ladj_sum zeroed without BJX_ACCUMULATE, kept with it), batch = −1, K = 0, K = 1 of the Simplex, every NULL an entry
    checks, a bad dtype, a leading dimension below the height: nothing launched, nothing written, and an ordinary call afterwards"""
    c = _Call(bj, dt)
    K, B = 12, 3
    for kind in R.TRANSFORMS:
        for inverse in R.DIRS:
            ri, ro = R.rows_io(kind, K, inverse)
            x = c.place(c.dev(R.draw(kind, dt.name, inverse, K, B)))
            o, p = _Guard(c, ro, B), _Guard(c, 1, B)
            s = torch.full((3,), MARK, dtype=torch.float64, device="cuda")
            f, fl = getattr(c.lib, f"bjx_{kind}"), getattr(c.lib, f"bjx_{kind}_ld")
            n0 = c.lib.bjx_launch_count()
            h, d, i = c.ctx.h, c.dtc, int(inverse)
            assert f(h, d, i, _p(x), _p(o.view), _p(p.view), None, K, -1, 0) == c.L.ERR_SHAPE
            assert f(h, d, i, _p(x), _p(o.view), _p(p.view), None, 0, B, 0) == c.L.ERR_SHAPE
            if kind == "simplex":
                assert f(h, d, i, _p(x), _p(o.view), _p(p.view), None, 1, B, 0) == c.L.ERR_SHAPE
                assert fl(h, d, i, _p(x), ri, _p(o.view), ro, _p(p.view), None, 1, B, 0) == c.L.ERR_SHAPE
            assert f(h, d, i, None, _p(o.view), _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            if kind == "ordered" or inverse:
                assert f(h, d, i, _p(x), None, _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            assert fl(h, d, i, None, ri, _p(o.view), ro, _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            assert fl(h, d, i, _p(x), ri, None, ro, _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            assert f(h, 7, i, _p(x), _p(o.view), _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            assert fl(h, 7, i, _p(x), ri, _p(o.view), ro, _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            assert f(None, d, i, _p(x), _p(o.view), _p(p.view), None, K, B, 0) == c.L.ERR_ARG
            assert fl(h, d, i, _p(x), ri - 1, _p(o.view), ro, _p(p.view), None, K, B, 0) == c.L.ERR_SHAPE
            assert fl(h, d, i, _p(x), ri, _p(o.view), ro - 1, _p(p.view), None, K, B, 0) == c.L.ERR_SHAPE
            assert fl(h, d, i, _p(x), ri, _p(o.view), ro, _p(p.view), None, K, -1, 0) == c.L.ERR_SHAPE
            torch.cuda.synchronize()
            assert o.intact(False) and p.intact(False) and c.lib.bjx_launch_count() == n0, f"{kind} {_dir(inverse)}: a refused call launched or wrote"
            # batch = 0
            assert f(h, d, i, None, None, None, None, K, 0, 0) == 0
            assert f(h, d, i, _p(x), _p(o.view), _p(p.view), _p(s[1:]), K, 0, ACC) == 0
            torch.cuda.synchronize()
            assert host(s).tolist() == [MARK] * 3, "batch = 0 with BJX_ACCUMULATE changed ladj_sum"
            assert f(h, d, i, _p(x), _p(o.view), _p(p.view), _p(s[1:]), K, 0, 0) == 0
            torch.cuda.synchronize()
            assert host(s).tolist() == [MARK, 0.0, MARK], "batch = 0 did not zero ladj_sum"
            assert fl(h, d, i, _p(x), ri + 3, _p(o.view), ro + 3, _p(p.view), _p(s[1:]), K, 0, ACC) == 0
            torch.cuda.synchronize()
            assert host(s).tolist() == [MARK, 0.0, MARK] and o.intact(False) and p.intact(False)
            what = f"seq_abi after-refusal {kind} {_dir(inverse)} {dt.name} K={K}"
            _check(c, c.transform(kind, inverse, R.draw(kind, dt.name, inverse, K, B), K, B, what=what), R.ref(kind, dt.name, inverse, K, B), kind, inverse, K, B, what)


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_refusals_of_the_pullbacks(bj, dt):
    c = _Call(bj, dt)
    K, B = 12, 3
    for kind in R.TRANSFORMS:
        for inverse in R.DIRS:
            ri, ro = R.rows_io(kind, K, inverse)
            a = c.place(c.dev(R.draw(kind, dt.name, inverse, K, B)))
            g_np, l_np = R.draw_bar(kind, dt.name, inverse, K, B)
            g, l = c.place(c.dev(g_np)), torch.from_numpy(np.array(l_np)).cuda()
            o = _Guard(c, ri, B)
            f = getattr(c.lib, f"bjx_{kind}_vjp")
            h, d, i = c.ctx.h, c.dtc, int(inverse)
            n0 = c.lib.bjx_launch_count()
            assert f(h, d, i, _p(a), _p(g), _p(l), _p(o.view), K, -1) == c.L.ERR_SHAPE
            assert f(h, d, i, _p(a), _p(g), _p(l), _p(o.view), 0, B) == c.L.ERR_SHAPE
            if kind == "simplex":
                assert f(h, d, i, _p(a), _p(g), _p(l), _p(o.view), 1, B) == c.L.ERR_SHAPE
            assert f(h, d, i, None, _p(g), _p(l), _p(o.view), K, B) == c.L.ERR_ARG
            assert f(h, d, i, _p(a), None, _p(l), _p(o.view), K, B) == c.L.ERR_ARG
            assert f(h, d, i, _p(a), _p(g), _p(l), None, K, B) == c.L.ERR_ARG
            assert f(h, 7, i, _p(a), _p(g), _p(l), _p(o.view), K, B) == c.L.ERR_ARG
            assert f(None, d, i, _p(a), _p(g), _p(l), _p(o.view), K, B) == c.L.ERR_ARG
            assert f(h, d, i, None, None, None, None, K, 0) == 0 and f(h, d, i, _p(a), _p(g), _p(l), _p(o.view), K, 0) == 0
            torch.cuda.synchronize()
            assert o.intact(False) and c.lib.bjx_launch_count() == n0, f"{kind}_vjp {_dir(inverse)}: a refused call launched or wrote"
            what = f"seq_abi after-refusal {kind}_vjp {_dir(inverse)} {dt.name} K={K}"
            flat_close(_np(c.vjp(kind, inverse, R.draw(kind, dt.name, inverse, K, B), g_np, l_np, K, B, what=what)), R.ref_vjp(kind, dt.name, inverse, K, B), c.dt, what, per="sample")


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_the_two_gib_range_of_a_buffer_descriptor(bj, dt):
    """launch_seq_chunk and the chunked Simplex pullback address a wave's 64 columns through one buffer descriptor: 64·ld·sizeof(T) < 2³¹.
    bjx_ordered_ld at ld = 2²³ | 2²² (dim 300, two columns) is refused, one less is served; bjx_simplex_vjp at K = 2²³ | 2²² (one column)
    is refused.  Every buffer has the size the call would need if served: a missing refusal fails an assertion, nothing else."""
    c = _Call(bj, dt)
    for inverse in R.DIRS:
        _two_gib_at(c, dt, inverse)
        torch.cuda.empty_cache()


def _two_gib_at(c, dt, inverse):
    ld, K, B = R.LD_REFUSED[dt.name], 300, 2
    assert R.form("ordered_ld", dt, inverse, K, B, ld_in=ld, ld_out=ld).family == "refused"
    x = R.draw("ordered", dt.name, inverse, K, B)
    ref = R.ref("ordered", dt.name, inverse, K, B)
    xb = torch.full((ld * B,), MARK, dtype=c.tdt, device="cuda")
    xb.view(B, ld)[:, :K] = c.dev(x)
    ob = torch.full((ld * B,), MARK, dtype=c.tdt, device="cuda")
    p = _Guard(c, 1, B)
    n0 = c.lib.bjx_launch_count()
    rc = c.lib.bjx_ordered_ld(c.ctx.h, c.dtc, int(inverse), _p(xb), ld, _p(ob), ld, _p(p.view), None, K, B, 0)
    torch.cuda.synchronize()
    assert rc == c.L.ERR_UNSUPPORTED and b"2 GiB" in c.lib.bjx_last_error(c.ctx.h), rc
    assert c.lib.bjx_launch_count() == n0 and bool((ob == MARK).all()) and p.intact(False), "the refused call launched or wrote"
    del xb, ob
    what = f"seq_abi 2GiB ordered_ld {_dir(inverse)} {dt.name} ld={ld - 1}"
    r = c.transform("ordered", inverse, x, K, B, ld_in=ld - 1, ld_out=ld - 1, twice=False, what=what)
    _check(c, r, ref, "ordered", inverse, K, B, what)
    del r
    torch.cuda.empty_cache()
    # the chunked Simplex pullback
    Kv = ld
    assert R.form("simplex_vjp", dt, inverse, Kv, 1).family == "refused"
    ri, ro = R.rows_io("simplex", Kv, inverse)
    a = torch.full((ri,), 0.5 / Kv if not inverse else -3.0, dtype=c.tdt, device="cuda")
    g = torch.ones(ro, dtype=c.tdt, device="cuda")
    o = torch.full((ri,), MARK, dtype=c.tdt, device="cuda")
    n0 = c.lib.bjx_launch_count()
    rc = c.lib.bjx_simplex_vjp(c.ctx.h, c.dtc, int(inverse), _p(a), _p(g), None, _p(o), Kv, 1)
    torch.cuda.synchronize()
    assert rc == c.L.ERR_UNSUPPORTED and c.lib.bjx_launch_count() == n0 and bool((o == MARK).all()), rc
    del a, g, o
    torch.cuda.empty_cache()
    what = f"seq_abi after-refusal simplex_vjp {_dir(inverse)} {dt.name} K=12"
    g_np, l_np = R.draw_bar("simplex", dt.name, inverse, 12, 3)
    flat_close(_np(c.vjp("simplex", inverse, R.draw("simplex", dt.name, inverse, 12, 3), g_np, l_np, 12, 3, what=what)), R.ref_vjp("simplex", dt.name, inverse, 12, 3), c.dt, what, per="sample")
