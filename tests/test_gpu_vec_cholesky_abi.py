"""The four VecCholesky entry points of include/bjx.h — bjx_vec_cholesky (both directions), bjx_vec_cholesky_inv_vjp and
bjx_vec_cholesky_fwd_vjp — through the C ABI at every kernel form, alignment and batch edge that their dispatchers (chol_impl,
chol_inv_vjp_impl, chol_fwd_vjp_impl at the end of csrc/bjx_seq.hip) choose among, against the Float64 oracle on the dt-rounded inputs
(tests/_vec_cholesky_ref.py: draws, references and the tables; tests/test_host_vec_cholesky_ref.py checks on the CPU that every table
shape reaches the form written next to it and that the Float32 oracle stays within a tenth of the bar on these inputs).  Default tuning
switches only.

Which shape reaches which instantiation (K lo, K hi per form; Float32 | Float64), every pointer aligned:
  bjx_vec_cholesky inverse -> chol_lane_kernel<T, true, V> / chol_inv_chunk_kernel<T, V, CHV, WRITE_W, LOWER> / chol_inv_kernel<T, WRITE_W>,
  forward -> chol_lane_kernel<T, false, V> / chol_fwd_chunk_kernel<T, V, CHV, LOWER, LADJ> / chol_fwd_kernel<T>,
  bjx_vec_cholesky_inv_vjp -> chol_inv_vjp_lane_kernel<T, V> / chol_inv_vjp_kernel<T, V, CHV, LOWER> / BJX_ERR_UNSUPPORTED:
    lane, V = pack   2, 11 | 2, 8        chunk (1, 2)     12, 15 | 10, 15      chunk (pack, 1)  16, 17 | 9, 16
    chunk (pack, 2)  24, 32 | 17, 21     chunk (1, 8)     18, 31 | 18, 31      chunk (pack, 4)  33, 41 | 24, 32
    chunk (pack, 8)  48, 64 | 33, 45     chunk (1, 16)    34, 45 | 34, 43      chunk (1, 32)    46, 63 | 46, 63
    chunk (2, 16)    —      | 48, 64     generic / refused 65, 100 | 65, 100
  each with both `uplo` (LOWER), with and without `out` (WRITE_W) and with a log-det (LADJ = true; LADJ = false in the variants test).
  With the deciding base pointer one element off the 16-byte boundary (`in` of the inverse, `out` of the forward, y / y_bar of inv_vjp)
  V = 1 at every K: K = 2, 11 | 8 the lane kernels in V = 1; K = 16, 17, 32, 33, 64 -> (1, 2), (1, 8), (1, 8), (1, 16), (1, 32); at
  K = 16, 33, 64 also only the y side, only the dense-W side and both offset.  The dense W (`out` of the inverse, `in` of the forward,
  W_bar of inv_vjp) takes the per-sample `bjx_aligned16_dev(Ws)` branch on the device: an offset base sends every sample (even K·K) to
  the unaligned branch, and with an odd K·K — K = 17, 33 and 41 of the Float32 table (and 9, 17, 21, 33, 45 ... of the Float64 one) —
  the samples of ONE aligned call alternate between the two branches.
  bjx_vec_cholesky_fwd_vjp -> chol_fwd_vjp_lane_kernel<T, V> (K = 2, 11 | 8, aligned and with each of the three pointers offset),
  chol_fwd_vjp_kernel<T, V, LOWER, SWZ>: swizzled K = 16, 64, 128 | 16, 64; pack 24, 160 | 12, 116; scalar 12, 13, 165 | 9, 13, 115 and
  K = 16, 24 with W_bar offset; refused 166 | 117.
Batches: lane 1, 63, 64, 65, 129 and, at K = 2 and 3, 2·(32·CUs)·64 + 65 samples (the second and third trip of the `s0` loop of a grid
capped at 32 tiles per CU); chunk 1, 2, 3, 5 (two samples per block: an idle second wave); generic 1, 4, 5; chol_fwd_vjp_kernel 1, 3
(2 at K >= 115: the oracle's pullback loops in Python per sample).

What every comparison asserts: outputs are views of marker-filled buffers one sample longer (one marker element in front of an offset
view), all markers intact; every call is made twice and gives identical bits; W, y, y_bar and W_bar under `_tol.flat_close`
per="sample" (flat 1e-3 / 1e-6 of the sample's max-norm); the per-sample log-dets per="element" with the floor logcosh(0.5) = 0.12
(_vec_cholesky_ref.LOG_DET_FLOOR: one term of the sum at the scale of the draws; at K = 2 the log-det is one term and can be near zero); ladj_sum against the Float64 sum of the
reference with test_gpu_parity.sum_close, n = nv·batch.  The inverse's W: the triangle `uplo` does not name exactly 0, W[0,0] exactly 1,
column norms 1 within the bar.  'L' results are the transpose of the 'U' results BIT FOR BIT at every form (LOWER only changes
addresses in every kernel here), and a sample gives the same bits alone and at every index of a batch of 5.

Worst measured |got − ref| / scale (MI355X, 256 CUs; the bar is 1e-3 | 1e-6), Float32 | Float64:
  inverse W     lane 2.7e-7 | 3.3e-16   chunk, every form <= 2.5e-7 | 7.8e-16   (1, 16) 2.5e-7 | 4.4e-16   generic 6.4e-7 | 1.6e-15
  inverse logJ  lane 1.6e-6 | 3.5e-15   chunk <= 2.0e-7 | 2.0e-15               (1, 16) 1.2e-7 | 1.1e-15   generic 2.2e-7 | 2.9e-15
  forward y     lane 5.4e-7 | 1.2e-15   chunk <= 2.2e-7 | 4.3e-16               (1, 16) 2.2e-7 | 3.2e-16   generic 8.7e-8 | 5.9e-16
  forward ladj  lane 7.2e-7 | 2.6e-15   chunk <= 3.5e-7 | 2.3e-15               (1, 16) 2.5e-7 | 1.6e-15   generic 2.2e-7 | 4.2e-15
  offset and mixed alignments: no figure above those of the aligned forms (W 2.0e-7 | 4.4e-16, y 1.8e-7 | 2.9e-16)
  inv_vjp y_bar lane 3.2e-7 | 8.0e-15   chunk <= 3.2e-7 | 2.1e-15   (1, 16) 2.4e-7 | 1.4e-15
  fwd_vjp W_bar lane 8.7e-7 | 2.0e-15   swizzled 2.6e-6 | 2.8e-15   pack 1.6e-6 | 3.0e-15   scalar 3.2e-6 | 6.2e-15
  the first row at |y| = 1e-6 ... 6, both signs: y 1.3e-7 | 9.0e-13, ladj 5.0e-7 | 6.4e-14
  the `s0` trips (1 048 641 samples): W 2.4e-7 | 5.6e-16, logJ 4.7e-6 | 7.7e-15, y 3.5e-7 | 3.4e-15, ladj 1.9e-6 | 6.7e-15, fwd_vjp
  5.4e-7 | 1.3e-15, inv_vjp K = 3 5.6e-6 | 1.6e-14, inv_vjp K = 2 6.0e-8 | 8.3e-11.
Found and fixed: the forward y of the Float32 lane kernel at K = 2 was 1.2e-2 off at |y| = 3e-6 (atanh as log((1+w)/(1−w)): an ulp of
1, not of y).  LinkMath<float>::atanh_lc_rel now takes ½·log1p(2a/(1−a)) on a = |w| and restores the sign: on w itself that form loses
e^{2|y|} ulp towards w = −1 (1e-3 at y = −6), which test_forward_first_row_at_both_ends_of_atanh_and_both_signs pins.  Upgraded, not a
defect: the Float32 y_bar of inv_vjp at K = 2 — one number per sample, a sum of two terms of either sign, up to 7.2e-2 of its own value
off on 26 of 1 048 641 samples, as any Float32 evaluation is — is evaluated in Float64 by chol_inv_vjp_lane_kernel.  The figures above are
after both changes.  Every 'L' result was the bitwise transpose of its 'U' result and every sample
position-independent at every form; no other defect."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _vec_cholesky_ref as R  # noqa: E402
from _tol import RTOL_FLAT, flat_close  # noqa: E402
from test_gpu_parity import bj, host, sum_close  # noqa: E402,F401

MARK = 7.25
ACC = 1                     # BJX_ACCUMULATE
T3 = (1, 0, 2)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Guard:
    """`per`·batch elements behind `off` marker elements, one more sample (at least one element) of markers behind them"""

    def __init__(self, c, per, batch, off=0):
        self.n, self.off = per * batch, off
        self.buf = torch.full((off + self.n + max(per, 1),), MARK, dtype=c.tdt, device="cuda")
        self.view = self.buf[off:]

    def intact(self, written=True):
        return bool((self.buf[:self.off] == MARK).all()) and bool((self.buf[self.off + (self.n if written else 0):] == MARK).all())

    def np(self, shape):
        return host(self.view[:self.n]).reshape(shape, order="F")


class _Res:
    out = ps = sum = None


class _Call:
    def __init__(self, bj, dt):
        self.L = bj._lib
        self.lib = self.L.load()
        self.ctx = bj.context()
        self.dt = np.dtype(dt)
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dtc = self.L.BJX_F32 if self.dt == np.float32 else self.L.BJX_F64
        self.rtol = RTOL_FLAT[self.dt]

    def put(self, a, off=0):
        """a column-major array -> its elements in memory order on the device, `off` elements into a marker-filled buffer"""
        flat = torch.from_numpy(np.array(np.asarray(a, self.dt).reshape(-1, order="F")))
        buf = torch.full((flat.numel() + off,), MARK, dtype=self.tdt, device="cuda")
        buf[off:] = flat.cuda()
        return buf[off:]

    def value(self, inverse, uplo, x, K, batch, out=True, ps=True, sm=True, flags=0, off_in=0, off_out=0, pre_ps=None, pre_sum=None, what=""):
        """bjx_vec_cholesky twice (identical bits), guards checked -> _Res(out (K, K, batch) | (n, batch), ps (batch,), sum)"""
        n_out = K * K if inverse else R.nvec(K)
        x_d = self.put(x, off_in) if x is not None else None
        runs = []
        for _ in range(2):
            o = _Guard(self, n_out, batch, off_out) if out else None
            p = _Guard(self, 1, batch) if ps else None
            s = torch.full((3,), MARK, dtype=torch.float64, device="cuda") if sm else None
            if pre_ps is not None:
                p.view[:batch] = torch.from_numpy(np.array(pre_ps, self.dt)).cuda()
            if pre_sum is not None:
                s[1] = pre_sum
            rc = self.lib.bjx_vec_cholesky(self.ctx.h, self.dtc, int(inverse), ord(uplo), _p(x_d), _p(o.view) if out else None, _p(p.view) if ps else None,
                                           _p(s[1:]) if sm else None, K, batch, flags)
            self.L.check(self.ctx.h, rc, "bjx_vec_cholesky")
            runs.append((o, p, s))
        (o, p, s), (o2, p2, s2) = runs
        r = _Res()
        if out:
            assert torch.equal(o.buf, o2.buf), f"{what}: out not repeatable"
            assert o.intact(), f"{what}: wrote outside out"
            r.out = o.np((K, K, batch) if inverse else (n_out, batch))
        if ps:
            assert torch.equal(p.buf, p2.buf), f"{what}: ladj_ps not repeatable"
            assert p.intact(), f"{what}: wrote outside ladj_ps"
            r.ps = p.np((batch,))
        if sm:
            assert torch.equal(s, s2), f"{what}: ladj_sum not repeatable"
            sh = host(s)
            assert sh[0] == MARK and sh[2] == MARK, f"{what}: wrote next to ladj_sum"
            r.sum = float(sh[1])
        return r

    def inv_vjp(self, uplo, y, Wb, lb, K, batch, off_y=0, off_yb=0, off_w=0, what=""):
        """bjx_vec_cholesky_inv_vjp twice (identical bits), guard checked -> y_bar (n, batch)"""
        n = R.nvec(K)
        y_d, w_d, l_d = self.put(y, off_y), self.put(Wb, off_w), (self.put(lb) if lb is not None else None)
        runs = []
        for _ in range(2):
            g = _Guard(self, n, batch, off_yb)
            rc = self.lib.bjx_vec_cholesky_inv_vjp(self.ctx.h, self.dtc, ord(uplo), _p(y_d), _p(w_d), _p(l_d), _p(g.view), K, batch)
            self.L.check(self.ctx.h, rc, "bjx_vec_cholesky_inv_vjp")
            runs.append(g)
        assert torch.equal(runs[0].buf, runs[1].buf), f"{what}: y_bar not repeatable"
        assert runs[0].intact(), f"{what}: wrote outside y_bar"
        return runs[0].np((n, batch))

    def fwd_vjp(self, uplo, W, yb, K, batch, off_w=0, off_yb=0, off_wb=0, what=""):
        """bjx_vec_cholesky_fwd_vjp twice (identical bits), guard checked -> W_bar (K, K, batch)"""
        w_d, g_d = self.put(W, off_w), self.put(yb, off_yb)
        runs = []
        for _ in range(2):
            g = _Guard(self, K * K, batch, off_wb)
            rc = self.lib.bjx_vec_cholesky_fwd_vjp(self.ctx.h, self.dtc, ord(uplo), _p(w_d), _p(g_d), _p(g.view), K, batch)
            self.L.check(self.ctx.h, rc, "bjx_vec_cholesky_fwd_vjp")
            runs.append(g)
        assert torch.equal(runs[0].buf, runs[1].buf), f"{what}: W_bar not repeatable"
        assert runs[0].intact(), f"{what}: wrote outside W_bar"
        return runs[0].np((K, K, batch))


# ------------------------------------------------------------------ references, computed once per (dtype, K, batch, uplo)
@functools.lru_cache(maxsize=None)
def _ref_inverse(dtname, K, batch, uplo):
    return R.ref_inverse(R.draw(dtname, K, batch)["y"], uplo)


@functools.lru_cache(maxsize=None)
def _ref_forward(dtname, K, batch, uplo):
    return R.ref_forward(R.for_uplo(R.draw(dtname, K, batch)["W"], uplo), uplo)


@functools.lru_cache(maxsize=None)
def _ref_inv_vjp(dtname, K, batch, uplo, with_l=True):
    d = R.draw(dtname, K, batch)
    return R.ref_inv_vjp(d["y"], R.for_uplo(d["W_bar"], uplo), d["logJ_bar"] if with_l else None, uplo)


@functools.lru_cache(maxsize=None)
def _ref_fwd_vjp(dtname, K, batch, uplo):
    d = R.draw(dtname, K, batch)
    return R.ref_fwd_vjp(R.for_uplo(d["W"], uplo), d["y_bar"], uplo)


def _name(form):
    return form[0] if len(form) == 1 else f"{form[0]}({','.join(str(v) for v in form[1:])})"


def _check_inverse(c, r, ref, uplo, K, batch, what):
    Wr, lr = ref
    if r.out is not None:
        flat_close(r.out, Wr, c.dt, f"{what} W", per="sample")
        assert (r.out[R.unused_triangle(K, uplo)] == 0).all(), f"{what}: the triangle that '{uplo}' does not name is not exactly zero"
        assert (r.out[0, 0] == 1).all(), f"{what}: W[0,0] is not exactly 1"
        U = np.asarray(r.out if uplo == "U" else np.transpose(r.out, T3), np.float64)
        assert np.abs(np.sqrt((U * U).sum(axis=0)) - 1.0).max() <= c.rtol, f"{what}: a column of the factor is not of unit norm"
    if r.ps is not None:
        flat_close(r.ps, lr, c.dt, f"{what} logJ", per="element", floor=R.LOG_DET_FLOOR)
    if r.sum is not None:
        sum_close(r.sum, np.asarray(lr, np.float64).sum(), c.dt.type, R.nvec(K) * batch, f"{what} ladj_sum")


def _check_forward(c, r, ref, K, batch, what):
    yr, lr = ref
    flat_close(r.out, yr, c.dt, f"{what} y", per="sample")
    if r.ps is not None:
        flat_close(r.ps, lr, c.dt, f"{what} ladj", per="element", floor=R.LOG_DET_FLOOR)
    if r.sum is not None:
        sum_close(r.sum, np.asarray(lr, np.float64).sum(), c.dt.type, R.nvec(K) * batch, f"{what} ladj_sum")


def _with_nan(W, K, uplo):
    Wn = np.array(W, order="F")
    Wn[R.unused_triangle(K, uplo)] = np.nan
    return Wn


def _zero_outside_strict_triangle(Wb, K, uplo):
    return bool((Wb[R.unused_triangle(K, uplo)] == 0).all()) and bool((Wb[np.arange(K), np.arange(K)] == 0).all())


VALUE_SHAPES = [(dt, K, form) for dt in R.DTS for form, lohi in R.VALUE_FORMS[dt] for K in lohi]
VALUE_IDS = [f"{dt.name}-{K}-{_name(form)}" for dt, K, form in VALUE_SHAPES]
OFFSET_SHAPES = [(dt, K, form) for dt in R.DTS for K, form in R.OFFSET_FORMS[dt]]
OFFSET_IDS = [f"{dt.name}-{K}-{_name(form)}" for dt, K, form in OFFSET_SHAPES]
FWD_VJP_SHAPES = [(dt, K, a, form) for dt in R.DTS for K, a, form in R.FWD_VJP_SHAPES[dt]]
FWD_VJP_IDS = [f"{dt.name}-{K}-{_name(form)}{'' if a else '-offset'}" for dt, K, a, form in FWD_VJP_SHAPES]
DT_IDS = [dt.name for dt in R.DTS]


# ------------------------------------------------------------------ bjx_vec_cholesky
def _value_both_uplo(c, d, K, batch, tag, off_y=0, off_w=0, nan_triangle=False):
    """inverse (with and without `out`) and forward at both `uplo`, each against the reference; 'L' == transpose of 'U' bit for bit"""
    name = c.dt.name
    got = {}
    for uplo in "UL":
        what = f"{tag} {uplo} batch={batch}"
        ri = c.value(1, uplo, d["y"], K, batch, off_in=off_y, off_out=off_w, what=f"{what} inverse")
        _check_inverse(c, ri, _ref_inverse(name, K, batch, uplo), uplo, K, batch, f"{what} inverse")
        rn = c.value(1, uplo, d["y"], K, batch, out=False, off_in=off_y, what=f"{what} inverse out=NULL")
        _check_inverse(c, rn, _ref_inverse(name, K, batch, uplo), uplo, K, batch, f"{what} inverse out=NULL")
        Wu = R.for_uplo(d["W"], uplo)
        rf = c.value(0, uplo, Wu, K, batch, off_in=off_w, off_out=off_y, what=f"{what} forward")
        _check_forward(c, rf, _ref_forward(name, K, batch, uplo), K, batch, f"{what} forward")
        if nan_triangle:
            rx = c.value(0, uplo, _with_nan(Wu, K, uplo), K, batch, off_in=off_w, off_out=off_y, what=f"{what} forward, NaN in the unused triangle")
            assert np.array_equal(rx.out, rf.out) and np.array_equal(rx.ps, rf.ps) and rx.sum == rf.sum, f"{what}: the forward link reads the triangle that '{uplo}' does not name"
        got[uplo] = (ri, rn, rf)
    (iu, nu, fu), (il, nl, fl) = got["U"], got["L"]
    assert np.array_equal(il.out, np.transpose(iu.out, T3)), f"{tag} batch={batch}: W of 'L' is not the transpose of W of 'U' bit for bit"
    assert np.array_equal(il.ps, iu.ps) and np.array_equal(nl.ps, nu.ps), f"{tag} batch={batch}: logJ differs between 'U' and 'L'"
    assert np.array_equal(fl.out, fu.out) and np.array_equal(fl.ps, fu.ps), f"{tag} batch={batch}: the forward of the transposed factor differs between 'U' and 'L'"


@pytest.mark.parametrize("dt,K,form", VALUE_SHAPES, ids=VALUE_IDS)
def test_value_every_form_and_batch_edge(bj, dt, K, form):
    c = _Call(bj, dt)
    bs = R.batches(form)
    for batch in bs:
        _value_both_uplo(c, R.draw(dt.name, K, batch), K, batch, f"vec_cholesky_abi value {_name(form)} {dt.name} K={K}", nan_triangle=batch == bs[-1])


@pytest.mark.parametrize("dt,K,form", OFFSET_SHAPES, ids=OFFSET_IDS)
def test_value_with_the_deciding_pointer_off_the_pack_boundary(bj, dt, K, form):
    """the packed vector (`in` of the inverse, `out` of the forward) one element off: V = 1 at every K"""
    c = _Call(bj, dt)
    for batch in R.batches(form)[-2:]:
        _value_both_uplo(c, R.draw(dt.name, K, batch), K, batch, f"vec_cholesky_abi value offset {_name(form)} {dt.name} K={K}", off_y=1, nan_triangle=True)


@pytest.mark.parametrize("dt,K", [(dt, K) for dt in R.DTS for K in R.FIRST_ROW_KS[dt]], ids=[f"{dt.name}-{K}" for dt in R.DTS for K in R.FIRST_ROW_KS[dt]])
def test_forward_first_row_at_both_ends_of_atanh_and_both_signs(bj, dt, K):
    """y = atanh(W[1, j]) of the lane kernel at |y| = 1e-6 ... 1e-4 (at K = 2 the entry is the whole sample: an ulp of 1 is 1e-2 of it) and
    at |y| = 5 ... 6 (|w| within 200 Float32 ulp of 1: a form that rounds 1 + x near x = -1 loses e^{2|y|} ulp), both signs; sample
    2m + 1 is the negative of sample 2m and, in Float32, must come back as its negative bit for bit (the link is odd in every entry), with the same log-det"""
    c = _Call(bj, dt)
    d = R.draw_first_row_edges(dt.name, K)
    batch = d["y"].shape[1]
    for uplo in "UL":
        what = f"vec_cholesky_abi first_row lane {dt.name} K={K} {uplo} batch={batch} forward"
        Wu = R.for_uplo(d["W"], uplo)
        r = c.value(0, uplo, Wu, K, batch, what=what)
        _check_forward(c, r, R.ref_forward(Wu, uplo), K, batch, what)
        if c.dt == np.float32:      # the Float32 link takes every entry's magnitude and restores the sign; the Float64 x_atanh is odd to 1e-11 only (under the bar above)
            assert np.array_equal(r.out[:, 1::2], -r.out[:, ::2]), f"{what}: atanh(-w) is not -atanh(w) bit for bit"
        assert np.array_equal(r.ps[1::2], r.ps[::2]), f"{what}: the log-det changes with the sign of the factor's entries"
        ri = c.value(1, uplo, d["y"], K, batch, what=what.replace("forward", "inverse"))
        _check_inverse(c, ri, R.ref_inverse(d["y"], uplo), uplo, K, batch, what.replace("forward", "inverse"))


@pytest.mark.parametrize("K", R.MIXED_KS)
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_value_mixed_alignments(bj, dt, K):
    """only the packed vector offset, only the dense W offset (the device-side unaligned branch at every sample), both"""
    c = _Call(bj, dt)
    batch = 3
    for off_y, off_w in ((1, 0), (0, 1), (1, 1)):
        _value_both_uplo(c, R.draw(dt.name, K, batch), K, batch, f"vec_cholesky_abi value mixed y+{off_y} W+{off_w} {dt.name} K={K}", off_y=off_y, off_w=off_w)


@pytest.mark.parametrize("dt,K,form", VALUE_SHAPES, ids=VALUE_IDS)
def test_a_sample_gives_the_same_bits_alone_and_at_every_index_of_a_batch(bj, dt, K, form):
    """every kernel works one sample per lane or per wave with arithmetic that does not depend on the sample's index"""
    c = _Call(bj, dt)
    d = R.draw(dt.name, K, 5)
    refused = R.inv_vjp_form(dt, K) == ("refused",)
    for uplo in "UL":
        what = f"vec_cholesky_abi position {_name(form)} {dt.name} K={K} {uplo}"
        W, Wb = R.for_uplo(d["W"], uplo), R.for_uplo(d["W_bar"], uplo)
        i0 = c.value(1, uplo, d["y"][:, :1], K, 1, what=what)
        f0 = c.value(0, uplo, W[:, :, :1], K, 1, what=what)
        g0 = None if refused else c.inv_vjp(uplo, d["y"][:, :1], Wb[:, :, :1], d["logJ_bar"][:1], K, 1, what=what)
        h0 = c.fwd_vjp(uplo, W[:, :, :1], d["y_bar"][:, :1], K, 1, what=what)
        for j in range(5):
            perm = np.arange(5)
            perm[[0, j]] = [j, 0]                       # samples 0 and j change places
            ri = c.value(1, uplo, d["y"][:, perm], K, 5, what=what)
            assert np.array_equal(ri.out[:, :, j], i0.out[:, :, 0]) and ri.ps[j] == i0.ps[0], f"{what}: the inverse of sample 0 differs at index {j}"
            rf = c.value(0, uplo, W[:, :, perm], K, 5, what=what)
            assert np.array_equal(rf.out[:, j], f0.out[:, 0]) and rf.ps[j] == f0.ps[0], f"{what}: the forward of sample 0 differs at index {j}"
            h = c.fwd_vjp(uplo, W[:, :, perm], d["y_bar"][:, perm], K, 5, what=what)
            assert np.array_equal(h[:, :, j], h0[:, :, 0]), f"{what}: the forward link's pullback of sample 0 differs at index {j}"
            if not refused:
                g = c.inv_vjp(uplo, d["y"][:, perm], Wb[:, :, perm], d["logJ_bar"][perm], K, 5, what=what)
                assert np.array_equal(g[:, j], g0[:, 0]), f"{what}: the inverse's pullback of sample 0 differs at index {j}"


def _variant_shapes(dt):
    """one small and one large K per form family (lane, chunk, generic), and the smallest K of chunk (1, 16)"""
    forms = dict(R.VALUE_FORMS[dt])
    lane = forms[("lane", R.vw(dt))]
    return [(lane[0], 65), (lane[1], 65), (forms[("chunk", 1, 2)][0], 3), (forms[("chunk", 1, 16)][0], 3), (64, 3), (65, 5), (100, 5)]


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_value_every_combination_of_optional_pointers(bj, dt):
    """inverse: out NULL with ladj_ps, out NULL with ladj_sum only, out with no log-det pointer, everything; forward: no log-det pointer
    (LADJ = false), ladj_ps only, ladj_sum only, both"""
    c = _Call(bj, dt)
    for K, batch in _variant_shapes(dt):
        d = R.draw(dt.name, K, batch)
        for uplo in "UL":
            for out, ps, sm in ((0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 1), (1, 0, 1)):
                what = f"vec_cholesky_abi variants {dt.name} K={K} {uplo} inverse out={out} ps={ps} sum={sm}"
                _check_inverse(c, c.value(1, uplo, d["y"], K, batch, out=out, ps=ps, sm=sm, what=what), _ref_inverse(dt.name, K, batch, uplo), uplo, K, batch, what)
            for ps, sm in ((0, 0), (1, 0), (0, 1), (1, 1)):
                what = f"vec_cholesky_abi variants {dt.name} K={K} {uplo} forward ps={ps} sum={sm}"
                _check_forward(c, c.value(0, uplo, R.for_uplo(d["W"], uplo), K, batch, ps=ps, sm=sm, what=what), _ref_forward(dt.name, K, batch, uplo), K, batch, what)


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_accumulate_adds_into_both_log_det_outputs(bj, dt):
    """BJX_ACCUMULATE: ladj_ps == p + l EXACTLY in the type (l = what the same call returns without the flag; the kernels add in T),
    ladj_sum == s + Σ l within the sum bar"""
    c = _Call(bj, dt)
    s0 = -3.5
    for K, batch in _variant_shapes(dt):
        d = R.draw(dt.name, K, batch)
        pre = R.rng_for("accumulate", dt.name, K, batch).normal(size=batch).astype(dt)
        for uplo in "UL":
            for inverse, x, outs in ((1, d["y"], (1, 0)), (0, R.for_uplo(d["W"], uplo), (1,))):
                for out in outs:
                    what = f"vec_cholesky_abi accumulate {dt.name} K={K} {uplo} inverse={inverse} out={out}"
                    plain = c.value(inverse, uplo, x, K, batch, out=out, what=what)
                    acc = c.value(inverse, uplo, x, K, batch, out=out, flags=ACC, pre_ps=pre, pre_sum=s0, what=what)
                    assert np.array_equal(acc.ps, pre + plain.ps), f"{what}: ladj_ps is not p + l in the type"
                    sum_close(acc.sum, s0 + np.asarray(plain.ps, np.float64).sum(), c.dt.type, R.nvec(K) * batch, f"{what} ladj_sum")
                    if out:
                        assert np.array_equal(acc.out, plain.out), f"{what}: the flag changes out"


# ------------------------------------------------------------------ bjx_vec_cholesky_inv_vjp
def _inv_vjp_both_uplo(c, d, K, batch, tag, off_y=0, off_yb=0, off_w=0, null_l=False):
    name = c.dt.name
    got = {}
    for uplo in "UL":
        what = f"{tag} {uplo} batch={batch}"
        Wb = R.for_uplo(d["W_bar"], uplo)
        g = c.inv_vjp(uplo, d["y"], Wb, d["logJ_bar"], K, batch, off_y, off_yb, off_w, what=what)
        flat_close(g, _ref_inv_vjp(name, K, batch, uplo), c.dt, f"{what} y_bar", per="sample")
        if null_l:
            g0 = c.inv_vjp(uplo, d["y"], Wb, None, K, batch, off_y, off_yb, off_w, what=f"{what} logJ_bar=NULL")
            flat_close(g0, _ref_inv_vjp(name, K, batch, uplo, False), c.dt, f"{what} logJ_bar=NULL y_bar", per="sample")
        got[uplo] = g
    assert np.array_equal(got["L"], got["U"]), f"{tag} batch={batch}: y_bar of the transposed W_bar differs between 'U' and 'L'"


@pytest.mark.parametrize("dt,K,form", [s for s in VALUE_SHAPES if s[2] != ("generic",)], ids=[i for i, s in zip(VALUE_IDS, VALUE_SHAPES) if s[2] != ("generic",)])
def test_inv_vjp_every_form_and_batch_edge(bj, dt, K, form):
    c = _Call(bj, dt)
    bs = R.batches(form)
    for batch in bs:
        _inv_vjp_both_uplo(c, R.draw(dt.name, K, batch), K, batch, f"vec_cholesky_abi inv_vjp {_name(form)} {dt.name} K={K}", null_l=batch == bs[-1])


@pytest.mark.parametrize("dt,K,form", OFFSET_SHAPES, ids=OFFSET_IDS)
def test_inv_vjp_with_a_deciding_pointer_off_the_pack_boundary(bj, dt, K, form):
    """y, y_bar or both one element off: V = 1 at every K; at K = 16, 33, 64 also only W_bar (the device-side branch), and all three"""
    c = _Call(bj, dt)
    batch = R.batches(form)[-1]
    d = R.draw(dt.name, K, batch)
    offs = [(1, 1, 0), (1, 0, 0), (0, 1, 0)] + ([(0, 0, 1), (1, 1, 1)] if K in R.MIXED_KS else [])
    for off_y, off_yb, off_w in offs:
        _inv_vjp_both_uplo(c, d, K, batch, f"vec_cholesky_abi inv_vjp offset y+{off_y} y_bar+{off_yb} W_bar+{off_w} {dt.name} K={K}", off_y, off_yb, off_w, null_l=True)


# ------------------------------------------------------------------ bjx_vec_cholesky_fwd_vjp
@pytest.mark.parametrize("dt,K,aligned,form", FWD_VJP_SHAPES, ids=FWD_VJP_IDS)
def test_fwd_vjp_every_form_and_batch_edge(bj, dt, K, aligned, form):
    c = _Call(bj, dt)
    if aligned:
        offsets = [(0, 0, 0)]
    else:
        offsets = [(1, 0, 0), (0, 1, 0), (0, 0, 1)] if form[0] == "lane" else [(0, 0, 1)]
    bs = R.fwd_vjp_batches(K, form)
    for batch in bs if aligned else bs[-2:]:
        d = R.draw(dt.name, K, batch)
        for offs in offsets:
            got = {}
            for uplo in "UL":
                what = f"vec_cholesky_abi fwd_vjp {_name(form)} {dt.name} K={K} {uplo} batch={batch}" + ("" if aligned else f" offsets {offs}")
                W = R.for_uplo(d["W"], uplo)
                g = c.fwd_vjp(uplo, W, d["y_bar"], K, batch, *offs, what=what)
                flat_close(g, _ref_fwd_vjp(dt.name, K, batch, uplo), c.dt, f"{what} W_bar", per="sample")
                assert _zero_outside_strict_triangle(g, K, uplo), f"{what}: W_bar is not exactly zero on the diagonal and in the unused triangle"
                if batch == bs[-1]:
                    gx = c.fwd_vjp(uplo, _with_nan(W, K, uplo), d["y_bar"], K, batch, *offs, what=f"{what} NaN in the unused triangle")
                    assert np.array_equal(gx, g), f"{what}: the pullback reads the triangle that '{uplo}' does not name"
                got[uplo] = g
            assert np.array_equal(got["L"], np.transpose(got["U"], T3)), f"fwd_vjp {dt.name} K={K} batch={batch}: W_bar of 'L' is not the transpose of W_bar of 'U' bit for bit"


# ------------------------------------------------------------------ the `s0` loop of the lane kernels
@pytest.mark.parametrize("entry", ["value", "inv_vjp", "fwd_vjp"])
@pytest.mark.parametrize("K", R.LANE_TRIP_KS)
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_lane_kernels_second_and_third_trip_of_the_capped_grid(bj, dt, K, entry):
    """2·(32·CUs)·64 + 65 samples: the grid of the four lane kernels is capped at 32 tiles of 64 samples per CU, so every block takes a
    second trip of its `s0` loop and the first two a third.  The oracle's forward-link pullback loops in Python per sample: its operands
    repeat with the prime period 997 (no multiple of the trip stride), the reference of the first 997 samples is tiled.

    [float32-2-inv_vjp] is the regression test of the Float64 evaluation of the K = 2 pullback: at K = 2 a sample of y_bar is ONE number,
    the sum (1 − z²)·W̄[1,2] − z·(W[2,2]·W̄[2,2] + 2·ℓ̄) of two terms of either sign, and among a million standard normal cotangents some
    cancel to 1e-6 of their terms.  In Float32 arithmetic the kernel was up to 7.2e-2 of the sample's value off (26 samples over 1e-3,
    largest absolute error 1.2e-6; the reference's own loops in Float32 on the same draw: 0.12, 20 samples); now 6.0e-8."""
    c = _Call(bj, dt)
    batch = R.lane_trip_batch(torch.cuda.get_device_properties(0).multi_processor_count)
    d = R.draw(dt.name, K, batch)
    for uplo in "UL":
        what = f"vec_cholesky_abi trips lane {dt.name} K={K} {uplo} batch={batch}"
        if entry == "value":
            _check_inverse(c, c.value(1, uplo, d["y"], K, batch, what=what), R.ref_inverse(d["y"], uplo), uplo, K, batch, f"{what} inverse")
            W = R.for_uplo(d["W"], uplo)
            _check_forward(c, c.value(0, uplo, W, K, batch, what=what), R.ref_forward(W, uplo), K, batch, f"{what} forward")
        elif entry == "inv_vjp":
            Wb = R.for_uplo(d["W_bar"], uplo)
            flat_close(c.inv_vjp(uplo, d["y"], Wb, d["logJ_bar"], K, batch, what=what), R.ref_inv_vjp(d["y"], Wb, d["logJ_bar"], uplo), c.dt, f"{what} inv_vjp y_bar", per="sample")
        else:
            period = 997
            rep = np.arange(batch) % period
            Wp, gp = R.for_uplo(np.asfortranarray(d["W"][:, :, rep]), uplo), np.asfortranarray(d["y_bar"][:, rep])
            flat_close(c.fwd_vjp(uplo, Wp, gp, K, batch, what=what), R.ref_fwd_vjp(Wp, gp, uplo, period=period), c.dt, f"{what} fwd_vjp W_bar", per="sample")


# ------------------------------------------------------------------ K = 1, batch == 0, contracts
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_k_equal_one(bj, dt):
    """K = 1 (n = 0): the inverse writes W = 1 and log-det 0 from a NULL input, the forward writes nothing and log-det 0, fwd_vjp writes
    zeros, inv_vjp returns BJX_OK and touches nothing"""
    c = _Call(bj, dt)
    for batch in (1, 5):
        for uplo in "UL":
            what = f"K=1 {dt.name} {uplo} batch={batch}"
            r = c.value(1, uplo, None, 1, batch, what=what)
            assert (r.out == 1).all() and (r.ps == 0).all() and r.sum == 0.0, what
            r = c.value(1, uplo, None, 1, batch, out=False, what=what)
            assert (r.ps == 0).all() and r.sum == 0.0, what
            for x in (None, np.ones((1, 1, batch))):
                r = c.value(0, uplo, x, 1, batch, what=what)            # `out` has no element: its guard stays all markers
                assert r.out.size == 0 and (r.ps == 0).all() and r.sum == 0.0, what
            g = _Guard(c, 1, batch)
            rc = c.lib.bjx_vec_cholesky_fwd_vjp(c.ctx.h, c.dtc, ord(uplo), _p(c.put(np.ones(batch))), None, _p(g.view), 1, batch)
            c.L.check(c.ctx.h, rc, "bjx_vec_cholesky_fwd_vjp")
            assert g.intact() and (g.np((batch,)) == 0).all(), what
            g = _Guard(c, 1, batch)
            assert c.lib.bjx_vec_cholesky_inv_vjp(c.ctx.h, c.dtc, ord(uplo), None, None, None, None, 1, batch) == 0
            assert c.lib.bjx_vec_cholesky_inv_vjp(c.ctx.h, c.dtc, ord(uplo), None, _p(g.view), None, _p(g.view), 1, batch) == 0
            torch.cuda.synchronize()
            assert g.intact(False), what


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_empty_batch(bj, dt):
    """batch == 0: BJX_OK, nothing written; ladj_sum zeroed without BJX_ACCUMULATE and left alone with it"""
    c = _Call(bj, dt)
    K = 12
    d = R.draw(dt.name, K, 3)
    for inverse, x in ((1, d["y"]), (0, d["W"])):
        x_d = c.put(x)
        for flags, want in ((0, 0.0), (ACC, MARK)):
            o, p = _Guard(c, K * K, 3), _Guard(c, 1, 3)
            s = torch.full((3,), MARK, dtype=torch.float64, device="cuda")
            assert c.lib.bjx_vec_cholesky(c.ctx.h, c.dtc, inverse, ord("U"), _p(x_d), _p(o.view), _p(p.view), _p(s[1:]), K, 0, flags) == 0
            assert c.lib.bjx_vec_cholesky(c.ctx.h, c.dtc, inverse, ord("L"), None, None, None, None, K, 0, flags) == 0
            torch.cuda.synchronize()
            assert o.intact(False) and p.intact(False) and host(s).tolist() == [MARK, want, MARK], (inverse, flags)
    g, w = _Guard(c, K * K, 3), _Guard(c, R.nvec(K), 3)
    assert c.lib.bjx_vec_cholesky_inv_vjp(c.ctx.h, c.dtc, ord("U"), _p(c.put(d["y"])), _p(c.put(d["W_bar"])), None, _p(w.view), K, 0) == 0
    assert c.lib.bjx_vec_cholesky_fwd_vjp(c.ctx.h, c.dtc, ord("U"), _p(c.put(d["W"])), _p(c.put(d["y_bar"])), _p(g.view), K, 0) == 0
    assert c.lib.bjx_vec_cholesky_inv_vjp(c.ctx.h, c.dtc, ord("U"), None, None, None, None, K, 0) == 0
    assert c.lib.bjx_vec_cholesky_fwd_vjp(c.ctx.h, c.dtc, ord("U"), None, None, None, K, 0) == 0
    torch.cuda.synchronize()
    assert g.intact(False) and w.intact(False)


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_contracts_and_refusals_write_nothing(bj, dt):
    """a bad `uplo` and the forward link without `out`: BJX_ERR_ARG; inv_vjp above K = 64 and fwd_vjp above K = 165 (Float32) / 116
    (Float64): BJX_ERR_UNSUPPORTED with K in the message; nothing launched, every output still all markers"""
    c = _Call(bj, dt)
    K, batch = 12, 3
    d = R.draw(dt.name, K, batch)
    y_d, W_d, Wb_d, yb_d = c.put(d["y"]), c.put(d["W"]), c.put(d["W_bar"]), c.put(d["y_bar"])
    o, w, p = _Guard(c, K * K, batch), _Guard(c, R.nvec(K), batch), _Guard(c, 1, batch)
    s = torch.full((3,), MARK, dtype=torch.float64, device="cuda")
    n0 = c.lib.bjx_launch_count()
    for bad in (ord("X"), ord("u"), 0):
        assert c.lib.bjx_vec_cholesky(c.ctx.h, c.dtc, 1, bad, _p(y_d), _p(o.view), _p(p.view), _p(s[1:]), K, batch, 0) == c.L.ERR_ARG
        assert c.lib.bjx_vec_cholesky(c.ctx.h, c.dtc, 0, bad, _p(W_d), _p(w.view), _p(p.view), _p(s[1:]), K, batch, 0) == c.L.ERR_ARG
        assert c.lib.bjx_vec_cholesky_inv_vjp(c.ctx.h, c.dtc, bad, _p(y_d), _p(Wb_d), None, _p(w.view), K, batch) == c.L.ERR_ARG
        assert c.lib.bjx_vec_cholesky_fwd_vjp(c.ctx.h, c.dtc, bad, _p(W_d), _p(yb_d), _p(o.view), K, batch) == c.L.ERR_ARG
    assert c.lib.bjx_vec_cholesky(c.ctx.h, c.dtc, 0, ord("U"), _p(W_d), None, _p(p.view), _p(s[1:]), K, batch, 0) == c.L.ERR_ARG
    assert c.lib.bjx_vec_cholesky(c.ctx.h, c.dtc, 0, ord("U"), None, None, _p(p.view), _p(s[1:]), 1, batch, 0) == c.L.ERR_ARG
    torch.cuda.synchronize()
    assert o.intact(False) and w.intact(False) and p.intact(False) and host(s).tolist() == [MARK] * 3
    for uplo in "UL":
        Kr = R.INV_VJP_REFUSED
        d = R.draw(dt.name, Kr, 1)
        g = _Guard(c, R.nvec(Kr), 1)
        for off in (0, 1):
            assert c.lib.bjx_vec_cholesky_inv_vjp(c.ctx.h, c.dtc, ord(uplo), _p(c.put(d["y"], off)), _p(c.put(d["W_bar"])), _p(c.put(d["logJ_bar"])), _p(g.view), Kr, 1) == c.L.ERR_UNSUPPORTED
            assert str(Kr) in c.lib.bjx_last_error(c.ctx.h).decode()
        Kr = R.FWD_VJP_REFUSED[c.dt]
        n = R.nvec(Kr)
        gw = _Guard(c, Kr * Kr, 1)
        W_z, g_z = torch.zeros(Kr * Kr, dtype=c.tdt, device="cuda"), torch.zeros(n + 1, dtype=c.tdt, device="cuda")
        for off in (0, 1):
            assert c.lib.bjx_vec_cholesky_fwd_vjp(c.ctx.h, c.dtc, ord(uplo), _p(W_z), _p(g_z[off:]), _p(gw.view), Kr, 1) == c.L.ERR_UNSUPPORTED
            assert str(Kr) in c.lib.bjx_last_error(c.ctx.h).decode()
        torch.cuda.synchronize()
        assert g.intact(False) and gw.intact(False)
    assert c.lib.bjx_launch_count() == n0


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_the_largest_served_k_of_both_pullbacks(bj, dt):
    """inv_vjp at K = 64 with every pointer offset (chunk (1, 32), the largest tile) and fwd_vjp at K = 165 | 116 with W_bar offset (the scalar
    form at the LDS limit): served, one step below the refusals of test_contracts_and_refusals_write_nothing"""
    c = _Call(bj, dt)
    K = R.INV_VJP_SERVED
    _inv_vjp_both_uplo(c, R.draw(dt.name, K, 3), K, 3, f"vec_cholesky_abi inv_vjp largest {dt.name} K={K}", 1, 1, 1)
    K = R.FWD_VJP_SERVED[c.dt]
    d = R.draw(dt.name, K, 2)
    g = c.fwd_vjp("U", d["W"], d["y_bar"], K, 2, 0, 0, 1, what=f"fwd_vjp K={K} W_bar offset")
    flat_close(g, _ref_fwd_vjp(dt.name, K, 2, "U"), c.dt, f"vec_cholesky_abi fwd_vjp largest scalar {dt.name} K={K} W_bar offset", per="sample")
    assert _zero_outside_strict_triangle(g, K, "U")
