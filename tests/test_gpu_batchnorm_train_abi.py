"""Training-mode InvertibleBatchNorm through the C ABI at every kernel form and edge (include/bjx.h; csrc/bjx_elem.hip):
bjx_batchnorm_stats -> bjx_batchnorm_train_apply, bjx_batchnorm_train, bjx_row_moments -> bjx_batchnorm_train_vjp.

What the shapes reach (tests/_elem_pullback_ref.py; tests/test_host_elem_pullback_ref.py checks the list against the dispatch rules):
  * the six template forms of `bn_stats_kernel<T, V, R>` (V = a 16-byte pack or one element, R = 1 / 2 / 4 packs per lane), every lane-group
    width, a (dim, batch) view one element into its buffer, today's tallest register-accumulator shapes (1024 / 512 rows);
  * batches that take the tail loop only, one block, two blocks with one trip of the unrolled loop, three and five blocks (the empty
    quarters and the k-tail of `bn_stats_reduce_kernel`), and 4100 columns at 1024 / 512 rows (63 partial sets in the scratch, 65 wanted);
  * columns of more than 256 packs (257, 301, 1028, 2051 rows, ...), REFUSED until the windows of bjx_row_moments were given the per-row
    shift: 2 launches (4 when dim is no multiple of the pack width), whatever the batch;
  * every NULL output of the pullback, `in_bar` aliasing `out_bar`, `in_bar == in`, one operand off the 16-byte boundary, the second
    block of `bn_train_vjp_coef_kernel` (dim > 256);
  * an exactly constant row (variance 0 -> out == b bit for bit), |mean| >> std in both types;
  * the remaining refusals as contracts: BJX_ERR_UNSUPPORTED before any launch, nothing written, the message names the limit.

Bars: `_tol.flat_close`, the flat 1e-3 (Float32) / 1e-6 (Float64): sums per tensor on the largest summand, values and x̄ on the max-norm
of their column (per="sample"), log-dets per element with floor = dim; the moving statistics and the parameter cotangents (one small
tensor each) per tensor.  Every call is made twice and must give identical bits; the outputs are views of marker-filled buffers one
column / one element longer, whose guards must keep the marker."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _elem_pullback_ref as R  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, host  # noqa: E402,F401

MARK = 7.25                                            # guard value: exact in both types, nothing the kernels compute
DTS = [np.float32, np.float64]


def _ids(shapes):
    return [f"{np.dtype(t).name}-{d}{'' if a else '-offset'}" for t, d, a in shapes]


def _shapes(table):
    return [(t, d, a) for t in DTS for d, a in table[np.dtype(t)]]


STATS = _shapes(R.STATS_SHAPES)
LIFTED = _shapes(R.LIFTED_SHAPES)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Ctx:
    def __init__(self, bj, dt):
        self.L = bj._lib
        self.lib = self.L.load()
        self.ctx = bj.context()
        self.dt = np.dtype(dt)
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dtc = self.L.BJX_F32 if self.dt == np.float32 else self.L.BJX_F64

    def launches(self):
        return int(self.lib.bjx_launch_count())

    def mat(self, a, aligned=True):
        """(dim, batch) numpy -> the flat column-major device array, as a view `1 - aligned` elements into its buffer"""
        flat = torch.from_numpy(np.array(np.asarray(a, self.dt).T, order="C").reshape(-1))       # (a copy: the drawn arrays are read-only)
        off = 0 if aligned else 1
        buf = torch.full((flat.numel() + off,), MARK, dtype=self.tdt, device="cuda")
        buf[off:] = flat.cuda()
        v = buf[off:]
        assert (v.data_ptr() % 16 == 0) == bool(aligned) or flat.numel() == 0
        return v

    def vec(self, a, dtype=None):
        return torch.from_numpy(np.array(a, dtype=dtype or self.dt)).cuda()

    def guarded(self, n, guard, tdt=None, aligned=True, prefill=None):
        """n elements + `guard` marker elements behind them (and one in front when the view is to start off the 16-byte boundary)"""
        off = 0 if aligned else 1
        buf = torch.full((off + n + guard,), MARK, dtype=tdt or self.tdt, device="cuda")
        if prefill is not None:
            buf[off:off + n] = torch.from_numpy(np.array(prefill)).cuda()
        return buf, buf[off:]

    def ok(self, rc, what):
        self.L.check(self.ctx.h, rc, what)


def _marked(buf, lo=0, hi=None):
    return bool((buf[lo:hi] == MARK).all())


def _colmat(v, dim, batch):
    return host(v)[:dim * batch].reshape(batch, dim).T


# ------------------------------------------------------------------ bjx_batchnorm_stats
def _stats(c, shift_d, x_d, dim, batch, what, launches=None):
    """two calls with identical bits into guarded buffers -> host stats (2 dim + 1,)"""
    res = []
    for _ in range(2):
        buf, v = c.guarded(2 * dim + 1, 1, torch.float64)
        n0 = c.launches()
        c.ok(c.lib.bjx_batchnorm_stats(c.ctx.h, c.dtc, _p(shift_d), _p(x_d), _p(v), dim, batch), "bjx_batchnorm_stats")
        if launches is not None:
            assert c.launches() - n0 == launches, f"{what}: {c.launches() - n0} launches, {launches} stated in bjx.h"
        res.append(buf)
    assert torch.equal(res[0], res[1]) or bool(torch.isnan(res[0]).any()), f"{what}: stats are not repeatable"
    assert float(res[0][2 * dim + 1]) == MARK, f"{what}: wrote past stats[2 dim]"
    return host(res[0])[:2 * dim + 1]


def _stats_close(got, x, shift, dt, what):
    dim = x.shape[0]
    s1, s2, n = R.ref_stats(x, shift)
    d = np.asarray(x, np.float64) - (0.0 if shift is None else np.asarray(shift, np.float64)[:, None])
    fin = np.isfinite(d)
    t1 = float(np.abs(d[fin]).max()) if fin.any() else 0.0
    flat_close(got[:dim], s1, dt, f"{what} Σ(x−c)", per="tensor", term_scale=t1)
    flat_close(got[dim:2 * dim], s2, dt, f"{what} Σ(x−c)²", per="tensor", term_scale=t1 * t1)
    assert got[2 * dim] == n, f"{what}: count {got[2 * dim]}"


@pytest.mark.parametrize("dt,dim,aligned", STATS + LIFTED, ids=_ids(STATS + LIFTED))
def test_stats_every_form_block_count_and_shift(bj, dt, dim, aligned):
    c = _Ctx(bj, dt)
    form = R.stats_form(dt, dim, aligned)
    batches = R.stats_batches(dt, dim, aligned) if form[2] else list(R.LIFTED_BATCHES)
    if (np.dtype(dt), dim) in ((R.F32, 1024), (R.F64, 512)):
        batches = batches + [4100]                    # the block count capped by the scratch: 63 sets of partials where 65 are wanted
    for batch in batches:
        d = R.draw_bn(np.dtype(dt).name, dim, batch)
        x_d = c.mat(d["x"], aligned)
        for shift in (None, d["m0"]):
            what = f"batchnorm_stats V={form[0]} G={form[1]} R={form[2]} dim={dim} batch={batch} shift={'m' if shift is not None else 'NULL'}{'' if aligned else ' offset'}"
            got = _stats(c, None if shift is None else c.vec(shift), x_d, dim, batch, what, R.stats_launches(dt, dim, aligned))
            _stats_close(got, d["x"], shift, dt, what)


@pytest.mark.parametrize("dt,dim,aligned", STATS + LIFTED, ids=_ids(STATS + LIFTED))
def test_stats_a_nan_poisons_its_own_row_only_and_an_empty_batch_gives_zeros(bj, dt, dim, aligned):
    c = _Ctx(bj, dt)
    g = R.stats_form(dt, dim, aligned)[1]
    batch = 16 * (256 // g) + 1 if R.stats_form(dt, dim, aligned)[2] else 65
    d = R.draw_bn(np.dtype(dt).name, dim, batch)
    x = d["x"].copy(order="F")
    r, col = dim - 1 - (dim // 3), batch - 2
    x[r, col] = np.nan
    got = _stats(c, c.vec(d["m0"]), c.mat(x, aligned), dim, batch, "NaN call")
    assert np.isnan(got[r]) and np.isnan(got[dim + r])
    assert np.isfinite(np.delete(got, [r, dim + r])).all()
    _stats_close(got, x, d["m0"], dt, f"batchnorm_stats NaN at ({r}, {col}) dim={dim} batch={batch}")
    buf, v = c.guarded(2 * dim + 1, 1, torch.float64)
    c.ok(c.lib.bjx_batchnorm_stats(c.ctx.h, c.dtc, _p(c.vec(d["m0"])), None, _p(v), dim, 0), "bjx_batchnorm_stats")
    assert bool((buf[:2 * dim + 1] == 0).all()) and float(buf[2 * dim + 1]) == MARK


# ------------------------------------------------------------------ bjx_batchnorm_train, stats -> bjx_batchnorm_train_apply
def _train(c, d, dim, batch, aligned, variant, two_calls, eps=R.EPS):
    """-> (out buffer, ladj buffer, ladj_sum buffer, m, v) after one training call (or stats -> apply); out / ladj_ps / ladj_sum guarded"""
    Lm = c.L
    pre_l = R.rng_for("pre", dim, batch).normal(size=batch).astype(c.dt)
    acc = variant == "accumulate"
    x_d = c.mat(d["x"], aligned)
    ob, ov = c.guarded(dim * batch, dim, aligned=aligned)
    lb, lv = c.guarded(batch, 1, prefill=pre_l if acc else None)
    sb, sv = c.guarded(1, 1, torch.float64, prefill=np.array([3.5]) if acc else None)
    m_d, v_d = c.guarded(dim, 1, prefill=d["m0"])[0], c.guarded(dim, 1, prefill=d["v0"])[0]
    b_d, logs_d = c.vec(d["b"]), c.vec(d["logs"])
    flags = Lm.BJX_ACCUMULATE if acc else 0
    lp = None if variant == "no_ladj_ps" else lv
    if two_calls:
        stb, stv = c.guarded(2 * dim + 1, 1, torch.float64)
        c.ok(c.lib.bjx_batchnorm_stats(c.ctx.h, c.dtc, _p(m_d), _p(x_d), _p(stv), dim, batch), "bjx_batchnorm_stats")
        c.ok(c.lib.bjx_batchnorm_train_apply(c.ctx.h, c.dtc, _p(b_d), _p(logs_d), _p(m_d), _p(v_d), eps, R.MTM, _p(stv), _p(x_d), _p(ov), _p(lp), _p(sv), dim, batch, flags),
             "bjx_batchnorm_train_apply")
        assert float(stb[2 * dim + 1]) == MARK
    else:
        c.ok(c.lib.bjx_batchnorm_train(c.ctx.h, c.dtc, _p(b_d), _p(logs_d), _p(m_d), _p(v_d), eps, R.MTM, _p(x_d), _p(ov), _p(lp), _p(sv), dim, batch, flags), "bjx_batchnorm_train")
    return ob, lb, sb, m_d, v_d, pre_l


def _check_train(c, orc, d, dim, batch, aligned, what, eps=R.EPS, center=0.0, variants=("both", "accumulate", "no_ladj_ps")):
    f64 = lambda k: np.asarray(d[k], np.float64)
    y_ref, l_ref, m_ref, v_ref = orc.batchnorm_train(f64("b"), f64("logs"), f64("m0") - center, f64("v0"), eps, R.MTM, f64("x") - center)
    m_ref = m_ref + center
    off = 0 if aligned else 1
    for variant in variants:
        runs = [_train(c, d, dim, batch, aligned, variant, two, eps) for two in (False, False, True)]
        for other, name in ((runs[1], "is not repeatable"), (runs[2], "stats -> train_apply gives other bits than bjx_batchnorm_train")):
            for a, b_ in zip(runs[0][:5], other[:5]):
                assert torch.equal(a, b_), f"{what} {variant}: {name}"
        ob, lb, sb, m_d, v_d, pre_l = runs[0]
        assert _marked(ob, off + dim * batch) and _marked(ob, 0, off), f"{what} {variant}: wrote outside out"
        assert float(lb[batch]) == MARK and float(sb[1]) == MARK and float(m_d[dim]) == MARK and float(v_d[dim]) == MARK, f"{what} {variant}: a guard was overwritten"
        flat_close(_colmat(ob[off:], dim, batch), y_ref, c.dt, f"{what} {variant} out", per="sample")
        acc = variant == "accumulate"
        if variant == "no_ladj_ps":
            assert _marked(lb), f"{what}: ladj_ps == NULL but something was stored"
        else:
            flat_close(host(lb)[:batch], l_ref + (pre_l.astype(np.float64) if acc else 0.0), c.dt, f"{what} {variant} ladj_ps", per="element", floor=dim)
        flat_close(host(sb)[:1], np.array([l_ref.sum() + (3.5 if acc else 0.0)]), c.dt, f"{what} {variant} ladj_sum", per="element", floor=dim)
        flat_close(host(m_d)[:dim], m_ref, c.dt, f"{what} {variant} moving mean", per="tensor")
        flat_close(host(v_d)[:dim], v_ref, c.dt, f"{what} {variant} moving variance", per="tensor")
    return runs[0]


@pytest.mark.parametrize("dt,dim,aligned", STATS, ids=_ids(STATS))
def test_train_one_call_and_two_calls_at_every_form(bj, orc, dt, dim, aligned):
    c = _Ctx(bj, dt)
    g = R.stats_form(dt, dim, aligned)[1]
    batch = 16 * (256 // g) + 1                        # two blocks of statistics
    _check_train(c, orc, R.draw_bn(np.dtype(dt).name, dim, batch), dim, batch, aligned, f"batchnorm_train dim={dim} batch={batch}{'' if aligned else ' offset'}")
    _check_train(c, orc, R.draw_bn(np.dtype(dt).name, dim, 2), dim, 2, aligned, f"batchnorm_train dim={dim} batch=2{'' if aligned else ' offset'}", variants=("both",))


@pytest.mark.parametrize("dt,dim,aligned", LIFTED, ids=_ids(LIFTED))
def test_train_on_columns_of_more_than_256_packs(bj, orc, dt, dim, aligned):
    c = _Ctx(bj, dt)
    for batch in R.LIFTED_BATCHES:
        _check_train(c, orc, R.draw_bn(np.dtype(dt).name, dim, batch), dim, batch, aligned, f"batchnorm_train[windows] dim={dim} batch={batch}{'' if aligned else ' offset'}",
                     variants=("both", "accumulate") if batch == 65 else ("both",))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dim", [12, 130, 301])
def test_train_exactly_constant_row(bj, orc, dt, dim):
    """x = 0.5 with moving mean 0.25 in one row: every sum is exact, the variance exactly 0 (the clamp branch) — out == b bit for bit, and
    the log-det carries that row's −log(eps)/2 like every other row's term (the oracle's value, at the flat bar)."""
    c = _Ctx(bj, dt)
    batch = 33
    d = R.draw_bn_constant_row(np.dtype(dt).name, dim, batch)
    ob, lb, sb, m_d, v_d, _ = _check_train(c, orc, d, dim, batch, True, f"batchnorm_train constant row dim={dim}", variants=("both",))
    out = _colmat(ob, dim, batch)
    assert np.array_equal(out[d["row"]], np.full(batch, d["b"][d["row"]])), "variance 0: out != b"
    st = _stats(c, c.vec(d["m0"]), c.mat(d["x"]), dim, batch, "constant row")
    assert st[d["row"]] == 0.25 * batch and st[dim + d["row"]] == 0.0625 * batch


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dim", [8, 257])
def test_train_mean_far_from_zero(bj, orc, dt, dim):
    """|mean| >> std (Float64: mean 1e6, std 1e-2, eps 1e-12, the data of test_batchnorm_training_large_mean_float64; Float32: mean = 100 std
    with the moving mean at 0): the reference in the exact-shift form, the flat bar."""
    c = _Ctx(bj, dt)
    batch = 1000
    d = R.draw_bn_conditioned(np.dtype(dt).name, dim, batch)
    _check_train(c, orc, d, dim, batch, True, f"batchnorm_train |mean|>>std dim={dim}", eps=d["eps"], center=d["center"], variants=("both",))


# ------------------------------------------------------------------ bjx_row_moments -> bjx_batchnorm_train_vjp
def _vjp_call(c, ops, mean_d, var_d, logs_d, eps, dim, batch, mom_d, lsum_d, outs, alias=False, off=(True, True, True)):
    """outs: which of in_bar / b_bar / logs_bar are asked for.  -> (in_bar buffer, b_bar buffer, logs_bar buffer, rc)"""
    x_d, g_d = ops
    ib, iv = c.guarded(dim * batch, dim, aligned=off[2])
    if alias:                                           # in_bar == out_bar: a private copy of the cotangent is overwritten
        gb, g_d = c.guarded(dim * batch, dim, aligned=off[1])
        g_d[:dim * batch] = ops[1]
        ib, iv = gb, g_d
    bb, bv = c.guarded(dim, 1)
    lgb, lgv = c.guarded(dim, 1)
    rc = c.lib.bjx_batchnorm_train_vjp(c.ctx.h, c.dtc, _p(logs_d), _p(mean_d), _p(var_d), eps, _p(mom_d), _p(lsum_d), _p(x_d), _p(g_d),
                                       _p(iv) if "in_bar" in outs else None, _p(bv) if "b_bar" in outs else None, _p(lgv) if "logs_bar" in outs else None, dim, batch)
    return ib, bb, lgb, rc


def _check_vjp(c, orc, d, dim, batch, what, eps=R.EPS, center=0.0, full=True):
    f64 = lambda k: np.asarray(d[k], np.float64)
    mean, var, _ = R.batch_mean_var(d["x"], center)
    xr, br, lr = orc.batchnorm_train_vjp(f64("logs"), eps, f64("x") - center, d["g"], d["lb"])
    xr0 = orc.batchnorm_train_vjp(f64("logs"), eps, f64("x") - center, d["g"], None)
    mean_d, var_d, logs_d = c.vec(mean), c.vec(var), c.vec(d["logs"])
    lsum_d = c.vec([f64("lb").sum()], np.float64)
    x_d, g_d = c.mat(d["x"]), c.mat(d["g"])
    # the moments, twice, guarded, against numpy
    moms = []
    for _ in range(2):
        mb, mv = c.guarded(2 * dim + 1, 1, torch.float64)
        c.ok(c.lib.bjx_row_moments(c.ctx.h, c.dtc, _p(g_d), _p(x_d), _p(mv), dim, batch), "bjx_row_moments")
        moms.append(mb)
    assert torch.equal(moms[0], moms[1]) and float(moms[0][2 * dim + 1]) == MARK, f"{what}: moments"
    mom = host(moms[0])[:2 * dim + 1]
    s1, s2 = R.ref_moments(d["g"], d["x"])
    flat_close(mom[:dim], s1, c.dt, f"{what} moments Σȳ", per="tensor", term_scale=float(np.abs(f64("g")).max()))
    flat_close(mom[dim:2 * dim], s2, c.dt, f"{what} moments Σȳx", per="tensor", term_scale=float(np.abs(f64("g") * f64("x")).max()))
    assert mom[2 * dim] == batch
    mom_d = moms[0][:2 * dim + 1]
    tg = float(np.abs(f64("g")).max())
    n = dim * batch

    def outputs(outs, lsum=lsum_d, ref=(xr, br, lr), tag="", **kw):
        res = [_vjp_call(c, (x_d, g_d), mean_d, var_d, logs_d, eps, dim, batch, mom_d, lsum, outs, **kw) for _ in range(2)]
        for a, b_ in zip(res[0][:3], res[1][:3]):
            assert torch.equal(a, b_), f"{what}{tag}: not repeatable"
        ib, bb, lgb, rc = res[0]
        c.ok(rc, "bjx_batchnorm_train_vjp")
        off = 0 if kw.get("off", (True,) * 3)[1 if kw.get("alias") else 2] else 1
        if "in_bar" in outs:
            assert _marked(ib, off + n) and _marked(ib, 0, off), f"{what}{tag}: wrote outside in_bar"
            flat_close(_colmat(ib[off:], dim, batch), ref[0], c.dt, f"{what}{tag} in_bar", per="sample")
        else:
            assert _marked(ib), f"{what}{tag}: in_bar == NULL but something was stored"
        for buf, name, r_, ts in ((bb, "b_bar", ref[1], tg), (lgb, "logs_bar", ref[2], None)):
            if name in outs:
                assert float(buf[dim]) == MARK, f"{what}{tag}: wrote past {name}"
                flat_close(host(buf)[:dim], r_, c.dt, f"{what}{tag} {name}", per="tensor", term_scale=ts)
            else:
                assert _marked(buf), f"{what}{tag}: {name} == NULL but something was stored"
        return ib

    ib = outputs(("in_bar", "b_bar", "logs_bar"))
    if not full:
        return
    outputs(("in_bar", "b_bar", "logs_bar"), lsum=None, ref=xr0, tag=" ladj_bar_sum=NULL")
    outputs(("b_bar", "logs_bar"), tag=" in_bar=NULL")
    outputs(("in_bar", "logs_bar"), tag=" b_bar=NULL")
    outputs(("in_bar", "b_bar"), tag=" logs_bar=NULL")
    ia = outputs(("in_bar", "b_bar", "logs_bar"), tag=" in_bar=out_bar", alias=True)
    assert torch.equal(ia, ib), f"{what}: in_bar aliasing out_bar gives other bits"
    # one of the three arrays one element off the 16-byte boundary: the one-element form at any dim
    for k, name in enumerate(("in", "out_bar", "in_bar")):
        off = tuple(j != k for j in range(3))
        xo, go = (c.mat(d["x"], off[0]), c.mat(d["g"], off[1]))
        r2 = _vjp_call(c, (xo, go), mean_d, var_d, logs_d, eps, dim, batch, mom_d, lsum_d, ("in_bar", "b_bar", "logs_bar"), off=off)
        c.ok(r2[3], "bjx_batchnorm_train_vjp")
        o = 0 if off[2] else 1
        assert _marked(r2[0], o + n) and _marked(r2[0], 0, o), f"{what} {name} offset: wrote outside in_bar"
        flat_close(_colmat(r2[0][o:], dim, batch), xr, c.dt, f"{what} {name} offset in_bar", per="sample")
    # in_bar == in: refused, nothing written
    n0 = c.launches()
    xcopy = x_d.clone()
    rc = c.lib.bjx_batchnorm_train_vjp(c.ctx.h, c.dtc, _p(logs_d), _p(mean_d), _p(var_d), eps, _p(mom_d), _p(lsum_d), _p(x_d), _p(g_d), _p(x_d), None, None, dim, batch)
    assert rc == c.L.ERR_ARG and c.launches() == n0 and torch.equal(x_d, xcopy), f"{what}: in_bar == in"


VJP = [(t, d) for t in DTS for d in R.VJP_DIMS[np.dtype(t)]]


@pytest.mark.parametrize("dt,dim", VJP, ids=[f"{np.dtype(t).name}-{d}" for t, d in VJP])
def test_pullback_every_output_combination_alias_and_offset(bj, orc, dt, dim):
    c = _Ctx(bj, dt)
    for batch in R.VJP_BATCHES:
        _check_vjp(c, orc, R.draw_bn(np.dtype(dt).name, dim, batch), dim, batch, f"batchnorm_train_vjp dim={dim} batch={batch}", full=batch in (37, 257))


@pytest.mark.parametrize("dt,dim,aligned", LIFTED, ids=_ids(LIFTED))
def test_pullback_on_columns_of_more_than_256_packs(bj, orc, dt, dim, aligned):
    c = _Ctx(bj, dt)
    for batch in R.LIFTED_BATCHES:
        _check_vjp(c, orc, R.draw_bn(np.dtype(dt).name, dim, batch), dim, batch, f"batchnorm_train_vjp[tall] dim={dim} batch={batch}", full=False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dim", [8, 257])
def test_pullback_mean_far_from_zero(bj, orc, dt, dim):
    """The conditioning cases at the flat bar.  A numpy emulation of the kernel's arithmetic (x̄ = p ȳ + q x + r with the coefficients rounded
    to the type) gives 6e-6 of the column scale in Float32 (mean / std = 100) and 7e-10 in Float64 (mean 1e6, std 1e-2, reference in the
    exact-shift form D = X − 1e6): 160x and 1400x of room under the bars."""
    c = _Ctx(bj, dt)
    batch = 1000
    d = R.draw_bn_conditioned(np.dtype(dt).name, dim, batch)
    _check_vjp(c, orc, d, dim, batch, f"batchnorm_train_vjp |mean|>>std dim={dim}", eps=d["eps"], center=d["center"], full=False)


# ------------------------------------------------------------------ the remaining limits, as contracts
STATS_MAX = {R.F32: 26214, R.F64: 21845}               # BnScratch: (2 dim + 2) doubles + 2 dim T + one set of 2 dim partials in the 1 MiB scratch
VJP_MAX = {R.F32: 87381, R.F64: 43690}                 # 3 dim T of coefficients in the 1 MiB scratch


@pytest.mark.parametrize("dt", DTS)
def test_heights_past_the_scratch_are_refused_with_nothing_written(bj, dt):
    c = _Ctx(bj, dt)
    batch = 2
    dim = STATS_MAX[c.dt] + 1
    r = R.rng_for("refused", c.dt.name)
    x_d = c.mat(r.normal(size=(dim, batch)))
    par = {k: c.guarded(dim, 1, prefill=r.uniform(0.5, 1.5, size=dim).astype(c.dt))[0] for k in ("b", "logs", "m", "v")}
    keep = {k: v.clone() for k, v in par.items()}
    stb, stv = c.guarded(2 * dim + 1, 1, torch.float64)
    ob, ov = c.guarded(dim * batch, dim)
    lb, lv = c.guarded(batch, 1)
    sb, sv = c.guarded(1, 1, torch.float64)
    n0 = c.launches()
    calls = {
        "bjx_batchnorm_stats": lambda: c.lib.bjx_batchnorm_stats(c.ctx.h, c.dtc, _p(par["m"]), _p(x_d), _p(stv), dim, batch),
        "bjx_batchnorm_train": lambda: c.lib.bjx_batchnorm_train(c.ctx.h, c.dtc, _p(par["b"]), _p(par["logs"]), _p(par["m"]), _p(par["v"]), R.EPS, R.MTM, _p(x_d), _p(ov), _p(lv), _p(sv), dim, batch, 0),
        "bjx_batchnorm_train_apply": lambda: c.lib.bjx_batchnorm_train_apply(c.ctx.h, c.dtc, _p(par["b"]), _p(par["logs"]), _p(par["m"]), _p(par["v"]), R.EPS, R.MTM, _p(stv), _p(x_d), _p(ov), _p(lv), _p(sv), dim, batch, 0),
    }
    for name, call in calls.items():
        assert call() == c.L.ERR_UNSUPPORTED, name
        msg = c.lib.bjx_last_error(c.ctx.h).decode()
        assert str(STATS_MAX[c.dt]) in msg and str(dim) in msg, f"{name}: the message does not name the limit: {msg!r}"
    torch.cuda.synchronize()
    assert c.launches() == n0, "a refused call launched a kernel"
    assert _marked(stb) and _marked(ob) and _marked(lb) and _marked(sb), "refused, yet something was written"
    assert all(torch.equal(par[k], keep[k]) for k in par), "refused, yet a parameter was written"
    # the tallest column that is served
    dim = STATS_MAX[c.dt]
    d = R.draw_bn(c.dt.name, dim, batch)
    got = _stats(c, c.vec(d["m0"]), c.mat(d["x"]), dim, batch, "tallest", R.stats_launches(dt, dim))
    _stats_close(got, d["x"], d["m0"], dt, f"batchnorm_stats dim={dim} (the scratch bound) batch={batch}")


@pytest.mark.parametrize("dt", DTS)
def test_pullback_past_the_coefficient_table_is_refused_with_nothing_written(bj, dt):
    c = _Ctx(bj, dt)
    batch = 2
    dim = VJP_MAX[c.dt] + 1
    r = R.rng_for("refused vjp", c.dt.name)
    vecs = [c.vec(r.uniform(0.5, 1.5, size=dim)) for _ in range(3)]
    mom = c.vec(r.normal(size=2 * dim + 1), np.float64)
    x_d, g_d = c.mat(r.normal(size=(dim, batch))), c.mat(r.normal(size=(dim, batch)))
    ib, iv = c.guarded(dim * batch, dim)
    bb, bv = c.guarded(dim, 1)
    lgb, lgv = c.guarded(dim, 1)
    n0 = c.launches()
    rc = c.lib.bjx_batchnorm_train_vjp(c.ctx.h, c.dtc, _p(vecs[0]), _p(vecs[1]), _p(vecs[2]), R.EPS, _p(mom), None, _p(x_d), _p(g_d), _p(iv), _p(bv), _p(lgv), dim, batch)
    assert rc == c.L.ERR_UNSUPPORTED
    msg = c.lib.bjx_last_error(c.ctx.h).decode()
    assert str(VJP_MAX[c.dt]) in msg and str(dim) in msg, f"the message does not name the limit: {msg!r}"
    torch.cuda.synchronize()
    assert c.launches() == n0 and _marked(ib) and _marked(bb) and _marked(lgb)


# ------------------------------------------------------------------ the same heights through the Python interface
TRAINING = [(np.float32, 257, True), (np.float32, 301, True), (np.float32, 300, False), (np.float32, 1028, True), (np.float64, 257, True), (np.float64, 514, True)]


@pytest.mark.parametrize("dt,dim,aligned", TRAINING, ids=_ids(TRAINING))
def test_heights_refused_before_pass_through_training(bj, orc, dt, dim, aligned):
    """`with bj.training()`: forward, moving statistics and vjp_params at the heights bjx_batchnorm_stats used to refuse."""
    c = _Ctx(bj, dt)
    batch = 65
    d = R.draw_bn(np.dtype(dt).name, dim, batch)
    f64 = lambda k: np.asarray(d[k], np.float64)
    t = lambda k: torch.from_numpy(np.array(d[k])).cuda()
    bn = bj.InvertibleBatchNorm(t("b"), t("logs"), t("m0"), t("v0"), eps=R.EPS, mtm=R.MTM)
    x_d = c.mat(d["x"], aligned).view(batch, dim).T
    assert (x_d.data_ptr() % 16 == 0) == aligned
    with bj.training():
        y, l = bj.with_logabsdet_jacobian(bn, x_d, per_sample=True)
        xb, grads = bj.vjp_params(bn, x_d, c.mat(d["g"]).view(batch, dim).T, t("lb"))
    y_ref, l_ref, m_ref, v_ref = orc.batchnorm_train(f64("b"), f64("logs"), f64("m0"), f64("v0"), R.EPS, R.MTM, f64("x"))
    xr, br, lr = orc.batchnorm_train_vjp(f64("logs"), R.EPS, f64("x"), d["g"], d["lb"])
    what = f"training() dim={dim}{'' if aligned else ' offset'}"
    flat_close(host(y), y_ref, dt, f"{what} out", per="sample")
    flat_close(host(l), l_ref, dt, f"{what} ladj", per="element", floor=dim)
    flat_close(host(bn.m), m_ref, dt, f"{what} moving mean", per="tensor")
    flat_close(host(bn.v), v_ref, dt, f"{what} moving variance", per="tensor")
    flat_close(host(xb), xr, dt, f"{what} x_bar", per="sample")
    flat_close(host(grads["b"]), br, dt, f"{what} b_bar", per="tensor", term_scale=float(np.abs(f64("g")).max()))
    flat_close(host(grads["logs"]), lr, dt, f"{what} logs_bar", per="tensor")
