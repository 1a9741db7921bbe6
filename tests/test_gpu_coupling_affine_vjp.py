"""bjx_coupling_affine_vjp (include/bjx.h; `coupling_affine_vjp_kernel<T, V, INV>` in csrc/bjx_elem.hip) through the C ABI at every form
and edge, against tests/_elem_pullback_ref.py (numpy Float64; pinned on central differences of the oracle by
tests/test_host_elem_pullback_ref.py, which also checks that the reference is finite on every input drawn here).

What the shapes reach (G lanes per column, c = 256 / G columns per block and step of the four-columns-in-flight unroll):
  * both pack widths (a 16-byte pack; one element when dim is no multiple of it or `in` is off the 16-byte boundary), G = 1 ... 64, the
    second trip of the row loop `for (v = gl; v < nvc; v += G)` on three lanes, on lane 0 alone and on every lane;
  * batches 1, c−1, c+1, 2c+1, 4c−1, 4c, 4c+1, 8c+3: one, two or three of the four columns in flight, the block edge, a second block with
    one column, a third block;
  * masks: scattered sorted rows, a contiguous range, an unsorted permutation of a subset, n1 == dim, n1 == 0 with idx1 == NULL;
  * scale / shift / scale_bar / shift_bar / ladj_bar NULL, negative scales, both directions, `in_bar` aliasing `out_bar`;
  * batch == 0, dim == 0, n1 > dim, and the LDS row map limit (dim 15361) as contracts.

Bars: `_tol.flat_close`, the flat 1e-3 (Float32) / 1e-6 (Float64) on the max-norm of each column (per="sample") for all three outputs;
scale_bar, a sum of two terms of either sign per entry, on the larger of that norm and the column's largest summand (`term_scale`: with
n1 == 1 a column is ONE such sum, and on its own value a cancelling sum measured 9.8e-4 in Float32 at dim 3 with correctly rounded terms).
Every call is made twice and must give identical bits; the outputs are views of marker-filled buffers one column longer."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _elem_pullback_ref as R  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, host  # noqa: E402,F401

MARK = 7.25
DTS = [np.float32, np.float64]
SHAPES = [(t, d, a) for t in DTS for d, a in R.COUPLING_SHAPES[np.dtype(t)]]
IDS = [f"{np.dtype(t).name}-{d}{'' if a else '-offset'}" for t, d, a in SHAPES]
# (scale, shift, ladj_bar, scale_bar, shift_bar) passed?
VARIANTS = {"all": (1, 1, 1, 1, 1), "scale=NULL": (0, 1, 1, 1, 1), "shift=NULL": (1, 0, 1, 1, 1), "scale=shift=NULL": (0, 0, 1, 1, 1),
            "scale_bar=NULL": (1, 1, 1, 0, 1), "shift_bar=NULL": (1, 1, 1, 1, 0), "ladj_bar=NULL": (1, 1, 0, 1, 1), "bars=NULL": (1, 1, 1, 0, 0)}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Call:
    def __init__(self, bj, dt, dim):
        self.L = bj._lib
        self.lib = self.L.load()
        self.ctx = bj.context()
        self.dt, self.dim = np.dtype(dt), dim
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dtc = self.L.BJX_F32 if self.dt == np.float32 else self.L.BJX_F64

    def mat(self, a, aligned=True):
        flat = torch.from_numpy(np.array(np.asarray(a, self.dt).T, order="C").reshape(-1))       # (a copy: the drawn arrays are read-only)
        off = 0 if aligned else 1
        buf = torch.full((flat.numel() + off,), MARK, dtype=self.tdt, device="cuda")
        buf[off:] = flat.cuda()
        return buf[off:]

    def guarded(self, rows, batch):
        return torch.full((rows * (batch + 1) + (1 if rows == 0 else 0),), MARK, dtype=self.tdt, device="cuda")

    def run(self, inverse, idx_d, n1, s_d, t_d, x_d, g_d, l_d, ib, sb, tb, batch, dim=None):
        return self.lib.bjx_coupling_affine_vjp(self.ctx.h, self.dtc, int(inverse), _p(idx_d), n1, _p(s_d), _p(t_d), _p(x_d), _p(g_d), _p(l_d), _p(ib), _p(sb), _p(tb),
                                                self.dim if dim is None else dim, batch)


def _mat(buf, rows, batch):
    return host(buf)[:rows * batch].reshape(batch, rows).T


def _operands(c, d, aligned):
    n1 = len(d["idx1"])
    return dict(idx=torch.from_numpy(np.array(d["idx1"])).cuda() if n1 else None, s=c.mat(d["scale"]) if n1 else None, t=c.mat(d["shift"]) if n1 else None,
                x=c.mat(d["x"], aligned), g=c.mat(d["gbar"]), l=torch.from_numpy(np.array(d["lbar"])).cuda())


def _check(c, d, o, batch, inverse, variant, what, alias=False):
    """One call variant, twice (identical bits), against the reference; guards; the rows outside idx1 pass out_bar through bit for bit."""
    dim, n1 = c.dim, len(d["idx1"])
    ws, wt, wl, wsb, wtb = VARIANTS[variant]
    ref = R.ref_coupling_affine_vjp(d["idx1"], d["scale"] if ws else None, d["shift"] if wt else None, d["x"], d["gbar"], d["lbar"] if wl else None, inverse)
    res = []
    for _ in range(2):
        ib, sb, tb = c.guarded(dim, batch), c.guarded(n1, batch), c.guarded(n1, batch)
        g_d = o["g"]
        if alias:
            ib[:dim * batch] = o["g"]
            g_d = ib
        rc = c.run(inverse, o["idx"], n1, o["s"] if ws else None, o["t"] if wt else None, o["x"], g_d, o["l"] if wl else None, ib, sb if wsb else None, tb if wtb else None, batch)
        c.L.check(c.ctx.h, rc, "bjx_coupling_affine_vjp")
        res.append((ib, sb, tb))
    for a, b_ in zip(res[0], res[1]):
        assert torch.equal(a, b_), f"{what}: not repeatable"
    ib, sb, tb = res[0]
    assert bool((ib[dim * batch:] == MARK).all()), f"{what}: wrote past in_bar[:, batch-1]"
    got = _mat(ib, dim, batch)
    flat_close(got, ref[0], c.dt, f"{what} in_bar", per="sample")
    rest = np.setdiff1d(np.arange(dim), d["idx1"])
    assert np.array_equal(got[rest], np.asarray(d["gbar"])[rest]), f"{what}: a row outside idx1 is not out_bar bit for bit"
    ts = R.scale_bar_term_scale(d["idx1"], d["scale"] if ws else None, d["shift"] if wt else None, d["x"], d["gbar"], d["lbar"] if wl else None, inverse)
    for buf, want, r_, name, term in ((sb, wsb, ref[1], "scale_bar", ts), (tb, wtb, ref[2], "shift_bar", None)):
        if want and n1:
            assert bool((buf[n1 * batch:] == MARK).all()), f"{what}: wrote past {name}"
            flat_close(_mat(buf, n1, batch), r_, c.dt, f"{what} {name}", per="sample", term_scale=term)
        else:
            assert bool((buf == MARK).all()), f"{what}: {name} was written"
    return ib


@pytest.mark.parametrize("dt,dim,aligned", SHAPES, ids=IDS)
def test_every_form_batch_mask_direction_and_null_combination(bj, dt, dim, aligned):
    c = _Call(bj, dt, dim)
    v, g = R.lanes(dt, dim, aligned)
    for batch in R.coupling_batches(dt, dim, aligned):
        for mask in R.MASKS:
            d = R.draw_coupling(np.dtype(dt).name, dim, batch, 0, mask)
            o = _operands(c, d, aligned)
            for inverse in (0, 1):
                for variant in (VARIANTS if mask == "scattered" else ("all",)):
                    what = f"coupling_affine_vjp V={v} G={g} dim={dim} batch={batch} {mask} inverse={inverse} {variant}{'' if aligned else ' offset'}"
                    ib = _check(c, d, o, batch, inverse, variant, what)
                    if mask == "none":
                        assert np.array_equal(_mat(ib, dim, batch), np.asarray(d["gbar"])), f"{what}: n1 == 0 must copy out_bar"
                if mask in ("scattered", "unsorted"):
                    ia = _check(c, d, o, batch, inverse, "all", f"coupling_affine_vjp dim={dim} batch={batch} {mask} inverse={inverse} in_bar=out_bar", alias=True)
                    assert torch.equal(ia, _check(c, d, o, batch, inverse, "all", "separate buffers")), "in_bar aliasing out_bar gives other bits"


@pytest.mark.parametrize("dt", DTS)
def test_empty_sizes_and_bad_sizes(bj, dt):
    """batch == 0 and dim == 0: BJX_OK, nothing written; n1 > dim: BJX_ERR_SHAPE, nothing written."""
    dim, batch = 12, 9
    c = _Call(bj, dt, dim)
    d = R.draw_coupling(np.dtype(dt).name, dim, batch, 0, "scattered")
    o = _operands(c, d, True)
    n1 = len(d["idx1"])
    ib, sb, tb = c.guarded(dim, batch), c.guarded(n1, batch), c.guarded(n1, batch)
    n0 = c.lib.bjx_launch_count()
    assert c.run(0, o["idx"], n1, o["s"], o["t"], o["x"], o["g"], o["l"], ib, sb, tb, 0) == 0
    assert c.run(1, o["idx"], 0, o["s"], o["t"], o["x"], o["g"], o["l"], ib, sb, tb, batch, dim=0) == 0
    assert c.run(0, None, 0, None, None, None, None, None, None, None, None, 0) == 0
    assert c.run(0, o["idx"], dim + 1, o["s"], o["t"], o["x"], o["g"], o["l"], ib, sb, tb, batch) == c.L.ERR_SHAPE
    torch.cuda.synchronize()
    assert c.lib.bjx_launch_count() == n0
    assert bool((ib == MARK).all()) and bool((sb == MARK).all()) and bool((tb == MARK).all())


@pytest.mark.parametrize("dt", DTS)
def test_a_row_map_past_the_lds_limit_is_refused_with_nothing_written(bj, dt):
    """dim 15361: the LDS row map would exceed 60 KiB -> BJX_ERR_UNSUPPORTED, nothing written; 15360 rows are served."""
    batch = 1
    for dim, served in ((15361, False), (15360, True)):
        c = _Call(bj, dt, dim)
        d = R.draw_coupling(np.dtype(dt).name, dim, batch, 0, "scattered")
        o = _operands(c, d, True)
        n1 = len(d["idx1"])
        if served:
            _check(c, d, o, batch, 0, "all", f"coupling_affine_vjp dim={dim} (the LDS row map limit) batch=1")
            continue
        ib, sb, tb = c.guarded(dim, batch), c.guarded(n1, batch), c.guarded(n1, batch)
        for inverse in (0, 1):
            assert c.run(inverse, o["idx"], n1, o["s"], o["t"], o["x"], o["g"], o["l"], ib, sb, tb, batch) == c.L.ERR_UNSUPPORTED
            assert "15361" in c.lib.bjx_last_error(c.ctx.h).decode()
        torch.cuda.synchronize()
        assert bool((ib == MARK).all()) and bool((sb == MARK).all()) and bool((tb == MARK).all())
