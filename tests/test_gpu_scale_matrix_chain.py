"""bjx_scale_matrix_chain (include/bjx.h; `scale_matrix_mfma_kernel<T, NRB, false, PRE = true>` in csrc/bjx_matrix.hip) through the C ABI
at every staging path and tile edge, against tests/_scale_matrix_chain_ref.py (numpy Float64; pinned on the oracle by
tests/test_scale_matrix_chain_ref.py, which also checks that the reference is finite on every input drawn here).

What the shapes reach (Gc = dim / (16 / sizeof(T)) lanes hold one column's log-det parts):
  * the DPP butterfly (Float32, dim 64), `__shfl_xor` (the other powers of two), Float64 LDS atomicAdd (every other dim), Gc == 1;
  * exp / log / Shift / Scale / Scale⁻¹ stages with host scalars and with one value per row (the `lpc[]` parameter-only log-det and the
    reciprocal table), n_ops = 0 … 4;  both directions;  every combination of `out` / `ladj_ps` / BJX_ACCUMULATE / BJX_BASE_STDNORMAL;
  * batches of 1, 15, 16, 17, 63, 64, 65, 257 (one wave / one block / ragged last tiles whose padded columns are log(0) = −inf in the
    MFMA B operand), row padding dim < 16·NRB;
  * the second and third trip of the grid-stride loop with its look-ahead fetch, up to the 160 KiB LDS limit (Float64 at 112 rows);
  * the limits as contracts: BJX_ERR_UNSUPPORTED with nothing written.

Bars: `_tol.flat_close` — the flat 1e-3 (Float32) / 1e-6 (Float64): values on the max-norm of each column (per="sample"), log-det and
density per element with floor = dim (a sum of dim terms of order one).  Every worst error is recorded by `flat_close` (see tests/_tol.py) with
the reduction path in its name."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _scale_matrix_chain_ref as R  # noqa: E402
from _tol import flat_close  # noqa: E402
from test_gpu_parity import bj, dev, host, rng  # noqa: E402,F401

MARK = 7.25                                            # guard value: exact in both types, nothing the kernel computes
SHAPES = [(np.float32, d) for d in R.F32_DIMS] + [(np.float64, d) for d in R.F64_DIMS]
SHAPE_IDS = [f"{np.dtype(t).name}-{d}" for t, d in SHAPES]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Call:
    """One (dtype, dim) of the entry: the library, the context, device operands with a guard column / element behind the outputs."""

    def __init__(self, bj, dt, dim):
        self.L = bj._lib
        self.lib = self.L.load()
        self.ctx = bj.context()
        self.dt, self.dim = np.dtype(dt), dim
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dtc = self.L.BJX_F32 if self.dt == np.float32 else self.L.BJX_F64
        self.keep = []

    def ops(self, ops):
        """the oracle's triples -> bjx_op[]: a host scalar (param_len 1, p0) or one value per row on the device (param_len dim, v0)."""
        arr = (self.L.BjxOp * max(len(ops), 1))()
        for i, (kind, p, _) in enumerate(ops):
            if p is None:
                arr[i] = self.L.BjxOp(kind, 0, 0.0, 0.0, None, None)
            elif np.ndim(p) == 0:
                arr[i] = self.L.BjxOp(kind, 1, float(p), 0.0, None, None)
            else:
                v = torch.from_numpy(np.ascontiguousarray(np.asarray(p, self.dt))).cuda()
                self.keep.append(v)
                arr[i] = self.L.BjxOp(kind, self.dim, 0.0, 0.0, v.data_ptr(), None)
        return arr

    def buffers(self, batch, prefill=None):
        """out (dim, batch) and ladj (batch,) as views of marker-filled buffers one column / one element longer."""
        ob = torch.full(((batch + 1) * self.dim,), MARK, dtype=self.tdt, device="cuda")
        lb = torch.full((batch + 1,), MARK, dtype=self.tdt, device="cuda")
        if prefill is not None:
            lb[:batch] = torch.from_numpy(prefill).cuda()
        return ob, lb

    def run(self, inverse, a_d, arr, n_ops, x_d, ob, lb, batch, flags):
        return self.lib.bjx_scale_matrix_chain(self.ctx.h, self.dtc, inverse, _p(a_d), arr, n_ops, _p(x_d), _p(ob), _p(lb), self.dim, batch, flags)

    def ok(self, *args):
        self.L.check(self.ctx.h, self.run(*args), "bjx_scale_matrix_chain")


def _views(c, ob, lb, batch):
    out = None if ob is None else host(ob)[:batch * c.dim].reshape(batch, c.dim).T
    return out, None if lb is None else host(lb)[:batch]


def _guards_intact(c, ob, lb, batch, what):
    if ob is not None:
        assert bool((ob[batch * c.dim:] == MARK).all()), f"{what}: wrote past out[:, batch-1]"
    if lb is not None:
        assert float(lb[batch]) == MARK, f"{what}: wrote past ladj_ps[batch-1]"


def _check_call(c, a_d, arr, n_ops, x_d, batch, inverse, variant, ref_out, ref_l, ref_lp, pre, what):
    """One call variant, run twice (identical bits), against the reference; the guards behind the outputs keep their marker."""
    Lm = c.L
    want_out, want_l, flags, prefill = {
        "both": (True, True, 0, None),
        "out_only": (True, False, 0, None),
        "ladj_only": (False, True, 0, None),
        "accumulate": (True, True, Lm.BJX_ACCUMULATE, pre),
        "density": (False, True, Lm.BJX_BASE_STDNORMAL, None),
        "density_out": (True, True, Lm.BJX_BASE_STDNORMAL, None),
        "density_accumulate": (False, True, Lm.BJX_BASE_STDNORMAL | Lm.BJX_ACCUMULATE, pre),
    }[variant]
    res = []
    for _ in range(2):
        ob, lb = c.buffers(batch, prefill)
        c.ok(inverse, a_d, arr, n_ops, x_d, ob if want_out else None, lb if want_l else None, batch, flags)
        res.append((ob, lb))
    (ob, lb), (ob2, lb2) = res
    if want_out:
        assert torch.equal(ob, ob2), f"{what}: out is not repeatable"
    if want_l:
        assert torch.equal(lb, lb2), f"{what}: ladj_ps is not repeatable"
    _guards_intact(c, ob, lb, batch, what)
    out, l = _views(c, ob, lb, batch)
    if want_out:
        assert np.isfinite(out).all(), f"{what}: a padded column leaked into out"
        flat_close(out, ref_out, c.dt, f"{what} out", per="sample")
    else:
        assert bool((ob == MARK).all()), f"{what}: out == NULL but something was stored"
    if want_l:
        want = (ref_lp if flags & Lm.BJX_BASE_STDNORMAL else ref_l) + (0.0 if prefill is None else prefill.astype(np.float64))
        assert np.isfinite(l).all(), f"{what}: a padded column leaked into ladj_ps"
        flat_close(l, want, c.dt, f"{what} ladj_ps", per="element", floor=c.dim)
    else:
        assert bool((lb == MARK).all()), f"{what}: ladj_ps == NULL but something was stored"


ALL_VARIANTS = ("both", "out_only", "ladj_only", "accumulate", "density", "density_out", "density_accumulate")


@pytest.mark.parametrize("dt,dim", SHAPES, ids=SHAPE_IDS)
def test_every_family_direction_batch_and_call_variant(bj, dt, dim):
    """Every chain family, both directions (+ a Cholesky factor for the inverse), batches 1 / 17 / 257 (the whole edge list at the edge dims):
    the vector families through all seven call variants, the others with both outputs and with the density and `out` stored."""
    c = _Call(bj, dt, dim)
    path = R.reduction_path(dt, dim)
    mats = [("general", 0), ("general", 1), ("cholesky", 1)]
    for name in R.FAMILIES:
        for batch in R.batches_of(dt, dim):
            ops, x = R.family(name, dim, batch, dt)
            arr, x_d = c.ops(ops), dev(x)
            pre = R.rng_for("pre", name, dim, batch).normal(size=batch).astype(dt) * 3.0 + 1.0
            for kind, inverse in mats:
                if kind == "cholesky" and name not in R.VECTOR_FAMILIES:
                    continue
                a = R.matrix(dim, dt, kind)
                a_d = dev(np.asfortranarray(a))
                ref_out, ref_l = R.ref(a, ops, x, inverse, False)
                ref_lp = R.ref(a, ops, x, inverse, True)[1]
                for variant in (ALL_VARIANTS if name in R.VECTOR_FAMILIES else ("both", "density_out")):
                    _check_call(c, a_d, arr, len(ops), x_d, batch, inverse, variant, ref_out, ref_l, ref_lp, pre,
                                f"scale_matrix_chain[{path}] {name} {kind} inverse={inverse} dim={dim} batch={batch} {variant}")


@pytest.mark.parametrize("dt,dim", SHAPES, ids=SHAPE_IDS)
def test_no_stages_is_bit_identical_to_scale_matrix(bj, dt, dim):
    """n_ops == 0: the same operand order through the same MFMA loop as bjx_scale_matrix — `out` (and the constant log-det) bit for bit;
    the density within the flat bar of the plain entry's."""
    c = _Call(bj, dt, dim)
    for batch in R.batches_of(dt, dim):
        _, x = R.family("none", dim, batch, dt)
        x_d, a_d = dev(x), dev(np.asfortranarray(R.matrix(dim, dt)))
        for inverse in (0, 1):
            for flags in (0, c.L.BJX_BASE_STDNORMAL):
                ob, lb = c.buffers(batch)
                c.ok(inverse, a_d, c.ops([]), 0, x_d, ob, lb, batch, flags)
                ob0, lb0 = c.buffers(batch)
                c.L.check(c.ctx.h, c.lib.bjx_scale_matrix(c.ctx.h, c.dtc, inverse, _p(a_d), _p(x_d), _p(ob0), _p(lb0), None, dim, batch, flags), "bjx_scale_matrix")
                assert torch.equal(ob, ob0), (dim, batch, inverse, flags)
                if flags == 0:
                    assert torch.equal(lb, lb0), (dim, batch, inverse, flags)
                else:                                    # the density: the same accumulators, the constant added in another expression
                    flat_close(host(lb)[:batch], host(lb0)[:batch], dt, f"scale_matrix_chain n_ops=0 density dim={dim} batch={batch} inverse={inverse}", per="element", floor=dim)


@pytest.mark.parametrize("dt,dim", SHAPES, ids=SHAPE_IDS)
def test_a_nan_poisons_its_own_column_only(bj, dt, dim):
    """Column independence: one NaN planted in column j of the ragged last tile (batch 40, j = 35) makes column j of `out` and ladj_ps[j]
    NaN; every other column keeps the bits of the clean call."""
    c = _Call(bj, dt, dim)
    batch, j = 40, 35
    for name in R.VECTOR_FAMILIES:
        ops, x = R.family(name, dim, batch, dt)
        arr = c.ops(ops)
        xn = x.copy(order="F")
        xn[dim // 2, j] = np.nan
        a_d = dev(np.asfortranarray(R.matrix(dim, dt)))
        for inverse in (0, 1):
            for flags in (0, c.L.BJX_BASE_STDNORMAL):
                ob, lb = c.buffers(batch)
                c.ok(inverse, a_d, arr, len(ops), dev(x), ob, lb, batch, flags)
                obn, lbn = c.buffers(batch)
                c.ok(inverse, a_d, arr, len(ops), dev(xn), obn, lbn, batch, flags)
                _guards_intact(c, obn, lbn, batch, "NaN call")
                (out, l), (outn, ln) = _views(c, ob, lb, batch), _views(c, obn, lbn, batch)
                others = np.arange(batch) != j
                assert np.isfinite(out).all() and np.isfinite(l).all()
                assert np.array_equal(outn[:, others], out[:, others]) and np.array_equal(ln[others], l[others]), (name, dim, inverse, flags)
                assert np.isnan(outn[:, j]).all() and np.isnan(ln[j]), (name, dim, inverse, flags)


# ---- the grid-stride loop: (type, dim, blocks per CU the launch is capped at: LDS per block <= 40 KiB -> 4, <= 80 KiB -> 2, above -> 1)
LOOP_SHAPES = [(np.float32, 16, 4), (np.float32, 128, 1), (np.float64, 112, 1)]


def _loop_batch(factor):
    cap = torch.cuda.get_device_properties(0).multi_processor_count * factor
    return 2 * cap * 64 + 64 + 16 + 3        # every wave makes a second trip, some a third that ends in a ragged tile; the last prefetch is past the batch


@pytest.mark.parametrize("dt,dim,factor", LOOP_SHAPES, ids=[f"{np.dtype(t).name}-{d}" for t, d, _ in LOOP_SHAPES])
def test_second_and_third_trip_of_the_tile_loop_with_a_chain(bj, dt, dim, factor):
    """More columns than the capped grid holds in one trip: the look-ahead fetch of the next tile, its zero fill past the batch and the
    hand-over cur = nxt — the four-stage vector family with the density and `out` stored; Float64 at 112 rows is the largest launch the
    kernel can make (163 840 bytes of LDS)."""
    c = _Call(bj, dt, dim)
    batch = _loop_batch(factor)
    ops, x = R.family("log_v", dim, batch, dt)
    arr, x_d = c.ops(ops), dev(x)
    path = R.reduction_path(dt, dim)
    for kind, inverse in (("cholesky", 1), ("general", 0)):
        a = R.matrix(dim, dt, kind)
        ref_out, ref_lp = R.ref(a, ops, x, inverse, True)
        ob, lb = c.buffers(batch)
        c.ok(inverse, dev(np.asfortranarray(a)), arr, len(ops), x_d, ob, lb, batch, c.L.BJX_BASE_STDNORMAL)
        _guards_intact(c, ob, lb, batch, "loop")
        out, l = _views(c, ob, lb, batch)
        flat_close(out, ref_out, dt, f"scale_matrix_chain[{path}] loop {kind} inverse={inverse} dim={dim} batch={batch} out", per="sample")
        flat_close(l, ref_lp, dt, f"scale_matrix_chain[{path}] loop {kind} inverse={inverse} dim={dim} batch={batch} ladj_ps", per="element", floor=dim)


@pytest.mark.parametrize("dt,dim,factor", LOOP_SHAPES, ids=[f"{np.dtype(t).name}-{d}" for t, d, _ in LOOP_SHAPES])
def test_second_and_third_trip_of_the_tile_loop_without_a_chain(bj, dt, dim, factor):
    """The plain bjx_scale_matrix MFMA loop has the same second trip: both directions against numpy."""
    c = _Call(bj, dt, dim)
    batch = _loop_batch(factor)
    _, x = R.family("none", dim, batch, dt)
    a = R.matrix(dim, dt)
    a_d, x_d = dev(np.asfortranarray(a)), dev(x)
    for inverse in (0, 1):
        ref_out, ref_l = R.ref(a, [], x, inverse, False)
        ob, lb = c.buffers(batch)
        c.L.check(c.ctx.h, c.lib.bjx_scale_matrix(c.ctx.h, c.dtc, inverse, _p(a_d), _p(x_d), _p(ob), _p(lb), None, dim, batch, 0), "bjx_scale_matrix")
        _guards_intact(c, ob, lb, batch, "loop")
        out, l = _views(c, ob, lb, batch)
        flat_close(out, ref_out, dt, f"scale_matrix loop inverse={inverse} dim={dim} batch={batch} out", per="sample")
        flat_close(l, ref_l, dt, f"scale_matrix loop inverse={inverse} dim={dim} batch={batch} ladj_ps", per="element", floor=dim)


# ---- the limits, as contracts
def _refused(c, inverse, a_d, arr, n_ops, x_d, ob, lb, batch, flags, what, out_ptr=None, in_ptr=None):
    rc = c.lib.bjx_scale_matrix_chain(c.ctx.h, c.dtc, inverse, _p(a_d), arr, n_ops, in_ptr if in_ptr is not None else _p(x_d),
                                      out_ptr if out_ptr is not None else _p(ob), _p(lb), c.dim, batch, flags)
    assert rc == c.L.ERR_UNSUPPORTED, f"{what}: status {rc}"
    torch.cuda.synchronize()
    assert bool((ob == MARK).all()) and bool((lb == MARK).all()), f"{what}: refused, yet something was written"


@pytest.mark.parametrize("dt,dim", [(np.float64, 114), (np.float64, 128), (np.float32, 130), (np.float32, 6), (np.float64, 5)],
                         ids=["float64-114", "float64-128", "float32-130", "float32-6", "float64-5"])
def test_sizes_past_the_lds_tile_or_off_the_pack_are_refused(bj, dt, dim):
    """Float64 stops at 112 rows (113 … 128 pad to 128: (128² + 64·132)·8 bytes > the 160 KiB LDS tile), Float32 at 128; rows that are no whole
    number of 16-byte packs: BJX_ERR_UNSUPPORTED, nothing written — in both directions, with and without stages and the density."""
    c = _Call(bj, dt, dim)
    batch = 33
    r = rng(dim)
    a_d = dev(np.asfortranarray((r.normal(size=(dim, dim)) / np.sqrt(dim) + 1.5 * np.eye(dim)).astype(dt)))
    x_d = dev(np.asfortranarray(np.exp(r.normal(size=(dim, batch))).astype(dt)))
    vec = np.linspace(0.5, 1.5, dim).astype(dt)
    for ops in ([], [(R.OP_LOG, None, None), (R.OP_SCALE_INV, vec, None), (R.OP_SHIFT, vec, None)]):
        arr = c.ops(ops)
        for inverse in (0, 1):
            for flags in (0, c.L.BJX_BASE_STDNORMAL):
                ob, lb = c.buffers(batch)
                _refused(c, inverse, a_d, arr, len(ops), x_d, ob, lb, batch, flags, f"dim={dim} n_ops={len(ops)} inverse={inverse} flags={flags}")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_arguments_the_kernel_does_not_serve_are_refused(bj, dt):
    """`in` or `out` one element off the 16-byte boundary, five stages, a stage kind outside exp / log / Shift / Scale / Scale⁻¹, a scalar
    parameter passed as a device pointer: BJX_ERR_UNSUPPORTED, nothing written.  batch == 0: BJX_OK, nothing written."""
    dim, batch = 16, 33
    c = _Call(bj, dt, dim)
    Lm = c.L
    ops, x = R.family("log_v", dim, batch + 1, dt)
    arr = c.ops(ops)
    a_d, x_d = dev(np.asfortranarray(R.matrix(dim, dt))), dev(x)
    item = np.dtype(dt).itemsize
    ob, lb = c.buffers(batch + 1)
    _refused(c, 1, a_d, arr, 4, x_d, ob, lb, batch, 0, "in + 1 element", in_ptr=C.c_void_p(x_d.data_ptr() + item))
    _refused(c, 1, a_d, arr, 4, x_d, ob, lb, batch, 0, "out + 1 element", out_ptr=C.c_void_p(ob.data_ptr() + item))
    five = c.ops(list(ops) + [(R.OP_EXP, None, None)])
    _refused(c, 1, a_d, five, 5, x_d, ob, lb, batch, 0, "n_ops == 5")
    for kind in (Lm.OP_LOGIT, Lm.OP_SIGNFLIP, Lm.OP_IDENTITY):
        bad = (Lm.BjxOp * 2)(Lm.BjxOp(Lm.OP_LOG, 0, 0.0, 0.0, None, None), Lm.BjxOp(kind, 1, 0.0, 1.0, None, None))
        _refused(c, 1, a_d, bad, 2, x_d, ob, lb, batch, 0, f"stage kind {kind}")
    s_d = torch.full((1,), 0.5, dtype=c.tdt, device="cuda")
    for kind in (Lm.OP_SHIFT, Lm.OP_SCALE, Lm.OP_SCALE_INV):
        bad = (Lm.BjxOp * 1)(Lm.BjxOp(kind, 1, 0.5, 0.0, s_d.data_ptr(), None))
        _refused(c, 0, a_d, bad, 1, x_d, ob, lb, batch, 0, f"device scalar for stage kind {kind}")
    for inverse in (0, 1):
        for flags in (0, Lm.BJX_BASE_STDNORMAL, Lm.BJX_ACCUMULATE):
            assert c.run(inverse, a_d, arr, 4, x_d, ob, lb, 0, flags) == 0
            if not flags & Lm.BJX_BASE_STDNORMAL:        # (the density is written to ladj_ps: without it the call is BJX_ERR_ARG at any batch)
                assert c.run(inverse, a_d, arr, 4, None, None, None, 0, flags) == 0
    torch.cuda.synchronize()
    assert bool((ob == MARK).all()) and bool((lb == MARK).all()), "batch == 0 wrote something"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_parameter_epoch_keeps_and_renews_the_factorisation(bj, dt):
    """BJX_OPT_PARAM_EPOCH != 0: the second inverse call skips the factorisation and gives the same bits; `a` rewritten in place under a
    new epoch is followed."""
    dim, batch = 48, 77
    c = _Call(bj, dt, dim)
    Lm = c.L
    ops, x = R.family("log_v", dim, batch, dt)
    arr, x_d = c.ops(ops), dev(x)
    a0, a1 = R.matrix(dim, dt, "cholesky"), R.matrix(dim, dt, "general")
    a_d = dev(np.asfortranarray(a0))
    flags = Lm.BJX_BASE_STDNORMAL
    try:
        Lm.check(c.ctx.h, c.lib.bjx_set_option(c.ctx.h, Lm.BJX_OPT_PARAM_EPOCH, 1234), "bjx_set_option")
        res = []
        for _ in range(2):
            ob, lb = c.buffers(batch)
            c.ok(1, a_d, arr, 4, x_d, ob, lb, batch, flags)
            res.append((ob, lb))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "the kept factorisation gives other bits"
        ref_out, ref_lp = R.ref(a0, ops, x, 1, True)
        out, l = _views(c, *res[1], batch)
        flat_close(out, ref_out, dt, f"scale_matrix_chain epoch kept dim={dim} out", per="sample")
        flat_close(l, ref_lp, dt, f"scale_matrix_chain epoch kept dim={dim} ladj_ps", per="element", floor=dim)
        a_d.copy_(dev(np.asfortranarray(a1)))           # the same address, another matrix
        Lm.check(c.ctx.h, c.lib.bjx_set_option(c.ctx.h, Lm.BJX_OPT_PARAM_EPOCH, 1235), "bjx_set_option")
        ob, lb = c.buffers(batch)
        c.ok(1, a_d, arr, 4, x_d, ob, lb, batch, flags)
        ref_out, ref_lp = R.ref(a1, ops, x, 1, True)
        out, l = _views(c, ob, lb, batch)
        flat_close(out, ref_out, dt, f"scale_matrix_chain epoch renewed dim={dim} out", per="sample")
        flat_close(l, ref_lp, dt, f"scale_matrix_chain epoch renewed dim={dim} ladj_ps", per="element", floor=dim)
    finally:
        Lm.check(c.ctx.h, c.lib.bjx_set_option(c.ctx.h, Lm.BJX_OPT_PARAM_EPOCH, 0), "bjx_set_option")
