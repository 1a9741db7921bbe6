"""The host layer's op-list marshaller and plan-cache scaffold (no GPU, the library is not loaded).

`_fill_op` / `_marshal_ops` / `_fill_segment` turn [(kind, p0, p1)] into the `bjx_op` / `bjx_segment` arrays every chain entry of the
library takes.  The expected fields are written out from the struct comment in include/bjx.h: `param_len` 0 = no parameter, 1 = host
scalars in p0 / p1, == rows = one device value per row behind v0 / v1 (which then override p0 / p1).  They run on CPU tensors, so
each pointer can be compared with `data_ptr()` of the tensor it must name."""
import pytest
import torch

ROWS = (1, 3, 5)
DTYPES = (torch.float32, torch.float64)


@pytest.fixture(scope="module")
def I():
    from bijectors_amd import interface

    return interface


@pytest.fixture(params=[(r, d) for r in ROWS for d in DTYPES], ids=lambda p: f"{p[0]}-{str(p[1])[6:]}")
def case(request):
    rows, dt = request.param
    like = torch.zeros((3, rows), dtype=dt).T             # (rows, 3), column-major
    return rows, dt, like


def fields(o):
    return (o.kind, o.param_len, o.p0, o.p1, o.v0, o.v1)


def vals(rows, shift=0.0):
    return [0.25 * (i + 1) + shift for i in range(rows)]      # exact in both formats


def other(dt):
    return torch.float64 if dt is torch.float32 else torch.float32


def same_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_op_without_parameter(I, case):
    rows, dt, like = case
    arr, keep = I._marshal_ops([(I.L.OP_EXP, None, None)], like, rows)
    assert fields(arr[0]) == (I.L.OP_EXP, 0, 0.0, 0.0, None, None)
    assert keep == []


def test_scalars(I, case):
    rows, dt, like = case
    arr, keep = I._marshal_ops([(I.L.OP_SHIFT, 0.5, None), (I.L.OP_SCALE, 2, None), (I.L.OP_LOGIT, 0.0, 1.5)], like, rows)
    assert fields(arr[0]) == (I.L.OP_SHIFT, 1, 0.5, 0.0, None, None)
    assert fields(arr[1]) == (I.L.OP_SCALE, 1, 2.0, 0.0, None, None)
    assert fields(arr[2]) == (I.L.OP_LOGIT, 1, 0.0, 1.5, None, None)
    assert keep == []


def test_vector_of_the_input_dtype_is_passed_by_its_own_address(I, case):
    rows, dt, like = case
    t = torch.tensor(vals(rows), dtype=dt)
    col = torch.tensor(vals(rows, 1.0), dtype=dt).reshape(rows, 1)
    arr, keep = I._marshal_ops([(I.L.OP_SHIFT, t, None), (I.L.OP_SCALE, col, None)], like, rows)
    assert fields(arr[0]) == (I.L.OP_SHIFT, rows, 0.0, 0.0, t.data_ptr(), None)
    assert fields(arr[1]) == (I.L.OP_SCALE, rows, 0.0, 0.0, col.data_ptr(), None)
    assert len(keep) == 2 and same_storage(keep[0], t) and same_storage(keep[1], col)


@pytest.mark.parametrize("form", ["list", "tuple", "other_dtype"])
def test_sequence_and_other_dtype_are_converted(I, case, form):
    rows, dt, like = case
    v = vals(rows, 2.0)
    p = {"list": v, "tuple": tuple(v), "other_dtype": torch.tensor(v, dtype=other(dt))}[form]
    arr, keep = I._marshal_ops([(I.L.OP_SCALE, p, None)], like, rows)
    assert len(keep) == 1
    assert fields(arr[0]) == (I.L.OP_SCALE, rows, 0.0, 0.0, keep[0].data_ptr(), None)
    assert keep[0].dtype is dt and keep[0].shape == (rows,) and keep[0].is_contiguous()
    assert keep[0].tolist() == v
    if form == "other_dtype":
        assert not same_storage(keep[0], p)


def test_scalar_next_to_a_vector_is_broadcast(I, case):
    rows, dt, like = case
    a = torch.tensor(vals(rows, -9.0), dtype=dt)
    ub = torch.tensor(vals(rows, 3.0), dtype=dt)
    arr, keep = I._marshal_ops([(I.L.OP_LOGIT, a, 7.5), (I.L.OP_TRUNCATED, -1.0, ub)], like, rows)
    assert len(keep) == 4
    assert fields(arr[0]) == (I.L.OP_LOGIT, rows, 0.0, 0.0, a.data_ptr(), keep[1].data_ptr())
    assert keep[1].dtype is dt and keep[1].tolist() == [7.5] * rows and not same_storage(keep[1], a)
    assert fields(arr[1]) == (I.L.OP_TRUNCATED, rows, 0.0, 0.0, keep[2].data_ptr(), ub.data_ptr())
    assert keep[2].dtype is dt and keep[2].tolist() == [-1.0] * rows and same_storage(keep[3], ub)


def test_wrong_length_messages(I, case):
    rows, dt, like = case
    long = torch.ones(rows + 1, dtype=dt)
    with pytest.raises(ValueError) as e:
        I._marshal_ops([(I.L.OP_SHIFT, long, None)], like, rows)
    assert str(e.value) == f"DimensionMismatch: parameter of length {rows + 1} for input with {rows} rows"
    with pytest.raises(ValueError) as e:
        I._marshal_ops([(I.L.OP_EXP, None, None), (I.L.OP_SCALE, [1.0] * (rows + 2), None)], like, rows)
    assert str(e.value) == f"DimensionMismatch: parameter of length {rows + 2} for input with {rows} rows"
    seg = (I.L.BjxSegment * 1)()
    with pytest.raises(ValueError) as e:
        I._fill_segment(seg[0], 0, 0, rows, [(I.L.OP_SHIFT, long, None)], like, [])
    assert str(e.value) == f"DimensionMismatch: parameter of length {rows + 1} for a segment of {rows} rows"
    st = I.Stacked([I.Shift(long), I.identity], [(1, rows), (rows + 1, rows + 1)])
    I._CHAIN_OPS.clear()
    with pytest.raises(ValueError) as e:
        st._segments([I._elementwise_ops(b) for b in st.bs], [0, 1], torch.zeros((3, rows + 1), dtype=dt).T)
    assert str(e.value) == f"DimensionMismatch: parameter of length {rows + 1} for a segment of {rows} rows"


def test_segments_are_zero_based(I, case):
    """Stacked(bs, ranges) has Julia's 1-based inclusive ranges; bjx_segment has 0-based in_lo / out_lo, len and n_ops."""
    rows, dt, like = case
    a = torch.tensor(vals(rows), dtype=dt)
    c = torch.tensor([1.5, -2.5], dtype=dt)
    st = I.Stacked([I.elementwise(I.exp) @ I.Shift(a), I.identity, I.Scale(c)], [(1, rows), (rows + 1, rows + 1), (rows + 2, rows + 3)])
    xs = torch.zeros((3, rows + 3), dtype=dt).T
    I._CHAIN_OPS.clear()
    arr, keep = st._segments([I._elementwise_ops(b) for b in st.bs], [0, 1, 2], xs)
    s0, s1, s2 = arr[0], arr[1], arr[2]
    assert (s0.in_lo, s0.out_lo, s0.len, s0.n_ops) == (0, 0, rows, 2)
    assert fields(s0.ops[0]) == (I.L.OP_SHIFT, rows, 0.0, 0.0, a.data_ptr(), None)
    assert fields(s0.ops[1]) == (I.L.OP_EXP, 0, 0.0, 0.0, None, None)
    assert (s1.in_lo, s1.out_lo, s1.len, s1.n_ops) == (rows, rows, 1, 0)
    assert (s2.in_lo, s2.out_lo, s2.len, s2.n_ops) == (rows + 1, rows + 1, 2, 1)
    assert fields(s2.ops[0]) == (I.L.OP_SCALE, 2, 0.0, 0.0, c.data_ptr(), None)
    assert len(keep) == 2 and same_storage(keep[0], a) and same_storage(keep[1], c)
    arr2, keep2 = st._segments([I._elementwise_ops(b) for b in st.bs], [0, 1, 2], xs)
    if rows > 1:                                  # pointers only: the array is kept and found again
        assert arr2 is arr and keep2 == []
    else:                                         # a one-element tensor has no chain key: marshalled on every call
        assert arr2 is not arr and len(keep2) == 2


def test_segments_of_a_window_are_shifted_by_its_offsets(I, case, monkeypatch):
    """A Stacked with a structured segment: the elementwise segments go to bjx_stacked_mixed with their rows as they are, and — when
    that entry declines — to bjx_stacked_ld as a window of x and y that starts at the run's first row (in_lo - x_off, out_lo - y_off)."""
    rows, dt, like = case
    a = torch.tensor(vals(rows), dtype=dt)
    seen = []

    class Lib:
        def __getattr__(self, name):
            def fn(*args):
                if name in ("bjx_stacked_mixed", "bjx_stacked_ld"):       # (ctx, dt, segs, n_segs, ...): read while the parameters are alive
                    seen.append((name, [(s.in_lo, s.out_lo, s.len, s.n_ops, [fields(s.ops[k]) for k in range(s.n_ops)]) for s in args[2][:args[3]]], args))
                return I.L.ERR_UNSUPPORTED if name == "bjx_stacked_mixed" else 0
            return fn

    class Ctx:
        h = None

    monkeypatch.setattr(I.L, "load", lambda: Lib())
    monkeypatch.setattr(I, "context", lambda dev=None: Ctx())
    monkeypatch.setattr(I, "_check_dev", lambda x: None)
    # Simplex takes rows 1:3 to 1:2, so the elementwise run starts at row 3 of x (0-based) and row 2 of y
    st = I.Stacked([I.SimplexBijector(), I.Shift(a), I.Scale(2.0)], [(1, 3), (4, rows + 3), (rows + 4, rows + 5)])
    xs = torch.full((3, rows + 5), 0.25, dtype=dt).T
    st._wlj(xs, per_sample=True)
    shift_op = (I.L.OP_SHIFT, rows, 0.0, 0.0, a.data_ptr(), None)
    scale_op = (I.L.OP_SCALE, 1, 2.0, 0.0, None, None)
    assert [s[0] for s in seen] == ["bjx_stacked_mixed", "bjx_stacked_ld"]
    assert seen[0][1] == [(3, 2, rows, 1, [shift_op]), (rows + 3, rows + 2, 2, 1, [scale_op])]
    assert seen[1][1] == [(0, 0, rows, 1, [shift_op]), (rows, rows, 2, 1, [scale_op])]
    ld = seen[1][2]                                                 # (ctx, dt, segs, n, x, ldx, y, ldy, ps, sum, rows_run, batch, flags)
    assert ld[4].value == xs.data_ptr() + 3 * xs.element_size() and ld[5] == rows + 5 and ld[7] == rows + 4 and ld[10] == rows + 2


def battery(I, rows, dt):
    """name -> (ops, qualifies): qualifies = `_chain_key` gives a key (vector parameters are contiguous tensors of the input's dtype with
    `rows` elements — and more than one element —, everything else is a python number, no op mixes the two)."""
    T = lambda s=0.0: torch.tensor(vals(rows, s), dtype=dt)
    many = rows > 1
    return {
        "exp": ([(I.L.OP_EXP, None, None)], True),
        "scalar": ([(I.L.OP_SHIFT, 0.5, None)], True),
        "int": ([(I.L.OP_SCALE, 2, None)], True),
        "two_scalars": ([(I.L.OP_LOGIT, 0.0, 1.5)], True),
        "vec": ([(I.L.OP_SHIFT, T(), None)], many),
        "vec_vec": ([(I.L.OP_TRUNCATED, T(-9.0), T(3.0))], many),
        "col2d": ([(I.L.OP_SHIFT, T().reshape(rows, 1), None)], many),
        "multi": ([(I.L.OP_SCALE, T(4.0), None), (I.L.OP_SHIFT, 0.25, None), (I.L.OP_EXP, None, None), (I.L.OP_LEAKY_RELU, 0.1, None)], many),
        "list": ([(I.L.OP_SCALE, vals(rows, 1.0), None)], False),
        "other_dtype": ([(I.L.OP_SCALE, torch.tensor(vals(rows), dtype=other(dt)), None)], False),
        "vec_scalar": ([(I.L.OP_LOGIT, T(-9.0), 7.5)], False),
        "zero_d": ([(I.L.OP_SHIFT, torch.tensor(0.75, dtype=dt), None)], False),
        "strided": ([(I.L.OP_SHIFT, torch.zeros(2 * rows + 2, dtype=dt)[::2][:rows], None)], False),
        "wrong_len": ([(I.L.OP_SHIFT, torch.ones(rows + 1, dtype=dt), None)], False),
    }


def test_a_list_with_a_chain_key_is_marshalled_without_conversion(I, case):
    """What lets the plan builders use the general marshaller: for a list `_chain_key` accepts it converts nothing — every pointer is the
    original tensor's own, `keep` holds no new storage — so a plan built from it sees in-place parameter updates."""
    rows, dt, like = case
    for name, (ops, qualifies) in battery(I, rows, dt).items():
        assert (I._chain_key(ops, like, rows) is not None) == qualifies, name
        if not qualifies:
            continue
        expect, originals = [], []
        for kind, p0, p1 in ops:
            tensors = [p for p in (p0, p1) if isinstance(p, torch.Tensor)]
            originals += tensors
            plen = rows if tensors else (0 if p0 is None and p1 is None else 1)
            expect.append((kind, plen) + tuple(float(p) if isinstance(p, (int, float)) else 0.0 for p in (p0, p1))
                          + tuple(p.data_ptr() if isinstance(p, torch.Tensor) else None for p in (p0, p1)))
        arr, keep = I._marshal_ops(ops, like, rows)
        assert [fields(arr[i]) for i in range(len(ops))] == expect, name
        seg = (I.L.BjxSegment * 1)()
        keep_seg = []
        I._fill_segment(seg[0], 0, 0, rows, ops, like, keep_seg)
        assert (seg[0].in_lo, seg[0].out_lo, seg[0].len, seg[0].n_ops) == (0, 0, rows, len(ops)), name
        assert [fields(seg[0].ops[k]) for k in range(len(ops))] == expect, name
        for kp in (keep, keep_seg):
            assert len(kp) == len(originals) and all(same_storage(k, t) for k, t in zip(kp, originals)), name


def test_ops_stable(I):
    t = torch.tensor([0.5, 1.5, 2.5])
    sh = I.Shift(t)
    chain = I.elementwise(I.exp) @ sh @ I.Scale(2.0)
    assert I._ops_stable(I._fused_ops(sh), I._fused_ops(sh))
    assert I._ops_stable(I._fused_ops(chain), I._fused_ops(chain))
    inv = I.Inverse(sh)                                            # its op carries -t: a new tensor on every build
    assert I._fused_ops(inv)[0][1].tolist() == [-0.5, -1.5, -2.5]
    assert not I._ops_stable(I._fused_ops(inv), I._fused_ops(inv))
    assert not I._ops_stable(I._fused_ops(chain @ inv), I._fused_ops(chain @ inv))
    shifted = I.inverse(sh)                                        # `inverse` of a Shift is a Shift that owns its -t
    assert I._fused_ops(shifted)[0][1].tolist() == [-0.5, -1.5, -2.5]
    assert I._ops_stable(I._fused_ops(shifted), I._fused_ops(shifted))
    inv_scalar = I.Inverse(I.Shift(0.5))                           # numbers are copied into the op, nothing to go stale
    assert I._ops_stable(I._fused_ops(inv_scalar), I._fused_ops(inv_scalar))


def test_plan_cache_scaffold(I):
    sh = I.Shift(torch.tensor([0.5, 1.5]))
    assert I._plan_get(sh, "k") is None
    na = I._plan_na(sh, "k")
    assert type(na) is I._FastPlan and na.h is None and I._plan_get(sh, "k") is na
    nap = I._plan_na(sh, "p", I._ParamsPlan)
    assert type(nap) is I._ParamsPlan and nap.h is None and I._plan_get(sh, "p") is nap and I._plan_get(sh, "k") is na
    assert I._plan_get(I.Shift(1.0), "k") is None                  # kept on the bijector object
    sh.a = sh.a                                                    # a re-assigned parameter attribute ends every plan
    assert I._plan_get(sh, "k") is None and I._plan_get(sh, "p") is None
    again = I._plan_na(sh, "k")
    assert again is not na and I._plan_get(sh, "k") is again


def test_dense_input_rejects_before_it_asks_for_the_device(I):
    assert I._dense_input(torch.zeros((2, 3, 4))) is None          # neither a vector nor a matrix
    assert I._dense_input(torch.zeros((3, 4))) is None             # row-major
    assert I._dense_input(torch.zeros(8)[::2]) is None             # strided vector
    assert I._dense_input(torch.zeros((4, 0)).T) is None           # no rows
    assert I._dense_input(torch.zeros(0)) is None
    assert I._dense_input(torch.zeros((4, 3), dtype=torch.int32).T) is None
    assert I._dense_input(torch.zeros(3, dtype=torch.float16)) is None
