"""The amortised Householder flow (`AmortizedHouseholderFlow`, include/bjx_householder_cols.h) through bijectors_amd against the Float64
closed forms of tests/_householder_cols_ref.py (held to dense matrices, slogdet and central differences in
tests/test_host_householder_cols.py), on tests/_tol.py's flat bar (1e-3 Float32 / 1e-6 Float64), no conditioned bar anywhere: values,
x̄ and ȳ per="sample" at dim >= 2 and with floor=1.0 at dim 1 (a column of one entry has no scale of its own; the inputs are unit-scale
draws), log-dets per="element" with a floor of 1, v̄ / s̄ / m̄ on the column's TERM scale (`RefAll.scale`: at dim 1 v̄ is analytically 0
and at dim 2 its three terms nearly cancel).  No column is left out of any comparison; column 0 of every draw has v_0 == 0 exactly
(the degenerate layer: the identity, v̄_0 = 0).

Dispatcher edges by dim (V = 4 / 2 elements per 16-byte pack in Float32 / Float64, G lanes per column, R packs per lane):
  1, 2, 3, 5   partial first pack, element form; G = 1 (Float32; Float64: G = 1 at 1 and 2, G = 2 at 3, G = 4 at 5)
  4, 8, 16     whole packs, vector form, G = 1, 2, 4 (Float32) / 2, 4, 8 (Float64)
  64           vector form, G = 16 (Float32) / 32 (Float64)
  65           element form, partial last pack, G = 32 / 64
  260 / 256    two packs per lane (R = 2), whole packs: Float32 / Float64
  261 / 257    Float32: R = 2 with a partial pack; Float64: 129 packs = three per lane on lane 0, the R = 4 kernels with dead packs
  516, 765 / 384   three packs per lane on some (516: 129 packs) or all lanes (765 Float32: 192 packs, the last partial; 384
               Float64: 192 packs): the R = 4 kernels with a dead pack
  1 024 / 512  the limits: R = 4, every pack live
Every case runs the batches 1, C − 1, C, C + 1 with C = 256/G columns per block.

The GPU suite is kept at 5 000 test ids, so the cases are TWO ids here: the parts below are plain functions called in turn (every
failure names its part in the traceback and its dtype, dim, L and batch in the message)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _householder_cols_ref import HEADS, RefAll, draws, rounded, seed  # noqa: E402
from _radial_cols_ref import RefAll as RadialRefAll  # noqa: E402
from _radial_cols_ref import draws as radial_draws  # noqa: E402
from _tol import flat_close  # noqa: E402

F32, F64 = np.float32, np.float64
DIMS = {F32: [1, 2, 3, 5, 4, 8, 16, 64, 65, 260, 261, 516, 765, 1024], F64: [1, 2, 3, 5, 4, 8, 16, 64, 65, 256, 257, 384, 512]}


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def lanes(dim, dt):
    packs = -(-dim // (16 // np.dtype(dt).itemsize))
    G = 1
    while G < 64 and G < packs:
        G *= 2
    return G


def dev3(a, dt):
    """(dim, L, N) numpy -> cuda tensor laid out column-major per column (a permute(2, 1, 0) view of a (N, L, dim) array)."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 1, 0))).astype(dt)).cuda().permute(2, 1, 0)


def dev2(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_flow(bj, v, s, m, dt):
    return bj.AmortizedHouseholderFlow(dev3(v, dt), dev2(s, dt), dev2(m, dt))


def close_cols(got, ref, dt, what):
    """Values and input cotangents (dim, n): per sample; a column of ONE entry on a floor of 1."""
    return flat_close(got, ref, dt, what, per="sample", floor=1.0 if ref.shape[0] == 1 else 0.0)


def cut(a, n):
    return None if a is None else a[..., :n]


class Ref:
    """Every reference quantity of one parameter draw, computed once; the tests slice its first n columns.  F: the flow at z with the
    cotangents (g, lb); I: its inverse at the SAME input and cotangents."""

    def __init__(self, dt, dim, L, N, key, head="both"):
        self.dt, self.N = dt, N
        self.v, self.s, self.m, self.z, self.g, self.lb = draws(seed(*key), dim, L, N, dt, head)
        self.F = RefAll(self.v, self.s, self.m, self.z, self.g, self.lb)
        self.I = RefAll(self.v, self.s, self.m, self.z, self.g, self.lb, inverse=True)


def check_params(grads, ref, n, dt, what):
    want = {"v": ref.vb}
    if ref.sb is not None:
        want["log_scale"] = ref.sb
    if ref.mb is not None:
        want["shift"] = ref.mb
    assert set(grads) == set(want), (what, sorted(grads))
    for k, r in want.items():
        got = host(grads[k])
        assert got.shape == r[..., :n].shape, (what, k, got.shape)
        flat_close(got.reshape(-1, n), r[..., :n].reshape(-1, n), dt, f"{what} {k} cotangent", term_scale=ref.scale[:n])


def check_all(bj, R, n, what):
    """Maps, round trip and pullbacks of the first n columns of the draw R, both directions."""
    dt = R.dt
    flow = make_flow(bj, R.v[:, :, :n], cut(R.s, n), cut(R.m, n), dt)
    inv = bj.inverse(flow)
    zd, gd, lbd = dev2(R.z[:, :n], dt), dev2(R.g[:, :n], dt), dev1(R.lb[:n], dt)
    y, l = bj.with_logabsdet_jacobian(flow, zd, per_sample=True)
    close_cols(host(y), R.F.out[:, :n], dt, what + " values")
    flat_close(host(l), R.F.ladj[:n], dt, what + " ladj", per="element", floor=1.0)
    xi, li = bj.with_logabsdet_jacobian(inv, zd, per_sample=True)
    close_cols(host(xi), R.I.out[:, :n], dt, what + " inverse values")
    flat_close(host(li), R.I.ladj[:n], dt, what + " inverse ladj", per="element", floor=1.0)
    close_cols(host(bj.transform(inv, y)), R.z[:, :n], dt, what + " round trip")
    if R.s is None:
        assert not host(l).any() and not host(li).any(), what + ": the log-det without log_scale is not an exact zero"
    for f, ref, name in ((flow, R.F, "forward"), (inv, R.I, "inverse")):
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        close_cols(host(xb), ref.in_bar[:, :n], dt, f"{what} {name} input cotangent")
        assert torch.equal(bj.vjp(f, zd, gd, lbd), xb), f"{what} {name}: vjp and vjp_params disagree on the input cotangent"
        check_params(grads, ref, n, dt, f"{what} {name}")
        assert not host(grads["v"])[:, 0, 0].any(), f"{what} {name}: the cotangent of the degenerate layer is not 0"


def batches(C, more=()):
    return sorted({n for n in (1, C - 1, C, C + 1) + tuple(more) if n >= 1})


def maps_and_pullbacks_match_reference(bj, dt):
    """Every dim of the table above at L = 1, 2 and 8, head present (each failure names its dtype, dim, L and batch)."""
    for L in (1, 2, 8):
        for dim in DIMS[dt]:
            C = 256 // lanes(dim, dt)
            ns = batches(C, (257,) if dim == 64 else ())
            R = Ref(dt, dim, L, max(ns), ("cols", np.dtype(dt).name, dim, L))
            for n in ns:
                check_all(bj, R, n, f"householder_cols {np.dtype(dt).name} dim={dim} L={L} batch={n}")


def head_combinations(bj, head):
    """No head, only log_scale, only shift, both: dim 5, 64 and 65, L = 2, both dtypes.  The cotangent dictionary has the keys of the
    present parameters only, and without log_scale both log-dets are exact zeros (per column and summed)."""
    for dt in (F32, F64):
        for dim in (5, 64, 65):
            N = 256 // lanes(dim, dt) + 1
            R = Ref(dt, dim, 2, N, ("head", np.dtype(dt).name, dim, head), head)
            what = f"householder_cols {np.dtype(dt).name} dim={dim} head={head}"
            check_all(bj, R, N, what)
            flow = make_flow(bj, R.v, R.s, R.m, dt)
            for f, ref in ((flow, R.F), (bj.inverse(flow), R.I)):
                _, (l, tot) = bj.with_logabsdet_jacobian(f, dev2(R.z, dt), per_sample="both")
                if R.s is None:
                    assert not host(l).any() and float(tot) == 0.0, what
                else:
                    flat_close(host(tot.reshape(1)), ref.ladj.sum().reshape(1), dt, what + " summed ladj", per="element", floor=1.0)


def long_stack_in_float32(bj):
    """L = 64 at dim 3 and dim 64, 70 columns, both directions, Float32, on the flat bar: the reflections are orthogonal and the rewind
    is the reflection itself, so the rounding of the reverse sweep does not grow with the depth as it does where a contracting step
    is re-applied forwards (numpy Float32 of the same operation order: 3e-6 of the scale)."""
    for dim in (3, 64):
        R = Ref(F32, dim, 64, 70, ("long", dim))
        check_all(bj, R, 70, f"householder_cols float32 dim={dim} L=64 batch=70")


def parameter_pullbacks_are_one_launch_in_either_direction(bj):
    """vjp_params(flow, …) and vjp_params(inverse(flow), …) are ONE hot launch each."""
    R = Ref(F32, 16, 3, 20, ("launches",))
    flow = make_flow(bj, R.v, R.s, R.m, F32)
    zd, gd, lbd = dev2(R.z, F32), dev2(R.g, F32), dev1(R.lb, F32)
    for f in (flow, bj.inverse(flow)):
        bj.vjp_params(f, zd, gd, lbd)
        _, _, k = bj.kernel_timed(lambda: bj.vjp_params(f, zd, gd, lbd))
        assert k == 1, f"{type(f).__name__}: {k} hot launches"


# ------------------------------------------------------------------ refusals
def sizes_beyond_the_limits_raise_value_errors(bj):
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        v = torch.ones((1, 1, lim + 1), dtype=dt, device="cuda").permute(2, 1, 0)
        flow = bj.AmortizedHouseholderFlow(v)
        x = torch.zeros((1, lim + 1), dtype=dt, device="cuda").T
        for call in (lambda: bj.transform(flow, x), lambda: bj.transform(bj.inverse(flow), x), lambda: bj.vjp(flow, x, x), lambda: bj.vjp_params(flow, x, x),
                     lambda: bj.vjp_params(bj.inverse(flow), x, x)):
            with pytest.raises(ValueError, match=str(lim)):
                call()
    for L in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.AmortizedHouseholderFlow(torch.zeros((3, L, 4), device="cuda"))
    flow = bj.AmortizedHouseholderFlow(torch.ones((3, 2, 4), device="cuda"))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(flow, torch.zeros((5, 4), device="cuda").T.contiguous().T)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(flow, torch.zeros((5, 3), device="cuda").T)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.AmortizedHouseholderFlow(torch.ones((3, 2, 4), device="cuda"), torch.ones((4, 4), device="cuda"))


# ------------------------------------------------------------------ grid-stride sweeps
def grid_stride_sweeps_match_reference(bj):
    """dim 2, L 1, Float32, head present: G = 1, 256 columns per block, the grid capped at 8 blocks per CU.  Three and a half sweeps
    with a ragged last group, checked on the first group, the groups either side of every sweep boundary, the last group and 256 random
    columns; the summed log-det of the same launch against the Float64 sum of the per-column values."""
    dt, dim, L, C = F32, 2, 1, 256
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    batch = (3 * cap + cap // 2) * C - 17
    groups = (batch + C - 1) // C
    assert groups > 3 * cap and batch % C != 0
    rng = seed("hh-sweep")
    gs = {0, groups - 1}
    for s_ in range(1, (groups - 1) // cap + 1):
        gs |= {s_ * cap - 1, s_ * cap}
    cols = set(rng.choice(batch, size=256, replace=False).tolist())
    for gr in gs:
        cols |= set(range(gr * C, min(batch, (gr + 1) * C)))
    cols = np.array(sorted(cols))
    v, s, m, z, g, lb = draws(rng, dim, L, batch, dt)
    flow = make_flow(bj, v, s, m, dt)
    zd, gd, lbd, ci = dev2(z, dt), dev2(g, dt), dev1(lb, dt), torch.from_numpy(cols).cuda()
    sub = [a[..., cols] for a in (v, s, m, z, g, lb)]
    n = len(cols)
    what = f"householder_cols sweeps batch={batch}"
    for inverse in (False, True):
        V = RefAll(*sub, inverse=inverse)
        f = bj.inverse(flow) if inverse else flow
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        flat_close(host(y[:, ci]), V.out, dt, f"{what} inv={inverse} values")
        flat_close(host(l[ci]), V.ladj, dt, f"{what} inv={inverse} ladj", per="element", floor=1.0)
        _, (l2, tot) = bj.with_logabsdet_jacobian(f, zd, per_sample="both")
        assert torch.equal(l2, l)
        flat_close(host(tot.reshape(1)), host(l.double().sum().reshape(1)), F64, f"{what} inv={inverse} summed ladj", per="element", floor=1.0)
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        flat_close(host(xb[:, ci]), V.in_bar, dt, f"{what} inv={inverse} input cotangent")
        for k, ref in (("v", V.vb), ("log_scale", V.sb), ("shift", V.mb)):
            flat_close(host(grads[k][..., ci]).reshape(-1, n), ref.reshape(-1, n), dt, f"{what} inv={inverse} {k} cotangent", term_scale=V.scale)


# ------------------------------------------------------------------ layouts
def parameter_layouts_match_reference(bj):
    """dim 64, L 2: one head [dim·L + 2·dim + pad, batch] sliced three ways (pad = 4 keeps every column stride a multiple of the pack and
    the vector form, pad = 3 makes them odd: element form), and a dense v whose base pointer is ONE element off 16-byte alignment
    (element form).  No copy is made (data_ptr), and the values meet the bar in every form."""
    for dt in (F32, F64):
        R = Ref(dt, 64, 2, 37, ("layout", np.dtype(dt).name))
        for layout in ("head_vector", "head_element", "off_by_one"):
            _check_layout(bj, R, dt, layout)


def _check_layout(bj, R, dt, layout):
    dim, L, N = 64, 2, 37
    tdt = torch.float32 if dt == F32 else torch.float64
    vn = np.ascontiguousarray(np.transpose(R.v, (2, 1, 0))).reshape(N, L * dim)       # (N, L·dim): rows = columns
    sn, mn = np.ascontiguousarray(R.s.T), np.ascontiguousarray(R.m.T)
    if layout.startswith("head"):
        rows = dim * L + 2 * dim + (4 if layout == "head_vector" else 3)
        head = torch.zeros((N, rows), dtype=tdt, device="cuda")
        head[:, :dim * L] = torch.from_numpy(vn.astype(dt)).cuda()
        head[:, dim * L:dim * L + dim] = torch.from_numpy(sn.astype(dt)).cuda()
        head[:, dim * L + dim:dim * L + 2 * dim] = torch.from_numpy(mn.astype(dt)).cuda()
        v = head[:, :dim * L].view(N, L, dim).permute(2, 1, 0)
        s = head[:, dim * L:dim * L + dim].T
        m = head[:, dim * L + dim:dim * L + 2 * dim].T
        want = (rows, rows, rows)
        assert (rows % (16 // np.dtype(dt).itemsize) == 0) == (layout == "head_vector")
    else:
        buf = torch.zeros(N * L * dim + 1, dtype=tdt, device="cuda")
        buf[1:] = torch.from_numpy(vn.astype(dt).reshape(-1)).cuda()
        v = buf[1:].view(N, L, dim).permute(2, 1, 0)
        assert v.data_ptr() % 16 == np.dtype(dt).itemsize
        s, m = torch.from_numpy(sn.astype(dt)).cuda().T, torch.from_numpy(mn.astype(dt)).cuda().T
        want = (dim * L, dim, dim)
    flow = bj.AmortizedHouseholderFlow(v, s, m)
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    pv, ps, pm, lv, ls, lm = flow._col_params(zd, dim, N)
    assert (pv.data_ptr(), ps.data_ptr(), pm.data_ptr()) == (v.data_ptr(), s.data_ptr(), m.data_ptr()) and (lv, ls, lm) == want
    what = f"householder_cols {layout} {np.dtype(dt).name}"
    for f, ref, name in ((flow, R.F, "forward"), (bj.inverse(flow), R.I, "inverse")):
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        flat_close(host(y), ref.out, dt, f"{what} {name} values")
        flat_close(host(l), ref.ladj, dt, f"{what} {name} ladj", per="element", floor=1.0)
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        flat_close(host(xb), ref.in_bar, dt, f"{what} {name} input cotangent")
        check_params(grads, ref, N, dt, f"{what} {name}")


def one_layer_given_as_a_matrix_and_a_vector_input(bj):
    """v (dim, batch): one layer; its cotangent comes back in that shape.  A 1-D input is one column."""
    dt, dim, N = F64, 5, 9
    R = Ref(dt, dim, 1, N, ("one-layer",))
    flow = bj.AmortizedHouseholderFlow(dev2(R.v[:, 0, :], dt), dev2(R.s, dt), dev2(R.m, dt))
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    y, l = bj.with_logabsdet_jacobian(flow, zd)                 # the siblings' shape: a per-column vector
    flat_close(host(y), R.F.out, dt, "householder_cols one layer values")
    flat_close(host(l), R.F.ladj, dt, "householder_cols one layer ladj", per="element", floor=1.0)
    flat_close(host(bj.logabsdetjac(flow, zd)), R.F.ladj, dt, "householder_cols one layer logabsdetjac", per="element", floor=1.0)
    for f, ref, name in ((flow, R.F, "forward"), (bj.inverse(flow), R.I, "inverse")):
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        assert grads["v"].shape == (dim, N) and grads["log_scale"].shape == (dim, N) and grads["shift"].shape == (dim, N)
        flat_close(host(xb), ref.in_bar, dt, f"householder_cols one layer {name} input cotangent")
        for k, r in (("v", ref.vb[:, 0, :]), ("log_scale", ref.sb), ("shift", ref.mb)):
            flat_close(host(grads[k]), r, dt, f"householder_cols one layer {name} {k} cotangent", term_scale=ref.scale)
    one = bj.AmortizedHouseholderFlow(dev2(R.v[:, 0, 1:2], dt), dev2(R.s[:, 1:2], dt), dev2(R.m[:, 1:2], dt))
    yv, lv = bj.with_logabsdet_jacobian(one, dev1(R.z[:, 1], dt), per_sample=True)
    assert yv.shape == (dim,)
    flat_close(host(yv).reshape(dim, 1), R.F.out[:, 1:2], dt, "householder_cols vector input values")
    flat_close(host(lv).reshape(1), R.F.ladj[1:2], dt, "householder_cols vector input ladj", per="element", floor=1.0)


# ------------------------------------------------------------------ host routing
def logpdf_of_a_transformed_normal_and_its_gradients(bj):
    """logpdf(transformed(MvNormal, flow), y) = N(f⁻¹(y)) − Σs and its gradients through the generic path: the inverse flow's pullback
    seeded with (−x, 1).  Both dtypes."""
    for dt in (F32, F64):
        dim, L, N = 6, 2, 50
        R = Ref(dt, dim, L, N, ("logpdf", np.dtype(dt).name))
        flow = make_flow(bj, R.v, R.s, R.m, dt)
        td = bj.transformed(bj.MvNormal(dim), flow)
        yd = dev2(R.z, dt)
        lp_ref = -0.5 * (R.I.out ** 2).sum(axis=0) - 0.5 * dim * np.log(2 * np.pi) + R.I.ladj
        what = f"householder_cols logpdf {np.dtype(dt).name}"
        flat_close(host(bj.logpdf(td, yd)), lp_ref, dt, what, per="element", floor=1.0)
        lp, yb, G = bj.logpdf_vjp_params(td, yd)
        flat_close(host(lp), lp_ref, dt, what + " (with gradients)", per="element", floor=1.0)
        ref = RefAll(R.v, R.s, R.m, R.z, -R.I.out, np.ones(N), inverse=True)
        flat_close(host(yb), ref.in_bar, dt, what + " input cotangent")
        check_params(G["transform"], ref, N, dt, what)


def composition_with_other_stages(bj, orc):
    dt, dim, L, N = F64, 5, 2, 20
    R = Ref(dt, dim, L, N, ("compose",))
    flow = make_flow(bj, R.v, R.s, R.m, dt)
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    # a Shift first, then the flow
    t = rounded(seed("shift").normal(size=dim), dt)
    comp = flow @ bj.Shift(dev1(t, dt))
    assert [type(s).__name__ for s in comp._plan()[0]] == ["Shift", "AmortizedHouseholderFlow"]
    y, l = bj.with_logabsdet_jacobian(comp, zd, per_sample=True)
    S = RefAll(R.v, R.s, R.m, R.z + t[:, None], R.g, R.lb)
    flat_close(host(y), S.out, dt, "householder_cols ∘ Shift values")
    flat_close(host(l), S.ladj, dt, "householder_cols ∘ Shift ladj", per="element", floor=1.0)
    flat_close(host(bj.transform(bj.inverse(comp), y)), R.z, dt, "householder_cols ∘ Shift round trip")
    flat_close(host(bj.vjp(comp, zd, gd, lbd)), S.in_bar, dt, "householder_cols ∘ Shift input cotangent")
    # an amortised radial stack first, then the flow: each stays a stage of its own
    al, be, z0, _, _, _ = radial_draws(seed("compose-radial"), dim, L, N, dt)
    radial = bj.AmortizedRadialLayer(dev2(al, dt), dev2(be, dt), dev3(z0, dt))
    comp = flow @ radial
    assert [type(s).__name__ for s in comp._plan()[0]] == ["AmortizedRadialLayer", "AmortizedHouseholderFlow"]
    mid = RadialRefAll(orc, al, be, z0, R.z, R.g, R.lb)             # its values and log-det; its cotangents are recomputed below
    P = RefAll(R.v, R.s, R.m, mid.out, R.g, R.lb)
    y, l = bj.with_logabsdet_jacobian(comp, zd, per_sample=True)
    flat_close(host(y), P.out, dt, "householder_cols ∘ radial_cols values")
    flat_close(host(l), P.ladj + mid.ladj, dt, "householder_cols ∘ radial_cols ladj", per="element", floor=1.0)
    back = RadialRefAll(orc, al, be, z0, R.z, P.in_bar, R.lb)
    flat_close(host(bj.vjp(comp, zd, gd, lbd)), back.in_bar, dt, "householder_cols ∘ radial_cols input cotangent")


# ------------------------------------------------------------------ special input
def a_nan_column_stays_in_its_column(bj):
    """A NaN in one column of z, and separately in one column of v: every output of that column that depends on the poisoned input
    is NaN in every row, and every other column meets the bar.  What does NOT depend on it stays what it was: the log-det Σs is a
    function of log_scale alone, x̄ = eˢ⊙H_0⋯H_{L−1}ȳ does not read z, and m̄ = ȳ (forward) reads neither."""
    for dt, dim in ((F32, 3), (F32, 64), (F64, 65)):
        for where in ("z", "v"):
            _check_nan_column(bj, dt, dim, where)


def _check_nan_column(bj, dt, dim, where):
    L = 2
    N = 2 * (256 // lanes(dim, dt)) + 3
    R = Ref(dt, dim, L, N, ("nan", np.dtype(dt).name, dim))
    bad = N // 2
    z, v = R.z.copy(), R.v.copy()
    if where == "z":
        z[0, bad] = np.nan
    else:
        v[dim - 1, 1, bad] = np.nan
    flow = make_flow(bj, v, R.s, R.m, dt)
    zd, gd, lbd = dev2(z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    keep = np.arange(N) != bad
    what = f"householder_cols NaN in {where} {np.dtype(dt).name} dim={dim}"
    for f, ref, name in ((flow, R.F, "forward"), (bj.inverse(flow), R.I, "inverse")):
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        y, l = host(y), host(l)
        assert np.isnan(y[:, bad]).all(), what
        flat_close(y[:, keep], ref.out[:, keep], dt, f"{what} {name} values")
        flat_close(l, ref.ladj, dt, f"{what} {name} ladj", per="element", floor=1.0)          # Σs: the poisoned column included
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        xb, vb, sb, mb = host(xb), host(grads["v"]), host(grads["log_scale"]), host(grads["shift"])
        assert np.isnan(vb[:, :, bad]).all() and np.isnan(sb[:, bad]).all(), what
        if where == "v":
            assert np.isnan(xb[:, bad]).all(), what
            assert np.isnan(mb[:, bad]).all() if name == "inverse" else np.array_equal(mb[:, bad], host(gd)[:, bad]), what
        else:
            flat_close(xb, ref.in_bar, dt, f"{what} {name} input cotangent of every column")
        flat_close(xb[:, keep], ref.in_bar[:, keep], dt, f"{what} {name} input cotangent")
        for k, got, r in (("v", vb, ref.vb), ("log_scale", sb, ref.sb), ("shift", mb, ref.mb)):
            flat_close(got[..., keep].reshape(-1, N - 1), r[..., keep].reshape(-1, N - 1), dt, f"{what} {name} {k} cotangent", term_scale=ref.scale[keep])


# ------------------------------------------------------------------ the two test ids
def test_kernels_at_every_form_edge_head_layout_and_special_input(bj):
    for dt in (F32, F64):
        maps_and_pullbacks_match_reference(bj, dt)
    for head in HEADS:
        head_combinations(bj, head)
    long_stack_in_float32(bj)
    grid_stride_sweeps_match_reference(bj)
    parameter_layouts_match_reference(bj)
    one_layer_given_as_a_matrix_and_a_vector_input(bj)
    a_nan_column_stays_in_its_column(bj)


def test_host_class_launch_count_routing_and_refusals(bj, orc):
    parameter_pullbacks_are_one_launch_in_either_direction(bj)
    sizes_beyond_the_limits_raise_value_errors(bj)
    logpdf_of_a_transformed_normal_and_its_gradients(bj)
    composition_with_other_stages(bj, orc)
