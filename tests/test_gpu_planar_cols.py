"""The amortised planar flow (`AmortizedPlanarLayer`, include/bjx_planar_cols.h) through bijectors_amd against the Float64 oracle applied
column by column (tests/_planar_cols_ref.py), on tests/_tol.py's flat bar (1e-3 Float32 / 1e-6 Float64): values and x̄ per="sample",
log-dets per="element" with a floor of 1, w̄ / ū / b̄ on the JOINT largest parameter-cotangent entry of the column (term_scale); only
the inverse pullback passes cond=planar_inverse_amp.  No column is left out of any comparison.

Dispatcher edges by dim (V = 4 / 2 elements per 16-byte pack in Float32 / Float64, G lanes per column, R packs per lane):
  1, 2, 3, 5   partial first pack, element form; G = 1 (Float32; Float64: G = 1 at 1 and 2, G = 2 at 3, G = 4 at 5)
  4, 8, 16     whole packs, vector form, G = 1, 2, 4 (Float32) / 2, 4, 8 (Float64)
  64           vector form, G = 16 (Float32) / 32 (Float64)
  65           element form, partial last pack, G = 32 / 64
  260 / 256    two packs per lane (R = 2), whole packs: Float32 / Float64
  261 / 257    Float32: R = 2 with a partial pack; Float64: 129 packs = three per lane on lane 0, the R = 4 kernels with dead packs
  1 024 / 512  the limits: R = 4, every pack live
Every case runs the batches 1, C − 1, C, C + 1 with C = 256/G columns per block.  L = 33 and 64 at dim 2 in Float64 take the
one-wave block of the pullback (their t table [L][256] would be 66 and 128 KiB, over the 64 KiB switch; L = 32 is exactly 64 KiB and
stays at 256 threads): there C = 64 in the pullback and 256 in the maps.

The round trip inverse(f)(f(x)) is compared with x on the flat bar per sample, on the largest state of the column's trajectory
z_0 … z_L (_tol.py's term_scale: x = f(x) − Σ û_k t_k cancels when a layer's ‖w‖ is tiny, û ~ 1/‖w‖, and the Float32 y itself is only
known to eps·|y|).  Measured on the MI355X at Float32, dim 1, L 8, column 18 of the draw: x = 0.0199, a layer with w = −0.00116 takes
the state to 49.6, f(x) = 49.1; the round trip returns x to 5e-5 absolute — 2.5e-3 of |x|, 1e-6 of the trajectory's scale; half an
ulp of the stored y alone moves x by 3e-4 of |x|."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _planar_cols_ref import (draws, inverse_amp, joint_scale, ref_inverse_param_vjp, ref_map, ref_param_vjp, ref_vjp, rounded,  # noqa: E402
                              seed, trajectory_scale)
from _tol import flat_close, planar_inverse_amp  # noqa: E402

F32, F64 = np.float32, np.float64
DIMS = {F32: [1, 2, 3, 5, 4, 8, 16, 64, 65, 260, 261, 1024], F64: [1, 2, 3, 5, 4, 8, 16, 64, 65, 256, 257, 512]}


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
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_layer(bj, w, u, b, dt):
    return bj.AmortizedPlanarLayer(dev3(w, dt), dev3(u, dt), dev2(b, dt))


class Ref:
    """Every reference quantity of one parameter draw, computed once; the tests slice its first n columns."""

    def __init__(self, orc, dt, dim, L, N, key):
        self.dt, self.N = dt, N
        self.w, self.u, self.b, self.z, self.g, self.lb = draws(seed(*key), dim, L, N, dt)
        w, u, b, z, g, lb = self.w, self.u, self.b, self.z, self.g, self.lb
        self.y, self.l = ref_map(orc, w, u, b, z)
        self.xi, self.li = ref_map(orc, w, u, b, z, inverse=True)
        self.xb = ref_vjp(orc, w, u, b, z, g, lb)
        self.yb = ref_vjp(orc, w, u, b, z, g, lb, inverse=True)
        self.wb, self.ub, self.bb = ref_param_vjp(orc, w, u, b, z, g, lb)
        self.amp = inverse_amp(orc, planar_inverse_amp, w, u, b, self.xi, dt)
        self.traj = trajectory_scale(w, u, b, z, self.y)


def check_all(bj, R, n, what):
    """Maps, round trip and pullbacks of the first n columns of the draw R, both directions."""
    dt = R.dt
    layer = make_layer(bj, R.w[:, :, :n], R.u[:, :, :n], R.b[:, :n], dt)
    inv = bj.inverse(layer)
    zd, gd, lbd = dev2(R.z[:, :n], dt), dev2(R.g[:, :n], dt), dev1(R.lb[:n], dt)
    y, l = bj.with_logabsdet_jacobian(layer, zd, per_sample=True)
    flat_close(host(y), R.y[:, :n], dt, what + " values")
    flat_close(host(l), R.l[:n], dt, what + " ladj", per="element", floor=1.0)
    xi, li = bj.with_logabsdet_jacobian(inv, zd, per_sample=True)
    flat_close(host(xi), R.xi[:, :n], dt, what + " inverse values")
    flat_close(host(li), R.li[:n], dt, what + " inverse ladj", per="element", floor=1.0)
    flat_close(host(bj.transform(inv, y)), R.z[:, :n], dt, what + " round trip", term_scale=R.traj[:n])
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    flat_close(host(xb), R.xb[:, :n], dt, what + " x̄")
    assert torch.equal(bj.vjp(layer, zd, gd, lbd), xb), "vjp and vjp_params disagree on x̄"
    ts = joint_scale(R.wb[:, :, :n], R.ub[:, :, :n], R.bb[:, :n])
    for k, ref in (("w", R.wb), ("u", R.ub), ("b", R.bb)):
        got = host(grads[k])
        assert got.shape == ref[..., :n].shape, (k, got.shape)
        flat_close(got.reshape(-1, n), ref[..., :n].reshape(-1, n), dt, f"{what} {k}̄", term_scale=ts)
    yb = bj.vjp(inv, zd, gd, lbd)
    flat_close(host(yb), R.yb[:, :n], dt, what + " inverse ȳ", cond=R.amp[:n])


def batches(C, more=()):
    return sorted({n for n in (1, C - 1, C, C + 1) + tuple(more) if n >= 1})


@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_maps_and_pullbacks_match_oracle(bj, orc, dt, L):
    """Every dim of the table above (one test per dtype and L: each failure names its dim and batch)."""
    for dim in DIMS[dt]:
        C = 256 // lanes(dim, dt)
        ns = batches(C, (257,) if dim == 64 else ())
        R = Ref(orc, dt, dim, L, max(ns), ("cols", np.dtype(dt).name, dim, L))
        for n in ns:
            check_all(bj, R, n, f"planar_cols {np.dtype(dt).name} dim={dim} L={L} batch={n}")


def test_long_stacks_at_the_one_wave_switch(bj, orc):
    """dim 2, Float64, G = 1: the t table of a 256-thread block is L·256·8 B — 64 KiB at L = 32 (kept), 66 KiB at 33 and 128 KiB at 64
    (one-wave blocks, 64 columns each).  Batches around both block sizes."""
    for L in (32, 33, 64):
        R = Ref(orc, F64, 2, L, 130, ("long", L))
        for n in (1, 63, 64, 65, 130):
            check_all(bj, R, n, f"planar_cols float64 dim=2 L={L} batch={n}")


# ------------------------------------------------------------------ refusals
def test_sizes_beyond_the_limits_raise_value_errors(bj):
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        w = torch.zeros((1, 1, lim + 1), dtype=dt, device="cuda").permute(2, 1, 0)
        layer = bj.AmortizedPlanarLayer(w, w, torch.zeros((1, 1), dtype=dt, device="cuda"))
        x = torch.zeros((1, lim + 1), dtype=dt, device="cuda").T
        for call in (lambda: bj.transform(layer, x), lambda: bj.transform(bj.inverse(layer), x), lambda: bj.vjp(layer, x, x), lambda: bj.vjp_params(layer, x, x)):
            with pytest.raises(ValueError, match=str(lim)):
                call()
    for L in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.AmortizedPlanarLayer(torch.zeros((3, L, 4), device="cuda"), torch.zeros((3, L, 4), device="cuda"), torch.zeros((L, 4), device="cuda"))
    layer = bj.AmortizedPlanarLayer(torch.zeros((3, 2, 4), device="cuda"), torch.zeros((3, 2, 4), device="cuda"), torch.zeros((2, 4), device="cuda"))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((5, 4), device="cuda").T.contiguous().T)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((5, 3), device="cuda").T)


# ------------------------------------------------------------------ grid-stride sweeps
def test_grid_stride_sweeps_match_oracle(bj, orc):
    """dim 2, L 1, Float32: G = 1, 256 columns per block, the grid capped at 8 blocks per CU.  Three and a half sweeps with a
    ragged last group, checked on the first group, the groups either side of every sweep boundary, the last group and 256 random
    columns."""
    dt, dim, L, C = F32, 2, 1, 256
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    batch = (3 * cap + cap // 2) * C - 17
    groups = (batch + C - 1) // C
    assert groups > 3 * cap and batch % C != 0
    rng = seed("sweep")
    gs = {0, groups - 1}
    for s in range(1, (groups - 1) // cap + 1):
        gs |= {s * cap - 1, s * cap}
    cols = set(rng.choice(batch, size=256, replace=False).tolist())
    for gr in gs:
        cols |= set(range(gr * C, min(batch, (gr + 1) * C)))
    cols = np.array(sorted(cols))
    s = 0.8 * dim ** -0.25
    w = np.asarray(s * rng.normal(size=(dim, L, batch)), dt)
    u = np.asarray(s * rng.normal(size=(dim, L, batch)), dt)
    b, z, g, lb = (np.asarray(rng.normal(size=sh), dt) for sh in ((L, batch), (dim, batch), (dim, batch), (batch,)))
    layer = make_layer(bj, w, u, b, dt)
    zd, gd, lbd, ci = dev2(z, dt), dev2(g, dt), dev1(lb, dt), torch.from_numpy(cols).cuda()
    ws, us, bs, zs, gs_, lbs = (a[..., cols].astype(np.float64) for a in (w, u, b, z, g, lb))
    what = f"planar_cols sweeps batch={batch}"
    for inverse in (False, True):
        f = bj.inverse(layer) if inverse else layer
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        y_ref, l_ref = ref_map(orc, ws, us, bs, zs, inverse=inverse)
        flat_close(host(y[:, ci]), y_ref, dt, f"{what} inv={inverse} values")
        flat_close(host(l[ci]), l_ref, dt, f"{what} inv={inverse} ladj", per="element", floor=1.0)
        # the summed log-det of the same launch: the Float64 sum of the per-column values
        _, (l2, tot) = bj.with_logabsdet_jacobian(f, zd, per_sample="both")
        assert torch.equal(l2, l)
        flat_close(host(tot.reshape(1)), host(l.double().sum().reshape(1)), F64, f"{what} inv={inverse} summed ladj", per="element", floor=1.0)
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    flat_close(host(xb[:, ci]), ref_vjp(orc, ws, us, bs, zs, gs_, lbs), dt, what + " x̄")
    wb, ub, bb = ref_param_vjp(orc, ws, us, bs, zs, gs_, lbs)
    ts = joint_scale(wb, ub, bb)
    n = len(cols)
    for k, ref in (("w", wb), ("u", ub), ("b", bb)):
        flat_close(host(grads[k][..., ci]).reshape(-1, n), ref.reshape(-1, n), dt, f"{what} {k}̄", term_scale=ts)
    yb = bj.vjp(bj.inverse(layer), zd, gd, lbd)
    x_pre, _ = ref_map(orc, ws, us, bs, zs, inverse=True)
    flat_close(host(yb[:, ci]), ref_vjp(orc, ws, us, bs, zs, gs_, lbs, inverse=True), dt, what + " inverse ȳ",
               cond=inverse_amp(orc, planar_inverse_amp, ws, us, bs, x_pre, dt))


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_parameter_layouts_match_oracle(bj, orc, dt):
    """dim 64, L 2: one head [2·dim·L + L + pad, batch] sliced three ways (ld > dim·L; pad = 6 keeps ld a multiple of the pack and the
    vector form, pad = 3 makes ld odd: element form), and dense parameters whose base pointer is ONE element off 16-byte alignment
    (element form).  No copy is made (data_ptr), and the values meet the bar in every form."""
    R = Ref(orc, dt, 64, 2, 37, ("layout", np.dtype(dt).name))
    for layout in ("head_vector", "head_element", "off_by_one"):
        _check_layout(bj, R, dt, layout)


def _check_layout(bj, R, dt, layout):
    dim, L, N = 64, 2, 37
    tdt = torch.float32 if dt == F32 else torch.float64
    wn, un = (np.ascontiguousarray(np.transpose(a, (2, 1, 0))).reshape(N, L * dim) for a in (R.w, R.u))       # (N, L·dim) rows = columns
    bn = np.ascontiguousarray(R.b.T)
    if layout.startswith("head"):
        rows = 2 * dim * L + L + (6 if layout == "head_vector" else 3)
        head = torch.zeros((N, rows), dtype=tdt, device="cuda")
        head[:, :dim * L] = torch.from_numpy(wn.astype(dt)).cuda()
        head[:, dim * L:2 * dim * L] = torch.from_numpy(un.astype(dt)).cuda()
        head[:, 2 * dim * L:2 * dim * L + L] = torch.from_numpy(bn.astype(dt)).cuda()
        w = head[:, :dim * L].view(N, L, dim).permute(2, 1, 0)
        u = head[:, dim * L:2 * dim * L].view(N, L, dim).permute(2, 1, 0)
        b = head[:, 2 * dim * L:2 * dim * L + L].T
        want_ld = rows
    else:
        bufs = [torch.zeros(N * L * dim + 1, dtype=tdt, device="cuda") for _ in range(2)]
        for buf, a in zip(bufs, (wn, un)):
            buf[1:] = torch.from_numpy(a.astype(dt).reshape(-1)).cuda()
        w, u = (buf[1:].view(N, L, dim).permute(2, 1, 0) for buf in bufs)
        assert w.data_ptr() % 16 == np.dtype(dt).itemsize
        b = torch.from_numpy(bn.astype(dt)).cuda().T
        want_ld = dim * L
    layer = bj.AmortizedPlanarLayer(w, u, b)
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    pw, pu, pb, lw, lu, _ = layer._col_params(zd, dim, N)
    assert (pw.data_ptr(), pu.data_ptr(), pb.data_ptr()) == (w.data_ptr(), u.data_ptr(), b.data_ptr()) and (lw, lu) == (want_ld, want_ld)
    what = f"planar_cols {layout} {np.dtype(dt).name}"
    y, l = bj.with_logabsdet_jacobian(layer, zd, per_sample=True)
    flat_close(host(y), R.y, dt, what + " values")
    flat_close(host(l), R.l, dt, what + " ladj", per="element", floor=1.0)
    xi, li = bj.with_logabsdet_jacobian(bj.inverse(layer), zd, per_sample=True)
    flat_close(host(xi), R.xi, dt, what + " inverse values")
    flat_close(host(li), R.li, dt, what + " inverse ladj", per="element", floor=1.0)
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    flat_close(host(xb), R.xb, dt, what + " x̄")
    ts = joint_scale(R.wb, R.ub, R.bb)
    for k, ref in (("w", R.wb), ("u", R.ub), ("b", R.bb)):
        flat_close(host(grads[k]).reshape(-1, N), ref.reshape(-1, N), dt, f"{what} {k}̄", term_scale=ts)
    flat_close(host(bj.vjp(bj.inverse(layer), zd, gd, lbd)), R.yb, dt, what + " inverse ȳ", cond=R.amp)


def test_one_layer_given_as_matrices_and_a_vector_input(bj, orc):
    """w, u (dim, batch) and b (batch,): one layer; the cotangents come back in those shapes.  A 1-D input is one column."""
    dt, dim, N = F64, 5, 9
    R = Ref(orc, dt, dim, 1, N, ("one-layer",))
    layer = bj.AmortizedPlanarLayer(dev2(R.w[:, 0, :], dt), dev2(R.u[:, 0, :], dt), dev1(R.b[0], dt))
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    y, l = bj.with_logabsdet_jacobian(layer, zd)                 # the reference's shape: a per-column vector, as PlanarLayer
    flat_close(host(y), R.y, dt, "planar_cols one layer values")
    flat_close(host(l), R.l, dt, "planar_cols one layer ladj", per="element", floor=1.0)
    flat_close(host(bj.logabsdetjac(layer, zd)), R.l, dt, "planar_cols one layer logabsdetjac", per="element", floor=1.0)
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    assert grads["w"].shape == (dim, N) and grads["u"].shape == (dim, N) and grads["b"].shape == (N,)
    ts = joint_scale(R.wb, R.ub, R.bb)
    for k, ref in (("w", R.wb[:, 0, :]), ("u", R.ub[:, 0, :]), ("b", R.bb[0])):
        flat_close(host(grads[k]).reshape(-1, N), ref.reshape(-1, N), dt, f"planar_cols one layer {k}̄", term_scale=ts)
    one = bj.AmortizedPlanarLayer(dev2(R.w[:, 0, :1], dt), dev2(R.u[:, 0, :1], dt), dev1(R.b[0, :1], dt))
    yv, lv = bj.with_logabsdet_jacobian(one, dev1(R.z[:, 0], dt), per_sample=True)
    assert yv.shape == (dim,)
    flat_close(host(yv).reshape(dim, 1), R.y[:, :1], dt, "planar_cols vector input values")
    flat_close(host(lv).reshape(1), R.l[:1], dt, "planar_cols vector input ladj", per="element", floor=1.0)


# ------------------------------------------------------------------ host routing
@pytest.mark.parametrize("dt", [F32, F64])
def test_inverse_parameter_pullback_matches_composed_reference(bj, orc, dt):
    dim, L, N = 7, 3, 40
    R = Ref(orc, dt, dim, L, N, ("inv-params", np.dtype(dt).name))
    layer = make_layer(bj, R.w, R.u, R.b, dt)
    yb, grads = bj.vjp_params(bj.inverse(layer), dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt))
    yb_ref, wb, ub, bb = ref_inverse_param_vjp(orc, R.w, R.u, R.b, R.z, R.g, R.lb)
    what = f"planar_cols inverse vjp_params {np.dtype(dt).name}"
    flat_close(host(yb), yb_ref, dt, what + " ȳ", cond=R.amp)
    ts = joint_scale(wb, ub, bb)
    for k, ref in (("w", wb), ("u", ub), ("b", bb)):
        flat_close(host(grads[k]).reshape(-1, N), ref.reshape(-1, N), dt, f"{what} {k}̄", term_scale=ts)


@pytest.mark.parametrize("dt", [F32, F64])
def test_logpdf_of_a_transformed_normal_and_its_gradients(bj, orc, dt):
    dim, L, N = 6, 2, 50
    R = Ref(orc, dt, dim, L, N, ("logpdf", np.dtype(dt).name))
    layer = make_layer(bj, R.w, R.u, R.b, dt)
    td = bj.transformed(bj.MvNormal(dim), layer)
    yd = dev2(R.z, dt)
    lp_ref = -0.5 * (R.xi ** 2).sum(axis=0) - 0.5 * dim * np.log(2 * np.pi) + R.li
    what = f"planar_cols logpdf {np.dtype(dt).name}"
    flat_close(host(bj.logpdf(td, yd)), lp_ref, dt, what, per="element", floor=1.0)
    lp, yb, G = bj.logpdf_vjp_params(td, yd)
    flat_close(host(lp), lp_ref, dt, what + " (with gradients)", per="element", floor=1.0)
    ones = np.ones(N)
    yb_ref, wb, ub, bb = ref_inverse_param_vjp(orc, R.w, R.u, R.b, R.z, -R.xi, ones)
    flat_close(host(yb), yb_ref, dt, what + " ȳ", cond=R.amp)
    ts = joint_scale(wb, ub, bb)
    for k, ref in (("w", wb), ("u", ub), ("b", bb)):
        flat_close(host(G["transform"][k]).reshape(-1, N), ref.reshape(-1, N), dt, f"{what} {k}̄", term_scale=ts)


def test_composition_with_other_stages(bj, orc):
    dt, dim, L, N = F64, 5, 2, 20
    R = Ref(orc, dt, dim, L, N, ("compose",))
    layer = make_layer(bj, R.w, R.u, R.b, dt)
    t = rounded(seed("shift").normal(size=dim), dt)
    zd = dev2(R.z, dt)
    flow = layer @ bj.Shift(dev1(t, dt))                         # Shift first, then the layer
    y, l = bj.with_logabsdet_jacobian(flow, zd, per_sample=True)
    y_ref, l_ref = ref_map(orc, R.w, R.u, R.b, R.z + t[:, None])
    flat_close(host(y), y_ref, dt, "planar_cols ∘ Shift values")
    flat_close(host(l), l_ref, dt, "planar_cols ∘ Shift ladj", per="element", floor=1.0)
    flat_close(host(bj.transform(bj.inverse(flow), y)), R.z, dt, "planar_cols ∘ Shift round trip")
    xb = bj.vjp(flow, zd, dev2(R.g, dt), dev1(R.lb, dt))
    flat_close(host(xb), ref_vjp(orc, R.w, R.u, R.b, R.z + t[:, None], R.g, R.lb), dt, "planar_cols ∘ Shift x̄")


def test_planar_layer_still_reads_a_matrix_as_layers(bj, orc):
    """PlanarLayer is untouched: a (dim, n) matrix is (dim, n_layers) — the bits of the run of its single layers — also when n
    equals the batch."""
    dim = n = 6
    rng = seed("planar-matrix")
    w, u, b = rng.normal(size=(dim, n)) / 3, rng.normal(size=(dim, n)) / 3, rng.normal(size=n)
    z = rng.normal(size=(dim, n))
    zd = dev2(z, F64)
    stack = bj.PlanarLayer(torch.tensor(w).cuda(), torch.tensor(u).cuda(), torch.tensor(b).cuda())
    assert stack.n_layers == n
    res = bj.with_logabsdet_jacobian(stack, zd)
    run = bj.PlanarLayer.stack([bj.PlanarLayer(torch.tensor(w[:, k]).cuda(), torch.tensor(u[:, k]).cuda(), torch.tensor(b[k:k + 1]).cuda()) for k in range(n)])
    res2 = bj.with_logabsdet_jacobian(run, zd)
    assert torch.equal(res.result, res2.result) and torch.equal(res.logabsdetjac, res2.logabsdetjac)
    y_ref, l_ref = orc.planar(w, u, b, np.asfortranarray(z))
    flat_close(host(res.result), y_ref, F64, "PlanarLayer (dim, n_layers) values")
    flat_close(host(res.logabsdetjac), l_ref, F64, "PlanarLayer (dim, n_layers) ladj", per="element", floor=1.0)


# ------------------------------------------------------------------ special input
def test_a_nan_column_stays_in_its_column(bj, orc):
    for dt, dim in ((F32, 3), (F32, 64), (F64, 65)):
        _check_nan_column(bj, orc, dt, dim)


def _check_nan_column(bj, orc, dt, dim):
    L = 2
    N = 2 * (256 // lanes(dim, dt)) + 3
    R = Ref(orc, dt, dim, L, N, ("nan", np.dtype(dt).name, dim))
    bad = N // 2
    z = R.z.copy()
    z[0, bad] = np.nan
    layer = make_layer(bj, R.w, R.u, R.b, dt)
    zd, gd, lbd = dev2(z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    keep = np.arange(N) != bad
    what = f"planar_cols NaN column {np.dtype(dt).name} dim={dim}"
    for inverse, yr, lr in ((False, R.y, R.l), (True, R.xi, R.li)):
        y, l = bj.with_logabsdet_jacobian(bj.inverse(layer) if inverse else layer, zd, per_sample=True)
        y, l = host(y), host(l)
        assert np.isnan(y[:, bad]).all() and np.isnan(l[bad]), what
        flat_close(y[:, keep], yr[:, keep], dt, f"{what} inv={inverse} values")
        flat_close(l[keep], lr[keep], dt, f"{what} inv={inverse} ladj", per="element", floor=1.0)
    xb, grads = bj.vjp_params(layer, zd, gd, lbd)
    assert np.isnan(host(xb)[:, bad]).all() and np.isnan(host(grads["b"])[:, bad]).all() and np.isnan(host(grads["w"])[:, :, bad]).all(), what
    flat_close(host(xb)[:, keep], R.xb[:, keep], dt, what + " x̄")
    assert np.isfinite(host(grads["w"])[:, :, keep]).all() and np.isfinite(host(grads["u"])[:, :, keep]).all() and np.isfinite(host(grads["b"])[:, keep]).all(), what
