"""The amortised radial flow (`AmortizedRadialLayer`, include/bjx_radial_cols.h) through bijectors_amd against the Float64 oracle applied
column by column (tests/_radial_cols_ref.py), on tests/_tol.py's flat bar (1e-3 Float32 / 1e-6 Float64), no conditioned bar anywhere:
values, x̄ and ȳ per="sample" at dim >= 2 and with floor=1.0 at dim 1 (a column of one entry has no scale of its own; the inputs are
unit-scale draws), log-dets per="element" with a floor of 1, ᾱ_ / β̄ / z̄₀ on the JOINT largest parameter-cotangent entry of the column
(term_scale).  No column is left out of any comparison; column 0 of every draw sits exactly on z₀ of the first layer (r = 0).

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
Every case runs the batches 1, C − 1, C, C + 1 with C = 256/G columns per block.  L = 33 and 64 at dim 2 in Float64 take the
one-wave block of the forward pullback (its r table [L][256] would be 66 and 128 KiB, over the 64 KiB switch; L = 32 is exactly
64 KiB and stays at 256 threads): there C = 64 in the forward pullback and 256 everywhere else.

The closed forms with these draws were evaluated in numpy Float32 against Float64 before the first GPU run (the kernel's operation
order, rewind included; 300 columns per case, dim 1 … 64, L 1 … 8): x̄ and the parameter cotangents stay below 4e-5 of their scale."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _planar_cols_ref import draws as planar_draws  # noqa: E402
from _planar_cols_ref import ref_map as planar_ref_map  # noqa: E402
from _planar_cols_ref import ref_vjp as planar_ref_vjp  # noqa: E402
from _radial_cols_ref import RefAll, VecAll, draws, rounded, seed  # noqa: E402
from _tol import flat_close  # noqa: E402

F32, F64 = np.float32, np.float64
DIMS = {F32: [1, 2, 3, 5, 4, 8, 16, 64, 65, 260, 261, 516, 765, 1024], F64: [1, 2, 3, 5, 4, 8, 16, 64, 65, 256, 257, 384, 512]}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radial_layer_bits.npz")


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


def make_layer(bj, al, be, z0, dt):
    return bj.AmortizedRadialLayer(dev2(al, dt), dev2(be, dt), dev3(z0, dt))


def close_cols(got, ref, dt, what):
    """Values and input cotangents (dim, n): per sample; a column of ONE entry on a floor of 1."""
    return flat_close(got, ref, dt, what, per="sample", floor=1.0 if ref.shape[0] == 1 else 0.0)


class Ref:
    """Every reference quantity of one parameter draw, computed once; the tests slice its first n columns.  F: the flow at z with the
    cotangents (g, lb); I: its inverse at the SAME input and cotangents."""

    def __init__(self, orc, dt, dim, L, N, key):
        self.dt, self.N = dt, N
        self.al, self.be, self.z0, self.z, self.g, self.lb = draws(seed(*key), dim, L, N, dt)
        self.F = RefAll(orc, self.al, self.be, self.z0, self.z, self.g, self.lb)
        self.I = RefAll(orc, self.al, self.be, self.z0, self.z, self.g, self.lb, inverse=True)


def check_params(grads, ref, n, dt, what):
    for k, r in (("alpha_", ref.ab), ("beta", ref.bb), ("z_0", ref.zb)):
        got = host(grads[k])
        assert got.shape == r[..., :n].shape, (what, k, got.shape)
        flat_close(got.reshape(-1, n), r[..., :n].reshape(-1, n), dt, f"{what} {k} cotangent", term_scale=ref.scale[:n])


def check_all(bj, R, n, what):
    """Maps, round trip and pullbacks of the first n columns of the draw R, both directions."""
    dt = R.dt
    layer = make_layer(bj, R.al[:, :n], R.be[:, :n], R.z0[:, :, :n], dt)
    inv = bj.inverse(layer)
    zd, gd, lbd = dev2(R.z[:, :n], dt), dev2(R.g[:, :n], dt), dev1(R.lb[:n], dt)
    y, l = bj.with_logabsdet_jacobian(layer, zd, per_sample=True)
    close_cols(host(y), R.F.out[:, :n], dt, what + " values")
    flat_close(host(l), R.F.ladj[:n], dt, what + " ladj", per="element", floor=1.0)
    xi, li = bj.with_logabsdet_jacobian(inv, zd, per_sample=True)
    close_cols(host(xi), R.I.out[:, :n], dt, what + " inverse values")
    flat_close(host(li), R.I.ladj[:n], dt, what + " inverse ladj", per="element", floor=1.0)
    close_cols(host(bj.transform(inv, y)), R.z[:, :n], dt, what + " round trip")
    for f, ref, name in ((layer, R.F, "forward"), (inv, R.I, "inverse")):
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        close_cols(host(xb), ref.in_bar[:, :n], dt, f"{what} {name} input cotangent")
        assert torch.equal(bj.vjp(f, zd, gd, lbd), xb), f"{what} {name}: vjp and vjp_params disagree on the input cotangent"
        check_params(grads, ref, n, dt, f"{what} {name}")


def batches(C, more=()):
    return sorted({n for n in (1, C - 1, C, C + 1) + tuple(more) if n >= 1})


@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_maps_and_pullbacks_match_oracle(bj, orc, dt):
    """Every dim of the table above at L = 1, 2 and 8 (one test per dtype: each failure names its dim, L and batch)."""
    for L in (1, 2, 8):
        for dim in DIMS[dt]:
            C = 256 // lanes(dim, dt)
            ns = batches(C, (257,) if dim == 64 else ())
            R = Ref(orc, dt, dim, L, max(ns), ("cols", np.dtype(dt).name, dim, L))
            for n in ns:
                check_all(bj, R, n, f"radial_cols {np.dtype(dt).name} dim={dim} L={L} batch={n}")


def test_long_stacks_at_the_one_wave_switch(bj, orc):
    """dim 2, Float64, G = 1: the r table of a 256-thread block is L·256·8 B — 64 KiB at L = 32 (kept), 66 KiB at 33 and 128 KiB at 64
    (one-wave blocks, 64 columns each).  Batches around both block sizes.

    Long stacks are not run in Float32.  Tried once at dim 3, L 64, 70 columns: maps and log-dets 1.5e-6 of their scale, the forward
    pullback 8.5e-4 (numpy Float32 of the same closed forms: 8.6e-4), but the INVERSE pullback 3.4e-2 of ȳ's scale at column 49
    (numpy Float32: 6.3e-2 at the same column, 9 of the 70 columns over 1e-3; Float64 of the same code 7e-11).  The kernel is not at
    fault and neither is the draw's conditioning in y: the pre-image x is right to 4e-8, but the reverse sweep re-applies the 64
    layers forwards from it, and where the flow expands (the inverse contracts: gains down to 0.3 per layer here) that rounding grows
    to 1.6e-2 at z₆₃.  Any Float32 evaluation that rewinds instead of storing the L states has it; at L <= 8 it stays below 1e-4."""
    for L in (32, 33, 64):
        R = Ref(orc, F64, 2, L, 65, ("long", L))
        for n in (1, 63, 64, 65):
            check_all(bj, R, n, f"radial_cols float64 dim=2 L={L} batch={n}")


def test_parameter_pullbacks_are_one_launch_in_either_direction(bj, orc):
    """vjp_params(layer, …) and vjp_params(inverse(layer), …) are ONE hot launch each (the inverse is not composed of three)."""
    R = Ref(orc, F32, 16, 3, 20, ("launches",))
    layer = make_layer(bj, R.al, R.be, R.z0, F32)
    zd, gd, lbd = dev2(R.z, F32), dev2(R.g, F32), dev1(R.lb, F32)
    for f in (layer, bj.inverse(layer)):
        bj.vjp_params(f, zd, gd, lbd)
        _, _, k = bj.kernel_timed(lambda: bj.vjp_params(f, zd, gd, lbd))
        assert k == 1, f"{type(f).__name__}: {k} hot launches"


# ------------------------------------------------------------------ refusals
def test_sizes_beyond_the_limits_raise_value_errors(bj):
    for dt, lim in ((torch.float32, 1024), (torch.float64, 512)):
        z0 = torch.zeros((1, 1, lim + 1), dtype=dt, device="cuda").permute(2, 1, 0)
        s = torch.zeros((1, 1), dtype=dt, device="cuda")
        layer = bj.AmortizedRadialLayer(s, s, z0)
        x = torch.zeros((1, lim + 1), dtype=dt, device="cuda").T
        for call in (lambda: bj.transform(layer, x), lambda: bj.transform(bj.inverse(layer), x), lambda: bj.vjp(layer, x, x), lambda: bj.vjp_params(layer, x, x),
                     lambda: bj.vjp_params(bj.inverse(layer), x, x)):
            with pytest.raises(ValueError, match=str(lim)):
                call()
    for L in (0, 65):
        with pytest.raises(ValueError, match="64"):
            bj.AmortizedRadialLayer(torch.zeros((L, 4), device="cuda"), torch.zeros((L, 4), device="cuda"), torch.zeros((3, L, 4), device="cuda"))
    layer = bj.AmortizedRadialLayer(torch.zeros((2, 4), device="cuda"), torch.zeros((2, 4), device="cuda"), torch.zeros((3, 2, 4), device="cuda"))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((5, 4), device="cuda").T.contiguous().T)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(layer, torch.zeros((5, 3), device="cuda").T)


# ------------------------------------------------------------------ grid-stride sweeps
def test_grid_stride_sweeps_match_oracle(bj, orc):
    """dim 2, L 1, Float32: G = 1, 256 columns per block, the grid capped at 8 blocks per CU.  Three and a half sweeps with a
    ragged last group, checked on the first group, the groups either side of every sweep boundary, the last group and 256 random
    columns.  The reference of those ~4 000 columns is the vectorised numpy restatement of the closed forms (`VecAll`), held to the
    oracle column by column on its first 64 columns at 1e-12."""
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
    al, be, z0, z, g, lb = draws(rng, dim, L, batch, dt)
    layer = make_layer(bj, al, be, z0, dt)
    zd, gd, lbd, ci = dev2(z, dt), dev2(g, dt), dev1(lb, dt), torch.from_numpy(cols).cuda()
    sub = [a[..., cols] for a in (al, be, z0, z, g, lb)]
    n = len(cols)
    what = f"radial_cols sweeps batch={batch}"
    for inverse in (False, True):
        V = VecAll(*sub, inverse=inverse)
        O = RefAll(orc, *(a[..., :64] for a in sub), inverse=inverse)
        for k in ("out", "ladj", "in_bar", "ab", "bb", "zb"):
            assert np.abs(getattr(V, k)[..., :64] - getattr(O, k)).max() <= 1e-12 * max(1.0, np.abs(getattr(O, k)).max()), f"the restatement's {k} leaves the oracle"
        f = bj.inverse(layer) if inverse else layer
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        flat_close(host(y[:, ci]), V.out, dt, f"{what} inv={inverse} values")
        flat_close(host(l[ci]), V.ladj, dt, f"{what} inv={inverse} ladj", per="element", floor=1.0)
        # the summed log-det of the same launch: the Float64 sum of the per-column values
        _, (l2, tot) = bj.with_logabsdet_jacobian(f, zd, per_sample="both")
        assert torch.equal(l2, l)
        flat_close(host(tot.reshape(1)), host(l.double().sum().reshape(1)), F64, f"{what} inv={inverse} summed ladj", per="element", floor=1.0)
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        flat_close(host(xb[:, ci]), V.in_bar, dt, f"{what} inv={inverse} input cotangent")
        for k, ref in (("alpha_", V.ab), ("beta", V.bb), ("z_0", V.zb)):
            flat_close(host(grads[k][..., ci]).reshape(-1, n), ref.reshape(-1, n), dt, f"{what} inv={inverse} {k} cotangent", term_scale=V.scale)


# ------------------------------------------------------------------ layouts
def test_parameter_layouts_match_oracle(bj, orc):
    """dim 64, L 2: one head [dim·L + 2L + pad, batch] sliced three ways (ld_z > dim·L; pad = 4 keeps ld_z a multiple of the pack and the
    vector form, pad = 3 makes ld_z odd: element form), and a dense z₀ whose base pointer is ONE element off 16-byte alignment
    (element form).  No copy is made (data_ptr), and the values meet the bar in every form."""
    for dt in (F32, F64):
        R = Ref(orc, dt, 64, 2, 37, ("layout", np.dtype(dt).name))
        for layout in ("head_vector", "head_element", "off_by_one"):
            _check_layout(bj, R, dt, layout)


def _check_layout(bj, R, dt, layout):
    dim, L, N = 64, 2, 37
    tdt = torch.float32 if dt == F32 else torch.float64
    zn = np.ascontiguousarray(np.transpose(R.z0, (2, 1, 0))).reshape(N, L * dim)       # (N, L·dim): rows = columns
    an, bn = np.ascontiguousarray(R.al.T), np.ascontiguousarray(R.be.T)
    if layout.startswith("head"):
        rows = dim * L + 2 * L + (4 if layout == "head_vector" else 3)
        head = torch.zeros((N, rows), dtype=tdt, device="cuda")
        head[:, :dim * L] = torch.from_numpy(zn.astype(dt)).cuda()
        head[:, dim * L:dim * L + L] = torch.from_numpy(an.astype(dt)).cuda()
        head[:, dim * L + L:dim * L + 2 * L] = torch.from_numpy(bn.astype(dt)).cuda()
        z0 = head[:, :dim * L].view(N, L, dim).permute(2, 1, 0)
        a = head[:, dim * L:dim * L + L].T
        b = head[:, dim * L + L:dim * L + 2 * L].T
        want = (rows, rows, rows)
        assert (rows % (16 // np.dtype(dt).itemsize) == 0) == (layout == "head_vector")
    else:
        buf = torch.zeros(N * L * dim + 1, dtype=tdt, device="cuda")
        buf[1:] = torch.from_numpy(zn.astype(dt).reshape(-1)).cuda()
        z0 = buf[1:].view(N, L, dim).permute(2, 1, 0)
        assert z0.data_ptr() % 16 == np.dtype(dt).itemsize
        a, b = torch.from_numpy(an.astype(dt)).cuda().T, torch.from_numpy(bn.astype(dt)).cuda().T
        want = (L, L, dim * L)
    layer = bj.AmortizedRadialLayer(a, b, z0)
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    pa, pb, pz, la, lb_, lz = layer._col_params(zd, dim, N)
    assert (pa.data_ptr(), pb.data_ptr(), pz.data_ptr()) == (a.data_ptr(), b.data_ptr(), z0.data_ptr()) and (la, lb_, lz) == want
    what = f"radial_cols {layout} {np.dtype(dt).name}"
    for f, ref, name in ((layer, R.F, "forward"), (bj.inverse(layer), R.I, "inverse")):
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        flat_close(host(y), ref.out, dt, f"{what} {name} values")
        flat_close(host(l), ref.ladj, dt, f"{what} {name} ladj", per="element", floor=1.0)
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        flat_close(host(xb), ref.in_bar, dt, f"{what} {name} input cotangent")
        check_params(grads, ref, N, dt, f"{what} {name}")


def test_one_layer_given_as_matrices_and_a_vector_input(bj, orc):
    """z_0 (dim, batch) and alpha_, beta (batch,): one layer; the cotangents come back in those shapes.  A 1-D input is one column."""
    dt, dim, N = F64, 5, 9
    R = Ref(orc, dt, dim, 1, N, ("one-layer",))
    layer = bj.AmortizedRadialLayer(dev1(R.al[0], dt), dev1(R.be[0], dt), dev2(R.z0[:, 0, :], dt))
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    y, l = bj.with_logabsdet_jacobian(layer, zd)                 # the reference's shape: a per-column vector, as RadialLayer
    flat_close(host(y), R.F.out, dt, "radial_cols one layer values")
    flat_close(host(l), R.F.ladj, dt, "radial_cols one layer ladj", per="element", floor=1.0)
    flat_close(host(bj.logabsdetjac(layer, zd)), R.F.ladj, dt, "radial_cols one layer logabsdetjac", per="element", floor=1.0)
    for f, ref, name in ((layer, R.F, "forward"), (bj.inverse(layer), R.I, "inverse")):
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        assert grads["alpha_"].shape == (N,) and grads["beta"].shape == (N,) and grads["z_0"].shape == (dim, N)
        flat_close(host(xb), ref.in_bar, dt, f"radial_cols one layer {name} input cotangent")
        for k, r in (("alpha_", ref.ab[0]), ("beta", ref.bb[0]), ("z_0", ref.zb[:, 0, :])):
            flat_close(host(grads[k]).reshape(-1, N), r.reshape(-1, N), dt, f"radial_cols one layer {name} {k} cotangent", term_scale=ref.scale)
    one = bj.AmortizedRadialLayer(dev1(R.al[0, :1], dt), dev1(R.be[0, :1], dt), dev2(R.z0[:, 0, :1], dt))
    yv, lv = bj.with_logabsdet_jacobian(one, dev1(R.z[:, 0], dt), per_sample=True)
    assert yv.shape == (dim,)
    flat_close(host(yv).reshape(dim, 1), R.F.out[:, :1], dt, "radial_cols vector input values")
    flat_close(host(lv).reshape(1), R.F.ladj[:1], dt, "radial_cols vector input ladj", per="element", floor=1.0)


# ------------------------------------------------------------------ host routing
def test_logpdf_of_a_transformed_normal_and_its_gradients(bj, orc):
    """logpdf(transformed(MvNormal, layer), y) = N(f⁻¹(y)) − ℓ(f⁻¹(y)) and its gradients through the generic path: the inverse flow's
    pullback seeded with (−x, 1).  Both dtypes."""
    for dt in (F32, F64):
        _check_logpdf(bj, orc, dt)


def _check_logpdf(bj, orc, dt):
    dim, L, N = 6, 2, 50
    R = Ref(orc, dt, dim, L, N, ("logpdf", np.dtype(dt).name))
    layer = make_layer(bj, R.al, R.be, R.z0, dt)
    td = bj.transformed(bj.MvNormal(dim), layer)
    yd = dev2(R.z, dt)
    lp_ref = -0.5 * (R.I.out ** 2).sum(axis=0) - 0.5 * dim * np.log(2 * np.pi) + R.I.ladj
    what = f"radial_cols logpdf {np.dtype(dt).name}"
    flat_close(host(bj.logpdf(td, yd)), lp_ref, dt, what, per="element", floor=1.0)
    lp, yb, G = bj.logpdf_vjp_params(td, yd)
    flat_close(host(lp), lp_ref, dt, what + " (with gradients)", per="element", floor=1.0)
    ref = RefAll(orc, R.al, R.be, R.z0, R.z, -R.I.out, np.ones(N), inverse=True)
    flat_close(host(yb), ref.in_bar, dt, what + " input cotangent")
    check_params(G["transform"], ref, N, dt, what)


def test_composition_with_other_stages(bj, orc):
    dt, dim, L, N = F64, 5, 2, 20
    R = Ref(orc, dt, dim, L, N, ("compose",))
    layer = make_layer(bj, R.al, R.be, R.z0, dt)
    zd, gd, lbd = dev2(R.z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    # a Shift first, then the layer
    t = rounded(seed("shift").normal(size=dim), dt)
    flow = layer @ bj.Shift(dev1(t, dt))
    y, l = bj.with_logabsdet_jacobian(flow, zd, per_sample=True)
    S = RefAll(orc, R.al, R.be, R.z0, R.z + t[:, None], R.g, R.lb)
    flat_close(host(y), S.out, dt, "radial_cols ∘ Shift values")
    flat_close(host(l), S.ladj, dt, "radial_cols ∘ Shift ladj", per="element", floor=1.0)
    flat_close(host(bj.transform(bj.inverse(flow), y)), R.z, dt, "radial_cols ∘ Shift round trip")
    flat_close(host(bj.vjp(flow, zd, gd, lbd)), S.in_bar, dt, "radial_cols ∘ Shift input cotangent")
    # an amortised planar stack first, then the layer: each stays a stage of its own
    w, u, b, _, _, _ = planar_draws(seed("compose-planar"), dim, L, N, dt)
    planar = bj.AmortizedPlanarLayer(dev3(w, dt), dev3(u, dt), dev2(b, dt))
    flow = layer @ planar
    assert [type(s).__name__ for s in flow._plan()[0]] == ["AmortizedPlanarLayer", "AmortizedRadialLayer"]
    mid, l_mid = planar_ref_map(orc, w, u, b, R.z)
    P = RefAll(orc, R.al, R.be, R.z0, mid, R.g, R.lb)
    y, l = bj.with_logabsdet_jacobian(flow, zd, per_sample=True)
    flat_close(host(y), P.out, dt, "radial_cols ∘ planar_cols values")
    flat_close(host(l), P.ladj + l_mid, dt, "radial_cols ∘ planar_cols ladj", per="element", floor=1.0)
    flat_close(host(bj.vjp(flow, zd, gd, lbd)), planar_ref_vjp(orc, w, u, b, R.z, P.in_bar, R.lb), dt, "radial_cols ∘ planar_cols input cotangent")


def radial_layer_bits(bj, al, be, z0, z, g, lb):
    """What a RadialLayer, the fused run of three and the run's inverse return on one set of inputs -> {name: numpy array}."""
    dt = z.dtype.type
    layers = [bj.RadialLayer(dev1(al[k:k + 1], dt), dev1(be[k:k + 1], dt), dev1(z0[:, k], dt)) for k in range(al.shape[0])]
    flow = layers[2] @ layers[1] @ layers[0]
    zd, gd, lbd = dev2(z, dt), dev2(g, dt), dev1(lb, dt)
    got = {}
    got["one_y"], got["one_l"] = (host(t) for t in bj.with_logabsdet_jacobian(layers[0], zd, per_sample=True))
    got["one_xb"] = host(bj.vjp(layers[0], zd, gd, lbd))
    got["run_y"], got["run_l"] = (host(t) for t in bj.with_logabsdet_jacobian(flow, zd, per_sample=True))
    got["run_xb"] = host(bj.vjp(flow, zd, gd, lbd))
    got["inv_y"], got["inv_l"] = (host(t) for t in bj.with_logabsdet_jacobian(bj.inverse(flow), zd, per_sample=True))
    xb, grads = bj.vjp_params(flow, zd, gd, lbd)
    got["run_pxb"] = host(xb)
    for i, st in enumerate(grads["stages"]):
        for k in ("alpha_", "beta", "z_0"):
            got[f"run_p{i}_{k}"] = host(st[k])
    return got


def test_radial_layer_and_its_fused_run_give_the_bits_they_gave_before(bj):
    """RadialLayer and _RadialRun are untouched: on the inputs stored in tests/golden/radial_layer_bits.npz (Float32 and Float64, dim 5,
    three layers, 9 columns) the single layer, the fused run of three, its inverse and its parameter pullback return, bit for bit,
    what the commit before the amortised radial flow returned on an MI355X (stored next to the inputs)."""
    doc = np.load(GOLDEN)
    for name in ("float32", "float64"):
        got = radial_layer_bits(bj, *(doc[f"{name}_{k}"] for k in ("al", "be", "z0", "z", "g", "lb")))
        assert len(got) == 18
        for k, v in got.items():
            ref = doc[f"{name}_{k}"]
            assert v.dtype == ref.dtype and v.shape == ref.shape and v.tobytes() == ref.tobytes(), f"{name} {k}: the bits changed"


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
    layer = make_layer(bj, R.al, R.be, R.z0, dt)
    zd, gd, lbd = dev2(z, dt), dev2(R.g, dt), dev1(R.lb, dt)
    keep = np.arange(N) != bad
    what = f"radial_cols NaN column {np.dtype(dt).name} dim={dim}"
    for f, ref, name in ((layer, R.F, "forward"), (bj.inverse(layer), R.I, "inverse")):
        y, l = bj.with_logabsdet_jacobian(f, zd, per_sample=True)
        y, l = host(y), host(l)
        assert np.isnan(y[:, bad]).all() and np.isnan(l[bad]), what
        flat_close(y[:, keep], ref.out[:, keep], dt, f"{what} {name} values")
        flat_close(l[keep], ref.ladj[keep], dt, f"{what} {name} ladj", per="element", floor=1.0)
        xb, grads = bj.vjp_params(f, zd, gd, lbd)
        xb, ab, bb, zb = host(xb), host(grads["alpha_"]), host(grads["beta"]), host(grads["z_0"])
        assert np.isnan(xb[:, bad]).all() and np.isnan(ab[:, bad]).all() and np.isnan(bb[:, bad]).all() and np.isnan(zb[:, :, bad]).all(), what
        flat_close(xb[:, keep], ref.in_bar[:, keep], dt, f"{what} {name} input cotangent")
        assert np.isfinite(ab[:, keep]).all() and np.isfinite(bb[:, keep]).all() and np.isfinite(zb[:, :, keep]).all(), what
