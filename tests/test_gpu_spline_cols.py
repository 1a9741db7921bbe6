"""Per-column RationalQuadraticSpline (include/bjx_cols.h: bjx_rqs_cols / bjx_rqs_cols_vjp): the spline law of a Coupling whose θ
returns per-sample knots (neural spline flows), against the CPU oracle applied COLUMN BY COLUMN — oracle.rqs / rqs_params /
coupling_rqs / rqs_vjp / rqs_vjp_knots / rqs_params_vjp on the (n1, K+1) knots of one column.

Tolerances: tests/_tol.py's flat 1e-3 (Float32) / 1e-6 (Float64).  Scales: values and cotangents per="sample" (the column's
max-norm); log-dets per="element" with a floor of 1 (a log-det near 0 is compared on the scale of one bin's log-slope)."""
import copy
import ctypes as C
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _tol import flat_close  # noqa: E402

DT = {np.float32: torch.float32, np.float64: torch.float64}


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def dev3(a, dt):
    """(n, m, N) numpy -> cuda tensor laid out column-major per column (a permute(2, 1, 0) view)."""
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 1, 0))).astype(dt)).cuda()
    return t.permute(2, 1, 0)


def dev2(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def host(t):
    return t.detach().cpu().numpy()


def raw_params(rng, n, K, N, scale=1.0):
    return rng.normal(size=(n, K, N)) * scale, rng.normal(size=(n, K, N)) * scale, rng.normal(size=(n, max(K - 1, 0), N)) * scale


def knots_of(orc, rw, rh, rd, B, dt):
    """oracle.rqs_params column by column -> (n, K+1, N) knot arrays in `dt`."""
    n, K, N = rw.shape
    W, H, D = (np.empty((n, K + 1, N), dt) for _ in range(3))
    for c in range(N):
        w, h, d = orc.rqs_params(rw[:, :, c].astype(dt), rh[:, :, c].astype(dt), rd[:, :, c].astype(dt).reshape(n, K - 1), B)
        W[:, :, c], H[:, :, c], D[:, :, c] = w, h, d
    return W, H, D


def inputs(rng, W, H, B, inverse, dt):
    """Normal draws inside (-B, B) plus points outside, points exactly on knots and ±0."""
    n, K1, N = W.shape
    x = (rng.uniform(-0.95, 0.95, size=(n, N)) * B).astype(dt)
    kn = H if inverse else W
    specials = [1.5 * B, -2.0 * B, None, 0.0, -0.0, 1.01 * B, -1.01 * B]
    for c, v in enumerate(specials[:N]):
        if v is None:
            x[:, c] = kn[:, min(2, K1 - 1) if K1 > 2 else 0, c] if K1 > 2 else x[:, c]
        else:
            x[:, c] = v
    if N > 8:
        for r in range(n):                                 # one interior knot per row in column 8
            x[r, 8] = kn[r, 1 + r % max(K1 - 2, 1), 8]
    return x


def ref_spline(orc, W, H, D, x, inverse):
    n, K1, N = W.shape
    ys, ls = np.empty_like(x), np.empty(N, x.dtype)
    for c in range(N):
        y, l = orc.rqs(W[:, :, c], H[:, :, c], D[:, :, c], np.asfortranarray(x[:, c:c + 1]), inverse=inverse)
        ys[:, c], ls[c] = y[:, 0], l[0]
    return ys, ls


SHAPES = [(1, 1, 5), (7, 5, 333), (16, 8, 1000), (32, 16, 257), (3, 32, 65), (64, 10, 64), (5, 4, 40), (6, 2, 100), (4, 64, 50)]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", ["knots", "raw"])
@pytest.mark.parametrize("inverse", [False, True])
def test_per_column_spline_matches_oracle(bj, orc, dt, shape, form, inverse):
    dim, K, N = shape
    rng = np.random.default_rng(zlib.crc32(repr((dim, K, N, form, inverse)).encode()))
    B = 3.0
    rw, rh, rd = raw_params(rng, dim, K, N)
    W, H, D = knots_of(orc, rw, rh, rd, B, dt)
    x = inputs(rng, W, H, B, inverse, dt)
    if form == "raw":
        sp = bj.RationalQuadraticSpline(dev3(rw, dt), dev3(rh, dt), dev3(rd, dt), B)
    else:
        sp = bj.RationalQuadraticSpline(dev3(W, dt), dev3(H, dt), dev3(D, dt))
    b = bj.inverse(sp) if inverse else sp
    xd = dev2(x, dt)
    y, lps = bj.with_logabsdet_jacobian(b, xd, per_sample=True)
    y_ref, l_ref = ref_spline(orc, W, H, D, x, inverse)
    what = f"rqs_cols {form} inv={inverse} {shape}"
    flat_close(host(y), y_ref, dt, what + " values")
    flat_close(host(lps), l_ref, dt, what + " ladj", per="element", floor=1.0)
    _, s1 = bj.with_logabsdet_jacobian(b, xd)
    _, s2 = bj.with_logabsdet_jacobian(b, xd)
    flat_close(float(s1), float(np.sum(l_ref.astype(np.float64))), dt, what + " summed ladj", per="element", floor=float(np.abs(l_ref).sum()) + 1.0)
    assert float(s1) == float(s2), "two identical calls give identical summed log-det bits"
    assert torch.equal(bj.transform(b, xd), y)
    assert float(bj.logabsdetjac(b, xd)) == float(s1)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_round_trip_is_identity_and_log_dets_cancel(bj, orc, dt):
    rng = np.random.default_rng(11)
    dim, K, N, B = 12, 8, 777, 2.5
    rw, rh, rd = raw_params(rng, dim, K, N)
    sp = bj.RationalQuadraticSpline(dev3(rw, dt), dev3(rh, dt), dev3(rd, dt), B)
    x = dev2(rng.uniform(-1.2 * B, 1.2 * B, size=(dim, N)), dt)
    y, l1 = bj.with_logabsdet_jacobian(sp, x, per_sample=True)
    xr, l2 = bj.with_logabsdet_jacobian(bj.inverse(sp), y, per_sample=True)
    flat_close(host(xr), host(x), dt, "rqs_cols round trip")
    flat_close(host(l1 + l2), np.zeros(N), dt, "rqs_cols round-trip log-dets", per="element", floor=float(host(l1).__abs__().max()) + 1.0)


def test_vector_input_with_one_column_of_knots(bj, orc):
    rng = np.random.default_rng(5)
    dim, K, B = 9, 8, 2.0
    rw, rh, rd = raw_params(rng, dim, K, 1)
    W, H, D = knots_of(orc, rw, rh, rd, B, np.float64)
    sp = bj.RationalQuadraticSpline(dev3(W, np.float64), dev3(H, np.float64), dev3(D, np.float64))
    x = rng.uniform(-B, B, size=dim)
    y, l = bj.with_logabsdet_jacobian(sp, torch.from_numpy(x).cuda())
    y_ref, l_ref = ref_spline(orc, W, H, D, x[:, None], False)
    flat_close(host(y), y_ref[:, 0], np.float64, "rqs_cols vector input", per="tensor")
    flat_close(float(l), float(l_ref[0]), np.float64, "rqs_cols vector ladj", per="element", floor=1.0)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(sp, dev2(rng.normal(size=(dim, 3)), np.float64))


# ------------------------------------------------------------------ Coupling with a data-dependent spline law
class Head(torch.nn.Module):
    """θ: x₂ (n2, batch) -> one head (batch, 3K-1, n1), sliced with no copy into the raw spline parameters."""

    def __init__(self, n2, n1, K, B, dt, knots=False):
        super().__init__()
        self.n1, self.K, self.B, self.knots = n1, K, B, knots
        self.lin = torch.nn.Linear(n2, (3 * K - 1) * n1, dtype=dt)

    def head(self, x2):
        x2m = x2[:, None] if x2.dim() == 1 else x2
        return self.lin(x2m.T).reshape(-1, 3 * self.K - 1, self.n1).permute(2, 1, 0)      # (n1, 3K-1, batch), column-major per column

    def __call__(self, x2):
        import bijectors_amd as bj
        hd = self.head(x2)
        K, B = self.K, self.B
        rw, rh, rd = hd[:, :K], hd[:, K:2 * K], hd[:, 2 * K:]
        if not self.knots:
            return bj.RationalQuadraticSpline(rw, rh, rd, B)
        # normalised knots built in torch (the B constructor written out): a θ that returns (n1, K+1, batch) knots
        def cum(r):
            c = torch.cumsum(torch.softmax(r, dim=1), dim=1)
            return torch.cat([torch.zeros_like(c[:, :1]), c], dim=1) * (2 * B) - B
        one = torch.ones_like(rd[:, :1])
        return bj.RationalQuadraticSpline(cum(rw), cum(rh), torch.cat([one, torch.nn.functional.softplus(rd), one], dim=1))


def masks(dim):
    n1 = dim // 2
    return {"range": list(range(1, n1 + 1)), "scattered": [i for i in range(1, dim + 1) if i % 3 != 0][:n1]}


def coupling_ref(orc, th, bj, mask, x, inverse, dt):
    """oracle.coupling_rqs on each column with the knots θ gives that column (θ evaluated once, on the host)."""
    dim, N = x.shape
    i1 = np.array(mask.indices_1) - 1
    i2 = np.array(mask.indices_2) - 1
    with torch.no_grad():
        law = th(torch.from_numpy(np.ascontiguousarray(x[i2])).cuda().to(DT[dt]))
    if law._cols[0] == 1:
        W, H, D = knots_of(orc, host(law.widths).astype(np.float64), host(law.heights).astype(np.float64), host(law.derivatives).astype(np.float64), law._cols[2], dt)
    else:
        W, H, D = (host(t).astype(dt) for t in (law.widths, law.heights, law.derivatives))
    ys, ls = np.empty_like(x), np.empty(N, dt)
    for c in range(N):
        y, l = orc.coupling_rqs(i1, W[:, :, c], H[:, :, c], D[:, :, c], np.asfortranarray(x[:, c:c + 1]), inverse=inverse)
        ys[:, c], ls[c] = y[:, 0], l[0]
    return ys, ls


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("mname", ["range", "scattered"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("knots", [False, True])
def test_coupling_with_data_dependent_spline_matches_oracle(bj, orc, dt, mname, inverse, knots):
    rng = np.random.default_rng(7)
    dim, K, N, B = 10, 8, 1024, 3.0
    mask = bj.PartitionMask(dim, masks(dim)[mname])
    torch.manual_seed(1)
    th = Head(dim - len(mask.indices_1), len(mask.indices_1), K, B, DT[dt], knots=knots).cuda()
    cl = bj.Coupling(th, mask)
    x = rng.normal(size=(dim, N)).astype(dt) * 2
    y, l = bj.with_logabsdet_jacobian(bj.inverse(cl) if inverse else cl, dev2(x, dt), per_sample=True)
    y_ref, l_ref = coupling_ref(orc, th, bj, mask, x, inverse, dt)
    flat_close(host(y), y_ref, dt, f"coupling rqs_cols {mname} inv={inverse} knots={knots} values")
    flat_close(host(l), l_ref, dt, f"coupling rqs_cols {mname} inv={inverse} knots={knots} ladj", per="element", floor=1.0)
    i2 = np.array(mask.indices_2) - 1
    assert np.array_equal(host(y)[i2], x[i2]), "rows outside x₁ copy through"


# ------------------------------------------------------------------ pullbacks
def ref_cols_pullback(orc, W, H, D, x1, g1, lb, inverse, raw=None, B=None):
    """Per-column oracle: x̄₁ (rqs_vjp) and the knot (rqs_vjp_knots on a one-column batch) or raw (rqs_params_vjp) cotangents."""
    n, K1, N = W.shape
    xb = np.empty((n, N))
    cw, ch, cd = (np.empty((n, K1, N)) for _ in range(3))
    for c in range(N):
        args = (W[:, :, c], H[:, :, c], D[:, :, c], x1[:, c:c + 1], g1[:, c:c + 1])
        l_ = None if lb is None else lb[c:c + 1]
        xb[:, c] = orc.rqs_vjp(*args, ladj_bar=l_, inverse=inverse)[:, 0]
        cw[:, :, c], ch[:, :, c], cd[:, :, c] = orc.rqs_vjp_knots(*args, ladj_bar=l_, inverse=inverse)
    if raw is None:
        return xb, (cw, ch, cd)
    rw, rh, rd = raw
    K = K1 - 1
    ow, oh, od = np.empty((n, K, N)), np.empty((n, K, N)), np.empty((n, K - 1, N))
    for c in range(N):
        ow[:, :, c], oh[:, :, c], od[:, :, c] = orc.rqs_params_vjp(rw[:, :, c], rh[:, :, c], rd[:, :, c].reshape(n, K - 1), B, cw[:, :, c], ch[:, :, c], cd[:, :, c])
    return xb, (ow, oh, od)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["knots", "raw"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("with_lb", [True, False])
@pytest.mark.parametrize("K", [8, 5])
def test_per_column_parameter_cotangents_match_oracle(bj, orc, dt, form, inverse, with_lb, K):
    rng = np.random.default_rng(21)
    dim, N, B = 6, 300, 2.0
    rw, rh, rd = raw_params(rng, dim, K, N)
    W, H, D = knots_of(orc, rw, rh, rd, B, np.float64)
    x = rng.uniform(-1.1 * B, 1.1 * B, size=(dim, N))
    g = rng.normal(size=(dim, N))
    lb = rng.normal(size=N) if with_lb else None
    if form == "raw":
        sp = bj.RationalQuadraticSpline(dev3(rw, dt), dev3(rh, dt), dev3(rd, dt), B)
    else:
        sp = bj.RationalQuadraticSpline(dev3(W, dt), dev3(H, dt), dev3(D, dt))
    b = bj.inverse(sp) if inverse else sp
    xb, grads = bj.vjp_params(b, dev2(x, dt), dev2(g, dt), None if lb is None else torch.from_numpy(lb.astype(dt)).cuda())
    xb_ref, cots = ref_cols_pullback(orc, W, H, D, x, g, lb, inverse, raw=(rw, rh, rd) if form == "raw" else None, B=B)
    flat_close(host(xb), xb_ref, dt, f"rqs_cols vjp x̄ {form} inv={inverse}")
    flat_close(host(bj.vjp(b, dev2(x, dt), dev2(g, dt), None if lb is None else torch.from_numpy(lb.astype(dt)).cuda())), xb_ref, dt, "rqs_cols vjp x̄ (vjp)")
    keys = ("widths", "heights", "derivatives") if form == "knots" else ("raw_widths", "raw_heights", "raw_derivatives")
    for k, ref in zip(keys, cots):
        got = host(grads[k])
        assert got.shape == ref.shape
        if form == "knots" and k == "derivatives":
            ref = ref.copy()
            ref[:, -1] = 0.0                 # the derivative at the last knot is not read by the spline
        flat_close(got.reshape(-1, N), ref.reshape(-1, N), dt, f"rqs_cols {k} {form} inv={inverse}",
                   term_scale=np.abs(np.concatenate([c_.reshape(-1, N) for c_ in cots])).max(axis=0))


def _loss(bj, b, x, g, lb):
    y, l = bj.with_logabsdet_jacobian(b, x, per_sample=True)
    return float((y.double() * g).sum() + (l.double() * lb).sum())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("with_lb", [True, False])
@pytest.mark.parametrize("dt,mname", [(np.float64, "scattered"), (np.float64, "range"), (np.float32, "scattered"), (np.float32, "range")])
def test_coupling_pullback_matches_oracle_and_autograd_through_theta(bj, orc, dt, mname, inverse, with_lb):
    """The reference evaluates θ in Float64 on the host from the same weights and x (in Float32: the device runs θ in Float32)."""
    rng = np.random.default_rng(33)
    dim, K, N, B = 8, 8, 512, 3.0
    mask = bj.PartitionMask(dim, masks(dim)[mname])
    n1 = len(mask.indices_1)
    torch.manual_seed(2)
    th = Head(dim - n1, n1, K, B, DT[dt]).cuda()
    cl = bj.Coupling(th, mask)
    x = (rng.normal(size=(dim, N)) * 2).astype(dt).astype(np.float64)
    g = rng.normal(size=(dim, N)).astype(dt).astype(np.float64)
    lb = rng.normal(size=N).astype(dt).astype(np.float64) if with_lb else None
    xb = bj.vjp(bj.inverse(cl) if inverse else cl, dev2(x, dt), dev2(g, dt), None if lb is None else torch.from_numpy(lb.astype(dt)).cuda())
    # reference: the oracle's per-column cotangents, then θ's pullback by torch.autograd on the CPU
    i1, i2 = np.array(mask.indices_1) - 1, np.array(mask.indices_2) - 1
    thc = copy.deepcopy(th).cpu().double()
    x2 = torch.from_numpy(np.ascontiguousarray(x[i2])).requires_grad_(True)
    hd = thc.head(x2)
    raw = [host(hd[:, :K]), host(hd[:, K:2 * K]), host(hd[:, 2 * K:])]
    W, H, D = knots_of(orc, *raw, B, np.float64)
    xb1, (ow, oh, od) = ref_cols_pullback(orc, W, H, D, x[i1], g[i1], lb, inverse, raw=raw, B=B)
    cot = torch.from_numpy(np.concatenate([ow, oh, od], axis=1))
    g2, = torch.autograd.grad(hd, [x2], cot)
    ref = g.copy()
    ref[i1] = xb1
    ref[i2] += g2.numpy()
    flat_close(host(xb), ref, dt, f"coupling rqs_cols x̄ {mname} inv={inverse}")


def test_coupling_pullback_matches_finite_differences(bj):
    rng = np.random.default_rng(44)
    dim, K, N, B = 6, 4, 3, 3.0
    mask = bj.PartitionMask(dim, [1, 2, 5])
    torch.manual_seed(4)
    th = Head(3, 3, K, B, torch.float64).cuda()
    cl = bj.Coupling(th, mask)
    x = rng.normal(size=(dim, N))
    g = torch.from_numpy(rng.normal(size=(dim, N))).cuda()
    lb = torch.from_numpy(rng.normal(size=N)).cuda()
    xb = host(bj.vjp(cl, dev2(x, np.float64), g, lb))
    fd = np.empty_like(x)
    eps = 1e-6
    for i in range(dim):
        for c in range(N):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += eps
            xm[i, c] -= eps
            fd[i, c] = (_loss(bj, cl, dev2(xp, np.float64), g, lb) - _loss(bj, cl, dev2(xm, np.float64), g, lb)) / (2 * eps)
    flat_close(xb, fd, np.float64, "coupling rqs_cols x̄ vs central differences")


def _fd_weights(bj, cl, th, x, g, lb, idx, inverse=False):
    b = bj.inverse(cl) if inverse else cl
    w = th.lin.weight
    out = []
    for (i, j) in idx:
        old = float(w[i, j])
        h = 1e-6
        with torch.no_grad():
            w[i, j] = old + h
        fp = _loss(bj, b, x, g, lb)
        with torch.no_grad():
            w[i, j] = old - h
        fm = _loss(bj, b, x, g, lb)
        with torch.no_grad():
            w[i, j] = old
        out.append((fp - fm) / (2 * h))
    return np.array(out)


class AffineHead(torch.nn.Module):
    def __init__(self, n2, n1):
        super().__init__()
        self.lin = torch.nn.Linear(n2, 2 * n1, dtype=torch.float64)
        self.n1 = n1

    def __call__(self, x2):
        import bijectors_amd as bj
        o = self.lin(x2.T).T                           # (2 n1, batch)
        return bj.Shift(o[self.n1:]) @ bj.Scale(torch.exp(0.3 * o[:self.n1]), batched=True)


@pytest.mark.parametrize("law", ["spline_cols", "affine", "shared_knots"])
@pytest.mark.parametrize("inverse", [False, True])
def test_vjp_params_of_coupling_gives_theta_weight_gradients(bj, orc, law, inverse):
    rng = np.random.default_rng(55)
    dim, K, N, B = 8, 8, 64, 3.0
    mask = bj.PartitionMask(dim, [1, 2, 3, 4])
    torch.manual_seed(6)
    if law == "spline_cols":
        th = Head(4, 4, K, B, torch.float64).cuda()
    elif law == "affine":
        th = AffineHead(4, 4).cuda()
    else:
        base = torch.from_numpy(rng.normal(size=(4, K))).cuda()
        lin = torch.nn.Linear(4, 1, dtype=torch.float64).cuda()

        class Shared(torch.nn.Module):       # shared knots that depend on θ's weights (not on x₂)
            def __init__(self):
                super().__init__()
                self.lin = lin

            def __call__(self, x2):
                r = base * (1 + 0.1 * self.lin.weight.sum())
                c = torch.cumsum(torch.softmax(r, dim=1), dim=1)
                kn = torch.cat([torch.zeros_like(c[:, :1]), c], dim=1) * (2 * B) - B
                c2 = torch.cumsum(torch.softmax(0.5 * r, dim=1), dim=1)
                kh = torch.cat([torch.zeros_like(c2[:, :1]), c2], dim=1) * (2 * B) - B
                return bj.RationalQuadraticSpline(kn, kh, torch.ones(4, K + 1, dtype=torch.float64, device="cuda") * 1.1)
        th = Shared().cuda()
    cl = bj.Coupling(th, mask)
    x = dev2(rng.normal(size=(dim, N)) * (1.5 if law != "affine" else 1.0), np.float64)
    g = torch.from_numpy(rng.normal(size=(dim, N))).cuda()
    lb = torch.from_numpy(rng.normal(size=N)).cuda()
    b = bj.inverse(cl) if inverse else cl
    xb, grads = bj.vjp_params(b, x, g, lb)
    assert "theta" in grads and set(grads["theta"]) == {k for k, _ in th.named_parameters()}
    if law == "affine":
        assert grads["scale"].shape == (4, N) and grads["shift"].shape == (4, N)
    elif law == "shared_knots":
        assert grads["widths"].shape == (4, K + 1)
    else:
        assert grads["raw_widths"].shape == (4, K, N) and grads["raw_derivatives"].shape == (4, K - 1, N)
    idx = [(0, 0), (1, 2), (3, 1), (0, 3)] if law != "shared_knots" else [(0, 0), (0, 2)]
    fd = _fd_weights(bj, cl, th, x, g, lb, idx, inverse)
    got = np.array([float(grads["theta"]["lin.weight"][i, j]) for i, j in idx])
    flat_close(got, fd, np.float64, f"vjp_params(Coupling {law}) θ weights vs finite differences", per="tensor", term_scale=1e-3 * np.abs(fd).max())
    flat_close(host(xb), host(bj.vjp(b, x, g, lb)), np.float64, f"vjp_params(Coupling {law}) x̄ = vjp x̄", per="sample")


# ------------------------------------------------------------------ at size, compositions, capture, errors
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("inverse", [False, True])
def test_replicated_knots_match_the_shared_knot_path_at_size(bj, orc, dt, inverse):
    rng = np.random.default_rng(66)
    dim, K, N, B = 64, 8, 1 << 16, 3.0
    i1 = list(range(1, 33))
    rw, rh, rd = raw_params(rng, 32, K, 1)
    W, H, D = knots_of(orc, rw, rh, rd, B, dt)
    Wd, Hd, Dd = (dev2(a[:, :, 0], dt) for a in (W, H, D))
    rep = [t[:, :, None].expand(32, K + 1, N) for t in (Wd, Hd, Dd)]          # same knots in every column (stride 0: made dense once)
    x = dev2(rng.normal(size=(dim, N)) * 2, dt)
    g = dev2(rng.normal(size=(dim, N)), dt)
    mask = bj.PartitionMask(dim, i1)
    shared = bj.Coupling(lambda x2: bj.RationalQuadraticSpline(Wd, Hd, Dd), mask)
    cols = bj.Coupling(lambda x2: bj.RationalQuadraticSpline(*rep), mask)
    f = (lambda c: bj.inverse(c)) if inverse else (lambda c: c)
    y1, l1 = bj.with_logabsdet_jacobian(f(shared), x, per_sample=True)
    y2, l2 = bj.with_logabsdet_jacobian(f(cols), x, per_sample=True)
    flat_close(host(y2), host(y1), dt, "replicated knots vs shared-knot coupling values")
    flat_close(host(l2), host(l1), dt, "replicated knots vs shared-knot coupling ladj", per="element", floor=1.0)
    sp_s, sp_c = bj.RationalQuadraticSpline(Wd, Hd, Dd), bj.RationalQuadraticSpline(*rep)
    xs = x[:32]
    flat_close(host(bj.vjp(f(sp_c), xs, g[:32])), host(bj.vjp(f(sp_s), xs, g[:32])), dt, "replicated knots vs bjx_rqs_vjp")


def test_logpdf_of_a_four_layer_spline_coupling_flow(bj, orc):
    rng = np.random.default_rng(77)
    dim, K, N, B = 8, 8, 2048, 3.0
    torch.manual_seed(8)
    perm = [2, 4, 6, 8, 1, 3, 5, 7]
    layers, heads = [], []
    for li in range(4):
        mask = bj.PartitionMask(dim, list(range(1, 5)) if li % 2 == 0 else list(range(5, 9)))
        th = Head(4, 4, K, B, torch.float64).cuda()
        heads.append((th, mask))
        layers.append(bj.Coupling(th, mask))
    P = bj.Permute(perm)
    flow = layers[0]
    for c in layers[1:]:
        flow = c @ P @ flow
    td = bj.transformed(bj.MvNormal(dim), flow)
    y = rng.normal(size=(dim, N)) * 1.5
    lp = host(bj.logpdf(td, dev2(y, np.float64)))
    # NumPy composition of the oracle pieces: invert the flow layer by layer, the oracle coupling per column
    cur = y.copy()
    ladj = np.zeros(N)
    inv_perm = np.array(perm) - 1                        # Permute(perm): y[perm[i]] = x[i], so x = y[perm - 1]
    for li in reversed(range(4)):
        th, mask = heads[li]
        ys, ls = coupling_ref(orc, th, bj, mask, cur, True, np.float64)
        cur, ladj = ys, ladj + ls
        if li > 0:
            cur = orc.permute(inv_perm.astype(np.int32), np.asfortranarray(cur))
    ref = -0.5 * (cur ** 2).sum(axis=0) - 0.5 * dim * np.log(2 * np.pi) + ladj
    flat_close(lp, ref, np.float64, "logpdf(transformed(MvNormal, 4 x spline Coupling))", per="element", floor=float(np.abs(ref).max()))
    smp = bj.rand(td, 256, seed=3, dtype=torch.float64)
    assert tuple(smp.shape) == (dim, 256) and bool(torch.isfinite(smp).all())


def test_captured_step_replays_to_the_eager_bits(bj, orc):
    rng = np.random.default_rng(88)
    dim, K, N, B = 32, 8, 4096, 3.0
    rw, rh, rd = raw_params(rng, dim, K, N)
    sp = bj.RationalQuadraticSpline(dev3(rw, np.float32), dev3(rh, np.float32), dev3(rd, np.float32), B)
    x = dev2(rng.normal(size=(dim, N)) * 2, np.float32)
    y = torch.empty_like(x)
    y_ref, l_ref = bj.with_logabsdet_jacobian(sp, x, per_sample=True)

    def step():
        return bj.shard.with_logabsdet_jacobian_sharded(sp, x, out=y)

    cs = bj.CapturedStep(step)
    y.zero_()
    yy, lps, lsum = cs.replay()
    cs.wait()
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref) and torch.equal(lps, l_ref)
    cs.replay(2)
    cs.wait()
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref)
    cs.close()


def test_errors_through_the_c_abi(bj):
    L = bj._lib
    lib = L.load()
    ctx = bj.context(torch.device("cuda", 0))
    n, K, N = 4, 8, 16
    p = torch.zeros((N, K + 1, n), device="cuda").permute(2, 1, 0)
    x = torch.zeros((N, n), device="cuda").T
    y = torch.empty_like(x)
    P = C.c_void_p(p.data_ptr())
    X, Y = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    ld = n * (K + 1)

    def call(form=L.BJX_COLS_KNOTS, k=K, B=0.0, pw=P, ldw=ld, xin=X, dim=n, n1=n, idx=None):
        return lib.bjx_rqs_cols(ctx.h, L.BJX_F32, 0, form, idx, n1, pw, P, P, ldw, ld, ld, k, B, xin, Y, None, None, dim, N, 0)

    assert call(k=0) == L.ERR_UNSUPPORTED and b"bins" in lib.bjx_last_error(ctx.h)
    assert call(k=65) == L.ERR_UNSUPPORTED
    assert call(pw=None) == L.ERR_ARG
    assert call(xin=None) == L.ERR_ARG
    assert call(form=L.BJX_COLS_RAW, k=K, B=0.0) == L.ERR_ARG
    assert call(form=L.BJX_COLS_RAW, k=K, B=-1.0) == L.ERR_ARG
    assert call(ldw=ld - 1) == L.ERR_SHAPE
    assert call(n1=n - 1) == L.ERR_SHAPE                      # no idx1: every row is transformed
    assert lib.bjx_rqs_cols_vjp(ctx.h, L.BJX_F32, 0, L.BJX_COLS_KNOTS, None, n, P, P, P, ld, ld, ld, 0, 0.0, X, X, None, Y, None, None, None, n, N) == L.ERR_UNSUPPORTED
    # the context stays usable
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, x)                                  # zeros: knots all 0 -> outside every bin, identity
    sp = bj.RationalQuadraticSpline(torch.zeros(n, K + 1, N + 1, device="cuda"), torch.zeros(n, K + 1, N + 1, device="cuda"), torch.ones(n, K + 1, N + 1, device="cuda"))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        bj.transform(sp, x)
