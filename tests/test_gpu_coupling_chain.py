"""Coupling with a per-sample elementwise-chain law (include/bjx_coupling.h: bjx_coupling_chain / bjx_coupling_chain_vjp) against
the CPU oracle as it stands: oracle.chain (the fused restatement, which takes one parameter per row) and oracle.chain_vjp,
applied COLUMN BY COLUMN with that column's parameters.

Reference of a parameter cotangent: stage k's parameter a enters through that stage alone, so ā = g_k · ∂y_k/∂a + ℓ̄ · ∂ℓ_k/∂a with
g_k the cotangent of the stage's OUTPUT — oracle.chain_vjp of the stages after k, evaluated at the stage's output — and the two local
partials written out below (STAGE_PARTIALS).  Inverse direction: the implicit rule on the same pieces (x = law⁻¹(y) from the
oracle's inverse chain).  The Float64 central-difference test through θ(x₂) is independent of both.

Tolerances: tests/_tol.py's flat 1e-3 (Float32) / 1e-6 (Float64).  Scales: values and cotangents per="sample" (the column's
max-norm of the reference); log-dets per="element" with a floor of 1 (|ref| + 1)."""
import ctypes as C
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _tol import flat_close  # noqa: E402

DT = {np.float32: torch.float32, np.float64: torch.float64}
OP_AFFINE = 32
KIND = {"exp": 1, "log": 2, "shift": 3, "scale": 4, "scale_inv": 5, "logit": 6, "logit_inv": 7, "leaky": 8, "flip": 11, "id": 12, "affine": OP_AFFINE,
        "truncated": 9}

# The parameter table.  A law is a list of stages in application order, a stage is (op, source of p0, source of p1);
# a source is "s" (host scalar), "r" (device (n1,) vector, broadcast over the columns) or "c" (device (n1, batch) array), None: no such parameter.
LAWS = {
    "id": [("id", None, None)],
    "exp": [("exp", None, None)],
    "log": [("log", None, None)],
    "flip": [("flip", None, None)],
    "shift_c": [("shift", "c", None)],
    "shift_r": [("shift", "r", None)],
    "scale_c": [("scale", "c", None)],
    "scale_s": [("scale", "s", None)],
    "scale_inv_c": [("scale_inv", "c", None)],
    "logit_cc": [("logit", "c", "c")],
    "logit_sr": [("logit", "s", "r")],
    "logit_inv_cc": [("logit_inv", "c", "c")],
    "logit_inv_ss": [("logit_inv", "s", "s")],
    "leaky_c": [("leaky", "c", None)],
    "leaky_s": [("leaky", "s", None)],
    "affine_cc": [("affine", "c", "c")],
    "affine_rc": [("affine", "r", "c")],
    # the five chains of the issue (a Scale directly followed by a Shift is one affine stage)
    "gated": [("logit", "s", "s"), ("affine", "c", "c"), ("logit_inv", "s", "s")],
    "exp_affine": [("affine", "c", "c"), ("exp", None, None)],
    "interval_affine": [("affine", "c", "c"), ("logit_inv", "s", "r")],
    "leaky_affine": [("affine", "c", "c"), ("leaky", "s", None)],
    "affine_leaky_affine": [("affine", "c", "c"), ("leaky", "c", None), ("affine", "c", "c")],
    # mixed sources, 4 stages
    "mixed4": [("shift", "r", None), ("scale", "c", None), ("leaky", "s", None), ("logit_inv", "c", "c")],
    "log4": [("log", None, None), ("scale_inv", "c", None), ("flip", None, None), ("exp", None, None)],
}
FIVE = ["gated", "exp_affine", "interval_affine", "leaky_affine", "affine_leaky_affine"]


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


def dev2(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------ parameters and inputs
def draw_param(rng, op, j, src, n1, N):
    """A value of parameter j of `op` from source `src`: float ("s"), (n1,) ("r") or (n1, N) ("c"), inside the op's domain."""
    shape = {"s": (), "r": (n1,), "c": (n1, N)}[src]
    if op == "shift" or (op == "affine" and j == 1):
        v = 0.5 * rng.normal(size=shape)
    elif op in ("scale", "scale_inv") or (op == "affine" and j == 0):
        v = rng.uniform(0.5, 1.5, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    elif op == "leaky":
        v = rng.uniform(0.05, 0.9, size=shape)
    elif op in ("logit", "logit_inv"):
        v = rng.uniform(-2.0, -1.0, size=shape) if j == 0 else rng.uniform(1.0, 3.0, size=shape)
    else:
        raise ValueError(op)
    return float(v) if src == "s" else v


def draw_law(rng, law, n1, N):
    """[(op, p0, p1)] with drawn parameter values (None where the op has none)."""
    return [(op, None if s0 is None else draw_param(rng, op, 0, s0, n1, N), None if s1 is None else draw_param(rng, op, 1, s1, n1, N)) for op, s0, s1 in law]


def full(p, n1, N):
    return np.broadcast_to(np.asarray(p, np.float64).reshape((-1, 1)) if np.ndim(p) == 1 else np.asarray(p, np.float64), (n1, N))


def draw_x1(rng, stages, n1, N):
    """x₁ inside the support of the law's first stage.  The ranges here and in draw_param keep a Logit⁻¹ output at least ~5e-4 of the
    interval away from its bounds: the inverse direction is compared with the ORACLE's logit((y-a)/(b-a)), which forms 1 - z from a
    rounded z and loses eps / (1 - z) itself (see test_support_edges_of_logit_and_log for the edges)."""
    op, p0, p1 = stages[0]
    if op == "log":
        return np.exp(rng.normal(size=(n1, N)))
    if op == "logit":
        a, b = full(p0, n1, N), full(p1, n1, N)
        return a + (b - a) * rng.uniform(0.1, 0.9, size=(n1, N))
    return rng.normal(size=(n1, N))


def col_param(p, c):
    return p if p is None or np.ndim(p) == 0 else (p if np.ndim(p) == 1 else p[:, c])


def oracle_ops(orc, stages, c, dt, inverse=False):
    """The oracle's op list of column c (per-row parameter vectors of that column); inverse: the inverted stages, last first."""
    out = []
    for op, p0, p1 in stages:
        a, b = col_param(p0, c), col_param(p1, c)
        a = a if a is None or np.ndim(a) == 0 else np.asarray(a, dt)
        b = b if b is None or np.ndim(b) == 0 else np.asarray(b, dt)
        if not inverse:
            # (identity: no oracle op — oracle.chain_vjp has none, and the fused chain passes an empty list through)
            out += [(orc.OP_SCALE, a, None), (orc.OP_SHIFT, b, None)] if op == "affine" else ([] if op == "id" else [(KIND[op], a, b)])
        else:
            inv = {"exp": lambda: [(orc.OP_LOG, None, None)], "log": lambda: [(orc.OP_EXP, None, None)], "flip": lambda: [(orc.OP_SIGNFLIP, None, None)], "id": lambda: [],
                   "shift": lambda: [(orc.OP_SHIFT, -a, None)], "scale": lambda: [(orc.OP_SCALE_INV, a, None)], "scale_inv": lambda: [(orc.OP_SCALE, a, None)],
                   "logit": lambda: [(orc.OP_LOGIT_INV, a, b)], "logit_inv": lambda: [(orc.OP_LOGIT, a, b)],
                   "leaky": lambda: [(orc.OP_LEAKY_RELU, 1.0 / a, None)],
                   "affine": lambda: [(orc.OP_SHIFT, -b, None), (orc.OP_SCALE_INV, a, None)]}[op]()
            out = inv + out
    return out


def ref_forward(orc, stages, idx1, x, dt, inverse=False):
    """Coupling forward / inverse by the oracle, column by column -> (y, per-column log-det)."""
    x = np.asarray(x, dt)
    y = x.copy()
    l = np.zeros(x.shape[1], np.float64)
    for c in range(x.shape[1]):
        yc, lc = orc.chain(oracle_ops(orc, stages, c, dt, inverse), np.asfortranarray(x[idx1, c:c + 1]), fused=True)
        y[idx1, c], l[c] = yc[:, 0], lc
    return y, l.astype(dt)


# ∂y/∂p and ∂ℓ/∂p of one stage at its input u, float64 (the stage's own closed forms: shift.jl:14, scale.jl:13-32, logit.jl:15-30, leaky_relu.jl:25-29)
def stage_partials(op, u, a, b):
    z = np.zeros_like(u)
    if op == "shift":
        return [(z + 1, z)]
    if op == "scale":
        return [(u, z + 1 / a)]
    if op == "scale_inv":
        return [(-u / a ** 2, z - 1 / a)]
    if op == "leaky":
        return [(np.where(u < 0, u, 0.0), np.where(u < 0, 1 / a, 0.0) + z)]
    if op == "affine":
        return [(u, z + 1 / a), (z + 1, z)]
    if op == "logit":
        return [(-1 / (u - a), 1 / (u - a) - 1 / (b - a)), (-1 / (b - u), 1 / (b - a) - 1 / (b - u))]
    if op == "logit_inv":
        sg = 1 / (1 + np.exp(-u))
        return [(1 - sg, z - 1 / (b - a)), (sg, z + 1 / (b - a))]
    return []


def ref_vjp(orc, stages, idx1, inp, gbar, lbar, inverse):
    """-> (in_bar, {(stage, j): (n1, N) cotangent of every parameter}) in float64, column by column."""
    inp, gbar = np.asarray(inp, np.float64), np.asarray(gbar, np.float64)
    n1, N = len(idx1), inp.shape[1]
    xb = gbar.copy()
    pb = {(k, j): np.zeros((n1, N)) for k, (op, p0, p1) in enumerate(stages) for j, p in enumerate((p0, p1)) if p is not None}
    for c in range(N):
        lb = 0.0 if lbar is None else float(lbar[c])
        g = gbar[idx1, c:c + 1]
        v = np.asfortranarray(inp[idx1, c:c + 1])
        if inverse:
            v = np.asfortranarray(orc.chain(oracle_ops(orc, stages, c, np.float64, True), v, fused=True)[0])
        fops = [oracle_ops(orc, [st], c, np.float64) for st in stages]                # per stage (affine: two oracle ops)
        flat = [o for f in fops for o in f]
        if inverse:
            A = orc.chain_vjp(flat, v, np.ones_like(g), 0.0)
            Bq = orc.chain_vjp(flat, v, np.zeros_like(g), 1.0)
            r = (g - lb * Bq) / A
            xb[idx1, c] = r[:, 0]
            g, lb = -r, -lb
        else:
            xb[idx1, c] = orc.chain_vjp(flat, v, g, lb)[:, 0]
        u = v
        for k, (op, p0, p1) in enumerate(stages):
            out = np.asfortranarray(orc.chain(fops[k], np.asfortranarray(u), fused=True)[0])
            rest = [o for f in fops[k + 1:] for o in f]
            gk = orc.chain_vjp(rest, out, g, lb) if rest else g
            a = None if p0 is None else np.asarray(col_param(p0, c), np.float64).reshape(-1, 1) * np.ones((n1, 1))
            b = None if p1 is None else np.asarray(col_param(p1, c), np.float64).reshape(-1, 1) * np.ones((n1, 1))
            for j, (ya, la) in enumerate(stage_partials(op, u, a, b)):
                pb[(k, j)][:, c] = (gk * ya + lb * la)[:, 0]
            u = out
    return xb, pb


# ------------------------------------------------------------------ the C entries through ctypes
class Call:
    """One marshalled law: device arrays for the "r" / "c" parameters, bjx_op list, params / ld_params."""

    def __init__(self, bj, stages, dt, n1, N, ld_extra=0):
        L = bj._lib
        n = len(stages)
        self.ops = (L.BjxOp * n)()
        self.params = (C.c_void_p * (2 * n))()
        self.lds = (C.c_int64 * (2 * n))()
        self.keep, self.src = [], {}
        for k, (op, p0, p1) in enumerate(stages):
            o = self.ops[k]
            o.kind, o.param_len, o.p0, o.p1, o.v0, o.v1 = KIND[op], 0, 0.0, 0.0, None, None
            for j, p in enumerate((p0, p1)):
                if p is None:
                    continue
                if np.ndim(p) == 0:
                    setattr(o, f"p{j}", float(p))
                    self.src[(k, j)] = "s"
                elif np.ndim(p) == 1:
                    t = dev1(p, dt)
                    self.keep.append(t)
                    self.params[2 * k + j], self.lds[2 * k + j] = t.data_ptr(), 0
                    self.src[(k, j)] = "r"
                else:
                    ld = n1 + ld_extra                                            # a strided slice: rows [0, n1) of a taller (ld, N) head
                    big = torch.full((N, ld), float("nan"), dtype=DT[dt], device="cuda")
                    big[:, :n1] = torch.from_numpy(np.ascontiguousarray(np.asarray(p, dt)[:, :N].T)).cuda()
                    self.keep.append(big)
                    self.params[2 * k + j], self.lds[2 * k + j] = big.data_ptr(), ld
                    self.src[(k, j)] = "c"
        self.n = n


def c_forward(bj, call, idx1, x, dt, inverse, want_ps=True, want_sum=True, flags=0, inplace=False, ps0=None, sum0=None):
    L, I = bj._lib, bj.interface
    xd = dev2(x, dt)
    dim, N = x.shape
    ctx = I.context(xd.device)
    i1 = torch.tensor(list(idx1), dtype=torch.int32, device="cuda")
    y = xd if inplace else torch.full((N, dim), float("nan"), dtype=DT[dt], device="cuda").T
    ps = (torch.zeros(N, dtype=DT[dt], device="cuda") if ps0 is None else dev1(ps0, dt)) if want_ps else None
    sm = torch.full((1,), 0.0 if sum0 is None else float(sum0), dtype=torch.float64, device="cuda") if want_sum else None
    rc = L.load().bjx_coupling_chain(ctx.h, I._dt(xd), int(inverse), I._ptr(i1), len(idx1), call.ops, call.n, call.params, call.lds, I._ptr(xd), I._ptr(y),
                                     I._ptr(ps), I._ptr(sm), dim, N, flags)
    L.check(ctx.h, rc, "bjx_coupling_chain")
    return host(y), None if ps is None else host(ps), None if sm is None else float(sm[0])


def c_vjp(bj, call, idx1, inp, gbar, lbar, dt, inverse, want=None, inplace=False):
    """-> (in_bar, {(k, j): cotangent}); want: the slots to request (default: every per-sample one)."""
    L, I = bj._lib, bj.interface
    xd, gd = dev2(inp, dt), dev2(gbar, dt)
    dim, N = inp.shape
    n1 = len(idx1)
    ctx = I.context(xd.device)
    i1 = torch.tensor(list(idx1), dtype=torch.int32, device="cuda")
    lb = None if lbar is None else dev1(lbar, dt)
    xb = gd if inplace else torch.full((N, dim), float("nan"), dtype=DT[dt], device="cuda").T
    bars = (C.c_void_p * (2 * call.n))()
    outs = {}
    for k, j in ([key for key, s in call.src.items() if s == "c"] if want is None else want):
        outs[(k, j)] = torch.full((N, n1), float("nan"), dtype=DT[dt], device="cuda").T
        bars[2 * k + j] = outs[(k, j)].data_ptr()
    rc = L.load().bjx_coupling_chain_vjp(ctx.h, I._dt(xd), int(inverse), I._ptr(i1), n1, call.ops, call.n, call.params, call.lds, I._ptr(xd), I._ptr(gd), I._ptr(lb),
                                         I._ptr(xb), bars, dim, N)
    L.check(ctx.h, rc, "bjx_coupling_chain_vjp")
    return host(xb), {key: host(t) for key, t in outs.items()}


def mask_rows(dim, n1, scattered, rng):
    return sorted(rng.choice(dim, size=n1, replace=False).tolist()) if scattered else list(range(n1))


def make_case(orc, name, dt, dim, n1, N, scattered, inverse):
    rng = np.random.default_rng(seed_of(name, dim, n1, N, scattered))
    stages = draw_law(rng, LAWS[name], n1, N)
    stages = [(op, p0 if p0 is None or np.ndim(p0) == 0 else np.asarray(p0, dt).astype(np.float64), p1 if p1 is None or np.ndim(p1) == 0 else np.asarray(p1, dt).astype(np.float64))
              for op, p0, p1 in stages]
    idx1 = mask_rows(dim, n1, scattered, rng)
    x = rng.normal(size=(dim, N))
    x[idx1] = draw_x1(rng, stages, n1, N)
    x = np.asarray(x, dt)
    if inverse:                                     # the inverse is fed the forward's output: inside its support by construction
        x = ref_forward(orc, stages, idx1, x, dt)[0]
    return stages, idx1, x


# ------------------------------------------------------------------ values and log-dets
SHAPES = [(2, 1, 1, False), (8, 4, 257, False), (64, 32, 257, False), (64, 32, 257, True), (13, 5, 100, True), (101, 50, 64, False), (300, 150, 33, False),
          (600, 300, 9, True), (7, 7, 40, False)]     # (dim, n1, batch, scattered mask)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", sorted(LAWS))
def test_every_op_and_chain_matches_oracle(bj, orc, name, inverse, dt):
    dim, n1, N, scattered = 64, 32, 257, name in ("mixed4", "leaky_c", "logit_cc")
    stages, idx1, x = make_case(orc, name, dt, dim, n1, N, scattered, inverse)
    call = Call(bj, stages, dt, n1, N)
    y, ps, sm = c_forward(bj, call, idx1, x, dt, inverse)
    y_ref, l_ref = ref_forward(orc, stages, idx1, x, dt, inverse)
    what = f"coupling_chain {name} inv={inverse}"
    flat_close(y, y_ref, dt, what + " values")
    flat_close(ps, l_ref, dt, what + " ladj", per="element", floor=1.0)
    flat_close(sm, float(l_ref.astype(np.float64).sum()), dt, what + " summed ladj", per="element", floor=float(np.abs(l_ref).sum()) + 1.0)
    rest = [r for r in range(dim) if r not in set(idx1)]
    assert np.array_equal(y[rest], x[rest]), "rows outside idx1 are copied through bit for bit"
    assert c_forward(bj, call, idx1, x, dt, inverse)[2] == sm, "two identical calls give identical summed log-det bits"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["affine_leaky_affine", "mixed4", "gated"])
def test_heights_masks_and_batches(bj, orc, name, shape, dt):
    dim, n1, N, scattered = shape
    for inverse in (False, True):
        stages, idx1, x = make_case(orc, name, dt, dim, n1, N, scattered, inverse)
        call = Call(bj, stages, dt, n1, N)
        y, ps, sm = c_forward(bj, call, idx1, x, dt, inverse)
        y_ref, l_ref = ref_forward(orc, stages, idx1, x, dt, inverse)
        what = f"coupling_chain {name} {shape} inv={inverse}"
        flat_close(y, y_ref, dt, what + " values")
        flat_close(ps, l_ref, dt, what + " ladj", per="element", floor=1.0)
        flat_close(sm, float(l_ref.astype(np.float64).sum()), dt, what + " summed ladj", per="element", floor=float(np.abs(l_ref).sum()) + 1.0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["exp_affine", "interval_affine"])
def test_large_batch(bj, orc, name, dt):
    dim, n1, N = 16, 8, 20011
    stages, idx1, x = make_case(orc, name, dt, dim, n1, N, False, False)
    call = Call(bj, stages, dt, n1, N)
    y, ps, sm = c_forward(bj, call, idx1, x, dt, False)
    y_ref, l_ref = ref_forward(orc, stages, idx1, x, dt)
    flat_close(y, y_ref, dt, f"coupling_chain {name} large batch values")
    flat_close(ps, l_ref, dt, f"coupling_chain {name} large batch ladj", per="element", floor=1.0)
    flat_close(sm, float(l_ref.astype(np.float64).sum()), dt, f"coupling_chain {name} large batch summed ladj", per="element", floor=float(np.abs(l_ref).sum()) + 1.0)
    xr, ps2, _ = c_forward(bj, call, idx1, y, dt, True)
    flat_close(xr, x, dt, f"coupling_chain {name} round trip")
    flat_close(ps + ps2, np.zeros(N), dt, f"coupling_chain {name} round-trip log-dets", per="element", floor=float(np.abs(ps).max()) + 1.0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", FIVE)
def test_round_trip(bj, orc, name, dt):
    dim, n1, N = 40, 20, 257
    stages, idx1, x = make_case(orc, name, dt, dim, n1, N, True, False)
    call = Call(bj, stages, dt, n1, N)
    y, ps, _ = c_forward(bj, call, idx1, x, dt, False)
    xr, ps2, _ = c_forward(bj, call, idx1, y, dt, True)
    # the forward's conditioning at the point: a rounding of y moves x by |dx/dy| · eps |y|
    flat_close(xr, x, dt, f"coupling_chain {name} round trip", floor=1.0)
    flat_close(ps + ps2, np.zeros(N), dt, f"coupling_chain {name} round-trip log-dets", per="element", floor=float(np.abs(ps).max()) + 1.0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("outs", ["ps", "sum", "both", "neither"])
def test_log_det_outputs_flags_and_edges(bj, orc, outs, dt):
    dim, n1, N = 24, 12, 130
    stages, idx1, x = make_case(orc, "affine_leaky_affine", dt, dim, n1, N, False, False)
    y_ref, l_ref = ref_forward(orc, stages, idx1, x, dt)
    call = Call(bj, stages, dt, n1, N, ld_extra=5)                                   # strided parameter slices via ld_params
    want_ps, want_sum = outs in ("ps", "both"), outs in ("sum", "both")
    y, ps, sm = c_forward(bj, call, idx1, x, dt, False, want_ps, want_sum)
    flat_close(y, y_ref, dt, f"coupling_chain outputs={outs} values")
    if want_ps:
        flat_close(ps, l_ref, dt, "coupling_chain ladj_ps", per="element", floor=1.0)
    if want_sum:
        flat_close(sm, float(l_ref.astype(np.float64).sum()), dt, "coupling_chain ladj_sum", per="element", floor=float(np.abs(l_ref).sum()) + 1.0)
    # BJX_ACCUMULATE adds into both
    ps0 = np.linspace(-1, 1, N)
    y2, psa, sma = c_forward(bj, call, idx1, x, dt, False, want_ps, want_sum, flags=bj._lib.BJX_ACCUMULATE, ps0=ps0, sum0=2.5)
    assert np.array_equal(y2, y)
    if want_ps:
        flat_close(psa, np.asarray(ps0, dt) + l_ref, dt, "coupling_chain accumulate ladj_ps", per="element", floor=1.0)
    if want_sum:
        flat_close(sma, 2.5 + float(l_ref.astype(np.float64).sum()), dt, "coupling_chain accumulate ladj_sum", per="element", floor=float(np.abs(l_ref).sum()) + 1.0)
    # in place
    y3, ps3, sm3 = c_forward(bj, call, idx1, x, dt, False, want_ps, want_sum, inplace=True)
    assert np.array_equal(y3, y) and (not want_sum or sm3 == sm)
    # an empty batch: nothing launched, the sum written as 0 (kept when accumulating)
    e = c_forward(bj, Call(bj, stages, dt, n1, 0), idx1, np.zeros((dim, 0), dt), dt, False, want_ps, want_sum, sum0=7.0)
    assert not want_sum or e[2] == 0.0
    e = c_forward(bj, Call(bj, stages, dt, n1, 0), idx1, np.zeros((dim, 0), dt), dt, False, want_ps, want_sum, flags=bj._lib.BJX_ACCUMULATE, sum0=7.0)
    assert not want_sum or e[2] == 7.0


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_support_edges_of_logit_and_log(bj, orc, dt):
    """On and next to the edges of the supports.  The reference has no clamp in Logit or log (logit.jl:15-30, exp_log.jl:8-9): ±Inf on
    a bound, NaN outside, and so has the oracle's chain; flat_close wants non-finite entries to agree exactly.  Next to the LOWER
    bound the points are one ulp and 16 eps inside.  Next to the UPPER bound the reference's own formula logit((x-a)/(b-a)) forms
    1 - z with z rounded (relative error eps / (1 - z) in the odds), so the point is 2^-8 inside: there the reference's error,
    eps · 2^8 · 3, is a tenth of the bar."""
    n1 = 8
    eps = np.finfo(dt).eps
    a, b = -1.0, 2.0
    edge = np.array([a, b, np.nextafter(dt(a), dt(3)), a + 16 * eps, b - 2.0 ** -8, 0.5, a - 0.5, b + 0.5], dt)
    x = np.tile(edge[:, None], (1, 3)).astype(dt)
    inside = [2, 3, 4, 5]
    for rows in (list(range(n1)), inside):
        for stages in ([("logit", a, b)], [("logit", a, np.full(len(rows), b))], [("logit", np.full((len(rows), 3), a), np.full((len(rows), 3), b))]):
            y, ps, _ = c_forward(bj, Call(bj, stages, dt, len(rows), 3), rows, x, dt, False)
            y_ref, l_ref = ref_forward(orc, stages, rows, x, dt)
            flat_close(y, y_ref, dt, "coupling_chain logit on and next to the edges of its support", per="element", floor=1.0)
            flat_close(ps, l_ref, dt, "coupling_chain logit on and next to the edges ladj", per="element", floor=1.0)
            assert np.isfinite(ps).all() == (rows == inside)
    xl = np.tile(np.array([0.0, np.finfo(dt).tiny, eps, 1.0, 3.0, -1.0, 1e30, 0.25], dt)[:, None], (1, 3))
    for rows in (list(range(n1)), [1, 2, 3, 4, 6, 7]):
        y, ps, _ = c_forward(bj, Call(bj, [("log", None, None)], dt, len(rows), 3), rows, xl, dt, False)
        y_ref, l_ref = ref_forward(orc, [("log", None, None)], rows, xl, dt)
        flat_close(y, y_ref, dt, "coupling_chain log on and next to the edge of its support", per="element", floor=1.0)
        flat_close(ps, l_ref, dt, "coupling_chain log on and next to the edge ladj", per="element", floor=1.0)


# ------------------------------------------------------------------ pullback
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("with_lbar", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", sorted(LAWS))
def test_pullback_matches_oracle_closed_forms(bj, orc, name, inverse, with_lbar, dt):
    dim, n1, N, scattered = 24, 12, 67, name in ("mixed4", "leaky_c", "logit_cc", "gated")
    stages, idx1, inp = make_case(orc, name, dt, dim, n1, N, scattered, inverse)
    rng = np.random.default_rng(seed_of(name, "bar"))
    gbar = rng.normal(size=(dim, N)).astype(dt)
    lbar = rng.normal(size=N).astype(dt) if with_lbar else None
    call = Call(bj, stages, dt, n1, N)
    xb, pb = c_vjp(bj, call, idx1, inp, gbar, lbar, dt, inverse)
    xb_ref, pb_ref = ref_vjp(orc, stages, idx1, inp, gbar, lbar, inverse)
    what = f"coupling_chain_vjp {name} inv={inverse} lbar={with_lbar}"
    flat_close(xb, xb_ref, dt, what + " in_bar")
    assert sorted(pb) == sorted(k for k, s in call.src.items() if s == "c")
    for key in pb:
        flat_close(pb[key], pb_ref[key], dt, what + f" params_bar{key}")
    # each params_bar NULL on its own: the others and in_bar keep their bits
    for drop in pb:
        xb2, pb2 = c_vjp(bj, call, idx1, inp, gbar, lbar, dt, inverse, want=[k for k in pb if k != drop])
        assert np.array_equal(xb2, xb, equal_nan=True) and all(np.array_equal(pb2[k], pb[k], equal_nan=True) for k in pb2) and drop not in pb2


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(2, 1, 1, False), (101, 50, 64, True), (300, 150, 33, False), (64, 32, 1030, False), (7, 3, 40, True)])
def test_pullback_heights_and_in_place(bj, orc, shape, dt):
    dim, n1, N, scattered = shape
    for inverse in (False, True):
        stages, idx1, inp = make_case(orc, "affine_leaky_affine", dt, dim, n1, N, scattered, inverse)
        rng = np.random.default_rng(seed_of(shape, "bar"))
        gbar, lbar = rng.normal(size=(dim, N)).astype(dt), rng.normal(size=N).astype(dt)
        call = Call(bj, stages, dt, n1, N, ld_extra=3)
        xb, pb = c_vjp(bj, call, idx1, inp, gbar, lbar, dt, inverse)
        xb_ref, pb_ref = ref_vjp(orc, stages, idx1, inp, gbar, lbar, inverse)
        flat_close(xb, xb_ref, dt, f"coupling_chain_vjp {shape} inv={inverse} in_bar")
        for key in pb:
            flat_close(pb[key], pb_ref[key], dt, f"coupling_chain_vjp {shape} inv={inverse} params_bar{key}")
        xb2, pb2 = c_vjp(bj, call, idx1, inp, gbar, lbar, dt, inverse, inplace=True)                 # in_bar == out_bar
        assert np.array_equal(xb2, xb) and all(np.array_equal(pb2[k], pb[k]) for k in pb)


def test_cotangent_of_a_scalar_or_per_row_parameter_is_refused(bj, orc):
    dt, n1, N = np.float64, 4, 6
    stages, idx1, inp = make_case(orc, "mixed4", dt, 8, n1, N, False, False)
    call = Call(bj, stages, dt, n1, N)
    g = np.ones((8, N))
    for slot in [(0, 0), (2, 0), (0, 1)]:            # per-row, scalar, and a parameter the stage does not have
        with pytest.raises(ValueError, match="params_bar"):
            c_vjp(bj, call, idx1, inp, g, None, dt, False, want=[slot])
    with pytest.raises(NotImplementedError):        # TruncatedBijector's branches are not served
        c_forward(bj, Call(bj, [("truncated", 0.0, 1.0)], dt, n1, N), idx1, inp, dt, False)
    with pytest.raises(NotImplementedError):
        c_forward(bj, Call(bj, [("exp", None, None)] * 5, dt, n1, N), idx1, inp, dt, False)


# ------------------------------------------------------------------ agreement with the affine entries
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("inverse", [False, True])
def test_affine_law_agrees_with_the_affine_entries(bj, orc, inverse, dt):
    L, I = bj._lib, bj.interface
    dim, n1, N = 64, 32, 513
    stages, idx1, x = make_case(orc, "affine_cc", dt, dim, n1, N, False, False)
    rng = np.random.default_rng(3)
    gbar, lbar = rng.normal(size=(dim, N)).astype(dt), rng.normal(size=N).astype(dt)
    call = Call(bj, stages, dt, n1, N)
    y, ps, sm = c_forward(bj, call, idx1, x, dt, inverse)
    xb, pb = c_vjp(bj, call, idx1, x, gbar, lbar, dt, inverse)
    xd, gd, lb, s, t = dev2(x, dt), dev2(gbar, dt), dev1(lbar, dt), dev2(stages[0][1], dt), dev2(stages[0][2], dt)
    i1 = torch.tensor(idx1, dtype=torch.int32, device="cuda")
    ctx = I.context(xd.device)
    y0, ps0, sm0 = torch.empty_like(xd), torch.empty(N, dtype=DT[dt], device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    L.check(ctx.h, L.load().bjx_coupling_affine(ctx.h, I._dt(xd), int(inverse), I._ptr(i1), n1, I._ptr(s), I._ptr(t), I._ptr(xd), I._ptr(y0), I._ptr(ps0), I._ptr(sm0), dim, N, 0), "affine")
    xb0, sb0, tb0 = torch.empty_like(xd), torch.empty_like(s), torch.empty_like(t)
    L.check(ctx.h, L.load().bjx_coupling_affine_vjp(ctx.h, I._dt(xd), int(inverse), I._ptr(i1), n1, I._ptr(s), I._ptr(t), I._ptr(xd), I._ptr(gd), I._ptr(lb), I._ptr(xb0),
                                                    I._ptr(sb0), I._ptr(tb0), dim, N), "affine_vjp")
    what = f"coupling_chain vs coupling_affine inv={inverse}"
    flat_close(y, host(y0), dt, what + " y")
    flat_close(ps, host(ps0), dt, what + " ladj", per="element", floor=1.0)
    flat_close(sm, float(sm0[0]), dt, what + " summed ladj", per="element", floor=float(np.abs(host(ps0)).sum()) + 1.0)
    flat_close(xb, host(xb0), dt, what + " x_bar")
    flat_close(pb[(0, 0)], host(sb0), dt, what + " s_bar")
    flat_close(pb[(0, 1)], host(tb0), dt, what + " t_bar")


# ------------------------------------------------------------------ the Python Coupling
def build_law(bj, name, tensors):
    """The law `name` of FIVE as the user writes it (outer @ inner), from device tensors s, t (s2, t2, alpha)."""
    el = bj.elementwise
    s, t = tensors["s"], tensors["t"]
    aff = bj.Shift(t) @ bj.Scale(s, batched=True)
    if name == "gated":
        return bj.inverse(bj.Logit(0.0, 1.0)) @ aff @ bj.Logit(0.0, 1.0)
    if name == "exp_affine":
        return el(bj.exp) @ aff
    if name == "interval_affine":
        return bj.inverse(bj.Logit(-1.0, 2.0)) @ aff
    if name == "leaky_affine":
        return bj.LeakyReLU(0.2) @ aff
    if name == "affine_leaky_affine":
        return bj.Shift(tensors["t2"]) @ bj.Scale(tensors["s2"], batched=True) @ bj.LeakyReLU(0.3) @ aff
    raise ValueError(name)


def law_stages(name, p):
    """The same law as a stage list for the oracle (numpy parameters)."""
    aff = ("affine", p["s"], p["t"])
    return {"gated": [("logit", 0.0, 1.0), aff, ("logit_inv", 0.0, 1.0)], "exp_affine": [aff, ("exp", None, None)],
            "interval_affine": [aff, ("logit_inv", -1.0, 2.0)], "leaky_affine": [aff, ("leaky", 0.2, None)],
            "affine_leaky_affine": [aff, ("leaky", 0.3, None)] + ([("affine", p["s2"], p["t2"])] if "s2" in p else [])}[name]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", FIVE)
def test_coupling_with_a_chain_law(bj, orc, name, inverse, dt):
    dim, n1, N = 10, 5, 130
    rng = np.random.default_rng(seed_of(name, "py"))
    p = {k: np.asarray(draw_param(rng, "affine", j, "c", n1, N), dt).astype(np.float64) for k, j in (("s", 0), ("t", 1), ("s2", 0), ("t2", 1))}
    stages = law_stages(name, p)
    idx1 = list(range(n1))
    x = rng.normal(size=(dim, N))
    x[idx1] = draw_x1(rng, stages, n1, N)
    x = np.asarray(x, dt)
    if inverse:
        x = ref_forward(orc, stages, idx1, x, dt)[0]
    tens = {k: dev2(v, dt) for k, v in p.items()}
    cpl = bj.Coupling(lambda x2: build_law(bj, name, tens), bj.PartitionMask(dim, [i + 1 for i in idx1]))
    b = bj.inverse(cpl) if inverse else cpl
    y, l = bj.with_logabsdet_jacobian(b, dev2(x, dt), per_sample=True)
    y_ref, l_ref = ref_forward(orc, stages, idx1, x, dt, inverse)
    flat_close(host(y), y_ref, dt, f"Coupling {name} inv={inverse} values")
    flat_close(host(l), l_ref, dt, f"Coupling {name} inv={inverse} ladj", per="element", floor=1.0)
    # pullback and the law's per-column cotangents through vjp_params
    gbar, lbar = rng.normal(size=(dim, N)).astype(dt), rng.normal(size=N).astype(dt)
    xb, grads = bj.vjp_params(b, dev2(x, dt), dev2(gbar, dt), dev1(lbar, dt))
    xb_ref, pb_ref = ref_vjp(orc, stages, idx1, x, gbar, lbar, inverse)
    flat_close(host(xb), xb_ref, dt, f"Coupling {name} inv={inverse} x_bar")
    assert torch.equal(bj.vjp(b, dev2(x, dt), dev2(gbar, dt), dev1(lbar, dt)), xb)
    k_aff = [k for k, st in enumerate(stages) if st[0] == "affine"]
    user_stage = {"gated": [1], "exp_affine": [0], "interval_affine": [0], "leaky_affine": [0], "affine_leaky_affine": [0, 3]}[name]
    for k, us in zip(k_aff, user_stage):             # user stages: Scale at us, Shift at us + 1
        flat_close(host(grads["params"][us]["a"]), pb_ref[(k, 0)], dt, f"Coupling {name} inv={inverse} scale_bar")
        flat_close(host(grads["params"][us + 1]["a"]), pb_ref[(k, 1)], dt, f"Coupling {name} inv={inverse} shift_bar")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", FIVE)
def test_pullback_through_theta_against_central_differences(bj, orc, name, inverse):
    """Float64: x̄ of vjp(Coupling) with θ(x₂) = a fixed linear map, against central differences of the ORACLE's forward."""
    dt, dim, n1, N = np.float64, 6, 3, 4
    rng = np.random.default_rng(seed_of(name, "fd"))
    Ws, Wt = rng.normal(size=(n1, dim - n1)) * 0.2, rng.normal(size=(n1, dim - n1)) * 0.3
    bs = rng.uniform(1.0, 1.5, size=(n1, 1))
    idx1, idx2 = list(range(n1)), list(range(n1, dim))

    def theta_np(x2):
        return {"s": Ws @ x2 + bs, "t": Wt @ x2, "s2": 1.2 + 0.1 * (Wt @ x2), "t2": Ws @ x2}

    def theta(x2):
        W1, W2, b1 = (torch.from_numpy(a).cuda() for a in (Ws, Wt, bs))
        return build_law(bj, name, {"s": W1 @ x2 + b1, "t": W2 @ x2, "s2": 1.2 + 0.1 * (W2 @ x2), "t2": W1 @ x2})

    x = rng.normal(size=(dim, N)) * 0.5
    if name == "gated":
        x[idx1] = rng.uniform(0.2, 0.8, size=(n1, N))
    gbar, lbar = rng.normal(size=(dim, N)), rng.normal(size=N)

    def fwd(xx):
        return ref_forward(orc, law_stages(name, theta_np(xx[idx2])), idx1, xx, dt, inverse)

    if inverse:
        x = fwd_y = ref_forward(orc, law_stages(name, theta_np(x[idx2])), idx1, x, dt, False)[0]

    def loss(xx):
        y, l = fwd(xx)
        return float((gbar * y).sum() + (lbar * l).sum())

    cpl = bj.Coupling(theta, bj.PartitionMask(dim, [i + 1 for i in idx1]))
    b = bj.inverse(cpl) if inverse else cpl
    xb = host(bj.vjp(b, dev2(x, dt), dev2(gbar, dt), dev1(lbar, dt)))
    fd = np.zeros_like(x)
    h = 1e-6
    for i in range(dim):
        for c in range(N):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h
            xm[i, c] -= h
            fd[i, c] = (loss(xp) - loss(xm)) / (2 * h)
    # central differences with h = 1e-6 carry O(h²) truncation and eps/h ≈ 2e-10 rounding: inside the 1e-6 bar
    flat_close(xb, fd, dt, f"Coupling {name} inv={inverse} x_bar vs central differences")


def test_affine_dispatch_is_unchanged(bj, orc):
    """Shift ∘ Scale through the Python Coupling still takes bjx_coupling_affine: the same launches as a direct call of that entry
    and bit-identical outputs."""
    L, I = bj._lib, bj.interface
    dt, dim, n1, N = np.float32, 64, 32, 1000
    rng = np.random.default_rng(1)
    s, t, x = dev2(rng.uniform(0.5, 2, size=(n1, N)), dt), dev2(rng.normal(size=(n1, N)), dt), dev2(rng.normal(size=(dim, N)), dt)
    cpl = bj.Coupling(lambda x2: bj.Shift(t) @ bj.Scale(s, batched=True), dim)
    bj.with_logabsdet_jacobian(cpl, x, per_sample=True)
    n0 = L.load().bjx_launch_count()
    y, l = bj.with_logabsdet_jacobian(cpl, x, per_sample=True)
    d_py = L.load().bjx_launch_count() - n0
    ctx = I.context(x.device)
    i1 = torch.arange(n1, dtype=torch.int32, device="cuda")
    y0, l0 = torch.empty_like(x), torch.empty(N, dtype=torch.float32, device="cuda")
    n0 = L.load().bjx_launch_count()
    L.check(ctx.h, L.load().bjx_coupling_affine(ctx.h, I._dt(x), 0, I._ptr(i1), n1, I._ptr(s), I._ptr(t), I._ptr(x), I._ptr(y0), I._ptr(l0), None, dim, N, 0), "affine")
    d_c = L.load().bjx_launch_count() - n0
    assert d_py == d_c, (d_py, d_c)
    assert torch.equal(y, y0) and torch.equal(l, l0)
    for law in (lambda x2: bj.Scale(s, batched=True), lambda x2: bj.Shift(t)):
        n0 = L.load().bjx_launch_count()
        bj.with_logabsdet_jacobian(bj.Coupling(law, dim), x, per_sample=True)
        assert L.load().bjx_launch_count() - n0 == d_c


def test_training_weight_gradients_match_autograd(bj, orc):
    """vjp_params(Coupling) with θ an nn.Module: the weight gradients against torch.autograd through a plain-PyTorch evaluation of
    the same law, Float64."""
    dim, n1, N = 8, 4, 50
    torch.manual_seed(0)

    class Theta(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(dim - n1, 2 * n1, dtype=torch.float64)

        def heads(self, x2):
            h = self.lin(x2.T).T                                     # (2 n1, N)
            return torch.exp(0.3 * h[:n1]) + 0.5, h[n1:]

        def forward(self, x2):
            s, t = self.heads(x2)
            return bj.LeakyReLU(0.2) @ bj.Shift(t) @ bj.Scale(s, batched=True)

    th = Theta().cuda()
    cpl = bj.Coupling(th, dim)
    rng = np.random.default_rng(9)
    x, gbar, lbar = dev2(rng.normal(size=(dim, N)), np.float64), dev2(rng.normal(size=(dim, N)), np.float64), dev1(rng.normal(size=N), np.float64)
    xb, grads = bj.vjp_params(cpl, x, gbar, lbar)
    xt = x.clone().requires_grad_(True)
    s, t = th.heads(xt[n1:])
    v = t + s * xt[:n1]
    y1 = torch.where(v < 0, 0.2 * v, v)
    ladj = torch.log(s.abs()).sum(0) + torch.where(v < 0, torch.full_like(v, float(np.log(0.2))), torch.zeros_like(v)).sum(0)
    loss = (gbar[:n1] * y1).sum() + (gbar[n1:] * xt[n1:]).sum() + (lbar * ladj).sum()
    named = list(th.named_parameters())
    gs = torch.autograd.grad(loss, [xt] + [p for _, p in named])
    flat_close(host(xb), host(gs[0]), np.float64, "Coupling training x_bar vs autograd")
    for (k, _), g in zip(named, gs[1:]):
        flat_close(host(grads["theta"][k]), host(g), np.float64, f"Coupling training grad {k} vs autograd", per="tensor")


def test_chain_law_inside_a_composition_and_logpdf(bj, orc):
    """Coupling(chain law) ∘ Permute ∘ Coupling(chain law) through the piecewise planner, and the logpdf of a transformed(...) built on it."""
    dt, dim, n1, N = np.float64, 8, 4, 60
    rng = np.random.default_rng(21)
    idx1 = list(range(n1))
    ps_ = [{k: np.asarray(draw_param(rng, "affine", j, "c", n1, N), dt) for k, j in (("s", 0), ("t", 1))} for _ in range(2)]
    tens = [{k: dev2(v, dt) for k, v in p.items()} for p in ps_]
    cpl1 = bj.Coupling(lambda x2: build_law(bj, "leaky_affine", tens[0]), dim)
    cpl2 = bj.Coupling(lambda x2: build_law(bj, "exp_affine", tens[1]), dim)
    b = cpl2 @ bj.Permute(list(range(dim, 0, -1))) @ cpl1
    x = rng.normal(size=(dim, N))
    y1, l1 = ref_forward(orc, law_stages("leaky_affine", ps_[0]), idx1, x, dt)
    y2, l2 = ref_forward(orc, law_stages("exp_affine", ps_[1]), idx1, np.ascontiguousarray(y1[::-1]), dt)
    y, l = bj.with_logabsdet_jacobian(b, dev2(x, dt), per_sample=True)
    flat_close(host(y), y2, dt, "Coupling ∘ Permute ∘ Coupling (chain laws) values")
    flat_close(host(l), l1 + l2, dt, "Coupling ∘ Permute ∘ Coupling (chain laws) ladj", per="element", floor=1.0)
    lp = bj.logpdf(bj.transformed(bj.MvNormal(dim), b), dev2(y2, dt))
    ref = -0.5 * (x ** 2).sum(0) - 0.5 * dim * np.log(2 * np.pi) - (l1 + l2)
    flat_close(host(lp).reshape(-1), ref, dt, "logpdf(transformed(MvNormal, Coupling ∘ Permute ∘ Coupling))", per="element", floor=1.0)


def test_rejections(bj, orc):
    dim, n1, N = 8, 4, 6
    x = dev2(np.random.default_rng(0).normal(size=(dim, N)), np.float64)
    s = dev2(np.full((n1, N), 1.5), np.float64)
    el = bj.elementwise
    five = el(bj.exp) @ bj.LeakyReLU(0.5) @ bj.Scale(s, batched=True) @ bj.LeakyReLU(0.3) @ bj.Shift(s)          # 5 stages, nothing to fold
    with pytest.raises(NotImplementedError, match="supported"):
        bj.with_logabsdet_jacobian(bj.Coupling(lambda x2: five, dim), x)
    with pytest.raises(NotImplementedError, match="supported"):
        bj.with_logabsdet_jacobian(bj.Coupling(lambda x2: bj.OrderedBijector(), dim), x)
    with pytest.raises(NotImplementedError, match="supported"):
        bj.vjp(bj.Coupling(lambda x2: bj.OrderedBijector(), dim), x, x)
    for bad in (dev2(np.ones((n1 + 1, N)), np.float64), dev2(np.ones((n1, N + 1)), np.float64), dev1(np.ones(n1 + 2), np.float64)):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            bj.with_logabsdet_jacobian(bj.Coupling(lambda x2: el(bj.exp) @ bj.Scale(bad, batched=True), dim), x)
    w = torch.ones(n1, dtype=torch.float64, device="cuda", requires_grad=True)                                   # a per-row parameter that wants a cotangent
    with pytest.raises(NotImplementedError, match="sum over the batch"):
        bj.vjp(bj.Coupling(lambda x2: el(bj.exp) @ bj.Scale(w), dim), x, x)
