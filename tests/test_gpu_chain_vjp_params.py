"""One-pass parameter pullback of an elementwise chain with batch-shared parameters (include/bjx_chain_vjp.h:
bjx_chain_vjp_params, bjx_plan_chain_vjp_params / bjx_plan_run_vjp_params) and `vjp_params` on top of it, against the CPU oracle
as it stands, in Float64.

Reference (a), closed forms: stage k's parameter p enters through that stage alone, so p̄ = Σ_n g_k ∂y_k/∂p + ℓ̄_n ∂ℓ_k/∂p with g_k the
cotangent of the stage's OUTPUT — oracle.chain_vjp of the stages after k, evaluated at the stage's output (oracle.chain) — and the
two local partials restated in numpy (stage_partials, the construction of tests/test_gpu_coupling_chain.py); the summands are
summed over the batch (and over the rows for a scalar parameter) in Float64.
Reference (b), independent of (a): Float64 central differences of Σ ȳ·y(θ) + Σ ℓ̄·ladj(θ) through oracle.chain.

Bar: tests/_tol.py's flat 1e-3 (Float32) / 1e-6 (Float64); parameter cotangents per="tensor" with term_scale = max |summand|
(a sum of N terms of either sign rounds relative to its largest term), x̄ per="sample".  Inputs and parameters are rounded to the
dtype under test first and the reference is evaluated at those rounded values.  Draws keep the reference tame: Logit inputs at
least 5 % of the width inside (a, b), Log inputs in [0.2, 5], |scale| in [0.3, 3], LeakyReLU inputs of both signs, α in [0.05, 0.9]
(tests/test_chain_vjp_params_draws.py checks on the CPU that with these draws the closed forms with every stage input taken from
the Float32 oracle hold the Float32 bar against the Float64 ones)."""
import ctypes as C
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from _tol import flat_close  # noqa: E402

DT = {np.float32: torch.float32, np.float64: torch.float64}
KIND = {"exp": 1, "log": 2, "shift": 3, "scale": 4, "scale_inv": 5, "logit": 6, "logit_inv": 7, "leaky": 8, "truncated": 9, "flip": 11, "id": 12, "logpdf": 13}
NPAR = {"exp": 0, "log": 0, "flip": 0, "shift": 1, "scale": 1, "scale_inv": 1, "leaky": 1, "logit": 2, "logit_inv": 2}

# laws in APPLICATION order
LAWS = {
    "shift": ["shift"],
    "scale": ["scale"],
    "scale_inv": ["scale_inv"],
    "logit": ["logit"],
    "logit_inv": ["logit_inv"],
    "leaky": ["leaky"],
    "exp_affine": ["scale", "shift", "exp"],                      # exp ∘ Shift ∘ Scale (the mean-field chain)
    "interval_affine": ["scale", "shift", "logit_inv"],           # inverse(Logit) ∘ Shift ∘ Scale
    "leaky_affine": ["scale", "shift", "leaky"],                  # LeakyReLU ∘ Shift ∘ Scale
    "affine_leaky_affine4": ["scale", "shift", "leaky", "scale"],  # Shift ∘ Scale ∘ LeakyReLU ∘ Shift ∘ Scale cut at the fused limit
    "logit_scale_inv": ["scale_inv", "logit"],                    # Logit ∘ inverse(Scale)
    "log_flip": ["log", "scale", "flip", "shift"],
    "affine": ["scale", "shift"],                                 # Shift ∘ Scale: two one-parameter stages (the pack layout on whole packs)
    "shift_scale": ["shift", "scale"],                            # Scale ∘ Shift
}


@pytest.fixture(scope="module")
def bj():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd

    return bijectors_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


def dev2(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).T)).cuda().T


def dev1(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).reshape(-1))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------ draws
def draw_param(rng, op, j, src, dim, dt):
    """Parameter j of `op`, rounded to dt: a float (src "s" host scalar, "d" device scalar) or a (dim,) float64 array ("r")."""
    shape = (dim,) if src == "r" else ()
    if op == "shift":
        v = 0.5 * rng.normal(size=shape)
    elif op in ("scale", "scale_inv"):
        v = rng.uniform(0.3, 3.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    elif op == "leaky":
        v = rng.uniform(0.05, 0.9, size=shape)
    else:                                   # logit / logit_inv: a in [-2, -1], b in [1, 3]
        v = rng.uniform(-2.0, -1.0, size=shape) if j == 0 else rng.uniform(1.0, 3.0, size=shape)
    v = np.asarray(v, dt).astype(np.float64)
    return float(v) if src != "r" else v


def draw_case(law, src, dim, N, dt, lbar=True, tag=0):
    """-> (stages [(op, p0, p1)], X, ybar, lbar | None), float64 arrays holding dt-rounded values."""
    rng = np.random.default_rng(seed_of(law, src, dim, N, np.dtype(dt).name, tag))
    stages = [(op, draw_param(rng, op, 0, src, dim, dt) if NPAR[op] >= 1 else None, draw_param(rng, op, 1, src, dim, dt) if NPAR[op] >= 2 else None)
              for op in LAWS[law]]
    col = lambda p: np.asarray(p, np.float64).reshape(-1, 1) * np.ones((dim, 1))
    first = stages[0][0]
    if first == "log":
        X = rng.uniform(0.2, 5.0, size=(dim, N))
    elif first == "logit":
        a, b = col(stages[0][1]), col(stages[0][2])
        X = a + (b - a) * rng.uniform(0.05, 0.95, size=(dim, N))
    elif law == "logit_scale_inv":          # x / s inside (a, b) with the 5 % margin
        a, b = col(stages[1][1]), col(stages[1][2])
        X = col(stages[0][1]) * (a + (b - a) * rng.uniform(0.06, 0.94, size=(dim, N)))
    else:
        X = rng.normal(size=(dim, N))
    X = np.asfortranarray(np.asarray(X, dt).astype(np.float64))
    G = np.asfortranarray(np.asarray(rng.normal(size=(dim, N)), dt).astype(np.float64))
    lb = np.asarray(rng.normal(size=N), dt).astype(np.float64) if lbar else None
    return stages, X, G, lb


# ------------------------------------------------------------------ reference (a)
def stage_partials(op, u, a, b):
    """[(∂y/∂p_j, ∂ℓ/∂p_j)] of one stage at its input u (shift.jl:14, scale.jl:13-32, logit.jl:15-30, leaky_relu.jl:25-29)"""
    z = np.zeros_like(u)
    if op == "shift":
        return [(z + 1, z)]
    if op == "scale":
        return [(u, z + 1 / a)]
    if op == "scale_inv":
        return [(-u / a ** 2, z - 1 / a)]
    if op == "leaky":
        return [(np.where(u < 0, u, 0.0), np.where(u < 0, 1 / a, 0.0) + z)]
    if op == "logit":
        return [(-1 / (u - a), 1 / (u - a) - 1 / (b - a)), (-1 / (b - u), 1 / (b - a) - 1 / (b - u))]
    if op == "logit_inv":
        sg = 1 / (1 + np.exp(-u))
        return [(1 - sg, z - 1 / (b - a)), (sg, z + 1 / (b - a))]
    return []


def ref_closed(orc, stages, X, G, lb, fwd_dtype=np.float64):
    """-> (x̄, {slot: (cotangent: (dim,) per-row | float scalar, max |summand|)}).  fwd_dtype: the oracle arithmetic of the stage
    inputs (Float32 for the self-check of the draws; the sums are always Float64)."""
    dim, N = X.shape
    ops = [(KIND[op], p0, p1) for op, p0, p1 in stages]
    lbv = np.zeros(N) if lb is None else lb
    xb = orc.chain_vjp(ops, X, G, lbv)
    out = {}
    u = X
    for k, (op, p0, p1) in enumerate(stages):
        yk = np.asarray(orc.chain([ops[k]], np.asfortranarray(u.astype(fwd_dtype)), fused=True)[0], np.float64)
        gk = orc.chain_vjp(ops[k + 1:], yk, G, lbv) if k + 1 < len(ops) else G
        col = lambda p: None if p is None else np.asarray(p, np.float64).reshape(-1, 1) * np.ones((dim, 1))
        uu = u.astype(fwd_dtype).astype(np.float64)
        for j, (ya, la) in enumerate(stage_partials(op, uu, col(p0), col(p1))):
            s = gk * ya + lbv[None, :] * la
            p = (p0, p1)[j]
            out[2 * k + j] = (s.sum(axis=1) if np.ndim(p) else float(s.sum()), float(np.abs(s).max()) if s.size else 0.0)
        u = yk
    return xb, out


# ------------------------------------------------------------------ the C entries through ctypes
class Call:
    """One marshalled chain: bjx_op list with host scalars ("s"), device scalars ("d") or per-row device vectors ("r")."""

    def __init__(self, bj, stages, src, dt, dim):
        L = bj._lib
        self.L, self.dt, self.dim, self.n = L, dt, dim, len(stages)
        self.ops = (L.BjxOp * self.n)()
        self.dev = {}                       # slot -> device tensor of the parameter
        self.len = {}                       # slot -> length of its cotangent
        for k, (op, p0, p1) in enumerate(stages):
            o = self.ops[k]
            o.kind, o.param_len, o.p0, o.p1, o.v0, o.v1 = KIND[op], 0, 0.0, 0.0, None, None
            for j, p in enumerate((p0, p1)):
                if p is None:
                    continue
                if np.ndim(p):
                    t = dev1(p, dt)
                    o.param_len = dim
                elif src == "d":
                    t = dev1([p], dt)
                    o.param_len = max(o.param_len, 1)
                else:
                    t = None
                    o.param_len = max(o.param_len, 1)
                    setattr(o, f"p{j}", float(p))
                if t is not None:
                    self.dev[2 * k + j] = t
                    setattr(o, f"v{j}", t.data_ptr())
                self.len[2 * k + j] = dim if np.ndim(p) else 1

    def bars(self, want=None):
        want = sorted(self.len) if want is None else want
        out = {i: torch.full((self.len[i],), float("nan"), dtype=DT[self.dt], device="cuda") for i in want}
        pb = (C.c_void_p * (2 * self.n))()
        for i, t in out.items():
            pb[i] = t.data_ptr()
        return out, pb

    def run(self, bj, X, G, lb, want=None, xbar=True, alias=False, plan=None):
        """-> (rc, x̄ tensor | None, {slot: tensor}); X, G: device (dim, N), lb: device (N,) | None"""
        lib = self.L.load()
        ctx = bj.interface.context(X.device)
        N = X.shape[1]
        out, pb = self.bars(want)
        xb = G if alias else (torch.full((N, self.dim), float("nan"), dtype=X.dtype, device="cuda").T if xbar else None)
        args = (X.data_ptr(), G.data_ptr(), None if lb is None else lb.data_ptr(), None if xb is None else xb.data_ptr(), pb)
        if plan is None:
            rc = lib.bjx_chain_vjp_params(ctx.h, 0 if self.dt == np.float32 else 1, self.ops, self.n, *args, self.dim, N)
        else:
            rc = lib.bjx_plan_run_vjp_params(plan, *args, N)
        return rc, xb, out

    def plan(self, bj, want=None):
        lib = self.L.load()
        ctx = bj.interface.context(torch.device("cuda", torch.cuda.current_device()))
        mask = 0
        for i in (sorted(self.len) if want is None else want):
            mask |= 1 << i
        h = C.c_void_p()
        rc = lib.bjx_plan_chain_vjp_params(ctx.h, 0 if self.dt == np.float32 else 1, self.ops, self.n, mask, self.dim, C.byref(h))
        assert rc == 0, rc
        return h


def check_against_closed(bj, orc, law, src, dim, N, dt, lbar, want=None, xbar=True, alias=False, tag=0):
    stages, X, G, lb = draw_case(law, src, dim, N, dt, lbar, tag)
    call = Call(bj, stages, src, dt, dim)
    Xd, Gd = dev2(X, dt), dev2(G, dt)
    lbd = None if lb is None else dev1(lb, dt)
    rc, xb, out = call.run(bj, Xd, Gd, lbd, want=want, xbar=xbar, alias=alias)
    assert rc == 0, (rc, call.L.load().bjx_last_error(bj.interface.context(Xd.device).h))
    what = f"chain_vjp_params {law} src={src} {dim}x{N} lbar={lbar}"
    if N == 0:
        for i, t in out.items():
            assert (host(t) == 0).all(), (what, i)
        return
    ref_xb, ref = ref_closed(orc, stages, X, G, lb)
    if xb is not None:
        flat_close(host(xb), ref_xb, dt, what + " x̄", per="sample")
    assert set(out) == (set(ref) if want is None else set(want))
    for i, t in out.items():
        r, ts = ref[i]
        flat_close(host(t), np.asarray(r, np.float64).reshape(-1), dt, what + f" slot {i}", per="tensor", term_scale=ts)


# ------------------------------------------------------------------ closed forms: every kind, every source
@pytest.mark.parametrize("lbar", [True, False])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("src", ["s", "d", "r"])
@pytest.mark.parametrize("law", sorted(LAWS))
def test_every_kind_and_source(bj, orc, law, src, dt, lbar):
    """Every parameterised kind alone and the chains of the README, host-scalar / device-scalar / per-row parameters, with and
    without ℓ̄, on whole packs (64 x 257: more than one block) and on an odd height (5 x 63: a partial wave)."""
    check_against_closed(bj, orc, law, src, 64, 257, dt, lbar)
    check_against_closed(bj, orc, law, src, 5, 63, dt, lbar)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("N", [0, 1, 63, 65, 1000, 4099])
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 64, 67, 260])
@pytest.mark.parametrize("law,src", [("leaky_affine", "r"), ("logit_scale_inv", "r"), ("affine", "r"), ("scale", "s")])
def test_shapes(bj, orc, law, src, dim, N, dt):
    """Below a pack, whole packs, an odd tail, more packs than the pack layout holds; an empty batch (zeros), a partial wave, more
    than one block (the fold runs), a ragged last block.  Shift ∘ Scale with per-row parameters and a one-stage chain with a scalar
    parameter (summed over the rows) take the pack layout on whole aligned packs (dim 4, 64; 260 only in Float64 is too tall) and one
    row per lane elsewhere; the three-stage chain and Logit ∘ inverse(Scale) take one row per lane at every height."""
    check_against_closed(bj, orc, law, src, dim, N, dt, True)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("N", [65, 1000, 4099])
@pytest.mark.parametrize("law,src", [("affine", "r"), ("shift_scale", "r"), ("leaky", "r"), ("logit", "r")])
def test_sixty_four_packs_per_column(bj, orc, law, src, N, dt):
    """The widest lane group of the pack layout (64 lanes per column: 256 rows Float32, 128 Float64), per-row parameters, ragged batches."""
    check_against_closed(bj, orc, law, src, 256 if dt == np.float32 else 128, N, dt, True)


def test_mixed_sources_in_one_stage(bj, orc):
    """Logit with a per-row a next to a host-scalar b: the cotangent of a is T[dim], that of b T[1] (summed over the rows)."""
    for dt in (np.float32, np.float64):
        rng = np.random.default_rng(5)
        dim, N = 12, 130
        a = np.asarray(rng.uniform(-2, -1, size=dim), dt).astype(np.float64)
        b = float(np.asarray(2.25, dt))
        stages = [("logit", a, b)]
        X = np.asfortranarray(np.asarray(a[:, None] + (b - a[:, None]) * rng.uniform(0.05, 0.95, size=(dim, N)), dt).astype(np.float64))
        G = np.asfortranarray(np.asarray(rng.normal(size=(dim, N)), dt).astype(np.float64))
        lb = np.asarray(rng.normal(size=N), dt).astype(np.float64)
        call = Call(bj, stages, "s", dt, dim)
        rc, xb, out = call.run(bj, dev2(X, dt), dev2(G, dt), dev1(lb, dt))
        assert rc == 0
        ref_xb, ref = ref_closed(orc, stages, X, G, lb)
        assert out[0].numel() == dim and out[1].numel() == 1
        flat_close(host(xb), ref_xb, dt, "mixed logit x̄", per="sample")
        for i in (0, 1):
            flat_close(host(out[i]), np.asarray(ref[i][0]).reshape(-1), dt, f"mixed logit slot {i}", per="tensor", term_scale=ref[i][1])
        # the other way round: a host-scalar a next to a per-row b (v0 == NULL, v1 set)
        a2 = float(np.asarray(-1.5, dt))
        b2 = np.asarray(rng.uniform(1, 3, size=dim), dt).astype(np.float64)
        stages = [("logit", a2, b2)]
        X = np.asfortranarray(np.asarray(a2 + (b2[:, None] - a2) * rng.uniform(0.05, 0.95, size=(dim, N)), dt).astype(np.float64))
        call = Call(bj, stages, "s", dt, dim)
        rc, xb, out = call.run(bj, dev2(X, dt), dev2(G, dt), dev1(lb, dt))
        assert rc == 0
        ref_xb, ref = ref_closed(orc, stages, X, G, lb)
        assert out[0].numel() == 1 and out[1].numel() == dim
        flat_close(host(xb), ref_xb, dt, "mixed logit (scalar a, per-row b) x̄", per="sample")
        for i in (0, 1):
            flat_close(host(out[i]), np.asarray(ref[i][0]).reshape(-1), dt, f"mixed logit (scalar a, per-row b) slot {i}", per="tensor", term_scale=ref[i][1])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("law,dim", [("affine_leaky_affine4", 64), ("interval_affine", 67), ("logit_scale_inv", 8)])
def test_some_slots_no_xbar_and_alias(bj, orc, law, dim, dt):
    """params_bar with only some slots wanted; x_bar = NULL; x_bar aliasing y_bar."""
    slots = sorted(Call(bj, draw_case(law, "r", dim, 4, dt)[0], "r", dt, dim).len)
    check_against_closed(bj, orc, law, "r", dim, 300, dt, True, want=slots[::2])
    check_against_closed(bj, orc, law, "r", dim, 300, dt, True, want=slots[-1:], xbar=False)
    check_against_closed(bj, orc, law, "r", dim, 300, dt, True, want=[], xbar=True)
    check_against_closed(bj, orc, law, "r", dim, 300, dt, True, alias=True)


# ------------------------------------------------------------------ determinism, plans, launches
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("law,dim,N", [("exp_affine", 64, 4099), ("logit_scale_inv", 8, 1000), ("leaky_affine", 67, 1000), ("scale", 260, 65),
                                       ("affine", 64, 4099), ("shift_scale", 128, 1000)])
def test_bit_identical_calls_and_planned_run(bj, law, dim, N, dt):
    """Two identical calls give identical bits; a planned run equals the direct entry bit for bit."""
    stages, X, G, lb = draw_case(law, "r", dim, N, dt)
    call = Call(bj, stages, "r", dt, dim)
    Xd, Gd, lbd = dev2(X, dt), dev2(G, dt), dev1(lb, dt)
    rc1, xb1, o1 = call.run(bj, Xd, Gd, lbd)
    rc2, xb2, o2 = call.run(bj, Xd, Gd, lbd)
    h = call.plan(bj)
    try:
        rc3, xb3, o3 = call.run(bj, Xd, Gd, lbd, plan=h)
    finally:
        call.L.load().bjx_plan_destroy(h)
    assert rc1 == rc2 == rc3 == 0
    for xb, o in ((xb2, o2), (xb3, o3)):
        assert torch.equal(xb1, xb)
        for i in o1:
            assert torch.equal(o1[i], o[i]), i


def test_plan_sees_in_place_parameter_update(bj, orc):
    """The plan holds parameters by pointer: a per-row parameter rewritten in place between two runs is seen by the second."""
    dt, dim, N = np.float64, 16, 200
    stages, X, G, lb = draw_case("leaky_affine", "r", dim, N, dt)
    call = Call(bj, stages, "r", dt, dim)
    Xd, Gd, lbd = dev2(X, dt), dev2(G, dt), dev1(lb, dt)
    h = call.plan(bj)
    try:
        rc, _, o1 = call.run(bj, Xd, Gd, lbd, plan=h)
        assert rc == 0
        new_scale = stages[0][1] * 1.5 + 0.25
        call.dev[0].copy_(torch.from_numpy(new_scale).cuda())
        rc, xb, o2 = call.run(bj, Xd, Gd, lbd, plan=h)
        assert rc == 0
    finally:
        call.L.load().bjx_plan_destroy(h)
    stages2 = [(stages[0][0], new_scale, None)] + stages[1:]
    ref_xb, ref = ref_closed(orc, stages2, X, G, lb)
    assert not torch.equal(o1[0], o2[0])
    flat_close(host(xb), ref_xb, dt, "plan after in-place update x̄", per="sample")
    for i in o2:
        flat_close(host(o2[i]), np.asarray(ref[i][0]).reshape(-1), dt, f"plan after in-place update slot {i}", per="tensor", term_scale=ref[i][1])


def test_launch_count_of_a_planned_call(bj):
    """A planned call issues no more launches than bjx_stacked_vjp_moments on the same shape (counted here), and the count does not
    grow with the number of wanted slots."""
    L = bj._lib
    lib = L.load()
    dt, dim, N = np.float32, 64, 1000
    stages, X, G, lb = draw_case("exp_affine", "r", dim, N, dt)
    call = Call(bj, stages, "r", dt, dim)
    Xd, Gd, lbd = dev2(X, dt), dev2(G, dt), dev1(lb, dt)
    ctx = bj.interface.context(Xd.device)
    seg = (L.BjxSegment * 1)()
    seg[0].in_lo, seg[0].out_lo, seg[0].len, seg[0].n_ops = 0, 0, dim, call.n
    for k in range(call.n):
        seg[0].ops[k] = call.ops[k]
    mom = torch.empty(2 * dim + 1, dtype=torch.float64, device="cuda")
    xb = torch.empty((N, dim), dtype=torch.float32, device="cuda").T
    lib.bjx_stacked_vjp_moments(ctx.h, 0, seg, 1, Xd.data_ptr(), Gd.data_ptr(), lbd.data_ptr(), xb.data_ptr(), mom.data_ptr(), dim, N)   # warm
    n0 = lib.bjx_launch_count()
    assert lib.bjx_stacked_vjp_moments(ctx.h, 0, seg, 1, Xd.data_ptr(), Gd.data_ptr(), lbd.data_ptr(), xb.data_ptr(), mom.data_ptr(), dim, N) == 0
    d_mom = lib.bjx_launch_count() - n0
    counts = []
    for want in ([0], [0, 2]):
        h = call.plan(bj, want)
        try:
            call.run(bj, Xd, Gd, lbd, want=want, plan=h)
            n0 = lib.bjx_launch_count()
            rc, _, _ = call.run(bj, Xd, Gd, lbd, want=want, plan=h)
            counts.append(lib.bjx_launch_count() - n0)
            assert rc == 0
        finally:
            lib.bjx_plan_destroy(h)
    # four wanted slots of a four-stage chain
    stages4, X4, G4, lb4 = draw_case("affine_leaky_affine4", "r", dim, N, dt)
    call4 = Call(bj, stages4, "r", dt, dim)
    h = call4.plan(bj)
    try:
        call4.run(bj, Xd, Gd, lbd, plan=h)
        n0 = lib.bjx_launch_count()
        rc, _, _ = call4.run(bj, Xd, Gd, lbd, plan=h)
        counts.append(lib.bjx_launch_count() - n0)
        assert rc == 0
    finally:
        lib.bjx_plan_destroy(h)
    torch.cuda.synchronize()
    print("launches: bjx_stacked_vjp_moments", d_mom, "planned bjx_chain_vjp_params (1, 2, 4 slots)", counts)
    assert counts[0] == counts[1] == counts[2], counts
    assert counts[0] <= d_mom, (counts, d_mom)


def test_rejections_launch_nothing(bj):
    """TRUNCATED, STDNORMAL_LOGPDF and too many stages: BJX_ERR_UNSUPPORTED; a slot for a parameter that does not exist:
    BJX_ERR_ARG; the launch count is unchanged."""
    L = bj._lib
    lib = L.load()
    dt, dim, N = np.float32, 8, 16
    X = dev2(np.random.default_rng(0).uniform(0.2, 0.8, size=(dim, N)), dt)
    ctx = bj.interface.context(X.device)
    xb = torch.empty_like(X)
    slot = torch.empty(dim, dtype=torch.float32, device="cuda")

    def call(kinds, bar_slot=None):
        n = len(kinds)
        ops = (L.BjxOp * n)()
        for k, kind in enumerate(kinds):
            ops[k].kind, ops[k].param_len, ops[k].p0, ops[k].p1, ops[k].v0, ops[k].v1 = KIND[kind], (0 if NPAR.get(kind, 2) == 0 else 1), 0.5, 2.0, None, None
        pb = (C.c_void_p * (2 * n))()
        if bar_slot is not None:
            pb[bar_slot] = slot.data_ptr()
        n0 = lib.bjx_launch_count()
        rc = lib.bjx_chain_vjp_params(ctx.h, 0, ops, n, X.data_ptr(), X.data_ptr(), None, xb.data_ptr(), pb, dim, N)
        h = C.c_void_p()
        rc_plan = lib.bjx_plan_chain_vjp_params(ctx.h, 0, ops, n, 0 if bar_slot is None else 1 << bar_slot, dim, C.byref(h))
        assert rc_plan == rc, (kinds, rc, rc_plan)
        if rc == 0:
            lib.bjx_plan_destroy(h)
        else:                               # refused: nothing launched, no plan handed out
            assert not h.value, kinds
            assert lib.bjx_launch_count() == n0, kinds
        return rc

    assert call(["truncated"]) == L.ERR_UNSUPPORTED
    assert call(["scale", "logpdf"]) == L.ERR_UNSUPPORTED
    assert call(["shift"] * 5) == L.ERR_UNSUPPORTED
    assert call(["exp"], bar_slot=0) == L.ERR_ARG                  # exp has no parameter
    assert call(["scale", "shift"], bar_slot=3) == L.ERR_ARG       # Shift has no second parameter
    assert call(["scale", "shift"], bar_slot=2) == 0


def test_agrees_with_coupling_chain_vjp(bj):
    """The same parameters expanded to (n1, batch) with idx1 = all rows through bjx_coupling_chain_vjp: its per-column cotangents,
    summed on the host, are the batch sums of this entry."""
    L = bj._lib
    lib = L.load()
    dim, N = 8, 257
    for dt in (np.float32, np.float64):
        stages, X, G, lb = draw_case("affine_leaky_affine4", "r", dim, N, dt)
        call = Call(bj, stages, "r", dt, dim)
        Xd, Gd, lbd = dev2(X, dt), dev2(G, dt), dev1(lb, dt)
        rc, xb, out = call.run(bj, Xd, Gd, lbd)
        assert rc == 0
        ctx = bj.interface.context(Xd.device)
        n = call.n
        params = (C.c_void_p * (2 * n))()
        lds = (C.c_int64 * (2 * n))()
        pbar = (C.c_void_p * (2 * n))()
        keep, bars = [], {}
        for i in call.len:
            full = dev2(np.broadcast_to(np.asarray(stages[i // 2][1 + i % 2]).reshape(-1, 1), (dim, N)), dt)
            keep.append(full)
            params[i], lds[i] = full.data_ptr(), dim
            bars[i] = torch.empty((N, dim), dtype=DT[dt], device="cuda").T
            pbar[i] = bars[i].data_ptr()
        idx = torch.arange(dim, dtype=torch.int32, device="cuda")
        xb2 = torch.empty((N, dim), dtype=DT[dt], device="cuda").T
        rc = lib.bjx_coupling_chain_vjp(ctx.h, 0 if dt == np.float32 else 1, 0, idx.data_ptr(), dim, call.ops, n, params, lds, Xd.data_ptr(), Gd.data_ptr(),
                                        lbd.data_ptr(), xb2.data_ptr(), pbar, dim, N)
        assert rc == 0
        flat_close(host(xb), host(xb2).astype(np.float64), dt, "x̄ against bjx_coupling_chain_vjp", per="sample")
        for i in call.len:
            cols = host(bars[i]).astype(np.float64)
            flat_close(host(out[i]), cols.sum(axis=1), dt, f"slot {i} against bjx_coupling_chain_vjp summed on the host", per="tensor",
                       term_scale=float(np.abs(cols).max()))


# ------------------------------------------------------------------ reference (b): central differences through oracle.chain
@pytest.mark.parametrize("law", ["shift", "scale", "scale_inv", "logit", "logit_inv", "leaky", "interval_affine", "affine_leaky_affine4", "logit_scale_inv"])
@pytest.mark.parametrize("src", ["r", "s"])
def test_central_differences(bj, orc, law, src):
    """Float64 central differences of Σ ȳ·y(θ) + Σ ℓ̄·ladj(θ) through oracle.chain, one chain per parameterised kind, per-row and
    scalar parameters.  oracle.chain is called with fused=True, as tests/test_gpu_coupling_chain.py does: the unfused entry reads only
    the first element of a per-row Logit parameter (the reference's Logit has scalar bounds), so a bump of row r > 0 is invisible to it.  Step 1e-6: truncation ~1e-12·|f'''|, rounding ~1e-16·|f|/1e-6 = 1e-10·|f| — both below the 1e-6 bar on the
    scale max(|p̄|, max |summand|).  (LeakyReLU: the draws keep every stage input at least 4e-5 away from the kink, the step moves it by < 4e-6.)"""
    dt, dim, N = np.float64, 5, 33
    stages, X, G, lb = draw_case(law, src, dim, N, dt, True, tag="fd")
    call = Call(bj, stages, src, dt, dim)
    rc, _, out = call.run(bj, dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    assert rc == 0
    _, ref = ref_closed(orc, stages, X, G, lb)

    def total(st):
        ops = [(KIND[op], p0, p1) for op, p0, p1 in st]
        tot = 0.0
        for n in range(N):
            y, lj = orc.chain(ops, np.asfortranarray(X[:, n:n + 1]), fused=True)     # the restatement that takes one parameter per row
            tot += float((G[:, n:n + 1] * y).sum()) + float(lb[n]) * float(lj)
        return tot

    h = 1e-6
    for i in sorted(call.len):
        k, j = divmod(i, 2)
        got = host(out[i]).astype(np.float64)
        rows = [None] if src == "s" else [0, dim // 2, dim - 1]
        for r in rows:
            def bumped(sign):
                st = [list(s) for s in stages]
                p = np.array(st[k][1 + j], np.float64, copy=True)
                if r is None:
                    p = float(p) + sign * h
                else:
                    p[r] += sign * h
                st[k][1 + j] = p
                return [tuple(s) for s in st]

            fd = (total(bumped(+1)) - total(bumped(-1))) / (2 * h)
            g = float(got[0] if r is None else got[r])
            scale = max(abs(fd), ref[i][1])
            print(f"fd {law} src={src} slot {i} row {r}: got {g:.12g} fd {fd:.12g} scale {scale:.3g}")
            assert abs(g - fd) <= 1e-6 * scale, (law, src, i, r, g, fd, scale)


# ------------------------------------------------------------------ through Python
def _bij(bj, op, p0, p1, dt):
    t = lambda p: p if not np.ndim(p) else torch.from_numpy(np.asarray(p, dt)).cuda()
    e = bj.elementwise
    return {"exp": lambda: e(bj.exp), "log": lambda: e(bj.log), "shift": lambda: bj.Shift(t(p0)), "scale": lambda: bj.Scale(t(p0)),
            "scale_inv": lambda: bj.inverse(bj.Scale(t(p0))), "logit": lambda: bj.Logit(t(p0), t(p1)), "logit_inv": lambda: bj.inverse(bj.Logit(t(p0), t(p1))),
            "leaky": lambda: bj.LeakyReLU(t(p0))}[op]()


def _compose(bj, stages, dt):
    b = None
    for op, p0, p1 in stages:
        s = _bij(bj, op, p0, p1, dt)
        b = s if b is None else s @ b
    return b


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_vjp_params_of_logit_and_leaky_relu_stages(bj, orc, dt):
    """vjp_params(Logit(a, b) ∘ LeakyReLU(α), …) returns the stage dictionaries (it raised NotImplementedError: no Scale / Shift stage)."""
    rng = np.random.default_rng(11)
    dim, N = 12, 300
    alpha, a, b = float(np.asarray(0.3, dt)), -3.0, 2.5
    X = np.asfortranarray(np.asarray(rng.uniform(-2.0, 2.2, size=(dim, N)), dt).astype(np.float64))     # LeakyReLU output in (-0.6, 2.2): 5 % inside (a, b)
    G = np.asfortranarray(np.asarray(rng.normal(size=(dim, N)), dt).astype(np.float64))
    lb = np.asarray(rng.normal(size=N), dt).astype(np.float64)
    bij = bj.Logit(a, b) @ bj.LeakyReLU(alpha)
    xb, g = bj.vjp_params(bij, dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    assert set(g) == {"stages"} and len(g["stages"]) == 2
    assert set(g["stages"][0]) == {"alpha"} and set(g["stages"][1]) == {"a", "b"}
    stages = [("leaky", alpha, None), ("logit", a, b)]
    ref_xb, ref = ref_closed(orc, stages, X, G, lb)
    flat_close(host(xb), ref_xb, dt, "vjp_params Logit∘LeakyReLU x̄", per="sample")
    for slot, t in ((0, g["stages"][0]["alpha"]), (2, g["stages"][1]["a"]), (3, g["stages"][1]["b"])):
        assert t.shape == ()
        flat_close(host(t).reshape(-1), np.asarray(ref[slot][0]).reshape(-1), dt, f"vjp_params Logit∘LeakyReLU slot {slot}", per="tensor", term_scale=ref[slot][1])
    # the same through a per-row α and inverse(Scale): tensors shaped as the parameter
    stages, X, G, lb = draw_case("logit_scale_inv", "r", dim, N, dt)
    xb, g = bj.vjp_params(_compose(bj, stages, dt), dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    ref_xb, ref = ref_closed(orc, stages, X, G, lb)
    assert g["stages"][0].shape == (dim,) and g["stages"][1]["a"].shape == (dim,)
    flat_close(host(xb), ref_xb, dt, "vjp_params Logit∘inverse(Scale) x̄", per="sample")
    for slot, t in ((0, g["stages"][0]), (2, g["stages"][1]["a"]), (3, g["stages"][1]["b"])):
        flat_close(host(t), ref[slot][0], dt, f"vjp_params Logit∘inverse(Scale) slot {slot}", per="tensor", term_scale=ref[slot][1])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("src", ["r", "s"])
def test_vjp_params_mean_field_and_affine_anywhere_keep_their_formats(bj, orc, src, dt):
    """The mean-field chain keeps {"scale", "shift"} (and its bjx_stacked_vjp_moments path), a 3-stage chain with an affine stage
    behind a nonlinear one and the two-stage Scale ∘ Shift keep {"stages": [...]} with tensors shaped as the parameters — all
    against reference (a)."""
    dim, N = 64, 257
    stages, X, G, lb = draw_case("exp_affine", src, dim, N, dt)
    xb, g = bj.vjp_params(_compose(bj, stages, dt), dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    ref_xb, ref = ref_closed(orc, stages, X, G, lb)
    assert set(g) == {"scale", "shift"}
    shape = (dim,) if src == "r" else ()
    assert g["scale"].shape == shape and g["shift"].shape == shape and g["scale"].dtype == DT[dt]
    flat_close(host(xb), ref_xb, dt, "mean-field x̄", per="sample")
    flat_close(host(g["scale"]).reshape(-1), np.asarray(ref[0][0]).reshape(-1), dt, "mean-field scale", per="tensor", term_scale=ref[0][1])
    flat_close(host(g["shift"]).reshape(-1), np.asarray(ref[2][0]).reshape(-1), dt, "mean-field shift", per="tensor", term_scale=ref[2][1])
    # LeakyReLU, then Scale, then Shift: affine stages behind a nonlinear one
    rng = np.random.default_rng(seed_of("anywhere", src, np.dtype(dt).name))
    stages = [("leaky", 0.3, None), ("scale", draw_param(rng, "scale", 0, src, dim, dt), None), ("shift", draw_param(rng, "shift", 0, src, dim, dt), None)]
    xb, g = bj.vjp_params(_compose(bj, stages, dt), dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    ref_xb, ref = ref_closed(orc, [("leaky", float(np.asarray(0.3, dt)), None)] + stages[1:], X, G, lb)
    assert set(g) == {"stages"} and len(g["stages"]) == 3
    assert set(g["stages"][0]) == {"alpha"} and g["stages"][1].shape == shape and g["stages"][2].shape == shape
    flat_close(host(xb), ref_xb, dt, "affine-anywhere x̄", per="sample")
    flat_close(host(g["stages"][1]).reshape(-1), np.asarray(ref[2][0]).reshape(-1), dt, "affine-anywhere scale", per="tensor", term_scale=ref[2][1])
    flat_close(host(g["stages"][2]).reshape(-1), np.asarray(ref[4][0]).reshape(-1), dt, "affine-anywhere shift", per="tensor", term_scale=ref[4][1])
    # Scale ∘ Shift: two one-parameter stages, the pack layout
    stages, X, G, lb = draw_case("shift_scale", src, dim, N, dt)
    xb, g = bj.vjp_params(_compose(bj, stages, dt), dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    ref_xb, ref = ref_closed(orc, stages, X, G, lb)
    assert set(g) == {"stages"} and g["stages"][0].shape == shape and g["stages"][1].shape == shape
    flat_close(host(xb), ref_xb, dt, "Scale∘Shift x̄", per="sample")
    flat_close(host(g["stages"][0]).reshape(-1), np.asarray(ref[0][0]).reshape(-1), dt, "Scale∘Shift shift", per="tensor", term_scale=ref[0][1])
    flat_close(host(g["stages"][1]).reshape(-1), np.asarray(ref[2][0]).reshape(-1), dt, "Scale∘Shift scale", per="tensor", term_scale=ref[2][1])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_vjp_params_host_scalar_next_to_a_per_row_bound(bj, orc, dt):
    """Shift(c) ∘ Logit(0.0, b_vec): a host-scalar first parameter next to a per-row second one (the call returned a result before the
    one-pass entry existed and must keep doing so; the Logit stage now has its cotangents)."""
    rng = np.random.default_rng(23)
    dim, N = 12, 130
    bvec = np.asarray(rng.uniform(1, 3, size=dim), dt).astype(np.float64)
    c = float(np.asarray(0.25, dt))
    stages = [("logit", 0.0, bvec), ("shift", c, None)]
    X = np.asfortranarray(np.asarray(bvec[:, None] * rng.uniform(0.05, 0.95, size=(dim, N)), dt).astype(np.float64))
    G = np.asfortranarray(np.asarray(rng.normal(size=(dim, N)), dt).astype(np.float64))
    lb = np.asarray(rng.normal(size=N), dt).astype(np.float64)
    bij = bj.Shift(c) @ bj.Logit(0.0, torch.from_numpy(np.asarray(bvec, dt)).cuda())
    xb, g = bj.vjp_params(bij, dev2(X, dt), dev2(G, dt), dev1(lb, dt))
    ref_xb, ref = ref_closed(orc, stages, X, G, lb)
    flat_close(host(xb), ref_xb, dt, "Shift∘Logit(0, b_vec) x̄", per="sample")
    assert g["stages"][0]["a"].shape == () and g["stages"][0]["b"].shape == (dim,)
    flat_close(host(g["stages"][0]["a"]).reshape(-1), np.asarray(ref[0][0]).reshape(-1), dt, "Shift∘Logit(0, b_vec) a", per="tensor", term_scale=ref[0][1])
    flat_close(host(g["stages"][0]["b"]), ref[1][0], dt, "Shift∘Logit(0, b_vec) b", per="tensor", term_scale=ref[1][1])
    flat_close(host(g["stages"][1]).reshape(-1), np.asarray(ref[2][0]).reshape(-1), dt, "Shift∘Logit(0, b_vec) shift", per="tensor", term_scale=ref[2][1])
