#!/usr/bin/env python3
"""One measured line per SURVEY.md §8(a) row (forward and inverse where the row has both): dominant
kernel time from per-launch hipEvent pairs (bjx_kernel_time_begin/_end), algorithmic bytes
(read input once + write output once + 4 B/sample when a per-sample log-det is written) and the
fraction of the 8 TB/s HBM peak.  Float32, inputs resident in HBM.  Output: a markdown table.

    python scripts/bench_rows.py [--log2-batch 22] [--steps 10] [--only name,...]
"""
import argparse
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bijectors_amd as bj  # noqa: E402
from _timing import kernel_and_region_ms  # noqa: E402

PEAK = 8000.0


def cm(rows, batch, dev, dt=torch.float32):
    return torch.empty((batch, rows), dtype=dt, device=dev).T


def randn(rows, batch, dev, seed, std=1.0, mean=0.0):
    t = cm(rows, batch, dev)
    L, ctx = bj._lib, bj.context(dev)
    L.check(ctx.h, L.load().bjx_fill_normal(ctx.h, L.BJX_F32, t.data_ptr(), rows, batch, 0, seed, mean, std), "fill")
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-batch", type=int, default=22)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    N = 1 << a.log2_batch
    d = 64
    f32 = torch.float32
    x = randn(d, N, dev, 0)
    xpos = torch.exp(0.5 * x.T).T
    xunit = torch.sigmoid(x.T).T
    rows = []  # (name, reference, callable, bytes_per_sample, samples)
    torch_cols = []  # plain-PyTorch batched spline (softmax / cumsum / searchsorted / gather): the same coupling without bjx_rqs_cols

    def add(name, ref, b, inp, out_rows=None, per_sample=True, samples=None):
        n = inp.shape[-1] if samples is None else samples
        in_rows = inp.numel() // n
        orows = in_rows if out_rows is None else out_rows
        y = cm(orows, n, dev) if inp.dim() == 2 and orows * n < (1 << 34) else None
        bps = 4 * (in_rows + orows) + (4 if per_sample else 0)

        def step():
            return bj.shard.with_logabsdet_jacobian_sharded(b, inp, out=y, per_sample=per_sample)

        rows.append((name, ref, step, bps, n))

    e = bj.elementwise
    add("exp∘Shift∘Scale (sum)", "a1,a3,a4,a5", e(bj.exp) @ bj.Shift(0.1) @ bj.Scale(0.5), x, per_sample=False)
    add("exp∘Shift∘Scale (per-sample ladj)", "a1,a3,a4,a5", e(bj.exp) @ bj.Shift(0.1) @ bj.Scale(0.5), x)
    add("elementwise(log)", "a2", e(bj.log), xpos, per_sample=False)
    add("Logit(0,1)", "a6", bj.Logit(0.0, 1.0), xunit, per_sample=False)
    add("inverse(Logit(0,1))", "a6", bj.inverse(bj.Logit(0.0, 1.0)), x, per_sample=False)
    add("LeakyReLU(0.1)", "a7", bj.LeakyReLU(0.1), x, per_sample=False)
    add("TruncatedBijector(0,1)", "a8", bj.TruncatedBijector(0.0, 1.0), xunit, per_sample=False)
    add("inverse(TruncatedBijector(0,1))", "a8", bj.inverse(bj.TruncatedBijector(0.0, 1.0)), x, per_sample=False)
    add("OrderedBijector", "a9", bj.OrderedBijector(), x)
    xo = bj.transform(bj.OrderedBijector(), x)
    add("inverse(OrderedBijector)", "a9", bj.inverse(bj.OrderedBijector()), xo)
    Ns = 1 << min(a.log2_batch, 22)
    xs = torch.softmax(randn(d, Ns, dev, 1).T, dim=1).T
    add("SimplexBijector K=64", "a10,a12", bj.SimplexBijector(), xs, out_rows=d - 1)
    ys = randn(d - 1, Ns, dev, 2)
    add("inverse(SimplexBijector) K=64", "a11", bj.inverse(bj.SimplexBijector()), ys, out_rows=d)
    K = 64
    Nc = 1 << min(a.log2_batch, 16)
    n = K * (K - 1) // 2
    yv = randn(n, Nc, dev, 3, std=0.5)
    icb = bj.inverse(bj.VecCholeskyBijector("U"))
    rows.append(("inverse(VecCholesky) K=64", "a14", lambda: bj.shard.with_logabsdet_jacobian_sharded(icb, yv), 4 * (n + K * K) + 4, Nc))
    Wd, _, _ = bj.shard.with_logabsdet_jacobian_sharded(icb, yv)
    cb = bj.VecCholeskyBijector("U")
    rows.append(("VecCholesky K=64 (W→y)", "a13", lambda: bj.shard.with_logabsdet_jacobian_sharded(cb, Wd), 4 * (n + K * K) + 4, Nc))
    dp, nl = 128, 8
    Np = 1 << min(a.log2_batch, 22)
    z = randn(dp, Np, dev, 4)
    w = randn(dp, nl, dev, 5, std=1 / math.sqrt(dp))
    u = randn(dp, nl, dev, 6, std=1 / math.sqrt(dp))
    bb = randn(nl, 1, dev, 7).reshape(-1).contiguous()
    flow = bj.PlanarLayer(w, u, bb)
    add("8×PlanarLayer d=128", "a15", flow, z)
    zf = bj.transform(flow, z)
    add("inverse(8×PlanarLayer) d=128", "a16", bj.inverse(flow), zf)
    one = bj.PlanarLayer(w[:, 0].contiguous(), u[:, 0].contiguous(), bb[:1].contiguous())
    add("1×PlanarLayer d=128", "a15", one, z)
    rad = bj.RadialLayer(torch.tensor([0.3], device=dev), torch.tensor([0.5], device=dev), randn(dp, 1, dev, 8).reshape(-1).contiguous())
    add("RadialLayer d=128", "a17", rad, z)
    add("inverse(RadialLayer) d=128", "a17", bj.inverse(rad), z)
    bn = bj.InvertibleBatchNorm(torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.ones(d, device=dev))
    add("InvertibleBatchNorm (eval) d=64", "a18", bn, x)
    bnt = bj.InvertibleBatchNorm(torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.ones(d, device=dev))

    def bn_train_step():
        with bj.training():
            return bj.shard.with_logabsdet_jacobian_sharded(bnt, x, out=y_bn)

    y_bn = cm(d, N, dev)
    rows.append(("InvertibleBatchNorm (training mode: statistics pass + apply pass) d=64", "a18", bn_train_step, 3 * 4 * d + 4, N))   # x is read twice
    dr, Kb = 32, 16
    raw = [randn(dr, k, dev, 100 + i) for i, k in enumerate((Kb, Kb, Kb - 1))]
    rqs = bj.RationalQuadraticSpline(raw[0], raw[1], raw[2], 3.0)
    xr = randn(dr, N, dev, 9)
    add("RQS K=16 d=32 forward", "a19", rqs, xr)
    yr = bj.transform(rqs, xr)
    add("RQS K=16 d=32 inverse", "a19", bj.inverse(rqs), yr)
    gr = randn(dr, N, dev, 31)
    lbr = randn(N, 1, dev, 32).reshape(-1).contiguous()
    rows.append(("vjp(RQS K=16 d=32)", "f-1", lambda: bj.vjp(rqs, xr, gr, lbr), 4 * 3 * dr + 4, N))
    rows.append(("vjp(inverse(RQS K=16 d=32))", "f-1", lambda: bj.vjp(bj.inverse(rqs), yr, gr, lbr), 4 * 3 * dr + 4, N))
    rows.append(("vjp_params(RQS K=16 d=32): input pullback + knot and raw-parameter cotangents (one pass over x, ȳ, ℓ̄)", "f-1",
                 lambda: bj.vjp_params(rqs, xr, gr, lbr), 4 * 3 * dr + 4, N))
    perm = bj.Permute(list(torch.randperm(d, generator=torch.Generator().manual_seed(0)).add(1).tolist()))
    add("Permute d=64", "a21", perm, x, per_sample=False)
    mask = bj.PartitionMask(d, list(range(1, d // 2 + 1)), list(range(d // 2 + 1, d + 1)))
    sc = torch.full((d // 2,), 1.5, device=dev)
    cpl = bj.Coupling(lambda x2: bj.Shift(0.25) @ bj.Scale(sc), mask)
    add("Coupling(Shift∘Scale) d=64, θ = [n1,batch] scale + shift arrays", "a20", cpl, x)
    rows[-1] = rows[-1][:3] + (rows[-1][3] + 2 * (d // 2) * 4,) + rows[-1][4:]     # the per-sample θ arrays are read too

    stk = bj.Stacked([e(bj.exp), bj.Logit(0.0, 1.0), bj.identity, e(bj.exp) @ bj.Shift(0.1) @ bj.Scale(0.5)], [(1, 16), (17, 32), (33, 48), (49, 64)])
    xst = x.clone()
    xst[16:32] = xunit[16:32]
    add("Stacked(exp|Logit|identity|exp∘Shift∘Scale) d=64", "f-4", stk, xst)

    gb = randn(d, N, dev, 11)
    lbar = randn(N, 1, dev, 12).reshape(-1).contiguous()
    ob = bj.OrderedBijector()
    # pullbacks read the primal input + the output cotangent (+ 4 B/sample of log-det cotangent) and write the input cotangent
    rows.append(("vjp(OrderedBijector) d=64", "f-1", lambda: bj.vjp(ob, x, gb, lbar), 3 * d * 4 + 4, N))
    rows.append(("vjp(inverse(OrderedBijector)) d=64", "f-1", lambda: bj.vjp(bj.inverse(ob), xo, gb, lbar), 3 * d * 4 + 4, N))

    Wb = randn(K * K, Nc, dev, 13).T.reshape(Nc, K, K).permute(2, 1, 0)      # column-major (K, K, batch): strides (1, K, K²) — a plain reshape gives (K, 1, K²) and the call a layout copy (0.8 ms)
    lb2 = randn(Nc, 1, dev, 14).reshape(-1).contiguous()
    rows.append(("vjp(inverse(VecCholesky)) K=64", "f-1", lambda: bj.vjp(icb, yv, Wb, lb2), 4 * (2 * n + K * K) + 4, Nc))

    gyv = randn(n, Nc, dev, 23, std=1.0)
    rows.append(("vjp(VecCholesky forward link) K=64", "f-1", lambda: bj.vjp(cb, Wd, gyv), 4 * (n + 2 * K * K), Nc))

    gxs = randn(d, Ns, dev, 15)
    gys = randn(d - 1, Ns, dev, 16)
    lbs = randn(Ns, 1, dev, 17).reshape(-1).contiguous()
    sb_ = bj.SimplexBijector()
    rows.append(("vjp(SimplexBijector) K=64", "f-1", lambda: bj.vjp(sb_, xs, gys, lbs), 4 * (d + d - 1 + d) + 4, Ns))
    rows.append(("vjp(inverse(SimplexBijector)) K=64", "f-1", lambda: bj.vjp(bj.inverse(sb_), ys, gxs, lbs), 4 * (d - 1 + d + d - 1) + 4, Ns))
    rows.append(("vjp(Stacked(exp|Logit|identity|exp∘Shift∘Scale)) d=64", "f-1", lambda: bj.vjp(stk, xst, gb, lbar), 3 * d * 4 + 4, N))

    gz = randn(dp, Np, dev, 21)
    lbz = randn(Np, 1, dev, 22).reshape(-1).contiguous()
    rows.append(("vjp(8×PlanarLayer) d=128", "f-1", lambda: bj.vjp(flow, z, gz, lbz), 4 * 3 * dp + 4, Np))

    rows.append(("vjp(inverse(8×PlanarLayer)) d=128", "f-1", lambda: bj.vjp(bj.inverse(flow), zf, gz, lbz), 4 * 3 * dp + 4, Np))

    rows.append(("vjp(RadialLayer) d=128", "f-1", lambda: bj.vjp(rad, z, gz, lbz), 4 * 3 * dp + 4, Np))
    rows.append(("vjp_params(RadialLayer) d=128 (input pullback with the row sums for z̄₀ in the same pass)", "f-1", lambda: bj.vjp_params(rad, z, gz, lbz), 4 * 3 * dp + 4 + 8 + 64, Np))
    rows.append(("vjp_params(8×PlanarLayer) d=128 (input + w̄, ū, b̄; two passes)", "f-1", lambda: bj.vjp_params(flow, z, gz, lbz), 4 * 5 * dp + 4 + 4 * 4 * nl, Np))

    rows.append(("vjp_params(inverse(8×PlanarLayer)) d=128 (inverse transform + inverse input pullback + forward parameter pullback at the pre-image)", "f-1",
                 lambda: bj.vjp_params(bj.inverse(flow), zf, gz, lbz), 4 * 2 * dp + 4 * 3 * dp + 4 + 4 * 5 * dp + 4 + 4 * 4 * nl, Np))

    # §8(f) f-3: logpdf(td, Y) fused into the inverting kernel — Y is read once, x is never stored
    td_pl = bj.transformed(bj.MvNormal(dp), flow)
    rows.append(("logpdf(transformed(MvNormal(128), 8×PlanarLayer)) d=128", "f-3", lambda: bj.logpdf(td_pl, zf), 4 * dp + 4, Np))
    td_ch = bj.transformed(bj.MvNormal(torch.zeros(d, device=dev), torch.ones(d, device=dev)), e(bj.exp) @ bj.Shift(0.1) @ bj.Scale(0.5))
    rows.append(("logpdf(transformed(MvNormal(μ,σ), exp∘Shift∘Scale)) d=64", "f-3", lambda: bj.logpdf(td_ch, xpos), 4 * d + 4, N))

    rows.append(("rand(transformed(MvNormal(μ,σ), exp∘Shift∘Scale), 2^22) d=64 (samples drawn in the kernel)", "f-3", lambda: bj.rand(td_ch, N, seed=1), 4 * d, N))
    mf = e(bj.exp) @ bj.Shift(torch.zeros(d, device=dev)) @ bj.Scale(torch.ones(d, device=dev))
    rows.append(("vjp_params(exp∘Shift(μ)∘Scale(σ)) d=64 (input pullback with the row moments in the same pass)", "f-1", lambda: bj.vjp_params(mf, x, gb, lbar), 4 * 3 * d + 4 + 16, N))
    c2b = e(bj.exp) @ bj.Shift(0.1) @ bj.Scale(0.5)
    rows.append(("logabsdetjac(exp∘Shift∘Scale) alone (values not stored)", "a1,a5", lambda: bj.logabsdetjac(c2b, x), 4 * d, N))

    # §8(f) f-4: matrix-variate constraint bijectors (per-sample Cholesky), Scale with a matrix, Stacked with structured blocks
    # K = 4 and 8: the sizes LKJ / Wishart blocks have in models (one lane per sample); K = 32: lanes along the rows
    for Km, lbm in ((4, 22), (8, 20), (32, 18)):
        Nm = 1 << min(a.log2_batch, lbm)
        for nm, cls in (("VecCorrBijector", bj.VecCorrBijector), ("PDVecBijector", bj.PDVecBijector)):
            bm = cls()
            nvm = bm._n(Km)
            ym = randn(nvm, Nm, dev, 40, std=0.3)
            Xm = bj.transform(bj.inverse(bm), ym)
            bpsm = 4 * (Km * Km + nvm) + 4
            rows.append((f"{nm} K={Km} (X → Cholesky → y)", "f-4", (lambda b_=bm, X_=Xm: bj.shard.with_logabsdet_jacobian_sharded(b_, X_)), bpsm, Nm))
            rows.append((f"inverse({nm}) K={Km} (y → X = U'U)", "f-4", (lambda b_=bm, y_=ym: bj.shard.with_logabsdet_jacobian_sharded(bj.inverse(b_), y_)), bpsm, Nm))
    # §8(f) f-1 x f-4: pullbacks of the matrix bijectors (bjx_*_vjp).  Algorithmic bytes: primal input + output cotangent read, input
    # cotangent written, + the log-det cotangent
    for Km, lbm in ((3, 22), (4, 22), (8, 20), (12, 19), (16, 18), (24, 16), (32, 16), (48, 14), (64, 14)):
        Nm = 1 << min(a.log2_batch, lbm)
        for nm, cls in (("VecCorrBijector", bj.VecCorrBijector), ("PDVecBijector", bj.PDVecBijector)):
            bm = cls()
            nvm = bm._n(Km)
            ym = randn(nvm, Nm, dev, 40, std=0.3)
            Xm = bj.transform(bj.inverse(bm), ym)
            Xbar = randn(Km * Km, Nm, dev, 42).T.reshape(Nm, Km, Km).permute(2, 1, 0)      # column-major (K, K, batch): strides (1, K, K²)
            ybar = randn(nvm, Nm, dev, 43)
            lbm_ = randn(Nm, 1, dev, 44).reshape(-1).contiguous()
            rows.append((f"vjp(inverse({nm})) K={Km} (ȳ from X̄, ℓ̄)", "f-1", (lambda b_=bm, y_=ym, g_=Xbar, l_=lbm_: bj.vjp(bj.inverse(b_), y_, g_, l_)), 4 * (2 * nvm + Km * Km) + 4, Nm))
            rows.append((f"vjp({nm}) K={Km} (X̄ from ȳ, ℓ̄)", "f-1", (lambda b_=bm, X_=Xm, g_=ybar, l_=lbm_: bj.vjp(b_, X_, g_, l_)), 4 * (2 * Km * Km + nvm) + 4, Nm))
    Am = (randn(d, d, dev, 41, std=1 / math.sqrt(d)) + 1.5 * torch.eye(d, device=dev).T).T.contiguous().T
    add("Scale(64×64 matrix): a * x + logabsdet(a)", "f-4", bj.Scale(Am), x)
    add("inverse(Scale(64×64 matrix)): a \\ y", "f-4", bj.inverse(bj.Scale(Am)), x)
    # the parameter pullback of the matrix Scale (round 6): input pullback (x̄ = aᵀȳ: x, ȳ read, x̄ written) + ā = ȳxᵀ + Σℓ̄·a⁻ᵀ (x, ȳ read again by the
    # matrix-core outer-product kernel): 5 array passes + ℓ̄
    gsm = randn(d, N, dev, 45)
    lsm = randn(N, 1, dev, 46).reshape(-1).contiguous()
    rows.append(("vjp_params(Scale(64×64 matrix)): x̄ = aᵀȳ and ā = ȳxᵀ + Σℓ̄·a⁻ᵀ (outer-product sum on the matrix cores)", "f-1", lambda: bj.vjp_params(bj.Scale(Am), x, gsm, lsm), 4 * 5 * d + 4, N))
    # the same two calls with the reuse of parameter tables opted into (bj.cache_params: the factorisation of an unchanged matrix
    # is kept — no prep kernel in the steady state), and logpdf / rand with a FULL covariance (whitening = the matrix Scale)
    cached_rows = set()

    def cached(fn):          # measured inside ONE `with bj.cache_params():` region (entering and leaving per call would drop the tables each time)
        cached_rows.add(fn)
        return fn

    bsm, ibsm = bj.Scale(Am), bj.inverse(bj.Scale(Am))
    ysm = cm(d, N, dev)
    rows.append(("Scale(64×64 matrix) under cache_params (factorisation kept)", "f-4", cached(lambda: bj.shard.with_logabsdet_jacobian_sharded(bsm, x, out=ysm)), 4 * 2 * d + 4, N))
    rows.append(("inverse(Scale(64×64 matrix)) under cache_params", "f-4", cached(lambda: bj.shard.with_logabsdet_jacobian_sharded(ibsm, x, out=ysm)), 4 * 2 * d + 4, N))
    cov = (Am @ Am.T).T.contiguous().T
    td_cov = bj.transformed(bj.MvNormal(torch.zeros(d, device=dev), cov=cov), e(bj.exp))
    rows.append(("logpdf(transformed(MvNormal(μ, Σ full 64×64), exp)) d=64", "f-3", lambda: bj.logpdf(td_cov, xpos), 4 * d + 4, N))
    rows.append(("logpdf(… MvNormal(μ, Σ full)) under cache_params", "f-3", cached(lambda: bj.logpdf(td_cov, xpos)), 4 * d + 4, N))
    mix = bj.Stacked([e(bj.exp) @ bj.Shift(0.1) @ bj.Scale(0.5), bj.SimplexBijector(), bj.Logit(0.0, 1.0), bj.OrderedBijector()], [(1, 16), (17, 32), (33, 48), (49, 64)])
    xmix = x.clone()
    xmix[16:32] = torch.softmax(x[16:32].T, dim=1).T
    xmix[32:48] = xunit[32:48]
    add("Stacked(exp∘Shift∘Scale | Simplex | Logit | Ordered) d=64 → 63: structured blocks in the same launch", "f-4", mix, xmix, out_rows=d - 1)

    # Per-column spline coupling (include/bjx_cols.h, the neural spline coupling): dim 64, half mask (n1 = 32), K = 8 bins,
    # 2^20 columns Float32 / 2^19 Float64.  Algorithmic bytes: every parameter value once, x read and y written for every row, the
    # per-sample log-det; the pullback reads the parameters, x₁, ȳ and ℓ̄ and writes x̄ and the per-column parameter cotangents.
    if not only_given(a.only) or "RQS-cols" in a.only or "torch-spline" in a.only:
        for dtc, lgN in ((torch.float32, 20), (torch.float64, 19)):
            Nc_, n1c, Kc, Bc = 1 << lgN, 32, 8, 3.0
            es = 4 if dtc == torch.float32 else 8
            gq = torch.Generator(device=dev).manual_seed(9)
            xq = torch.randn((Nc_, d), dtype=dtc, device=dev, generator=gq).T * 1.5
            gy = torch.randn((Nc_, d), dtype=dtc, device=dev, generator=gq).T
            lq = torch.randn(Nc_, dtype=dtc, device=dev, generator=gq)
            head = torch.randn((Nc_, 3 * Kc - 1, n1c), dtype=dtc, device=dev, generator=gq).permute(2, 1, 0)    # one network head
            rwq, rhq, rdq = head[:, :Kc], head[:, Kc:2 * Kc], head[:, 2 * Kc:]
            sp_raw = bj.RationalQuadraticSpline(rwq, rhq, rdq, Bc)

            def knots_t(r):
                c_ = torch.cumsum(torch.softmax(r, dim=1), dim=1)
                return torch.cat([torch.zeros_like(c_[:, :1]), c_], dim=1) * (2 * Bc) - Bc
            one = torch.ones_like(rdq[:, :1])
            kw, kh = knots_t(rwq), knots_t(rhq)
            kd = torch.cat([one, torch.nn.functional.softplus(rdq), one], dim=1)
            kw, kh, kd = (t.permute(2, 1, 0).contiguous().permute(2, 1, 0) for t in (kw, kh, kd))
            sp_kn = bj.RationalQuadraticSpline(kw, kh, kd)
            maskc = bj.PartitionMask(d, list(range(1, n1c + 1)))
            cpl = {f: bj.Coupling((lambda s_: (lambda x2: s_))(s_), maskc) for f, s_ in (("raw", sp_raw), ("knots", sp_kn))}
            P = {"raw": (3 * Kc - 1) * n1c * es, "knots": 3 * (Kc + 1) * n1c * es}
            tag = "f32" if dtc == torch.float32 else "f64"
            for form in ("raw", "knots"):
                cb_ = cpl[form]
                yq = torch.empty_like(xq)
                bps_f = P[form] + 2 * d * es + es
                bps_v = 2 * P[form] + (n1c + 2 * d) * es + es
                rows.append((f"RQS-cols coupling {form} {tag} d=64 n1=32 K=8", "cols", (lambda c_=cb_, y_=yq, x_=xq: bj.shard.with_logabsdet_jacobian_sharded(c_, x_, out=y_)), bps_f, Nc_))
                rows.append((f"RQS-cols inverse(coupling) {form} {tag} d=64 n1=32 K=8", "cols", (lambda c_=cb_, y_=yq, x_=xq: bj.shard.with_logabsdet_jacobian_sharded(bj.inverse(c_), x_, out=y_)), bps_f, Nc_))
                rows.append((f"RQS-cols vjp_params(coupling) {form} {tag} (x̄ + per-column cotangents)", "cols", (lambda c_=cb_, x_=xq, g_=gy, l_=lq: bj.vjp_params(c_, x_, g_, l_)), bps_v, Nc_))
                rows.append((f"RQS-cols vjp_params(inverse(coupling)) {form} {tag} (x̄ + per-column cotangents)", "cols", (lambda c_=cb_, x_=xq, g_=gy, l_=lq: bj.vjp_params(bj.inverse(c_), x_, g_, l_)), bps_v, Nc_))
            torch_cols.append((tag, xq, rwq, rhq, rdq, Bc, n1c, P["raw"] + 2 * d * es + es, Nc_))

    # Coupling with a per-sample elementwise-chain law (include/bjx_coupling.h): dim 64, half mask (n1 = 32), Float32.  The yardstick
    # is the affine law Shift ∘ Scale with per-sample parameters on the existing kernels (bjx_coupling_affine / _vjp); the same law as
    # ONE affine stage of bjx_coupling_chain / _vjp is called through the C entry (the Python Coupling keeps the affine entries for it).
    # Algorithmic bytes: x read and y written for every row, the per-sample log-det, every per-sample parameter value once; the
    # pullback reads x, ȳ, ℓ̄ and the parameters and writes x̄ and one cotangent per parameter value.
    if not only_given(a.only) or "Coupling-chain" in a.only:
        n1c = 32
        I = bj.interface
        gq = torch.Generator(device=dev).manual_seed(11)
        head = torch.randn((N, 4 * n1c), dtype=f32, device=dev, generator=gq).T                       # one network head: s1, t1, s2, t2
        sc1, sh1 = 0.5 + torch.sigmoid(head[:n1c].T).T, 0.5 * head[n1c:2 * n1c]
        sc2, sh2 = 0.5 + torch.sigmoid(head[2 * n1c:3 * n1c].T).T, 0.5 * head[3 * n1c:]
        del head
        gyc = randn(d, N, dev, 5)
        lqc = torch.randn(N, dtype=f32, device=dev, generator=gq)
        maskc = bj.PartitionMask(d, list(range(1, n1c + 1)))
        aff = lambda: bj.Shift(sh1) @ bj.Scale(sc1, batched=True)
        laws = {
            "affine Shift∘Scale": (aff(), x, 2),
            "gated inverse(Logit(0,1))∘Shift∘Scale∘Logit(0,1)": (bj.inverse(bj.Logit(0.0, 1.0)) @ aff() @ bj.Logit(0.0, 1.0), xunit, 2),
            "exp∘Shift∘Scale": (e(bj.exp) @ aff(), x, 2),
            "inverse(Logit(-1,2))∘Shift∘Scale": (bj.inverse(bj.Logit(-1.0, 2.0)) @ aff(), x, 2),
            "LeakyReLU(0.2)∘Shift∘Scale": (bj.LeakyReLU(0.2) @ aff(), x, 2),
            "Shift∘Scale∘LeakyReLU(0.3)∘Shift∘Scale": (bj.Shift(sh2) @ bj.Scale(sc2, batched=True) @ bj.LeakyReLU(0.3) @ aff(), x, 4),
        }
        idx1c = maskc.idx1_dev(dev)
        for lname, (law, xin, npar) in laws.items():
            bps_f = 4 * (2 * d + 1 + npar * n1c)
            bps_v = 4 * (3 * d + 1 + 2 * npar * n1c)
            cplc = bj.Coupling((lambda l_: (lambda x2: l_))(law), maskc)
            yc = torch.empty_like(xin)
            kern = "bjx_coupling_affine" if lname.startswith("affine") else "bjx_coupling_chain"
            rows.append((f"Coupling-chain {lname} [{kern}]", "chain", (lambda c_=cplc, y_=yc, x_=xin: bj.shard.with_logabsdet_jacobian_sharded(c_, x_, out=y_)), bps_f, N))
            yin = bj.transform(cplc, xin)
            rows.append((f"Coupling-chain inverse: {lname} [{kern}]", "chain", (lambda c_=cplc, y_=yc, x_=yin: bj.shard.with_logabsdet_jacobian_sharded(bj.inverse(c_), x_, out=y_)), bps_f, N))
            rows.append((f"Coupling-chain vjp_params: {lname} [{kern}_vjp]", "chain", (lambda c_=cplc, x_=xin, g_=gyc, l_=lqc: bj.vjp_params(c_, x_, g_, l_)), bps_v, N))
            if lname.startswith("affine"):
                # the same law on the new kernels, through the C entries
                m = I._ChainLaw(law, x, n1c, N, False)
                ctxc = bj.context(dev)
                libc = bj._lib.load()
                psc = torch.empty(N, dtype=f32, device=dev)
                xbc = torch.empty_like(x)
                barsc = [torch.empty((N, n1c), dtype=f32, device=dev).T for _ in range(2)]
                pbars = (C.c_void_p * 2)(*[b_.data_ptr() for b_ in barsc])

                def fwd_c(inv, xi, m=m, yc=yc, psc=psc):
                    bj._lib.check(ctxc.h, libc.bjx_coupling_chain(ctxc.h, 0, inv, I._ptr(idx1c), n1c, m.ops, m.n, m.params, m.lds, I._ptr(xi), I._ptr(yc), I._ptr(psc), None, d, N, 0), "bjx_coupling_chain")

                def vjp_c(m=m):
                    bj._lib.check(ctxc.h, libc.bjx_coupling_chain_vjp(ctxc.h, 0, 0, I._ptr(idx1c), n1c, m.ops, m.n, m.params, m.lds, I._ptr(x), I._ptr(gyc), I._ptr(lqc), I._ptr(xbc), pbars, d, N),
                                  "bjx_coupling_chain_vjp")
                rows.append((f"Coupling-chain {lname} [bjx_coupling_chain, one affine stage]", "chain", (lambda: fwd_c(0, x)), bps_f, N))
                rows.append((f"Coupling-chain inverse: {lname} [bjx_coupling_chain, one affine stage]", "chain", (lambda yin=yin: fwd_c(1, yin)), bps_f, N))
                rows.append((f"Coupling-chain vjp_params: {lname} [bjx_coupling_chain_vjp, one affine stage]", "chain", vjp_c, bps_v, N))

    only = [s for s in a.only.split(",") if s]
    L, ctx = bj._lib, bj.context(dev)
    lib = L.load()
    # "kernel": the launch(es) inside the library's profiling scope; "stream": one event pair around all the calls of a separate
    # pass — helper launches (parameter preparation, finalize) and gaps included
    print("| row | §8(a) | kernel ms | samples | alg. B/sample | GB/s | % of 8 TB/s | stream ms | % of 8 TB/s by stream region |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, ref, step, bps, n in rows:
        if only and not any(o in name for o in only):
            continue
        try:
            if step in cached_rows:
                with bj.cache_params():
                    k, reg = kernel_and_region_ms(bj, step, steps=a.steps, device=dev)
            else:
                k, reg = kernel_and_region_ms(bj, step, steps=a.steps, device=dev)
            gbs = bps * n / (k * 1e-3) / 1e9
            gbr = bps * n / (reg * 1e-3) / 1e9
            print(f"| {name} | {ref} | {k:.4f} | 2^{int(math.log2(n))} | {bps} | {gbs:.0f} | {100 * gbs / PEAK:.1f} | {reg:.4f} | {100 * gbr / PEAK:.1f} |", flush=True)
        except Exception as ex:  # keep the table going
            print(f"| {name} | {ref} | failed: {ex!r} | | | | | | |", flush=True)
    for tag, xq, rwq, rhq, rdq, Bc, n1c, bps, n in torch_cols:
        if only and not any(o in "torch-spline" for o in only) and not any("RQS-cols" in o for o in only):
            continue
        ms = torch_spline_ms(xq, rwq, rhq, rdq, Bc, n1c, a.steps)
        gbs = bps * n / (ms * 1e-3) / 1e9
        print(f"| torch-spline: plain PyTorch batched spline coupling, raw form {tag} (softmax / cumsum / searchsorted / gather) | cols | | 2^{int(math.log2(n))} | {bps} | {gbs:.0f} | {100 * gbs / PEAK:.1f} | {ms:.4f} | {100 * gbs / PEAK:.1f} |", flush=True)


def only_given(s):
    return bool([t for t in s.split(",") if t])


def torch_spline_forward(x, rw, rh, rd, B, n1):
    """The forward coupling with per-column raw spline parameters in plain PyTorch (what a user writes without bjx_rqs_cols)."""
    x1 = x[:n1].T                                             # (N, n1)
    def knots(r):
        c = torch.cumsum(torch.softmax(r.permute(2, 0, 1).contiguous(), dim=-1), dim=-1)        # (N, n1, K)
        return torch.cat([torch.zeros_like(c[..., :1]), c], dim=-1) * (2 * B) - B
    w, h = knots(rw), knots(rh)
    one = torch.ones_like(w[..., :1])
    dd = torch.cat([one, torch.nn.functional.softplus(rd.permute(2, 0, 1).contiguous()), one], dim=-1)
    inside = (x1 > -B) & (x1 < B)
    k = torch.searchsorted(w.contiguous(), x1.unsqueeze(-1).contiguous()).clamp(1, w.shape[-1] - 1)
    g = lambda t, i: torch.gather(t, -1, i).squeeze(-1)
    wl, wu, hl, hu, dl, du = g(w, k - 1), g(w, k), g(h, k - 1), g(h, k), g(dd, k - 1), g(dd, k)
    wd, dy = wu - wl, hu - hl
    s = dy / wd
    xi = (x1 - wl) / wd
    om = 1 - xi
    den = s + (du + dl - 2 * s) * xi * om
    y1 = hl + dy * (s * xi * xi + dl * xi * om) / den
    lj = torch.log(s * s * (du * xi * xi + 2 * s * xi * om + dl * om * om)) - 2 * torch.log(den)
    y = x.clone()
    y[:n1] = torch.where(inside, y1, x1).T
    return y, torch.where(inside, lj, torch.zeros_like(lj)).sum(-1)


def torch_spline_ms(x, rw, rh, rd, B, n1, steps, chunk=1 << 16):
    """Stream time of the plain-PyTorch coupling, in slices of `chunk` columns (torch.cumsum rejects one launch over 2^25 rows)."""
    def run():
        for c0 in range(0, x.shape[1], chunk):
            sl = slice(c0, c0 + chunk)
            torch_spline_forward(x[:, sl], rw[:, :, sl], rh[:, :, sl], rd[:, :, sl], B, n1)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


if __name__ == "__main__":
    main()
