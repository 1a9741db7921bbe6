#!/usr/bin/env python
"""The amortised Sylvester layer (include/bjx_sylvester_cols.h, `AmortizedSylvesterLayer`) against the same computation written in
plain torch ops — what a user has without it — on one GPU, in one process: the map with its per-column log-det, `vjp` and `vjp_params`,
at dim ∈ {2, 16, 64, 256, 1 024 (Float64: 512)} x M ∈ {1, 4, 16} (M <= dim) in both dtypes, with the batch chosen so that the
parameters (Q, R, R̃, b) are about 1 GiB.

Per shape and operation the kernel and the torch composition ALTERNATE, `--repeats` (7) times, each repeat timing `--inner` calls
between two device events; the table gives the median time per call with the smallest and largest repeat (the spread), the fraction
of the 8 TB/s HBM peak and of the ≈ 0.79 copy ceiling (README) from the bytes the operation needs (derived from the shape, below), and
torch time / kernel time.  The torch composition gets the layout it likes best (the batch fastest: Q a contiguous (dim, M, batch)
array): two products with Q, two with the masked triangles, tanh and the log of the diagonal terms; its pullbacks are autograd through
that composition (`vjp`: the gradient of the input alone).  The four products are `einsum`s (batched matrix products, one per column)
where the batch is at most 65 535 columns and broadcast multiply-and-sum above that: the first timing run ended in a GPU memory fault
at 2 x 1 with 53 687 091 columns, and a batched matrix product with that many batches is the supposed cause, so none is launched.
The kernel is synchronised before the torch composition starts, so that an error names its side.

Algorithmic bytes per column (T = element size): the map (2·dim + dim·M + 2M² + M)·T — z in, y out, Q, R, R̃, b, whole squares counted
although only the upper triangles are read; the full pullback (4·dim + 2·dim·M + 4M² + 2M + 1)·T — z, ȳ, ℓ̄ in, z̄ out, the parameters
read once (the second read of Q goes through the caches or stays in registers) and their cotangents written; `vjp`
(3·dim + dim·M + 2M² + M + 1)·T.  The per-column log-det output is left out.

    python scripts/bench_sylvester_cols.py [--gib 1.0] [--repeats 7] [--inner 3] [--out table.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bijectors_amd as bj  # noqa: E402

SHAPES = {torch.float32: [(d, M) for d in (2, 16, 64, 256, 1024) for M in (1, 4, 16) if M <= d],
          torch.float64: [(d, M) for d in (2, 16, 64, 256, 512) for M in (1, 4, 16) if M <= d]}        # 1 024 rows are above the Float64 limit
PEAK = 8e12
COPY = 0.79
BMM_MAX_BATCH = 65535


def torch_forward(q, r, rt, b, mask, z):
    """q: (dim, M, batch), r, rt: (M, M, batch), b: (M, batch), z: (dim, batch), all batch-fastest; mask: (M, M, 1) upper triangle."""
    if z.shape[1] <= BMM_MAX_BATCH:
        s = torch.einsum("rmn,rn->mn", q, z)
        t = torch.einsum("ijn,jn->in", rt * mask, s) + b
        a = torch.tanh(t)
        p = torch.einsum("ijn,jn->in", r * mask, a)
        y = z + torch.einsum("rmn,mn->rn", q, p)
    else:
        s = (q * z[:, None, :]).sum(0)
        t = ((rt * mask) * s[None, :, :]).sum(1) + b
        a = torch.tanh(t)
        p = ((r * mask) * a[None, :, :]).sum(1)
        y = z + (q * p[None, :, :]).sum(1)
    d = 1 + (1 - a * a) * torch.diagonal(rt, dim1=0, dim2=1).T * torch.diagonal(r, dim1=0, dim2=1).T
    return y, torch.log(torch.abs(d)).sum(0)


def torch_pullback(q, r, rt, b, mask, z, g, lb, params):
    z = z.detach().requires_grad_(True)
    if params:
        q, r, rt, b = (t.detach().requires_grad_(True) for t in (q, r, rt, b))
    y, l = torch_forward(q, r, rt, b, mask, z)
    return torch.autograd.grad([y, l], [z, q, r, rt, b] if params else [z], [g, lb])


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def alternate(kern, ref, repeats, inner):
    """-> (median, min, max) ms of the kernel and (median, min, max) ms of `ref`."""
    kern()
    torch.cuda.synchronize()
    ref()
    torch.cuda.synchronize()
    tk, tr = [], []
    for _ in range(repeats):
        tk.append(timed(kern, inner) * 1e3)
        tr.append(timed(ref, 1) * 1e3)
    return statistics.median(tk), min(tk), max(tk), (statistics.median(tr), min(tr), max(tr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0, help="size of the parameters (Q, R, R̃, b) of one shape")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--only", default=None, help="one shape, e.g. float32:2x1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sylvester_cols.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; parameters {args.gib:g} GiB per shape; median (min – max) of {args.repeats} alternating repeats of "
             f"{args.inner} calls (torch: 1 call)", "",
             "| dtype | dim x M | batch | operation | bytes / column | kernel ms (min – max) | % of 8 TB/s | % of the copy ceiling | torch | torch ms (min – max) | torch ms / kernel ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, M in SHAPES[dt]:
            if args.only and args.only != f"{name.lower()}:{dim}x{M}":
                continue
            per = dim * M + 2 * M * M + M
            batch = max(1, int(args.gib * 2 ** 30 / (per * T)))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim + M)
            qt = torch.randn((dim, M, batch), dtype=dt, device=dev, generator=gen) / dim ** 0.5
            rt_ = torch.randn((M, M, batch), dtype=dt, device=dev, generator=gen) / M ** 0.5
            rtt = torch.randn((M, M, batch), dtype=dt, device=dev, generator=gen) / M ** 0.5
            idx = torch.arange(M, device=dev)
            rt_[idx, idx] = 0.9 * torch.tanh(torch.randn((M, batch), dtype=dt, device=dev, generator=gen))
            rtt[idx, idx] = 0.9 * torch.tanh(torch.randn((M, batch), dtype=dt, device=dev, generator=gen))
            bt = 0.5 * torch.randn((M, batch), dtype=dt, device=dev, generator=gen)
            zt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            gt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            lbt = torch.randn(batch, dtype=dt, device=dev, generator=gen)
            mask = torch.triu(torch.ones((M, M), dtype=dt, device=dev))[:, :, None]
            # the kernel's layout: column-major per column
            qk, rk, rtk = (t.permute(2, 1, 0).contiguous().permute(2, 1, 0) for t in (qt, rt_, rtt))
            bk, zk, gk = (t.T.contiguous().T for t in (bt, zt, gt))
            layer = bj.AmortizedSylvesterLayer(qk, rk, rtk, bk)
            b_map = (2 * dim + per) * T
            b_vjp = (3 * dim + per + 1) * T
            b_full = (4 * dim + 2 * per + 1) * T
            ops = [("map", lambda: bj.with_logabsdet_jacobian(layer, zk, per_sample=True), lambda: torch_forward(qt, rt_, rtt, bt, mask, zt), b_map),
                   ("vjp", lambda: bj.vjp(layer, zk, gk, lbt), lambda: torch_pullback(qt, rt_, rtt, bt, mask, zt, gt, lbt, False), b_vjp),
                   ("vjp_params", lambda: bj.vjp_params(layer, zk, gk, lbt), lambda: torch_pullback(qt, rt_, rtt, bt, mask, zt, gt, lbt, True), b_full)]
            for what, kern, ref, nbytes in ops:
                k_ms, k_lo, k_hi, (r_ms, r_lo, r_hi) = alternate(kern, ref, args.repeats, args.inner)
                frac = nbytes * batch / (k_ms * 1e-3) / PEAK
                emit(f"| {name} | {dim} x {M} | {batch} | {what} | {nbytes} | {k_ms:.3f} ({k_lo:.3f} – {k_hi:.3f}) | {100 * frac:.1f} | {100 * frac / COPY:.1f} | "
                     f"{'einsum' if batch <= BMM_MAX_BATCH else 'mul + sum'} | {r_ms:.2f} ({r_lo:.2f} – {r_hi:.2f}) | {r_ms / k_ms:.1f}{'' if r_ms >= k_ms else ' (SLOWER than torch)'} |")
            del qt, rt_, rtt, bt, zt, gt, lbt, qk, rk, rtk, bk, zk, gk, layer
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
