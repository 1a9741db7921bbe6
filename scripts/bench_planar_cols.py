#!/usr/bin/env python
"""The amortised planar flow (include/bjx_planar_cols.h, `AmortizedPlanarLayer`) against the same computation written in plain torch
ops, on one GPU, in one process: forward map, inverse map and forward pullback (x̄ and the per-column w̄, ū, b̄), Float32 and Float64,
at dim x L = 2 x 8, 16 x 8, 64 x 8, 256 x 4 and 1 024 x 2, with the batch chosen so that the parameters are about 1 GiB.

Per shape and operation the kernel and the torch composition ALTERNATE, `--repeats` (7) times, each repeat timing `--inner` calls
between two device events; the table gives the median time per call, the fraction of the 8 TB/s HBM peak from the bytes the
operation needs (derived from the shape, below), and torch time / kernel time.  The torch composition gets the layout it likes best
(the batch fastest: every w_k, u_k a contiguous (dim, batch) matrix), multiply-and-sum / softplus / tanh per layer (einsum takes a
batched-GEMM path that is 20 times slower in Float32 at short columns); its inverse solves
find_alpha by the fixed-point start and six Newton steps; its pullback is autograd through the forward composition.

Bytes per column (T = element size): maps (2·dim·L + L + 2·dim + 1)·T — the parameters, x in, y and the log-det out;
pullback (2·(2·dim·L + L) + 3·dim + 1 + 2·dim·L + L + dim)·T — the parameters twice (both sweeps), x, ȳ, ℓ̄, x̄ and the three
parameter cotangents.

    python scripts/bench_planar_cols.py [--gib 1.0] [--repeats 7] [--inner 3] [--out table.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bijectors_amd as bj  # noqa: E402

SHAPES = [(2, 8), (16, 8), (64, 8), (256, 4), (1024, 2)]
PEAK = 8e12
LIMIT = {torch.float32: 1024, torch.float64: 512}


def softplus(x):
    return torch.nn.functional.softplus(x)


def torch_scalars(wk, uk):
    a = (wk * uk).sum(0)
    n2 = (wk * wk).sum(0)
    return (softplus(-a) - 1) / n2, softplus(a) - 1


def torch_forward(w, u, b, z):
    """w, u: (L, dim, batch) contiguous; b: (L, batch); z: (dim, batch) batch-fastest."""
    ladj = torch.zeros(z.shape[1], dtype=z.dtype, device=z.device)
    for k in range(w.shape[0]):
        kap, c = torch_scalars(w[k], u[k])
        t = torch.tanh((w[k] * z).sum(0) + b[k])
        z = z + (u[k] + kap * w[k]) * t
        ladj = ladj + torch.log1p(c * (1 - t * t))
    return z, ladj


def torch_inverse(w, u, b, y):
    ladj = torch.zeros(y.shape[1], dtype=y.dtype, device=y.device)
    for k in range(w.shape[0] - 1, -1, -1):
        kap, c = torch_scalars(w[k], u[k])
        wy = (w[k] * y).sum(0)
        a = wy - c * torch.tanh(wy + b[k])
        for _ in range(6):
            t = torch.tanh(a + b[k])
            a = a - (a + c * t - wy) / (1 + c * (1 - t * t))
        t = torch.tanh(a + b[k])
        y = y - (u[k] + kap * w[k]) * t
        ladj = ladj - torch.log1p(c * (1 - t * t))
    return y, ladj


def torch_pullback(w, u, b, z, g, lb):
    w, u, b, z = (t.detach().requires_grad_(True) for t in (w, u, b, z))
    y, l = torch_forward(w, u, b, z)
    return torch.autograd.grad([y, l], [z, w, u, b], [g, lb])


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0, help="size of the parameters (w, u, b) of one shape")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_planar_cols.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; parameters {args.gib:g} GiB per shape; median of {args.repeats} alternating repeats of {args.inner} calls",
             "", "| dtype | dim x L | batch | operation | kernel ms | % of 8 TB/s | torch ms | torch / kernel |", "|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, L in SHAPES:
            if dim > LIMIT[dt]:
                row = f"| {name} | {dim} x {L} | — | all | refused: dim above {LIMIT[dt]} rows | — | — | — |"
                lines.append(row)
                print(row, flush=True)
                continue
            per_col = (2 * dim * L + L) * T
            batch = max(1, int(args.gib * 2 ** 30 / per_col))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim)
            s = 0.8 * dim ** -0.25
            # the torch layout (L, dim, batch), and the kernel's: column-major per column, [r + k*dim + n*dim*L]
            wt = s * torch.randn((L, dim, batch), dtype=dt, device=dev, generator=gen)
            ut = s * torch.randn((L, dim, batch), dtype=dt, device=dev, generator=gen)
            bt = torch.randn((L, batch), dtype=dt, device=dev, generator=gen)
            zt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            gt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            lbt = torch.randn(batch, dtype=dt, device=dev, generator=gen)
            wk = wt.permute(2, 0, 1).contiguous().permute(2, 1, 0)          # (dim, L, batch) view of a (batch, L, dim) array
            uk = ut.permute(2, 0, 1).contiguous().permute(2, 1, 0)
            bk = bt.T.contiguous().T
            zk, gk = zt.T.contiguous().T, gt.T.contiguous().T
            layer = bj.AmortizedPlanarLayer(wk, uk, bk)
            inv = bj.inverse(layer)
            yk = bj.transform(layer, zk)
            yt = yk.contiguous()
            map_bytes = (2 * dim * L + L + 2 * dim + 1) * T * batch
            vjp_bytes = (2 * (2 * dim * L + L) + 3 * dim + 1 + 2 * dim * L + L + dim) * T * batch
            ops = [("forward map", lambda: bj.with_logabsdet_jacobian(layer, zk, per_sample=True), lambda: torch_forward(wt, ut, bt, zt), map_bytes),
                   ("inverse map", lambda: bj.with_logabsdet_jacobian(inv, yk, per_sample=True), lambda: torch_inverse(wt, ut, bt, yt), map_bytes),
                   ("forward pullback", lambda: bj.vjp_params(layer, zk, gk, lbt), lambda: torch_pullback(wt, ut, bt, zt, gt, lbt), vjp_bytes)]
            for what, kern, ref, nbytes in ops:
                kern(), ref()                                    # warm-up of both, then alternate
                torch.cuda.synchronize()
                tk, tr = [], []
                for _ in range(args.repeats):
                    tk.append(timed(kern, args.inner))
                    tr.append(timed(ref, 1))
                k_ms, r_ms = statistics.median(tk) * 1e3, statistics.median(tr) * 1e3
                row = (f"| {name} | {dim} x {L} | {batch} | {what} | {k_ms:.3f} | {100 * nbytes / (k_ms * 1e-3) / PEAK:.1f} | {r_ms:.2f} | "
                       f"{r_ms / k_ms:.1f}{'' if r_ms >= k_ms else ' (SLOWER than torch)'} |")
                lines.append(row)
                print(row, flush=True)
            del wt, ut, bt, zt, gt, lbt, wk, uk, bk, zk, gk, yk, yt, layer, inv
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
