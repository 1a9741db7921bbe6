#!/usr/bin/env python
"""The amortised radial flow (include/bjx_radial_cols.h, `AmortizedRadialLayer`) against the same computation written in plain torch
ops, on one GPU, in one process: forward map, inverse map, forward pullback and inverse pullback (both with the per-column ᾱ_, β̄,
z̄₀), at dim ∈ {2, 16, 64, 256, 1 024} x L ∈ {1, 8} in Float32 and half of those shapes in Float64, with the batch chosen so that
the parameters are about 1 GiB.  Beside every shape: `bjx_planar_cols` (`AmortizedPlanarLayer`) at the same dim, L and batch — the
same geometry with twice the parameter bytes — and, for the inverse parameter pullback, the three-launch composition the one launch
replaces (inverse map, inverse `vjp`, forward `vjp_params` at the pre-image with (−ȳ, −ℓ̄)).

Per shape and operation the kernel and the torch composition ALTERNATE, `--repeats` (7) times, each repeat timing `--inner` calls
between two device events; the table gives the median time per call with the smallest and largest repeat, the fraction of the
8 TB/s HBM peak from the bytes the operation needs (derived from the shape, below), and torch time / kernel time.  The torch
composition gets the layout it likes best (the batch fastest: every z₀_k a contiguous (dim, batch) matrix), softplus / multiply-and-sum
/ sqrt per layer; its inverse is the closed form (compute_r); its pullbacks are autograd through those compositions.

Bytes per column (T = element size): maps (2·dim + L·dim + 2L + 1)·T — x in, y out, the parameters, the log-det out; pullbacks
(3·dim + 1 + 2·(L·dim + 2L))·T — x, ȳ, ℓ̄ in, x̄ out, the parameters read and their cotangents written; z₀ is counted once (its second
read goes through the caches), y and the log-det are not written by a pullback.

    python scripts/bench_radial_cols.py [--gib 1.0] [--repeats 7] [--inner 3] [--out table.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bijectors_amd as bj  # noqa: E402

SHAPES = {torch.float32: [(d, L) for d in (2, 16, 64, 256, 1024) for L in (1, 8)],
          torch.float64: [(2, 8), (16, 1), (64, 8), (256, 1), (512, 8)]}          # 1 024 rows are above the Float64 limit: 512 in their place
PEAK = 8e12


def softplus(x):
    return torch.nn.functional.softplus(x)


def torch_forward(a, b, z0, z):
    """a, b: (L, batch); z0: (L, dim, batch) contiguous; z: (dim, batch) batch-fastest."""
    d = z.shape[0]
    ladj = torch.zeros(z.shape[1], dtype=z.dtype, device=z.device)
    for k in range(z0.shape[0]):
        al = softplus(a[k])
        bh = softplus(b[k]) - al
        dl = z - z0[k]
        r = (dl * dl).sum(0).sqrt()
        h = 1 / (al + r)
        z = z + bh * h * dl
        ladj = ladj + (d - 1) * torch.log1p(bh * h) + torch.log1p(bh * h - bh * h * h * r)
    return z, ladj


def torch_inverse(a, b, z0, y):
    d = y.shape[0]
    ladj = torch.zeros(y.shape[1], dtype=y.dtype, device=y.device)
    for k in range(z0.shape[0] - 1, -1, -1):
        al, apb = softplus(a[k]), softplus(b[k])
        bh = apb - al
        dl = y - z0[k]
        gam = (dl * dl).sum(0).sqrt()
        aa = apb - gam
        r = ((aa * aa + 4 * al * gam).sqrt() - aa) / 2
        y = z0[k] + (al + r) / (apb + r) * dl
        h = 1 / (al + r)
        ladj = ladj - (d - 1) * torch.log1p(bh * h) - torch.log1p(bh * h - bh * h * h * r)
    return y, ladj


def torch_pullback(fn, a, b, z0, z, g, lb):
    a, b, z0, z = (t.detach().requires_grad_(True) for t in (a, b, z0, z))
    y, l = fn(a, b, z0, z)
    return torch.autograd.grad([y, l], [z, a, b, z0], [g, lb])


def three_launches(layer, y, xbar, lb):
    """The composition the one-launch inverse parameter pullback replaces (what `_vjp_params_inverse` does for the planar sibling)."""
    inv = bj.inverse(layer)
    x = bj.transform(inv, y)
    yb = bj.vjp(inv, y, xbar, lb)
    _, grads = bj.vjp_params(layer, x, -yb, -lb)
    return yb, grads


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def alternate(kern, ref, repeats, inner):
    """-> (median, min, max) ms of the kernel and the median ms of `ref` (None: nothing to alternate with)."""
    kern()
    if ref:
        ref()
    torch.cuda.synchronize()
    tk, tr = [], []
    for _ in range(repeats):
        tk.append(timed(kern, inner) * 1e3)
        if ref:
            tr.append(timed(ref, 1) * 1e3)
    return statistics.median(tk), min(tk), max(tk), (statistics.median(tr) if ref else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0, help="size of the parameters (alpha_, beta, z_0) of one shape")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radial_cols.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; parameters {args.gib:g} GiB per shape; median (min – max) of {args.repeats} alternating repeats of "
             f"{args.inner} calls", "",
             "| dtype | dim x L | batch | operation | kernel ms (min – max) | % of 8 TB/s | compared with | its ms | its ms / kernel ms |", "|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, L in SHAPES[dt]:
            per_col = (dim * L + 2 * L) * T
            batch = max(1, int(args.gib * 2 ** 30 / per_col))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim)
            # the torch layout (L, dim, batch), and the kernel's: column-major per column, [r + k*dim + n*dim*L]
            at = 0.5 * torch.randn((L, batch), dtype=dt, device=dev, generator=gen)
            bt = torch.randn((L, batch), dtype=dt, device=dev, generator=gen)
            z0t = 0.3 * torch.randn((L, dim, batch), dtype=dt, device=dev, generator=gen)
            zt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            gt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            lbt = torch.randn(batch, dtype=dt, device=dev, generator=gen)
            ak, bk = at.T.contiguous().T, bt.T.contiguous().T
            z0k = z0t.permute(2, 0, 1).contiguous().permute(2, 1, 0)        # (dim, L, batch) view of a (batch, L, dim) array
            zk, gk = zt.T.contiguous().T, gt.T.contiguous().T
            layer = bj.AmortizedRadialLayer(ak, bk, z0k)
            inv = bj.inverse(layer)
            yk = bj.transform(layer, zk)
            yt = yk.contiguous()
            map_bytes = (2 * dim + L * dim + 2 * L + 1) * T * batch
            vjp_bytes = (3 * dim + 1 + 2 * (L * dim + 2 * L)) * T * batch
            ops = [("forward map", lambda: bj.with_logabsdet_jacobian(layer, zk, per_sample=True), "torch", lambda: torch_forward(at, bt, z0t, zt), map_bytes),
                   ("inverse map", lambda: bj.with_logabsdet_jacobian(inv, yk, per_sample=True), "torch", lambda: torch_inverse(at, bt, z0t, yt), map_bytes),
                   ("forward pullback", lambda: bj.vjp_params(layer, zk, gk, lbt), "torch", lambda: torch_pullback(torch_forward, at, bt, z0t, zt, gt, lbt), vjp_bytes),
                   ("inverse pullback", lambda: bj.vjp_params(inv, yk, gk, lbt), "torch", lambda: torch_pullback(torch_inverse, at, bt, z0t, yt, gt, lbt), vjp_bytes),
                   ("inverse pullback", lambda: bj.vjp_params(inv, yk, gk, lbt), "three launches", lambda: three_launches(layer, yk, gk, lbt), vjp_bytes)]
            for what, kern, other, ref, nbytes in ops:
                k_ms, k_lo, k_hi, r_ms = alternate(kern, ref, args.repeats, args.inner)
                emit(f"| {name} | {dim} x {L} | {batch} | {what} | {k_ms:.3f} ({k_lo:.3f} – {k_hi:.3f}) | {100 * nbytes / (k_ms * 1e-3) / PEAK:.1f} | {other} | {r_ms:.2f} | "
                     f"{r_ms / k_ms:.1f}{'' if r_ms >= k_ms else ' (SLOWER than ' + other + ')'} |")
            del at, bt, z0t, yt, layer, inv, ak, bk, z0k
            torch.cuda.empty_cache()
            # the planar sibling at the same dim, L and batch: twice the parameter bytes
            s = 0.8 * dim ** -0.25
            wk = (s * torch.randn((batch, L, dim), dtype=dt, device=dev, generator=gen)).permute(2, 1, 0)
            uk = (s * torch.randn((batch, L, dim), dtype=dt, device=dev, generator=gen)).permute(2, 1, 0)
            pk = torch.randn((batch, L), dtype=dt, device=dev, generator=gen).T
            planar = bj.AmortizedPlanarLayer(wk, uk, pk)
            p_map = (2 * dim * L + L + 2 * dim + 1) * T * batch
            p_vjp = (3 * dim + 1 + 2 * (2 * dim * L + L)) * T * batch
            for what, kern, nbytes in (("planar_cols forward map", lambda: bj.with_logabsdet_jacobian(planar, zk, per_sample=True), p_map),
                                       ("planar_cols inverse map", lambda: bj.with_logabsdet_jacobian(bj.inverse(planar), yk, per_sample=True), p_map),
                                       ("planar_cols forward pullback", lambda: bj.vjp_params(planar, zk, gk, lbt), p_vjp)):
                k_ms, k_lo, k_hi, _ = alternate(kern, None, args.repeats, args.inner)
                emit(f"| {name} | {dim} x {L} | {batch} | {what} | {k_ms:.3f} ({k_lo:.3f} – {k_hi:.3f}) | {100 * nbytes / (k_ms * 1e-3) / PEAK:.1f} | — | — | — |")
            del wk, uk, pk, planar, zt, gt, lbt, zk, gk, yk
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
