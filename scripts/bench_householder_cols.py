#!/usr/bin/env python
"""The amortised Householder flow (include/bjx_householder_cols.h, `AmortizedHouseholderFlow`) against the same computation written in
plain torch ops, on one GPU, in one process: forward map, inverse map, `vjp` and `vjp_params` in both directions, head present
(log_scale and shift), at dim ∈ {2, 16, 64, 256, 1 024 (Float64: 512)} x L ∈ {1, 2, 8} in both dtypes, with the batch chosen so that
the parameters (v, log_scale, shift) are about 1 GiB.  Beside every shape, as context and not as a gate: the amortised radial kernels
(`AmortizedRadialLayer`) at the same dim, L and batch — the same v / z₀ bytes, but two softplus, a square root and the log-det's
logarithms per layer where a reflection has one division.

Per shape and operation the kernel and the torch composition ALTERNATE, `--repeats` (7) times, each repeat timing `--inner` calls
between two device events; the table gives the median time per call with the smallest and largest repeat, the fraction of the
8 TB/s HBM peak from the bytes the operation needs (derived from the shape, below), and torch time / kernel time.  The torch
composition gets the layout it likes best (the batch fastest: every v_k a contiguous (dim, batch) matrix): exp, multiply-and-sum and a
division per layer; its pullbacks are autograd through that composition (`vjp`: the gradient of the input alone).

Bytes per column (T = element size): maps (2 + L + 2)·dim·T — x in, y out, v, log_scale, shift; the full pullback (3 + 2L + 4)·dim·T —
x, ȳ in, x̄ out, the parameters read once (their second read goes through the caches) and their cotangents written; `vjp`
(3 + L + 1)·dim·T forwards (shift is not read) and (3 + L + 2)·dim·T for the inverse.  The per-column log-det and ℓ̄ are left out.

    python scripts/bench_householder_cols.py [--gib 1.0] [--repeats 7] [--inner 3] [--out table.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bijectors_amd as bj  # noqa: E402

SHAPES = {torch.float32: [(d, L) for d in (2, 16, 64, 256, 1024) for L in (1, 2, 8)],
          torch.float64: [(d, L) for d in (2, 16, 64, 256, 512) for L in (1, 2, 8)]}        # 1 024 rows are above the Float64 limit
PEAK = 8e12


def reflect(vk, z):
    return z - (2 * (vk * z).sum(0) / (vk * vk).sum(0)) * vk


def torch_forward(v, s, m, x):
    """v: (L, dim, batch) contiguous; s, m, x: (dim, batch) batch-fastest."""
    z = torch.exp(s) * x
    for k in range(v.shape[0]):
        z = reflect(v[k], z)
    return z + m, s.sum(0)


def torch_inverse(v, s, m, y):
    z = y - m
    for k in range(v.shape[0] - 1, -1, -1):
        z = reflect(v[k], z)
    return torch.exp(-s) * z, -s.sum(0)


def torch_pullback(fn, v, s, m, z, g, lb, params):
    z = z.detach().requires_grad_(True)
    if params:
        v, s, m = (t.detach().requires_grad_(True) for t in (v, s, m))
    else:
        s = s.detach().requires_grad_(True)          # the log-det needs a graph; only the input's gradient is asked for
    y, l = fn(v, s, m, z)
    return torch.autograd.grad([y, l], [z, v, s, m] if params else [z], [g, lb])


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def alternate(kern, ref, repeats, inner):
    """-> (median, min, max) ms of the kernel and (median, min, max) ms of `ref` (None: nothing to alternate with)."""
    kern()
    if ref:
        ref()
    torch.cuda.synchronize()
    tk, tr = [], []
    for _ in range(repeats):
        tk.append(timed(kern, inner) * 1e3)
        if ref:
            tr.append(timed(ref, 1) * 1e3)
    return statistics.median(tk), min(tk), max(tk), ((statistics.median(tr), min(tr), max(tr)) if ref else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0, help="size of the parameters (v, log_scale, shift) of one shape")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_householder_cols.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; parameters {args.gib:g} GiB per shape; median (min – max) of {args.repeats} alternating repeats of "
             f"{args.inner} calls (torch: 1 call)", "",
             "| dtype | dim x L | batch | operation | bytes / column | kernel ms (min – max) | % of 8 TB/s | compared with | its ms (min – max) | its ms / kernel ms |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, L in SHAPES[dt]:
            batch = max(1, int(args.gib * 2 ** 30 / ((L + 2) * dim * T)))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim)
            # the torch layout (L, dim, batch), and the kernel's: column-major per column, [r + k*dim + n*dim*L]
            vt = torch.randn((L, dim, batch), dtype=dt, device=dev, generator=gen)
            st = 0.5 * torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            mt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            zt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            gt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            lbt = torch.randn(batch, dtype=dt, device=dev, generator=gen)
            vk = vt.permute(2, 0, 1).contiguous().permute(2, 1, 0)          # (dim, L, batch) view of a (batch, L, dim) array
            sk, mk, zk, gk = (t.T.contiguous().T for t in (st, mt, zt, gt))
            flow = bj.AmortizedHouseholderFlow(vk, sk, mk)
            inv = bj.inverse(flow)
            yk = bj.transform(flow, zk)
            yt = yk.contiguous()
            b_map, b_full = (2 + L + 2) * dim * T, (3 + 2 * L + 4) * dim * T
            b_vf, b_vi = (3 + L + 1) * dim * T, (3 + L + 2) * dim * T
            ops = [("forward map", lambda: bj.with_logabsdet_jacobian(flow, zk, per_sample=True), lambda: torch_forward(vt, st, mt, zt), b_map),
                   ("inverse map", lambda: bj.with_logabsdet_jacobian(inv, yk, per_sample=True), lambda: torch_inverse(vt, st, mt, yt), b_map),
                   ("forward vjp", lambda: bj.vjp(flow, zk, gk, lbt), lambda: torch_pullback(torch_forward, vt, st, mt, zt, gt, lbt, False), b_vf),
                   ("inverse vjp", lambda: bj.vjp(inv, yk, gk, lbt), lambda: torch_pullback(torch_inverse, vt, st, mt, yt, gt, lbt, False), b_vi),
                   ("forward vjp_params", lambda: bj.vjp_params(flow, zk, gk, lbt), lambda: torch_pullback(torch_forward, vt, st, mt, zt, gt, lbt, True), b_full),
                   ("inverse vjp_params", lambda: bj.vjp_params(inv, yk, gk, lbt), lambda: torch_pullback(torch_inverse, vt, st, mt, yt, gt, lbt, True), b_full)]
            for what, kern, ref, nbytes in ops:
                k_ms, k_lo, k_hi, (r_ms, r_lo, r_hi) = alternate(kern, ref, args.repeats, args.inner)
                emit(f"| {name} | {dim} x {L} | {batch} | {what} | {nbytes} | {k_ms:.3f} ({k_lo:.3f} – {k_hi:.3f}) | {100 * nbytes * batch / (k_ms * 1e-3) / PEAK:.1f} | torch | "
                     f"{r_ms:.2f} ({r_lo:.2f} – {r_hi:.2f}) | {r_ms / k_ms:.1f}{'' if r_ms >= k_ms else ' (SLOWER than torch)'} |")
            del vt, st, mt, yt, flow, inv, vk, sk, mk
            torch.cuda.empty_cache()
            # context: the amortised radial kernels at the same dim, L and batch (the same z₀ bytes as v; scalars instead of the head)
            ak = (0.5 * torch.randn((batch, L), dtype=dt, device=dev, generator=gen)).T
            bk = torch.randn((batch, L), dtype=dt, device=dev, generator=gen).T
            z0k = (0.3 * torch.randn((batch, L, dim), dtype=dt, device=dev, generator=gen)).permute(2, 1, 0)
            radial = bj.AmortizedRadialLayer(ak, bk, z0k)
            rinv = bj.inverse(radial)
            r_map, r_vjp = (2 * dim + L * dim + 2 * L + 1) * T, (3 * dim + 1 + 2 * (L * dim + 2 * L)) * T
            for what, kern, nbytes in (("radial_cols forward map", lambda: bj.with_logabsdet_jacobian(radial, zk, per_sample=True), r_map),
                                       ("radial_cols inverse map", lambda: bj.with_logabsdet_jacobian(rinv, yk, per_sample=True), r_map),
                                       ("radial_cols forward vjp_params", lambda: bj.vjp_params(radial, zk, gk, lbt), r_vjp),
                                       ("radial_cols inverse vjp_params", lambda: bj.vjp_params(rinv, yk, gk, lbt), r_vjp)):
                k_ms, k_lo, k_hi, _ = alternate(kern, None, args.repeats, args.inner)
                emit(f"| {name} | {dim} x {L} | {batch} | {what} | {nbytes} | {k_ms:.3f} ({k_lo:.3f} – {k_hi:.3f}) | {100 * nbytes * batch / (k_ms * 1e-3) / PEAK:.1f} | — | — | — |")
            del ak, bk, z0k, radial, rinv, zt, gt, lbt, zk, gk, yk
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
