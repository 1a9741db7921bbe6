#!/usr/bin/env python
"""The shared Householder layer (include/bjx_householder.h, `HouseholderLayer`) against two baselines, on one GPU, in one process:
forward map, inverse map and `vjp_params` in both directions at dim ∈ {2, 16, 64, 256, 1 024 (Float64: 512)} x L ∈ {1, 2, 8} in both
dtypes, with the batch chosen so that one data array (x) is about 1 GiB.

Baselines, alternating with the new path, `--repeats` (7) times each; the table gives the median with the smallest and largest repeat:
  torch        the same computation in plain torch ops on the layout torch likes best (the batch fastest); the pullback is autograd
               through that composition.
  workaround   what a user of the parent commit had: v expanded to (dim, L, batch), `AmortizedHouseholderFlow` (bjx_householder_cols /
               bjx_householder_cols_vjp, unchanged entries) and a torch sum of the per-column v̄ over the batch.  The expansion itself is
               done ONCE outside the timing (in training it would be paid on every step): the comparison favours the workaround.

Bytes per column (T = element size), derived from the shape: a map 2·dim·T (x in, y out), the full pullback 3·dim·T (x, ȳ in, x̄ out);
the shared V is L·dim elements in all and is not counted.  The workaround moves (2 + L)·dim·T and (3 + 2L)·dim·T.  "launches" is the
library's own count (bjx_launch_count) of one call of the new path.

    python scripts/bench_householder.py [--gib 1.0] [--repeats 7] [--inner 3] [--out profiles/r17_householder.md]
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


def torch_map(V, x, inverse):
    """V: (dim, L); x: (dim, batch) batch-fastest."""
    L = V.shape[1]
    z = x
    for k in (range(L - 1, -1, -1) if inverse else range(L)):
        vk = V[:, k:k + 1]
        z = z - (2 * (vk * z).sum(0) / (vk * vk).sum()) * vk
    return z


def torch_pullback(V, x, g, inverse):
    V = V.detach().requires_grad_(True)
    x = x.detach().requires_grad_(True)
    return torch.autograd.grad([torch_map(V, x, inverse)], [x, V], [g])


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fns, repeats, inner):
    """fns: [(callable, calls per repeat)] -> [(median, min, max) ms per call], the callables taking turns within every repeat."""
    for f, _ in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, (f, n) in enumerate(fns):
            ts[i].append(timed(f, n))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0, help="size of one data array (x) of a shape")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_householder.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lib = bj._lib.load()
    lines = [f"device: {torch.cuda.get_device_name(0)}; data {args.gib:g} GiB per array; median (min – max) of {args.repeats} alternating repeats of "
             f"{args.inner} calls (torch and the workaround: 1 call); the workaround's expansion of v is outside the timing", "",
             "| dtype | dim x L | batch | operation | launches | bytes / column | shared ms (min – max) | % of 8 TB/s | torch ms (min – max) | torch / shared | "
             "workaround ms (min – max) | workaround / shared | beats the workaround by more than the spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, L in SHAPES[dt]:
            batch = max(1, int(args.gib * 2 ** 30 / (dim * T)))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim)
            Vt = torch.randn((dim, L), dtype=dt, device=dev, generator=gen)
            xt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)            # torch's layout: the batch fastest
            gt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            xk, gk = xt.T.contiguous().T, gt.T.contiguous().T                              # the library's: column-major
            layer = bj.HouseholderLayer(Vt.T.contiguous().T)
            inv = bj.inverse(layer)
            ve = Vt.T.reshape(1, L, dim).expand(batch, L, dim).contiguous().permute(2, 1, 0)   # (dim, L, batch), column-major per column
            flow = bj.AmortizedHouseholderFlow(ve)
            finv = bj.inverse(flow)

            def wa_params(f):
                xb, gr = bj.vjp_params(f, xk, gk)
                return xb, gr["v"].sum(dim=2)

            b_map, b_full = 2 * dim * T, 3 * dim * T
            ops = [("forward map", lambda: bj.transform(layer, xk), lambda: torch_map(Vt, xt, False), lambda: bj.transform(flow, xk), b_map),
                   ("inverse map", lambda: bj.transform(inv, xk), lambda: torch_map(Vt, xt, True), lambda: bj.transform(finv, xk), b_map),
                   ("forward vjp_params", lambda: bj.vjp_params(layer, xk, gk), lambda: torch_pullback(Vt, xt, gt, False), lambda: wa_params(flow), b_full),
                   ("inverse vjp_params", lambda: bj.vjp_params(inv, xk, gk), lambda: torch_pullback(Vt, xt, gt, True), lambda: wa_params(finv), b_full)]
            for what, kern, ref, wa, nbytes in ops:
                before = lib.bjx_launch_count()
                kern()
                launches = lib.bjx_launch_count() - before
                (k, klo, khi), (r, rlo, rhi), (w, wlo, whi) = alternate([(kern, args.inner), (ref, 1), (wa, 1)], args.repeats, args.inner)
                beats = "yes" if khi < wlo else ("NO (within the spread)" if k < w else "NO (slower)")
                emit(f"| {name} | {dim} x {L} | {batch} | {what} | {launches} | {nbytes} | {k:.3f} ({klo:.3f} – {khi:.3f}) | {100 * nbytes * batch / (k * 1e-3) / PEAK:.1f} | "
                     f"{r:.2f} ({rlo:.2f} – {rhi:.2f}) | {r / k:.1f} | {w:.3f} ({wlo:.3f} – {whi:.3f}) | {w / k:.2f} | {beats} |")
            del Vt, xt, gt, xk, gk, layer, inv, ve, flow, finv
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
