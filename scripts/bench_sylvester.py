#!/usr/bin/env python
"""The shared Sylvester layer (include/bjx_sylvester.h, `SylvesterLayer`) against two baselines, on one GPU, in one process: the map
with its per-column log-det, `vjp` and `vjp_params` at dim ∈ {2, 16, 64, 256, 1 024 (Float64: 512)} x M ∈ {1, 4, 16} (M <= dim) in both
dtypes.  The batch is sized to what the workaround can hold: its expanded parameters (Q, R, R̃, b per column) are about `--gib` GiB.

Baselines, alternating with the new path, `--repeats` (7) times each; the table gives the median with the smallest and largest repeat:
  workaround   what a user of the parent commit had: the parameters expanded to (dim, M, batch), (M, M, batch), (M, batch),
               `AmortizedSylvesterLayer` (bjx_sylvester_cols / bjx_sylvester_cols_vjp, unchanged entries) and, for `vjp_params`, a torch sum
               of the per-column cotangents over the batch.  The expansion itself is done ONCE outside the timing (in training it would be
               paid on every step): the comparison favours the workaround.
  torch        the same computation in plain torch ops on the layout torch likes best (the batch fastest), the four products written as
               broadcast multiply-and-sum, NOT as batched matrix products (the sibling's script met a GPU memory fault with batched
               products over tens of millions of columns, LAB_NOTEBOOK.md); the pullbacks are autograd through that composition.

Algorithmic bytes per column (T = element size): the map 2·dim·T (z in, y out), the pullbacks 3·dim·T (z, ȳ in, z̄
out); the shared parameters are dim·M + 2M² + M elements in all and are not counted, nor are the per-column log-det and its cotangent.
"launches" is the library's own count (bjx_launch_count) of one call of the new path; "fallback" marks the `vjp_params` rows whose
shape is over the LDS rule (BJX_SYLVESTER_LDS_BYTES(dim, M) > 64 KiB) and takes the host's chunked path.

    python scripts/bench_sylvester.py [--gib 2.0] [--repeats 7] [--inner 3] [--out profiles/r19_sylvester.md]
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


def torch_forward(q, r, rt, b, mask, z):
    """q: (dim, M), r, rt: (M, M), b: (M,), z: (dim, batch) batch-fastest; mask: (M, M) upper triangle.  Multiply-and-sum throughout."""
    s = (q[:, :, None] * z[:, None, :]).sum(0)
    t = ((rt * mask)[:, :, None] * s[None, :, :]).sum(1) + b[:, None]
    a = torch.tanh(t)
    p = ((r * mask)[:, :, None] * a[None, :, :]).sum(1)
    y = z + (q[:, :, None] * p[None, :, :]).sum(1)
    d = 1 + (1 - a * a) * (torch.diagonal(rt) * torch.diagonal(r))[:, None]
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
    return e0.elapsed_time(e1) / inner


def alternate(fns, repeats):
    """fns: [(callable, calls per repeat)] -> [(median, min, max) ms per call], the callables taking turns within every repeat."""
    for f, _ in fns:
        f()
        torch.cuda.synchronize()                        # an error names its side
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, (f, n) in enumerate(fns):
            ts[i].append(timed(f, n))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0, help="size of the workaround's expanded parameters of a shape")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sylvester.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lib = bj._lib.load()
    lines = [f"device: {torch.cuda.get_device_name(0)}; expanded parameters of the workaround {args.gib:g} GiB; median (min – max) of {args.repeats} alternating "
             f"repeats of {args.inner} calls (torch and the workaround: 1 call); the workaround's expansion is outside the timing", "",
             "| dtype | dim x M | batch | operation | path | launches | bytes / column | shared ms (min – max) | % of 8 TB/s | workaround ms (min – max) | "
             "workaround / shared | beats the workaround by more than the spread | torch ms (min – max) | torch / shared |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, M in SHAPES[dt]:
            per_col = dim * M + 2 * M * M + M
            batch = max(1, int(args.gib * 2 ** 30 / (per_col * T)))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim + M)
            q = torch.linalg.qr(torch.randn((dim, M), dtype=dt, generator=torch.Generator().manual_seed(dim + M)))[0].contiguous().to(dev)      # factored on the host
            r, rt = (torch.randn((M, M), dtype=dt, device=dev, generator=gen) / M ** 0.5 for _ in range(2))
            for t in (r, rt):
                t.diagonal().copy_(0.9 * torch.tanh(torch.randn(M, dtype=dt, device=dev, generator=gen)))
            b = 0.5 * torch.randn(M, dtype=dt, device=dev, generator=gen)
            mask = torch.triu(torch.ones((M, M), dtype=dt, device=dev))
            zt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)            # torch's layout: the batch fastest
            gt = torch.randn((dim, batch), dtype=dt, device=dev, generator=gen)
            lb = torch.randn(batch, dtype=dt, device=dev, generator=gen)
            zk, gk = zt.T.contiguous().T, gt.T.contiguous().T                              # the library's: column-major
            layer = bj.SylvesterLayer(q, r, rt, b)
            flow = bj.AmortizedSylvesterLayer(q.T.reshape(1, M, dim).expand(batch, M, dim).contiguous().permute(2, 1, 0),
                                              r.T.reshape(1, M, M).expand(batch, M, M).contiguous().permute(2, 1, 0),
                                              rt.T.reshape(1, M, M).expand(batch, M, M).contiguous().permute(2, 1, 0),
                                              b.reshape(1, M).expand(batch, M).contiguous().T)

            def wa_params():
                xb, gr = bj.vjp_params(flow, zk, gk, lb)
                return xb, gr["q"].sum(dim=2), gr["r"].sum(dim=2), gr["r_tilde"].sum(dim=2), gr["b"].sum(dim=1)

            fallback = bj._lib.sylvester_lds_bytes(dim, M) > bj._lib.BJX_SYLVESTER_LDS_BUDGET
            b_map, b_full = 2 * dim * T, 3 * dim * T
            ops = [("map", lambda: bj.with_logabsdet_jacobian(layer, zk, per_sample=True), lambda: bj.with_logabsdet_jacobian(flow, zk, per_sample=True),
                    lambda: torch_forward(q, r, rt, b, mask, zt), b_map, "fused"),
                   ("vjp", lambda: bj.vjp(layer, zk, gk, lb), lambda: bj.vjp(flow, zk, gk, lb), lambda: torch_pullback(q, r, rt, b, mask, zt, gt, lb, False), b_full,
                    "fused"),
                   ("vjp_params", lambda: bj.vjp_params(layer, zk, gk, lb), wa_params, lambda: torch_pullback(q, r, rt, b, mask, zt, gt, lb, True), b_full,
                    "fallback" if fallback else "fused")]
            for what, kern, wa, ref, nbytes, path in ops:
                kern()
                before = lib.bjx_launch_count()
                kern()
                launches = lib.bjx_launch_count() - before
                (k, klo, khi), (w, wlo, whi), (t_, tlo, thi) = alternate([(kern, args.inner), (wa, 1), (ref, 1)], args.repeats)
                beats = "yes" if khi < wlo else ("NO (within the spread)" if k < w else "NO (slower)")
                emit(f"| {name} | {dim} x {M} | {batch} | {what} | {path} | {launches} | {nbytes} | {k:.3f} ({klo:.3f} – {khi:.3f}) | "
                     f"{100 * nbytes * batch / (k * 1e-3) / PEAK:.1f} | {w:.3f} ({wlo:.3f} – {whi:.3f}) | {w / k:.2f} | {beats} | {t_:.2f} ({tlo:.2f} – {thi:.2f}) | {t_ / k:.1f} |")
            del zt, gt, zk, gk, lb, layer, flow
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
