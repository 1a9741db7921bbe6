#!/usr/bin/env python
"""The inverse of the shared Sylvester layer (include/bjx_sylvester_inv.h, `SylvesterLayer(..., orthonormal=True)`) next to the forward
direction of the same layer and to plain torch ops, on one GPU, in one process: dim ∈ {2, 16, 64, 256, 1 024 (Float64: 512)} x
M ∈ {1, 4, 16} (M <= dim) in both dtypes, the batch of scripts/bench_sylvester.py (`--gib` GiB / ((dim·M + 2M² + M)·sizeof(T)) columns), so
the rows line up with profiles/r19_sylvester.md.  The data y is the layer's image of a unit-scale z.

Per shape, the paths of an operation alternate `--repeats` (7) times; the table gives the median with the smallest and largest repeat:
  map          inverse(layer) with its per-column log-det | the forward map of the same layer and batch (it moves the same 2·dim·sizeof(T)
               bytes per column: the yardstick for what the M root solves cost) | the same inverse in plain torch ops
  vjp          vjp(inverse(layer)) | vjp(layer) | torch autograd through the torch inverse
  vjp_params   vjp_params(inverse(layer)) | vjp_params(layer) | torch autograd with the parameters
  logpdf       logpdf_vjp_params(transformed(MvNormal(dim), layer), y), the whole call
torch: the back-substitution on the layout torch likes best (the batch fastest), products as broadcast multiply-and-sum, every scalar
equation by the fixed-point start and a FIXED number of Newton steps — the smallest count (1 … 12) whose z meets the test bar (1e-3
Float32 / 1e-6 Float64 of the column's scale against the z the data was made from) on the first 65 536 columns of that shape; the count is
a column of the table.  Its pullbacks are autograd through that composition.

Algorithmic bytes per column (T = element size): map and logpdf 2·dim·T (y in, z or ȳ out), the pullbacks 3·dim·T (y, z̄ in, ȳ out).  The
inverse's `vjp_params` moves more than that: z is written by the first launch and read, with ȳ, by the forward parameter pullback.
"launches" is the library's own count (bjx_launch_count) of one call.

    python scripts/bench_sylvester_inv.py [--gib 2.0] [--repeats 7] [--inner 3] [--out table.md]
    python scripts/bench_sylvester_inv.py --table table.md --registers build.log --out profiles/r20_sylvester_inv.md

The second form measures nothing: it joins a measured table with the compiler's resource report (the stderr of a build of
bjx_sylvester_inv.hip with -Rpass-analysis=kernel-resource-usage added to HIPFLAGS) and, per instantiation, the waves per SIMD of the
forward sibling from profiles/r19_sylvester.md."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12
BAR = {"Float32": 1e-3, "Float64": 1e-6}


def registers(log, sibling):
    """The resource report of every instantiation as a table; `sibling`: profiles/r19_sylvester.md, for the forward kernels' waves."""
    fwd = {}
    if sibling and os.path.exists(sibling):
        for m in re.finditer(r"^\| (map|vjp) \| (f32|f64) \| (\d) \| (vec|elem) \| (\d+) \|.*\| (\d+) \|$", open(sibling).read(), flags=re.M):
            fwd[m.group(1, 2, 3, 4, 5)] = m.group(6)
    rows, bad = [], []
    for blk in re.split(r"remark: Function Name: ", open(log).read())[1:]:
        m = re.match(r"\S*sylvester_inv(_vjp)?_kernelI([fd])Li\d+ELi(\d+)ELb([01])ELi(\d+)E", blk)
        if not m:
            continue
        get = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        kern, T, R, form, MP = "vjp" if m.group(1) else "map", "f32" if m.group(2) == "f" else "f64", m.group(3), "vec" if m.group(4) == "1" else "elem", m.group(5)
        v, a, s, scr, vs, ss, occ = (get(k) for k in ("VGPRs", "AGPRs", "SGPRs", r"ScratchSize \[bytes/lane\]", "VGPRs Spill", "SGPRs Spill", r"Occupancy \[waves/SIMD\]"))
        if scr or vs:
            bad.append((kern, T, R, form, MP))
        rows.append((kern, T, int(R), form, int(MP), f"| {kern} | {T} | {R} | {form} | {MP} | {v}{' + ' + str(a) if a else ''} | {s} | {vs}/{ss} | {scr} | {occ} | "
                     f"{fwd.get((kern, T, R, form, MP), '—')} |"))
    rows.sort(key=lambda r: (r[0], r[1], r[3] != "vec", r[2], r[4]))
    head = ["## Registers (compiler resource report, gfx950)", "",
            f"`sylvester_inv_kernel` / `sylvester_inv_vjp_kernel<T, V, R, AL, MP>`: {len(rows)} instantiations.  "
            + ("No instantiation uses scratch or spills a vector register; " if not bad else f"SCRATCH OR VECTOR SPILLS in {bad}; ")
            + "scalar registers spill to vector lanes (column S of `spills V/S`), as in the forward sibling.  VGPRs are arch + accumulation registers "
            "where the allocation runs into the second file.  The last column is the forward sibling's kernel of the same instantiation "
            "(`sylvester_map_kernel` / `sylvester_vjp_kernel`, profiles/r19_sylvester.md).", "",
            "| kernel | T | R | form | MP | VGPRs | SGPRs | spills V/S | scratch B | waves/SIMD | forward sibling waves/SIMD |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    return head + [r[5] for r in rows]


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    import bijectors_amd as bj

    if not torch.cuda.is_available():
        raise SystemExit("bench_sylvester_inv.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lib = bj._lib.load()
    shapes = {torch.float32: [(d, M) for d in (2, 16, 64, 256, 1024) for M in (1, 4, 16) if M <= d],
              torch.float64: [(d, M) for d in (2, 16, 64, 256, 512) for M in (1, 4, 16) if M <= d]}

    def torch_inverse(q, r, rt, b, y, steps):
        """q (dim, M), r, rt (M, M), b (M,), y (dim, batch) batch-fastest -> z, ladj of the inverse."""
        M = q.shape[1]
        sp = (q[:, :, None] * y[:, None, :]).sum(0)
        s, a = [None] * M, [None] * M
        ladj = 0
        for m in range(M - 1, -1, -1):
            c, rho = b[m], sp[m]
            for j in range(m + 1, M):
                c = c + rt[m, j] * s[j]
                rho = rho - r[m, j] * a[j]
            k, w = r[m, m] * rt[m, m], rt[m, m] * rho
            al = w - k * torch.tanh(w + c)
            for _ in range(steps):
                t = torch.tanh(al + c)
                al = al - (al + k * t - w) / (1 + k * (1 - t * t))
            a[m] = torch.tanh(al + c)
            s[m] = rho - r[m, m] * a[m]
            ladj = ladj - torch.log(torch.abs(1 + (1 - a[m] * a[m]) * k))
        return y - (q[:, :, None] * (sp - torch.stack(s))[None, :, :]).sum(1), ladj

    def torch_pullback(q, r, rt, b, y, g, lb, steps, params):
        y = y.detach().requires_grad_(True)
        if params:
            q, r, rt, b = (t.detach().requires_grad_(True) for t in (q, r, rt, b))
        z, l = torch_inverse(q, r, rt, b, y, steps)
        return torch.autograd.grad([z, l], [y, q, r, rt, b] if params else [y], [g, lb])

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def alternate(fns):
        for f, _ in fns:
            f()
            torch.cuda.synchronize()                        # an error names its side
        ts = [[] for _ in fns]
        for _ in range(args.repeats):
            for i, (f, n) in enumerate(fns):
                ts[i].append(timed(f, n))
        return [(statistics.median(t), min(t), max(t)) for t in ts]

    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} – {t[2]:.3f})"
    lines = [f"device: {torch.cuda.get_device_name(0)}; batch as in scripts/bench_sylvester.py at {args.gib:g} GiB; median (min – max) of {args.repeats} alternating "
             f"repeats of {args.inner} calls (torch: 1 call)", "",
             "| dtype | dim x M | batch | operation | launches | bytes / column | inverse ms (min – max) | % of 8 TB/s | forward ms (min – max) | inverse / forward | "
             "torch Newton steps | torch ms (min – max) | torch / inverse |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    def emit(row):
        lines.append(row)
        print(row, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for dt in (torch.float32, torch.float64):
        T = torch.empty(0, dtype=dt).element_size()
        name = "Float32" if dt == torch.float32 else "Float64"
        for dim, M in shapes[dt]:
            batch = max(1, int(args.gib * 2 ** 30 / ((dim * M + 2 * M * M + M) * T)))
            gen = torch.Generator(device=dev).manual_seed(1234 + dim + M)
            q = torch.linalg.qr(torch.randn((dim, M), dtype=dt, generator=torch.Generator().manual_seed(dim + M)))[0].contiguous().to(dev)      # factored on the host
            r, rt = (torch.randn((M, M), dtype=dt, device=dev, generator=gen) / M ** 0.5 for _ in range(2))
            for t in (r, rt):
                t.diagonal().copy_(0.9 * torch.tanh(torch.randn(M, dtype=dt, device=dev, generator=gen)))
            b = 0.5 * torch.randn(M, dtype=dt, device=dev, generator=gen)
            layer = bj.SylvesterLayer(q, r, rt, b, orthonormal=True)
            inv = bj.inverse(layer)
            zk = torch.randn((batch, dim), dtype=dt, device=dev, generator=gen).T           # the library's layout: column-major
            yk = bj.transform(layer, zk)
            gk = torch.randn((batch, dim), dtype=dt, device=dev, generator=gen).T
            lb = torch.randn(batch, dtype=dt, device=dev, generator=gen)
            yt, gt = yk.contiguous(), gk.contiguous()                                       # torch's: the batch fastest
            # the smallest Newton count whose z meets the bar on the first columns
            nchk = min(batch, 65536)
            want, scale = zk[:, :nchk], zk[:, :nchk].abs().amax(dim=0)
            steps = None
            for k in range(1, 13):
                got = torch_inverse(q, r, rt, b, yt[:, :nchk].contiguous(), k)[0]
                if bool((((got - want).abs().amax(dim=0) / scale) <= BAR[name]).all()):
                    steps = k
                    break
            if steps is None:
                steps = 12
            ours = float(((bj.transform(inv, yk[:, :nchk].T.contiguous().T) - want).abs().amax(dim=0) / scale).max())
            td = bj.transformed(bj.MvNormal(dim), layer)
            b_map, b_full = 2 * dim * T, 3 * dim * T
            ops = [("map", lambda: bj.with_logabsdet_jacobian(inv, yk, per_sample=True), lambda: bj.with_logabsdet_jacobian(layer, zk, per_sample=True),
                    lambda: torch_inverse(q, r, rt, b, yt, steps), b_map),
                   ("vjp", lambda: bj.vjp(inv, yk, gk, lb), lambda: bj.vjp(layer, zk, gk, lb), lambda: torch_pullback(q, r, rt, b, yt, gt, lb, steps, False), b_full),
                   ("vjp_params", lambda: bj.vjp_params(inv, yk, gk, lb), lambda: bj.vjp_params(layer, zk, gk, lb),
                    lambda: torch_pullback(q, r, rt, b, yt, gt, lb, steps, True), b_full),
                   ("logpdf", lambda: bj.logpdf_vjp_params(td, yk), None, None, b_map)]
            for what, kern, fwd, ref, nbytes in ops:
                kern()
                before = lib.bjx_launch_count()
                kern()
                launches = lib.bjx_launch_count() - before
                res = alternate([(kern, args.inner)] + ([(fwd, args.inner), (ref, 1)] if fwd else []))
                k = res[0]
                pct = 100 * nbytes * batch / (k[0] * 1e-3) / PEAK
                if fwd:
                    emit(f"| {name} | {dim} x {M} | {batch} | {what} | {launches} | {nbytes} | {fmt(k)} | {pct:.1f} | {fmt(res[1])} | {k[0] / res[1][0]:.2f} | {steps} | "
                         f"{fmt(res[2])} | {res[2][0] / k[0]:.1f} |")
                else:
                    emit(f"| {name} | {dim} x {M} | {batch} | {what} | {launches} | {nbytes} | {fmt(k)} | {pct:.1f} | — | — | — | — | — |")
            print(f"# {name} {dim} x {M}: worst |z − z_true| / column scale of the library's inverse on {nchk} columns: {ours:.3g}", flush=True)
            del zk, yk, gk, lb, yt, gt, layer, inv, td
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0, help="sizes the batch as scripts/bench_sylvester.py does")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result to this file")
    ap.add_argument("--table", default=None, help="a table measured earlier with --out: measure nothing")
    ap.add_argument("--registers", default=None, help="stderr of a build with -Rpass-analysis=kernel-resource-usage: append the resource report")
    args = ap.parse_args()
    if args.table:
        lines = open(args.table).read().rstrip("\n").split("\n")
    else:
        lines = measure(args)
    if args.registers:
        lines += [""] + registers(args.registers, os.path.join(ROOT, "profiles", "r19_sylvester.md"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
