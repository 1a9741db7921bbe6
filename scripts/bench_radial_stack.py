"""Fused RadialLayer run (bjx_radial_stack, bjx_radial_stack_vjp_params) against the same layers applied one by one, in one process on
one GPU: forward, inverse, input pullback and parameter pullback (of the run and of its inverse); kernel time from `bj.kernel_timed`
(the hot kernels' own event pairs), median of the repeats after a warm-up.
The one-by-one side is what a composition cost before the planner grouped radial runs: L launches for the maps, L-1 forward
launches plus L pullback launches for `vjp`; for `vjp_params` L-1 forward launches plus L single-layer parameter pullbacks with their
reductions, and in the inverse direction three launches per layer (inverse map, inverse pullback, forward parameter pullback) and two
negations.  Writes a markdown table (stdout and --out)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bijectors_amd as bj  # noqa: E402

PEAK = 8.0e12
SHAPES = [(128, 8, 22, torch.float32), (64, 8, 21, torch.float64), (10, 8, 22, torch.float32), (10, 8, 22, torch.float64), (128, 2, 22, torch.float32)]


def med(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        _, ms, _ = bj.kernel_timed(fn)
        ts.append(ms)
    return statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ops", nargs="*", default=None, help="only these rows (forward, inverse, vjp, vjp_params, 'vjp_params inverse')")
    ap.add_argument("--log2-cap", type=int, default=None, help="cap log2(columns) (a quick run)")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(7)
    rows = ["| rows | layers | columns | dtype | op | fused ms | B/sample | of 8 TB/s | one by one ms | B/sample | of 8 TB/s | fused / one by one | spread % (max - min of the repeats, fused / one by one) |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for dim, nl, lg, dt in SHAPES:
        lg = min(lg, a.log2_cap) if a.log2_cap else lg
        N, sz = 1 << lg, torch.empty(0, dtype=dt).element_size()
        ls = [bj.RadialLayer(0.5 * torch.randn(1, generator=g, device="cuda", dtype=dt), torch.randn(1, generator=g, device="cuda", dtype=dt),
                             0.3 * torch.randn(dim, generator=g, device="cuda", dtype=dt)) for _ in range(nl)]
        flow = ls[0]
        for l in ls[1:]:
            flow = l @ flow
        inv = bj.inverse(flow)
        Z = torch.randn((N, dim), generator=g, device="cuda", dtype=dt).T
        Z[0] += 2.0
        G = torch.randn((N, dim), generator=g, device="cuda", dtype=dt).T
        lb = torch.randn(N, generator=g, device="cuda", dtype=dt)
        Y = bj.transform(flow, Z)

        def one_by_one(x, inverse):
            tot = None
            for l in (reversed(ls) if inverse else ls):
                x, lj = bj.with_logabsdet_jacobian(bj.inverse(l) if inverse else l, x, per_sample=True)
                tot = lj if tot is None else tot + lj
            return x, tot

        def vjp_one_by_one():
            xs = [Z]
            for l in ls[:-1]:
                xs.append(bj.transform(l, xs[-1]))
            gg = G
            for l, xin in zip(reversed(ls), reversed(xs)):
                gg = bj.vjp(l, xin, gg, lb)
            return gg

        def params_one_by_one(x, inverse):
            pieces = [bj.inverse(l) for l in reversed(ls)] if inverse else ls
            xs = [x]
            for pc in pieces[:-1]:
                xs.append(bj.transform(pc, xs[-1]))
            gg, out = G, []
            for pc, xin in zip(reversed(pieces), reversed(xs)):
                gg, gr = bj.vjp_params(pc, xin, gg, lb)
                out.append(gr)
            return gg, out

        map_b = (2 * dim + 1) * sz
        vjp_b = (3 * dim + 1) * sz
        vjp_u = (nl - 1) * 2 * dim * sz + nl * vjp_b
        # one layer's parameter pullback: the pullback pass, (r, δᵀȳ) written and read back with ℓ̄; its inverse: the inverse map, the
        # inverse pullback and the negations of ȳ and ℓ̄ before it
        par_l = vjp_b + 5 * sz
        par_u = (nl - 1) * 2 * dim * sz + nl * par_l
        par_ui = (nl - 1) * 2 * dim * sz + nl * (2 * dim * sz + vjp_b + (2 * dim + 2) * sz + par_l)
        for op, fused, unfused, fb, ub in (
                ("forward", lambda: bj.with_logabsdet_jacobian(flow, Z, per_sample=True), lambda: one_by_one(Z, False), map_b, nl * map_b),
                ("inverse", lambda: bj.with_logabsdet_jacobian(inv, Y, per_sample=True), lambda: one_by_one(Y, True), map_b, nl * map_b),
                ("vjp", lambda: bj.vjp(flow, Z, G, lb), vjp_one_by_one, vjp_b, vjp_u),
                ("vjp_params", lambda: bj.vjp_params(flow, Z, G, lb), lambda: params_one_by_one(Z, False), vjp_b, par_u),
                ("vjp_params inverse", lambda: bj.vjp_params(inv, Y, G, lb), lambda: params_one_by_one(Y, True), vjp_b, par_ui)):
            if a.ops and op not in a.ops:
                continue
            (tf, sf), (tu, su) = med(fused, a.warmup, a.reps), med(unfused, a.warmup, a.reps)
            rows.append(f"| {dim} | {nl} | 2^{lg} | {str(dt).split('.')[-1]} | {op} | {tf:.3f} | {fb} | {fb * N / (tf * 1e-3) / PEAK:.2f} | {tu:.3f} | {ub} | "
                        f"{ub * N / (tu * 1e-3) / PEAK:.2f} | {tf / tu:.2f} | {100 * sf:.1f} / {100 * su:.1f} |")
            print(rows[-1], flush=True)
        del Z, G, Y, lb
        torch.cuda.empty_cache()
    text = "\n".join(rows) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(f"device: {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, median of {a.reps}\n\n" + text)
    print(text)


if __name__ == "__main__":
    main()
