"""`bj.logpdf_vjp_params` of a flow of PlanarLayers over a diagonal normal base: the fused pass (bjx_planar_logpdf_vjp_params: one inverse
sweep with the base density and the cotangent sweep on the resident column, then the reduction stage of bjx_planar_vjp_params and the
two small μ̄ / σ̄ launches) against the generic path of the same function — `_preimage`, the base terms in torch, then `vjp_params` /
`vjp` of the inverse, which solve the inverse twice more — in one process on one GPU, on two distribution objects.

Timing: a HIP event pair (torch.cuda.Event) around a window of calls on the stream — at least `--inner` calls and as many as fill
`--min-window-ms` of the fused side —, so helper launches, torch's elementwise kernels and the gaps between launches are all inside —
what a training step sees, not only the hot kernels.  The two sides ALTERNATE inside every repeat; median of the repeats after a
warm-up, spread = (max − min) / median of the repeats of each side.
B/sample = algorithmic bytes of the fused side, DERIVED from the code (s = sizeof(T)): the pass reads y and writes ȳ, (2·dim + 2)·s; with
the parameters it also writes x and the (−s̄, t) tables, the reduction stage reads x, ȳ, the tables and c back once per group of eight
layers, and the μ̄ / σ̄ kernel reads x and c once more: (6·dim + 4·layers + 4)·s for up to eight layers — see `fused_bytes`.  Writes a markdown table
(stdout and --out) and, under it, the routing rule's verdict per shape: a shape stays fused only if its fused median beats the generic
median by more than the larger of the two spreads."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bijectors_amd as bj  # noqa: E402

PEAK = 8.0e12
SHAPES = [(128, 8, 22, torch.float32), (128, 2, 22, torch.float32), (64, 8, 21, torch.float64), (36, 8, 21, torch.float64), (1500, 8, 18, torch.float32),
          (256, 8, 21, torch.float32)]


def fused_bytes(dim, nl, sz, params):
    """Algorithmic bytes per column of the fused side, derived from the code."""
    if not params:
        return (2 * dim + 2) * sz                                    # y, ȳ, c, lp
    groups = (nl + 7) // 8
    pass_ = (3 * dim + 2 + 2 * nl) * sz                              # y read; ȳ, x, the tables, lp written; c read
    reduce_ = groups * (2 * dim + 2 * nl + 1) * sz                   # x, ȳ, the tables and c read per group of eight layers
    return pass_ + reduce_ + (dim + 1) * sz                          # μ̄ / σ̄: x and c once more


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fa, fb, warm, reps, inner):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(fa, inner))
        tb.append(event_ms(fb, inner))
    stat = lambda ts: (statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts))
    return stat(ta), stat(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--min-window-ms", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2-cap", type=int, default=None, help="cap log2(columns) (a quick run)")
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("at least five repeats")
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = ["| rows | layers | columns | dtype | call | fused ms | B/sample | of 8 TB/s | generic ms | fused / generic | spread % (max - min of the repeats, fused / generic) | launches (fused / generic hot kernels) | calls per window |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for dim, nl, lg, dt in SHAPES:
        lg = min(lg, a.log2_cap) if a.log2_cap else lg
        N, sz = 1 << lg, torch.empty(0, dtype=dt).element_size()
        ls = [bj.PlanarLayer(torch.randn(dim, generator=g, device="cuda", dtype=dt) / dim ** 0.5, 0.1 * torch.randn(dim, generator=g, device="cuda", dtype=dt) / dim ** 0.5,
                             torch.randn(1, generator=g, device="cuda", dtype=dt)) for _ in range(nl)]
        flow = ls[0]
        for l in ls[1:]:
            flow = l @ flow
        mu = 0.2 * torch.randn(dim, generator=g, device="cuda", dtype=dt)
        sigma = torch.exp(0.3 * torch.randn(dim, generator=g, device="cuda", dtype=dt))
        base = bj.MvNormal(mu, sigma)
        td_f, td_g = bj.transformed(base, flow), bj.transformed(base, flow)
        run_g = bj.interface._td_inverse(td_g)._plan()[0][0].orig
        run_g._refused.update({("logpdf", dt, dim, False), ("logpdf", dt, dim, True)})      # this distribution object always takes the generic path
        Y = torch.randn((N, dim), generator=g, device="cuda", dtype=dt).T
        c = torch.randn(N, generator=g, device="cuda", dtype=dt)
        for call, kw, fb in (("value, ȳ, all parameters", dict(params=True), fused_bytes(dim, nl, sz, True)),
                             ("value and ȳ (params=False)", dict(params=False), fused_bytes(dim, nl, sz, False)),
                             ("value and parameters (want_y_bar=False)", dict(want_y_bar=False), fused_bytes(dim, nl, sz, True))):
            fused = lambda: bj.logpdf_vjp_params(td_f, Y, c, **kw)
            generic = lambda: bj.logpdf_vjp_params(td_g, Y, c, **kw)
            rf, rg = fused(), generic()
            err = float((rf[0] - rg[0]).abs().max())
            assert err <= (1e-3 if dt == torch.float32 else 1e-6) * (nl + dim), f"fused and generic lp differ by {err}"
            kf, kg = bj.kernel_timed(fused)[2], bj.kernel_timed(generic)[2]
            del rf, rg
            inner = max(a.inner, int(a.min_window_ms / max(event_ms(fused, 1), 1e-3)) + 1)
            (tf, sf), (tg, sg) = alternate(fused, generic, a.warmup, a.reps, inner)
            rows.append(f"| {dim} | {nl} | 2^{lg} | {str(dt).split('.')[-1]} | {call} | {tf:.3f} | {fb} | {fb * N / (tf * 1e-3) / PEAK:.2f} | {tg:.3f} | {tf / tg:.2f} | "
                        f"{100 * sf:.1f} / {100 * sg:.1f} | {kf} / {kg} | {inner} |")
            print(rows[-1], flush=True)
            verdicts.append(f"- {dim} x {nl} {str(dt).split('.')[-1]}, {call}: fused {tf:.3f} ms, generic {tg:.3f} ms, margin {100 * (tg - tf) / tg:.1f} % of generic against a spread of "
                            f"{100 * max(sf, sg):.1f} % -> {'stays fused' if tf < tg and (tg - tf) / tg > max(sf, sg) else 'ROUTE TO THE GENERIC PATH'}")
        del Y, c
        torch.cuda.empty_cache()
    text = "\n".join(rows) + "\n\nRouting rule (fused median beats the generic median by more than the larger spread):\n\n" + "\n".join(verdicts) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(f"device: {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, {a.reps} repeats of a window of calls (last column; at least {a.min_window_ms:g} ms of the fused side), the two sides alternating\n\n" + text)
    print(text)


if __name__ == "__main__":
    main()
