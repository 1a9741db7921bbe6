"""Chains whose stages all have scalar parameters run as a resolved program: kinds and host scalars by value in the kernel
arguments, a device-resident scalar fetched once through its pointer, all of it in scalar registers before the data arrives
(`ScalarProg` / `run_prog`, csrc/bjx_chain.hip).  Checked here, through the C ABI:

* `y` is BIT-identical to the same stages applied one call at a time, each as a one-stage chain of the same dtype: no stored
  expectation, and any contraction of a multiply with the next stage's add, or any reordering, fails it;
* the log-det, summed and per sample, agrees with a float64 numpy evaluation of the reference formulas within the bar
  tests/test_gpu_parity.py sets for chain log-dets (`sum_close`);
* NaN / Inf / signed zero pass through exp ∘ Shift ∘ Scale bit for bit.

Shapes for the summed log-det: the flat kernel covers 256·U packs of 16 bytes per block; as shipped U = 2 for Float32 and 4 for
Float64 chains of several stages (2 for one stage), i.e. 2048 elements per block in both types (1024 for the one-stage Float64
chain).  (64, 129) = 8256: four full blocks, then a last block of whole packs; (3, 1367) = 4101: two full blocks, one (Float64:
two) whole packs, one tail element; (7, 5): all in the last block, 3 / 1 tail elements; (1, 1); and (3, 1367) starting one
element off a 16-byte boundary (one element per pack, 256 per block).
Per-sample shapes, batch never a multiple of the columns per block: 64 rows (flatcol), 100 (colbatch), 1024 (colgroup), 3 and 10
rows IN PLACE (an out-of-place call of so short a column is served by the Stacked walker; in place it is chain_tiny_kernel, and
colbatch for the Float64 10 rows)."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from test_gpu_parity import sum_close  # noqa: E402  (the bar for chain log-dets: RTOL·(|ref| + sqrt(n)), RTOL 1e-3 / 1e-6)

EXP, LOG, SHIFT, SCALE, LEAKY, TRUNC = 1, 2, 3, 4, 8, 9
TDT = {np.float32: torch.float32, np.float64: torch.float64}
BITS = {np.float32: torch.int32, np.float64: torch.int64}


class St:
    """One stage: kind, up to two scalars, and which of them live on the device (param_len = 1 with v0 / v1 set)."""

    def __init__(self, kind, p0=None, p1=None, dev0=False, dev1=False):
        self.kind, self.p0, self.p1, self.dev0, self.dev1 = kind, p0, p1, dev0, dev1


def _uniform(lo, hi):
    return lambda r, n: r.uniform(lo, hi, size=n)


CHAINS = {
    # BASELINE config 2: exp ∘ Shift(0.1) ∘ Scale(0.5)
    "c2": ([St(SCALE, 0.5), St(SHIFT, 0.1), St(EXP)], lambda r, n: r.normal(size=n)),
    "exp": ([St(EXP)], lambda r, n: r.normal(size=n)),
    # BJX_MAX_OPS stages; (0.1, 0.9) -> (0.15, 1.35) -> (0.4, 1.6) -> (-0.92, 0.47) -> (-0.28, 0.47) -> (0.75, 1.6), inside (0.5, 2)
    "eight": ([St(SCALE, 1.5), St(SHIFT, 0.25), St(LOG), St(LEAKY, 0.3), St(EXP), St(TRUNC, 0.5, 2.0), St(SHIFT, -0.1), St(SCALE, -2.0)],
              _uniform(0.1, 0.9)),
    "bare_first": ([St(EXP), St(SHIFT, -1.0), St(LEAKY, 0.5)], lambda r, n: r.normal(size=n)),
    # Scale's a and Truncated's upper bound on the device (their host slots hold a value that must not be used), the rest on the host
    "dev_scalar": ([St(SCALE, 0.5, dev0=True), St(SHIFT, 0.1), St(TRUNC, -4.0, 5.0, dev1=True)], lambda r, n: r.normal(size=n)),
}
SUM_SHAPES = [(64, 129, 0), (3, 1367, 0), (7, 5, 0), (1, 1, 0), (3, 1367, 1)]          # dim, batch, elements off alignment
PS_SHAPES = [(64, 67, False), (100, 45, False), (1024, 7, False), (3, 1031, True), (10, 517, True)]      # dim, batch, in place


@pytest.fixture(scope="module")
def abi():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import bijectors_amd
    from bijectors_amd import _lib as L, interface

    return L, L.load(), interface.context()


def _rt(v, dt):
    """the scalar as the library sees it: rounded to the data's type"""
    return float(dt(v))


def _call(abi, stages, x, dim, batch, dt, per_sample=False, in_place=False):
    """bjx_chain on the flat device tensor x (dim·batch elements, columns contiguous) -> y, Σ log-det, per-sample log-det."""
    L, lib, ctx = abi
    arr = (L.BjxOp * len(stages))()
    keep = []
    for o, s in zip(arr, stages):
        o.kind, o.param_len, o.p0, o.p1, o.v0, o.v1 = s.kind, 0, 0.0, 0.0, None, None
        for j, (p, on_dev) in enumerate(((s.p0, s.dev0), (s.p1, s.dev1))):
            if p is None:
                continue
            o.param_len = 1
            if on_dev:
                t = torch.full((1,), _rt(p, dt), dtype=TDT[dt], device="cuda")
                keep.append(t)
                setattr(o, f"v{j}", t.data_ptr())
                setattr(o, f"p{j}", 123.0)
            else:
                setattr(o, f"p{j}", float(p))
    y = x.clone() if in_place else torch.empty_like(x)
    src = y if in_place else x
    lsum = torch.zeros(1, dtype=torch.float64, device="cuda")
    lps = torch.zeros(batch, dtype=TDT[dt], device="cuda") if per_sample else None
    rc = lib.bjx_chain(ctx.h, 0 if dt == np.float32 else 1, arr, len(stages), src.data_ptr(), y.data_ptr(),
                       lps.data_ptr() if per_sample else None, lsum.data_ptr(), dim, batch, 0)
    L.check(ctx.h, rc, "bjx_chain")
    torch.cuda.synchronize()
    del keep
    return y, float(lsum.item()), (lps.cpu().numpy().astype(np.float64) if per_sample else None)


def _host_only(s):
    return St(s.kind, s.p0, s.p1)


def _staged(abi, stages, x, dim, batch, dt):
    """the same stages one call at a time, every scalar on the host"""
    y = x
    for s in stages:
        y, _, _ = _call(abi, [_host_only(s)], y, dim, batch, dt)
    return y


def _numpy_ladj(stages, x, dt):
    """float64 evaluation of the reference formulas; returns the per-element log-det terms"""
    v = x.astype(np.float64)
    l = np.zeros_like(v)
    for s in stages:
        a = None if s.p0 is None else _rt(s.p0, dt)
        b = None if s.p1 is None else _rt(s.p1, dt)
        if s.kind == EXP:
            l += v
            v = np.exp(v)
        elif s.kind == LOG:
            v = np.log(v)
            l -= v
        elif s.kind == SHIFT:
            v = a + v
        elif s.kind == SCALE:
            l += math.log(abs(a))
            v = a * v
        elif s.kind == LEAKY:
            J = np.where(v < 0, a, 1.0)
            l += np.log(np.abs(J))
            v = J * v
        elif s.kind == TRUNC:            # both bounds finite
            v = np.clip(v, a, b)
            l -= np.log((v - a) * (b - v) / (b - a))
            v = np.log((v - a) / (b - v))
        else:
            raise AssertionError(s.kind)
    return l


def _input(name, n, dt, off=0):
    gen = CHAINS[name][1]
    host = gen(np.random.default_rng(len(name) * 1000 + n), n).astype(dt)
    buf = torch.empty(n + off, dtype=TDT[dt], device="cuda")
    x = buf[off:]
    x.copy_(torch.from_numpy(host))
    assert (x.data_ptr() % 16 != 0) == (off != 0)
    return host, x


def _same_bits(a, b, dt, what):
    ai, bi = a.view(BITS[dt]), b.view(BITS[dt])
    bad = int((ai != bi).sum().item())
    if bad:
        i = int(torch.nonzero(ai != bi)[0].item())
        raise AssertionError(f"{what}: {bad} of {ai.numel()} elements differ from the stage-by-stage result, first at {i}: "
                             f"{a[i].item()!r} vs {b[i].item()!r}")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SUM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}" + ("_unaligned" if s[2] else ""))
@pytest.mark.parametrize("name", list(CHAINS))
def test_summed_logdet(abi, name, shape, dt):
    dim, batch, off = shape
    stages = CHAINS[name][0]
    n = dim * batch
    host, x = _input(name, n, dt, off)
    y, lsum, _ = _call(abi, stages, x, dim, batch, dt)
    _same_bits(y, _staged(abi, stages, x, dim, batch, dt), dt, f"{name} {shape}")
    ref = float(_numpy_ladj(stages, host, dt).sum())
    print(f"{name} {shape} {dt.__name__}: ladj {lsum!r} ref {ref!r} diff {abs(lsum - ref):.3g}")
    sum_close(lsum, ref, dt, n, what=f"{name} {shape} ladj")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", PS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}" + ("_inplace" if s[2] else ""))
@pytest.mark.parametrize("name", list(CHAINS))
def test_per_sample_logdet(abi, name, shape, dt):
    dim, batch, in_place = shape
    stages = CHAINS[name][0]
    n = dim * batch
    host, x = _input(name, n, dt)
    y, lsum, lps = _call(abi, stages, x, dim, batch, dt, per_sample=True, in_place=in_place)
    _same_bits(y, _staged(abi, stages, x, dim, batch, dt), dt, f"{name} {shape}")
    ref = _numpy_ladj(stages, host, dt).reshape(batch, dim).sum(axis=1)
    print(f"{name} {shape} {dt.__name__}: worst per-sample diff {np.abs(lps - ref).max():.3g}, sum diff {abs(lsum - ref.sum()):.3g}")
    for c in range(batch):
        sum_close(lps[c], ref[c], dt, dim, what=f"{name} {shape} per-sample ladj of column {c}")
    sum_close(lsum, float(ref.sum()), dt, n, what=f"{name} {shape} ladj")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_special_values_pass_through(abi, dt):
    stages = CHAINS["c2"][0]
    x = torch.tensor([0.0, -0.0, math.inf, math.nan], dtype=TDT[dt], device="cuda")
    y, _, _ = _call(abi, stages, x, 4, 1, dt)
    _same_bits(y, _staged(abi, stages, x, 4, 1, dt), dt, "special values")
    got = y.cpu().numpy()
    assert got[0] == got[1] and abs(float(got[0]) - math.exp(0.1)) < 1e-5
    assert np.isposinf(got[2]) and np.isnan(got[3])
