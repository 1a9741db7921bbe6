"""Reference of bjx_scale_matrix_chain (include/bjx.h; src/transformed_distribution.jl:164-169 with a full-covariance base): plain numpy in
Float64, no GPU and no torch — and the inputs the GPU suite (tests/test_gpu_scale_matrix_chain.py) runs it on, so that the CPU-side test
(tests/test_scale_matrix_chain_ref.py) can pin the reference against the oracle and check that it is finite on exactly those inputs.

    out        = a · c(x)                 (inverse: a \\ c(x)),      c = ops[-1] ∘ … ∘ ops[0] applied to every element
    ladj[n]    = logabsdetjac of c at column n  ±  logabsdet(a)      (− for the inverse)
    + density:   − ½ ‖out[:, n]‖² − dim · ½ log 2π

A stage is the oracle's triple (kind, p0, None) with p0 None, a scalar or one value per row (`oracle.chain` takes the same list)."""
import math
import zlib

import numpy as np

OP_EXP, OP_LOG, OP_SHIFT, OP_SCALE, OP_SCALE_INV = 1, 2, 3, 4, 5      # include/bjx.h: bjx_op_kind

F32_DIMS = [4, 8, 12, 16, 24, 32, 48, 64, 80, 96, 112, 128]
F64_DIMS = [2, 4, 6, 10, 16, 32, 50, 64, 96, 112]
EDGE_DIMS = {np.dtype(np.float32): (12, 64, 128), np.dtype(np.float64): (6, 64, 112)}
BATCHES = (1, 17, 257)
EDGE_BATCHES = (1, 15, 16, 17, 63, 64, 65, 257)
FAMILIES = ("none", "exp", "affexp_v", "log_v", "scalars")
VECTOR_FAMILIES = ("affexp_v", "log_v")


def dims_of(dt):
    return F32_DIMS if np.dtype(dt) == np.float32 else F64_DIMS


def batches_of(dt, dim):
    return EDGE_BATCHES if dim in EDGE_DIMS[np.dtype(dt)] else BATCHES


def reduction_path(dt, dim):
    """How the kernel adds the chain's log-det over the lanes of a column (Gc = dim / (16 / sizeof(T)) lanes)."""
    gc = dim // (16 // np.dtype(dt).itemsize)
    if gc == 1:
        return "Gc1"
    if gc & (gc - 1):
        return "lds_atomics"
    return "dpp" if np.dtype(dt) == np.float32 and gc == 16 else "shuffle"


def chain_ref(ops, x):
    """c(x) and its per-column log-det: +x for exp, −log x for log, Σ log|a_i| for Scale, −Σ log|a_i| for Scale⁻¹.  x: (dim, batch)."""
    x = np.array(x, dtype=np.float64)
    dim, batch = x.shape
    l = np.zeros(batch)
    for kind, p, _ in ops:
        col = None
        if p is not None:
            col = np.asarray(p, dtype=np.float64)
            col = np.full((dim, 1), float(col)) if col.ndim == 0 else col.reshape(dim, 1)
        if kind == OP_EXP:
            l += x.sum(axis=0)
            x = np.exp(x)
        elif kind == OP_LOG:
            x = np.log(x)
            l -= x.sum(axis=0)
        elif kind == OP_SHIFT:
            x = x + col
        elif kind == OP_SCALE:
            x = x * col
            l += np.log(np.abs(col)).sum()
        elif kind == OP_SCALE_INV:
            x = x / col
            l -= np.log(np.abs(col)).sum()
        else:
            raise ValueError(f"stage kind {kind} is not served by bjx_scale_matrix_chain")
    return x, l


def ref(a, ops, x, inverse, density):
    """-> (out (dim, batch), ladj (batch,)).  `a`, `x` and the stage parameters: already rounded to the call's type, then promoted."""
    a = np.asarray(a, dtype=np.float64)
    cx, l = chain_ref(ops, x)
    dim = a.shape[0]
    out = np.linalg.solve(a, cx) if inverse else a @ cx
    lad = np.linalg.slogdet(a)[1]
    ladj = l - lad if inverse else l + lad
    if density:
        ladj = ladj - 0.5 * np.sum(out * out, axis=0) - dim * 0.5 * math.log(2.0 * math.pi)
    return out, ladj


# ------------------------------------------------------------------ the inputs of the GPU suite (seeded; every log sees a positive argument)
def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def matrix(dim, dt, kind="general"):
    """"general": normal/√dim + 1.5·I, well conditioned and not symmetric (test_scale_with_a_matrix);
    "cholesky": the lower-triangular factor of AAᵀ + 0.3·I.  Rounded to `dt`."""
    r = rng_for("a", dim, kind)
    A = r.normal(size=(dim, dim)) / math.sqrt(dim)
    if kind == "cholesky":
        return np.linalg.cholesky(A @ A.T + 0.3 * np.eye(dim)).astype(dt)
    return (A + 1.5 * np.eye(dim)).astype(dt)


def family(name, dim, batch, dt):
    """-> (ops, x): the stages (parameters rounded to `dt`) and the (dim, batch) input rounded to `dt`, column-major."""
    dt = np.dtype(dt)
    a_vec = np.linspace(0.5, 1.5, dim)
    a_vec[::3] *= -1.0                                              # mixed sign, as a_vec in _chain_cases (tests/test_gpu_parity.py)
    b_vec = np.linspace(-0.3, 0.4, dim)
    a_vec, b_vec = a_vec.astype(dt), b_vec.astype(dt)
    s = lambda v: float(dt.type(v))
    r = rng_for("x", name, dim, batch)
    normal = r.normal(size=(dim, batch))
    if name == "none":
        ops = []
    elif name == "exp":
        ops = [(OP_EXP, None, None)]
    elif name == "affexp_v":
        ops = [(OP_SCALE, a_vec, None), (OP_SHIFT, b_vec, None), (OP_EXP, None, None)]
    elif name == "log_v":
        ops = [(OP_LOG, None, None), (OP_SHIFT, s(-0.1), None), (OP_SCALE_INV, a_vec, None), (OP_SHIFT, b_vec, None)]
        normal = np.exp(normal)
    elif name == "scalars":
        ops = [(OP_SCALE, s(-1.7), None), (OP_SHIFT, s(0.1), None), (OP_EXP, None, None), (OP_SCALE_INV, s(0.5), None)]
    else:
        raise KeyError(name)
    return ops, np.asfortranarray(normal.astype(dt))
