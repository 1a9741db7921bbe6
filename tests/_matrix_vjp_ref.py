"""Seeded inputs, Float64 references and the form / staging / trip tables of tests/test_gpu_matrix_vjp_abi.py (bjx_vec_corr_vjp, bjx_corr_vjp,
bjx_pd_vjp and bjx_pd_vec_vjp of include/bjx.h through the C ABI).  tests/test_host_matrix_vjp_ref.py checks on the CPU that every
table row reaches the form written next to it, that the tiled generator's index map is right, that `second_trip_batch` exceeds what
any occupancy can hold, and that the draws measure the kernel and not the conditioning of the data.  No GPU, no torch.

Draws: the `_matrix_free` draws of tests/test_gpu_parity.py restated (off-diagonal scale min(0.6, 1.6/√K), log-diagonal 0.4·N(0,1)), the
forward-direction X the Float64 oracle inverse of the rounded free parameters, rounded to the type; cotangents N(0,1), not symmetric;
ladj_bar N(0,1).  Reference: `oracle.matrix_bijector_vjp` in Float64 on the dt-rounded inputs (pinned by tests/test_oracle_golden.py).

`form` restates the dispatch of csrc/bjx_matrix_vjp.hip (matrix_vjp_impl), csrc/bjx_matrix_vjp_grp.hip (bjx_matrix_vjp_grp),
csrc/bjx_matrix_vjp_mfma.hip (bjx_matrix_inv_vjp_mfma, mf_kind, mf_launch) and csrc/bjx_matrix_vjp_mfma_fwd.{hip,inc}
(bjx_matrix_fwd_vjp_mfma, fw_kind, fw_launch) for the DEFAULT tuning switches."""
import functools
import math
import zlib

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTS = (F32, F64)
KINDS = ("vec_corr", "corr", "pd", "pd_vec")
DENSE, PACKED = ("corr", "pd"), ("vec_corr", "pd_vec")
CORR_KINDS = ("vec_corr", "corr")


def vw(dt):
    """elements of a 16-byte pack"""
    return 16 // np.dtype(dt).itemsize


def free_len(kind, K):
    return K * (K - 1) // 2 if kind == "vec_corr" else K * (K + 1) // 2 if kind == "pd_vec" else K * K


def sizes(kind, K, inverse):
    """(elements of a sample of `in` / `in_bar`, of `out_bar`)"""
    return (free_len(kind, K), K * K) if inverse else (K * K, free_len(kind, K))


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ the dispatchers, restated
# NOTHING ties `form` to the C++ but the reader: it was compared by hand with matrix_vjp_impl, bjx_matrix_vjp_grp, bjx_matrix_inv_vjp_mfma /
# mf_kind / mf_launch and bjx_matrix_fwd_vjp_mfma / fw_kind / fw_launch.  The host test checks the tables below against IT only, so whoever
# changes a threshold or a staging condition there must change it and the tables, or the GPU file quietly reaches other forms than it names.
K_MAX_SERVED, K_REFUSED = 1024, 1025
MEM_WS_BYTES = 512 << 20


def _geom_group(K, dt, nt64):
    """(GS, KMAX, NT) of the three group-per-sample kernels: MF_K / MF_W, FW_K / FW_W, GRP_K / GRP_W"""
    if K <= 12:
        return 16, 12, 256
    if K <= 16:
        return 16, 16, 256
    if K <= 24:
        return 32, 24, 256
    if K <= 32:
        return 32, 32, 256
    if K <= 48:
        return 64, 48, 256
    return 64, 64, nt64


def form(kind, K, dt, inverse, off_in=0, off_out_bar=0, off_in_bar=0):
    """-> (family, (GS, KMAX, NT), width).  Offsets: elements between a 16-byte boundary and the base of `in`, `out_bar`, `in_bar`
    (`off_out_bar` None: a NULL `out_bar`, K = 1 of VecCorr).  family: "none" (nothing to differentiate), "lane"
    (matrix_lane_vjp_kernel: one lane per sample, GS = 1, 64 samples a block), "mfma_inv" (matrix_inv_vjp_mfma_kernel), "mfma_fwd"
    (matrix_fwd_vjp_mfma_kernel), "grp" (matrix_grp_vjp_kernel: NOT only behind a switch — the forward direction at K = 9 … 12 and
    17 … 24, in Float64 at 9 … 24, is its by default), "mem" (matrix_mem_vjp_kernel, K = 65 … 1024), "refused".  width: elements per
    global access of the staging (V of the lane kernel, VWT of mf_launch, pack / 1 for VEC of fw_launch; 1 for grp and mem)."""
    dt = np.dtype(dt)
    sz, N = dt.itemsize, vw(dt)
    n_in, _ = sizes(kind, K, inverse)
    if n_in == 0:
        return "none", None, 0
    byte_offs = [0 if o is None else o * sz for o in (off_in, off_out_bar, off_in_bar)]
    al = lambda m: all(b & m == 0 for b in byte_offs)
    nf = free_len(kind, K)
    if K <= 8:                                                      # matrix_vjp_impl: K > 8 asks bjx_matrix_vjp_grp first
        return "lane", (1, 4 if K <= 4 else 8, 64), (N if al(15) else 1)
    if K > 64:                                                      # every group kernel returns 1 beyond 64 rows
        return ("mem", (1, 0, 64), 1) if K <= K_MAX_SERVED else ("refused", None, 0)
    nt64 = 256 if dt == F32 else 128
    if inverse:                                                     # bjx_matrix_inv_vjp_mfma serves 9 … 64 in both types
        if K % N == 0 and nf % N == 0 and al(15):
            w = N
        elif dt == F32 and K % 2 == 0 and nf % 2 == 0 and al(7):
            w = 2
        else:
            w = 1
        return "mfma_inv", _geom_group(K, dt, nt64), w
    if not (K < 13 or 16 < K < 25 or (dt != F32 and K < 25)):       # bjx_matrix_fwd_vjp_mfma, BJX_MATRIX_VJP_MFMA unset
        return "mfma_fwd", _geom_group(K, dt, nt64), (N if K % N == 0 and nf % N == 0 and al(15) else 1)
    assert K <= 32 or dt == F32                                     # bjx_matrix_vjp_grp's own refusal is never reached by default
    return "grp", _geom_group(K, dt, 256), 1


def samples_per_block(fm):
    family, geom, _ = fm
    return 64 if family in ("lane", "mem") else geom[2] // geom[0]


def mem_blocks_cap(K, dt, cus):
    """matrix_vjp_impl: blocks in flight of the workspace kernel before `need` limits them"""
    per_lane = 2 * K * K * np.dtype(dt).itemsize
    return min(max(MEM_WS_BYTES // (per_lane * 64), 1), cus * 16)


def second_trip_batch(fm, cus, K=None, dt=None):
    """The smallest batch that forces a second trip of the form's persistent loop WHATEVER the occupancy query returns, from limits
    that cannot be exceeded: 32 waves a CU, so at most 2048 / NT resident blocks of NT threads.
    MFMA forms: cus·(2048/NT)·(NT/GS) + NT/GS + 1 — a second trip of the first block plus a ragged tail (a wave with dead groups where
    GS < 64, a last-trip prefetch clamped to batch − 1).  The group kernel has no loop (its grid is the batch): the same batch.
    Lane kernel: 2·32·cus·64 + 65 (grid capped at 32 tiles a CU: a second trip of every block, a third of the first two).
    Workspace kernel (needs K and dt): blocks·64 + 1."""
    family, geom, _ = fm
    if family == "lane":
        return 2 * 32 * cus * 64 + 65
    if family == "mem":
        return mem_blocks_cap(K, dt, cus) * 64 + 1
    GS, _, NT = geom
    return cus * (2048 // NT) * (NT // GS) + NT // GS + 1


# ------------------------------------------------------------------ the tables
# (a) form edges: K lo, K hi of every form with every pointer aligned — (family, (GS, KMAX, NT)) by (dtype, inverse)
_INV = lambda nt: [((1, 4), "lane", (1, 4, 64)), ((5, 8), "lane", (1, 8, 64)), ((9, 12), "mfma_inv", (16, 12, 256)), ((13, 16), "mfma_inv", (16, 16, 256)),
                   ((17, 24), "mfma_inv", (32, 24, 256)), ((25, 32), "mfma_inv", (32, 32, 256)), ((33, 48), "mfma_inv", (64, 48, 256)),
                   ((49, 64), "mfma_inv", (64, 64, nt)), ((65, 1024), "mem", (1, 0, 64))]
FORM_EDGES = {
    (F32, True): _INV(256),
    (F64, True): _INV(128),
    (F32, False): [((1, 4), "lane", (1, 4, 64)), ((5, 8), "lane", (1, 8, 64)), ((9, 12), "grp", (16, 12, 256)), ((13, 16), "mfma_fwd", (16, 16, 256)),
                   ((17, 24), "grp", (32, 24, 256)), ((25, 32), "mfma_fwd", (32, 32, 256)), ((33, 48), "mfma_fwd", (64, 48, 256)),
                   ((49, 64), "mfma_fwd", (64, 64, 256)), ((65, 1024), "mem", (1, 0, 64))],
    (F64, False): [((1, 4), "lane", (1, 4, 64)), ((5, 8), "lane", (1, 8, 64)), ((9, 12), "grp", (16, 12, 256)), ((13, 16), "grp", (16, 16, 256)),
                   ((17, 24), "grp", (32, 24, 256)), ((25, 32), "mfma_fwd", (32, 32, 256)), ((33, 48), "mfma_fwd", (64, 48, 256)),
                   ((49, 64), "mfma_fwd", (64, 64, 128)), ((65, 1024), "mem", (1, 0, 64))],
}
EDGE_KS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65)
MEM_K = 65


def edge_batches(fm):
    """lane: one short tile, a full one (the pack walker of tile_stage_in at every K <= 8), a second block with one sample, a third;
    group forms (SPB = NT/GS samples a block): 1, SPB − 1 (a dead group in a live wave, a dead wave in a live block), SPB, SPB + 1;
    workspace kernel: 1, 63, 65"""
    family = fm[0]
    if family == "lane":
        return (1, 63, 64, 65, 129)
    if family == "mem":
        return (1, 63, 65)
    spb = samples_per_block(fm)
    return tuple(sorted({1, spb - 1, spb, spb + 1} - {0}))


# (b) staging: (dtype, directions, Ks, kinds, offset in elements, family, width).  K = 4, 8 | 12, 16, 24, 32, 48, 64 are whole packs of
# rows (alignment decides; at K = 12 the packed kinds' free length, 66 / 78, is half a Float32 pack: VWT = 2 even when aligned);
# at K = 10, 14 the parity of the free length decides (45, 55, 91, 105 odd: width 1; dense 100, 196: pairs).
STAGING = [
    (F32, (0, 1), (4, 8), KINDS, 0, "lane", 4), (F32, (0, 1), (4, 8), KINDS, 1, "lane", 1), (F32, (0, 1), (4, 8), KINDS, 2, "lane", 1),
    (F64, (0, 1), (4, 8), KINDS, 0, "lane", 2), (F64, (0, 1), (4, 8), KINDS, 1, "lane", 1),
    (F32, (1,), (16, 24, 32, 48, 64), KINDS, 0, "mfma_inv", 4), (F32, (1,), (16, 24, 32, 48, 64), KINDS, 2, "mfma_inv", 2), (F32, (1,), (16, 24, 32, 48, 64), KINDS, 1, "mfma_inv", 1),
    (F32, (1,), (12,), DENSE, 0, "mfma_inv", 4), (F32, (1,), (12,), PACKED, 0, "mfma_inv", 2), (F32, (1,), (12,), KINDS, 2, "mfma_inv", 2), (F32, (1,), (12,), KINDS, 1, "mfma_inv", 1),
    (F32, (1,), (10, 14), DENSE, 0, "mfma_inv", 2), (F32, (1,), (10, 14), PACKED, 0, "mfma_inv", 1), (F32, (1,), (10, 14), DENSE, 2, "mfma_inv", 2),
    (F32, (1,), (10, 14), PACKED, 2, "mfma_inv", 1), (F32, (1,), (10, 14), KINDS, 1, "mfma_inv", 1),
    (F64, (1,), (12, 16, 24, 32, 48, 64), KINDS, 0, "mfma_inv", 2), (F64, (1,), (12, 16, 24, 32, 48, 64), KINDS, 1, "mfma_inv", 1),
    (F64, (1,), (10, 14), DENSE, 0, "mfma_inv", 2), (F64, (1,), (10, 14), PACKED, 0, "mfma_inv", 1), (F64, (1,), (10, 14), KINDS, 1, "mfma_inv", 1),
    (F32, (0,), (16, 32, 48, 64), KINDS, 0, "mfma_fwd", 4), (F32, (0,), (16, 32, 48, 64), KINDS, 1, "mfma_fwd", 1), (F32, (0,), (16, 32, 48, 64), KINDS, 2, "mfma_fwd", 1),
    (F32, (0,), (14,), KINDS, 0, "mfma_fwd", 1), (F32, (0,), (14,), KINDS, 1, "mfma_fwd", 1), (F32, (0,), (14,), KINDS, 2, "mfma_fwd", 1),
    (F32, (0,), (10, 12, 24), KINDS, 0, "grp", 1), (F32, (0,), (10, 12, 24), KINDS, 1, "grp", 1), (F32, (0,), (10, 12, 24), KINDS, 2, "grp", 1),
    (F64, (0,), (32, 48, 64), KINDS, 0, "mfma_fwd", 2), (F64, (0,), (32, 48, 64), KINDS, 1, "mfma_fwd", 1),
    (F64, (0,), (10, 12, 14, 16, 24), KINDS, 0, "grp", 1), (F64, (0,), (10, 12, 14, 16, 24), KINDS, 1, "grp", 1),
]
STAGING_OFFSETS = {F32: (1, 2), F64: (1,)}
STAGING_KS = (4, 8, 10, 12, 14, 16, 24, 32, 48, 64)


def offset_patterns(off):
    """the offset on each of `in`, `out_bar`, `in_bar` alone, and on all three"""
    return ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off))


# (c) loop trips: one case per form at its smallest K; D distinct samples, coprime to every samples-per-block (2, 4, 8, 16, 64)
TRIP_KS = (2, 5, 9, 13, 17, 25, 33, 49)
TRIP_KINDS = ("vec_corr", "pd")
TRIP_D = 37
# (e) alias
ALIAS_KS = (4, 12, 32, 64, 65)
ALIAS_TRIP_K = 12


# ------------------------------------------------------------------ draws
def _f(a, dt):
    return np.asfortranarray(np.asarray(a).astype(dt))


def _keep(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def matrix_free(kind, K, batch, r, dt):
    """tests/test_gpu_parity.py `_matrix_free`, restated: the unconstrained side, free entries only (the rest zero)"""
    off = min(0.6, 1.6 / math.sqrt(K))
    if kind == "vec_corr":
        return (off * r.normal(size=(K * (K - 1) // 2, batch))).astype(dt)
    if kind == "corr":
        Y = (off * r.normal(size=(K, K, batch))).astype(dt)
        return Y * np.triu(np.ones((K, K), bool), 1)[:, :, None]
    L = off * r.normal(size=(K, K, batch)) * np.tril(np.ones((K, K), bool), -1)[:, :, None]
    L[np.arange(K), np.arange(K), :] = 0.4 * r.normal(size=(K, batch))
    if kind == "pd":
        return L.astype(dt)
    rows = [L[j, i] for j in range(K) for i in range(j + 1)]                       # triu_to_vec(L'), every sample at once
    return np.stack(rows, axis=0).astype(dt)


# (kind, K, batch) -> seed of a REDRAW (both types): a draw whose forward reference moves by more than 1e-4 of a sample's scale under a
# 1-ulp(Float32) perturbation of X (tests/test_host_matrix_vjp_ref.py; 1.0e-4 ... 2.3e-4 on these ten with seed 0, 2.0e-5 ... 8.6e-5 with
# the seed below) is drawn again with another seed; the bar is never widened.
RESEED = {("corr", 8, 129): 1, ("corr", 10, 17): 2, ("pd", 13, 37): 1, ("pd", 49, 37): 1, ("pd", 65, 65): 1, ("pd_vec", 8, 65): 1, ("pd_vec", 17, 9): 1,
          ("vec_corr", 8, 65): 1, ("vec_corr", 9, 37): 1, ("vec_corr", 14, 17): 1}


@functools.lru_cache(maxsize=None)
def draw(kind, dtname, K, batch):
    """y: free parameters, (n, batch) | (K, K, batch); Xbar (K, K, batch), lbar (batch,): standard normal; X (K, K, batch): the Float64
    oracle inverse of the rounded y, rounded; ybar: standard normal in the layout of y (dense kinds: on the free entries, zero elsewhere
    like the reference's outputs).  All rounded to the type, column-major, read-only."""
    from oracle import oracle

    dt = np.dtype(dtname)
    r = rng_for("matrix_vjp", kind, dtname, K, batch, RESEED.get((kind, K, batch), 0))
    y = _f(matrix_free(kind, K, batch, r, dt), dt)
    Xbar = _f(r.normal(size=(K, K, batch)), dt)
    lbar = r.normal(size=batch).astype(dt)
    X64, _ = oracle.matrix_bijector(kind, f64(y), inverse=True)
    ybar = r.normal(size=y.shape)
    if kind == "corr":
        ybar = ybar * np.triu(np.ones((K, K), bool), 1)[:, :, None]
    elif kind == "pd":
        ybar = ybar * np.tril(np.ones((K, K), bool))[:, :, None]
    return _keep(dict(y=y, Xbar=Xbar, lbar=lbar, X=_f(X64, dt), ybar=_f(ybar, dt)))


def operands(kind, dtname, K, batch, inverse):
    """(in, out_bar, ladj_bar) of a call"""
    d = draw(kind, dtname, K, batch)
    return (d["y"], d["Xbar"], d["lbar"]) if inverse else (d["X"], d["ybar"], d["lbar"])


def tiled_index(D, batch):
    """The index map of a tiled batch: sample s of the batch holds distinct sample s % D.  D is chosen coprime to every
    samples-per-block, so each distinct sample visits every group slot of a block."""
    assert 1 <= D <= 64
    return np.arange(batch, dtype=np.int64) % D


def tiled(kind, dtname, K, D, batch, inverse):
    """A batch of any length from D <= 64 distinct samples -> (in, out_bar, ladj_bar of the D samples, index map (batch,)): the
    reference is computed on the D samples only and the batch is built where it is used (`a[..., index]`, `index_select`)."""
    return operands(kind, dtname, K, D, inverse) + (tiled_index(D, batch),)


def f64(a):
    return np.asfortranarray(np.asarray(a, np.float64))


# ------------------------------------------------------------------ reference (Float64 oracle on the rounded inputs)
def ref_vjp(kind, inp, out_bar, ladj_bar, inverse):
    from oracle import oracle

    return np.asarray(oracle.matrix_bijector_vjp(kind, f64(inp), f64(out_bar), None if ladj_bar is None else np.asarray(ladj_bar, np.float64), inverse=bool(inverse)), np.float64)


@functools.lru_cache(maxsize=None)
def ref(kind, dtname, K, batch, inverse, with_l=True):
    """the reference of `operands(kind, dtname, K, batch, inverse)`, computed once"""
    a, g, l = operands(kind, dtname, K, batch, inverse)
    out = ref_vjp(kind, a, g, l if with_l else None, inverse)
    out.setflags(write=False)
    return out


def unread_triangle(kind, K):
    """index arrays (rows, cols) of the strict triangle of X the reference does not read: the forward pullback is exactly zero there"""
    return np.tril_indices(K, -1) if kind in CORR_KINDS else np.triu_indices(K, 1)
