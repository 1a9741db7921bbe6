"""Dispatch restated, Float64 references, draws and tables of tests/test_gpu_seq_abi.py: bjx_ordered, bjx_simplex, bjx_ordered_ld,
bjx_simplex_ld, bjx_ordered_vjp and bjx_simplex_vjp of include/bjx.h through the C ABI.  tests/test_host_seq_ref.py checks on the CPU
that every table height is the edge of the form written next to it, that the numpy references agree with the oracle, and that the draws
measure the kernel and not the conditioning of the data.  No GPU, no torch.

`form` restates, for the DEFAULT tuning switches, ordered_impl, simplex_impl, launch_quad_stream, launch_seq, launch_seq_chunk,
ordered_vjp_impl, simplex_vjp_impl and launch_simplex_vjp_stream of csrc/bjx_seq.hip, bjx_seq_tiny and bjx_seq_tiny_vjp of
csrc/bjx_tiny.hip, and bjx_tall_stream and bjx_tall_simplex_vjp of csrc/bjx_tall.hip.  NOTHING ties it to the C++ but the reader: whoever
changes a threshold there must change it here and in the tables, or the GPU file quietly reaches other kernels than it names.

Draws (well conditioned at every height: any Float32 evaluation of a Simplex column divides by the stick remainder 1 − Σx, so the
remainder is kept >= 0.5): Simplex forward x = (½·Dirichlet(5·1_{K−1}), ½) (K = 2, where that is one point: (½·U(0.1, 0.9), the rest)); Simplex inverse y ~ N(−3, 0.5²); Ordered y ~ 0.7·N(0, 1),
the inverse's input the Float64 reference's forward output rounded to the type; cotangents and ladj_bar N(0, 1)."""
import functools
import zlib

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTS = (F32, F64)
DIRS = (False, True)                      # inverse
TRANSFORMS = ("ordered", "simplex")
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
LDS_MAX = 160 * 1024                      # BJX_LDS_MAX of bjx_internal.h
CHUNK_MIN = 50 * 1024                     # launch_seq: whole-column tiles up to this many bytes
VJP_CHUNK_MIN = 80 * 1024                 # simplex_vjp_impl
TABLE_MAX = 40 * 1024                     # the log(K-1-i) table of both chunk walkers
KMAX_TINY = 8


def vw(dt):
    """elements of a 16-byte pack"""
    return 16 // np.dtype(dt).itemsize


def rpl(dt):
    """rows a lane of the tall kernels holds (128 bytes)"""
    return 128 // np.dtype(dt).itemsize


def rows_io(kind, K, inverse):
    """(rows of `in` / `in_bar`, rows of `out` / `out_bar`)"""
    if kind.startswith("ordered"):
        return K, K
    return (K - 1, K) if inverse else (K, K - 1)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


class Form(dict):
    """family + the template arguments that matter; hashable, `.family`"""

    def __hash__(self):
        return hash(tuple(sorted(self.items())))

    @property
    def family(self):
        return self["family"]

    def __repr__(self):
        return self["family"] + "(" + ",".join(f"{k}={v}" for k, v in self.items() if k != "family") + ")"


def _f(family, **kw):
    return Form(family=family, **kw)


def _refused(code):
    return _f("refused", code=code)


# ------------------------------------------------------------------ the dispatchers, restated
def _nsteps(batch, CPS):
    sets = (batch + CPS - 1) // CPS
    return min(max(sets // 4096, 1), 8)


def _tiny(kind, K, batch, has_in=True, has_out=True, inverse=False):
    """bjx_seq_tiny: 1 … 8 rows (Simplex 2 … 8), a lane per column in registers, 256 columns a block"""
    simplex = kind == "simplex"
    if batch <= 0 or K < (2 if simplex else 1) or K > KMAX_TINY or not has_in:
        return None
    if simplex and inverse and not has_out:
        return None
    ri, ro = rows_io(kind, K, inverse)
    return _f("tiny", KI=ri, KO=ro, group=256)


def _quad_try(dt, G, R, batch, al_in, al_out, has_out, in_less, out_less):
    """launch_quad_stream for an op with G lanes a column on a frame of R rows"""
    V, sz = vw(dt), np.dtype(dt).itemsize
    npk = R // (G * V)
    if batch <= 0 or R % (G * V) != 0 or npk < 1 or npk > 8 or not al_in or (has_out and not al_out):
        return None
    cps = 64 // G
    sb = cps * (G * npk * V + V) * sz
    H = 2 if (sb > 9 * 1024 and cps % 2 == 0 and (cps // 2 * (G * npk * V - in_less)) % V == 0 and (cps // 2 * (G * npk * V - out_less)) % V == 0) else 1
    return _f("quad", G=G, NP=npk, H=H, V=V, group=4 * cps)


def _quad(kind, dt, inverse, K, batch, al_in, al_out, has_out):
    if kind == "ordered":
        return _quad_try(dt, 4, K, batch, al_in, al_out, has_out, 0, 0)
    if not inverse:
        return _quad_try(dt, 4, K, batch, al_in, al_out, has_out, 0, 1)
    q = K // (2 * vw(dt))                                            # simplex_impl: two lanes a column unless the frame needs four
    fm = None
    if K % (2 * vw(dt)) != 0 or q > 8 or (q > 4 and q != 8):
        fm = _quad_try(dt, 4, K, batch, al_in, al_out, has_out, 1, 0)
    return fm or _quad_try(dt, 2, K, batch, al_in, al_out, has_out, 1, 0)


def tall_served(dt, rows, inverse_simplex=False, vjp=False, inverse=False):
    """the height conditions of bjx_tall_stream (vjp: bjx_tall_simplex_vjp) -> (G, CPS) or None"""
    r = rpl(dt)
    if rows < 65 or rows > 64 * r:
        return None
    if vjp:
        if inverse and rows > 2048:
            return None
    else:
        if inverse_simplex and (rows > 512 or rows < 129):
            return None
        if dt == F64 and (rows > 512 or inverse_simplex):
            return None
    G = (rows + r - 1) // r
    CPS = 64 // G
    if float(rows) * CPS / (64.0 * r) < 0.6:
        return None
    return G, CPS


def _tall(kind, dt, inverse, K, batch, al_in, al_out, has_out):
    ri, ro = rows_io(kind, K, inverse)
    if batch <= 0:
        return None
    g = tall_served(dt, max(ri, ro), inverse_simplex=(kind == "simplex" and inverse))
    if g is None:
        return None
    G, CPS = g
    V = vw(dt)
    return _f("tall", G=G, CPS=CPS, nsteps=_nsteps(batch, CPS), VIN=bool(al_in and ri % V == 0), VOUT=bool(has_out and al_out and ro % V == 0), group=CPS)


def _launch_seq(kind, dt, inverse, K, batch, al_in, al_out, has_out, ld_in, ld_out):
    sz, V = np.dtype(dt).itemsize, vw(dt)
    ri, ro = rows_io(kind, K, inverse)
    ld_in, ld_out = ld_in or ri, ld_out or ro
    if batch == 0:
        return _f("none")
    rows = max(ri, ro)
    nlk = K - 1 if kind == "simplex" else 0
    smem_w = (64 * (rows | 1) + nlk) * sz
    if smem_w > CHUNK_MIN:
        if 64 * max(ld_in, ld_out) * sz >= 1 << 31:
            return _refused(ERR_UNSUPPORTED)
        v_ok = al_in and (not has_out or al_out) and ld_in % V == 0 and ld_out % V == 0
        C = 256 // sz
        return _f("chunk", V=V if v_ok else 1, TABLE=nlk * sz <= TABLE_MAX, C=C, nchunks=(rows + C - 1) // C, group=64,
                  ragged_in=bool(v_ok and ri % V), ragged_out=bool(v_ok and ro % V))
    assert smem_w <= 64 * 1024
    v_ok = al_in and (not has_out or al_out) and not (ld_in != ri and ld_out != ro)
    return _f("wave", V=V if v_ok else 1, ld_in=ld_in != ri, ld_out=ld_out != ro, group=64)


def _transform(kind, dt, inverse, K, batch, off_in, off_out, ld_in, ld_out, has_out, is_ld):
    sz = np.dtype(dt).itemsize
    if kind == "ordered":
        if K < 1 or batch < 0:
            return _refused(ERR_SHAPE)
    else:
        if K <= 1 or batch < 0:
            return _refused(ERR_SHAPE)
    ri, ro = rows_io(kind, K, inverse)
    if is_ld and (ld_in < ri or ld_out < ro):
        return _refused(ERR_SHAPE)
    al_in, al_out = (off_in * sz) % 16 == 0, (off_out * sz) % 16 == 0
    strided = bool((ld_in and ld_in != ri) or (ld_out and ld_out != ro))
    if not strided:
        fm = _tiny(kind, K, batch, True, has_out, inverse) or _quad(kind, dt, inverse, K, batch, al_in, al_out, has_out) \
            or _tall(kind, dt, inverse, K, batch, al_in, al_out, has_out)
        if fm:
            return fm
    return _launch_seq(kind, dt, inverse, K, batch, al_in, al_out, has_out, ld_in, ld_out)


def _ordered_vjp(dt, inverse, K, batch, al, alias):
    sz, V = np.dtype(dt).itemsize, vw(dt)
    if K < 1 or batch < 0:
        return _refused(ERR_SHAPE)
    if batch == 0:
        return _f("none")
    if K <= KMAX_TINY and alias != "in":
        return _f("tiny_vjp", K=K, group=256)
    packs = (K + V - 1) // V
    if K >= 2 * V and packs <= 64 * 8:
        G = 1
        while G < 64 and G < packs:
            G <<= 1
        R = 1
        while R * G < packs:
            R <<= 1
        UC = 4 if R == 1 else 2 if R == 2 else 1
        return _f("ordered_stream", G=G, R=R, UC=UC, partial=K % V, group=(256 // G) * UC)
    if 2 * 64 * (K | 1) * sz > LDS_MAX:
        if alias == "out_bar":
            return _refused(ERR_ARG)
        if K >= 1024 and alias != "in":
            return _f("ordered_tall", V=V if (K % V == 0 and all(al)) else 1, group=1)
        return _f("ordered_column", group=256)
    return _f("ordered_lane", V=V if all(al) else 1, group=64)


def _simplex_stream(dt, G, K, batch, al):
    V = vw(dt)
    npk = K // (G * V)
    if batch <= 0 or K % (G * V) != 0 or npk < 1 or npk > 8 or not all(al):
        return None
    return _f("simplex_stream", G=G, NP=npk, V=V, group=4 * (64 // G))


def _simplex_vjp(dt, inverse, K, batch, al, alias):
    sz, V = np.dtype(dt).itemsize, vw(dt)
    if K <= 1 or batch < 0:
        return _refused(ERR_SHAPE)
    if batch == 0:
        return _f("none")
    if alias == "out_bar":                                           # in_bar [rows_in, batch] over out_bar [rows_out, batch]: another column's cotangent
        return _refused(ERR_ARG)
    if K <= KMAX_TINY and alias != "in":
        return _f("tiny_vjp", K=K, group=256)
    fm = _simplex_stream(dt, 2 if inverse else 4, K, batch, al)
    if fm is None and inverse:
        fm = _simplex_stream(dt, 4, K, batch, al)
    if fm:
        return fm
    g = tall_served(dt, K, vjp=True, inverse=inverse)
    if g:
        G, CPS = g
        return _f("tall_vjp", G=G, CPS=CPS, nsteps=_nsteps(batch, CPS), VK=bool(all(al) and K % V == 0), VK1=bool(all(al) and (K - 1) % V == 0), group=CPS)
    if (2 * 64 * (K | 1) + K) * sz > VJP_CHUNK_MIN:
        if 64 * K * sz >= 1 << 31:
            return _refused(ERR_UNSUPPORTED)
        CH = 128 // sz
        return _f("chunk_vjp", TABLE=K * sz <= TABLE_MAX, CH=CH, group=64)
    assert (2 * 64 * (K | 1) + K) * sz <= LDS_MAX                    # C stays 64
    return _f("simplex_lane", V=V if all(al) else 1, group=64)


def form(entry, dt, inverse, K, batch, *, off_in=0, off_out=0, off_bar=0, ld_in=0, ld_out=0, want_ladj=True, alias=None, has_out=True):
    """-> Form.  entry: "ordered", "simplex", "ordered_ld", "simplex_ld", "ordered_vjp", "simplex_vjp".  off_*: elements between a 16-byte
    boundary and the base of `in`, of `out` / `in_bar`, of `out_bar`; ld_*: leading dimensions (0: contiguous); alias: None, "in"
    (in_bar == in) or "out_bar" (in_bar == out_bar); has_out: False for the Simplex forward with out = NULL.  `want_ladj` selects the
    LADJ = false ops of the Simplex (the same kernels otherwise).
    families: "none" (batch = 0), "refused" (code), "tiny" (seq_tiny_kernel<KI, KO>), "quad" (quad_stream_kernel: G, NP, H),
    "tall" (tall_stream_kernel: G, CPS, nsteps, VIN, VOUT), "wave" (seq_wave_kernel: V, which sides are strided), "chunk"
    (seq_chunk_kernel: V, TABLE, C), "tiny_vjp", "ordered_stream" (G, R, UC, rows of the partial last pack), "ordered_tall" (V),
    "ordered_column", "ordered_lane" (ordered_vjp_kernel: V), "simplex_stream" (G, NP), "tall_vjp" (tall_simplex_vjp_kernel: G, CPS,
    nsteps, VK, VK1), "chunk_vjp" (simplex_vjp_chunk_kernel: TABLE, CH), "simplex_lane" (simplex_vjp_kernel: V).  `group`: columns of
    the family's column group."""
    dt = np.dtype(dt)
    sz = dt.itemsize
    if entry in ("ordered", "simplex", "ordered_ld", "simplex_ld"):
        fm = _transform(entry.split("_")[0], dt, bool(inverse), K, batch, off_in, off_out, ld_in, ld_out, has_out, entry.endswith("_ld"))
        if entry.startswith("simplex") and fm.family not in ("none", "refused"):
            fm = Form(fm, LADJ=bool(want_ladj))
        return fm
    if alias == "in":
        off_out = off_in
    elif alias == "out_bar":
        off_out = off_bar
    al = tuple((o * sz) % 16 == 0 for o in (off_in, off_bar, off_out))
    return (_ordered_vjp if entry == "ordered_vjp" else _simplex_vjp)(dt, bool(inverse), K, batch, al, alias)


KEY_ARGS = {"tiny": (), "quad": ("G", "NP", "H"), "tall": (), "wave": (), "chunk": ("TABLE",), "tiny_vjp": (), "ordered_stream": ("G", "R"),
            "ordered_tall": (), "ordered_column": (), "ordered_lane": (), "simplex_stream": ("G", "NP"), "tall_vjp": (), "chunk_vjp": ("TABLE",),
            "simplex_lane": (), "none": (), "refused": ("code",)}


def key(fm):
    """what a table row names: the family and the arguments that change with the height alone"""
    return (fm.family,) + tuple(fm[a] for a in KEY_ARGS[fm.family])


# ------------------------------------------------------------------ the tables
# RANGES[(entry, dtype name, inverse)]: (lo, hi, key) — contiguous aligned calls, batch 3, heights 1 … SCAN_MAX in ascending order; every
# maximal run of heights with one key.  lo and hi are the smallest and largest height of the run, lo − 1 and hi + 1 belong to another row.
SCAN_MAX = 11000
_T, _W, _L, _C1, _C0, _X = ("tiny",), ("wave",), ("tall",), ("chunk", True), ("chunk", False), ("refused", ERR_SHAPE)
_TV, _OT, _SL, _LV, _V1, _V0 = ("tiny_vjp",), ("ordered_tall",), ("simplex_lane",), ("tall_vjp",), ("chunk_vjp", True), ("chunk_vjp", False)


def _q(G, NP):
    return ("quad", G, NP, 1)


def _os(G, R):
    return ("ordered_stream", G, R)


def _ss(G, NP):
    return ("simplex_stream", G, NP)


def _comb(first, rest, between, frames, tail):
    """a tiny / refused head, then the quad / stream frames with `between` in the gaps up to 64 rows and `rest` above, then `tail`"""
    rows, lo = list(first), first[-1][1] + 1
    for k, fr in frames:
        b = between if k <= 64 else rest
        rows += [(lo, k - 1, b), (k, k, fr)]
        lo = k + 1
    return rows + [(lo,) + tail[0]] + list(tail[1:])


_ORD32 = _comb([(1, 8, _T)], _L, _W, [(16 * n, _q(4, n)) for n in range(1, 9)], [(1024, _L), (1025, 1228, _C1), (1229, 2048, _L), (2049, SCAN_MAX, _C1)])
_ORD64 = _comb([(1, 8, _T)], _L, _W, [(8 * n, _q(4, n)) for n in range(2, 9)], [(512, _L), (513, SCAN_MAX, _C1)])
_SINV32 = [(16, _q(2, 2)), (24, _q(2, 3)), (32, _q(2, 4)), (40, _q(2, 5)), (48, _q(4, 3)), (56, _q(2, 7)), (64, _q(2, 8)), (80, _q(4, 5)), (96, _q(4, 6)),
           (112, _q(4, 7)), (128, _q(4, 8))]
_SINV64 = [(12, _q(2, 3)), (16, _q(2, 4)), (20, _q(2, 5)), (24, _q(4, 3)), (28, _q(2, 7)), (32, _q(2, 8)), (40, _q(4, 5)), (48, _q(4, 6)), (56, _q(4, 7)),
           (64, _q(4, 8))]
_SV32 = [(1024, _LV), (1025, 1228, _V1), (1229, 2048, _LV), (2049, 10240, _V1), (10241, SCAN_MAX, _V0)]
_SV64 = [(512, _LV), (513, 614, _V1), (615, 1024, _LV), (1025, 5120, _V1), (5121, SCAN_MAX, _V0)]
RANGES = {
    ("ordered", "float32", False): _ORD32, ("ordered", "float32", True): _ORD32,
    ("ordered", "float64", False): _ORD64, ("ordered", "float64", True): _ORD64,
    ("simplex", "float32", False): _comb([(1, 1, _X), (2, 8, _T)], _L, _W, [(16 * n, _q(4, n)) for n in range(1, 9)],
                                         [(1024, _L), (1025, 1228, _C1), (1229, 2048, _L), (2049, 10241, _C1), (10242, SCAN_MAX, _C0)]),
    ("simplex", "float32", True): _comb([(1, 1, _X), (2, 8, _T)], _W, _W, _SINV32, [(512, _L), (513, 10241, _C1), (10242, SCAN_MAX, _C0)]),
    ("simplex", "float64", False): _comb([(1, 1, _X), (2, 8, _T)], _L, _W, [(8 * n, _q(4, n)) for n in range(2, 9)],
                                         [(512, _L), (513, 5121, _C1), (5122, SCAN_MAX, _C0)]),
    ("simplex", "float64", True): _comb([(1, 1, _X), (2, 8, _T)], _W, _W, _SINV64, [(97, _W), (98, 5121, _C1), (5122, SCAN_MAX, _C0)]),
    ("ordered_vjp", "float32", False): [(1, 8, _TV), (9, 16, _os(4, 1)), (17, 32, _os(8, 1)), (33, 64, _os(16, 1)), (65, 128, _os(32, 1)), (129, 256, _os(64, 1)),
                                        (257, 512, _os(64, 2)), (513, 1024, _os(64, 4)), (1025, 2048, _os(64, 8)), (2049, SCAN_MAX, _OT)],
    ("ordered_vjp", "float64", False): [(1, 8, _TV), (9, 16, _os(8, 1)), (17, 32, _os(16, 1)), (33, 64, _os(32, 1)), (65, 128, _os(64, 1)), (129, 256, _os(64, 2)),
                                        (257, 512, _os(64, 4)), (513, 1024, _os(64, 8)), (1025, SCAN_MAX, _OT)],
    ("simplex_vjp", "float32", False): _comb([(1, 1, _X), (2, 8, _TV)], _LV, _SL, [(16 * n, _ss(4, n)) for n in range(1, 9)], _SV32),
    ("simplex_vjp", "float32", True): _comb([(1, 1, _X), (2, 8, _TV)], _LV, _SL, [(8 * n, _ss(2, n)) for n in range(2, 9)] + [(16 * n, _ss(4, n)) for n in range(5, 9)], _SV32),
    ("simplex_vjp", "float64", False): _comb([(1, 1, _X), (2, 8, _TV)], _LV, _SL, [(8 * n, _ss(4, n)) for n in range(2, 9)], _SV64),
    ("simplex_vjp", "float64", True): _comb([(1, 1, _X), (2, 8, _TV)], _LV, _SL, [(4 * n, _ss(2, n)) for n in range(3, 9)] + [(8 * n, _ss(4, n)) for n in range(5, 9)], _SV64),
}
RANGES[("ordered_vjp", "float32", True)] = RANGES[("ordered_vjp", "float32", False)]
RANGES[("ordered_vjp", "float64", True)] = RANGES[("ordered_vjp", "float64", False)]

# served heights the rows above do not single out (the issue's list): the tall kernels at their smallest G, a middle G, the largest G
# and both sides of the `eff` hole (RANGES has those); the chunk walkers at rows mod C in {C − 1, 0, 1} (C = 64 | 32 rows for the
# transforms, 32 | 16 for the pullback; n·C + 1 rows put the HAS_LAST row alone in the last chunk and give the Simplex forward a last
# chunk without an output row); the Ordered pullback stream one row into a new pack; TABLE = false one row in.
EXTRA = {
    ("ordered", "float32"): (79, 81, 500, 2017, 1087, 1088, 1089, 2111, 2112, 2113), ("ordered", "float64"): (79, 81, 250, 497, 543, 544, 545),
    ("simplex", "float32", False): (79, 81, 500, 2017, 1087, 1088, 1089, 2111, 2112, 2113), ("simplex", "float64", False): (79, 81, 250, 497, 543, 544, 545),
    ("simplex", "float32", True): (160, 161, 300, 481, 575, 576, 577), ("simplex", "float64", True): (127, 128, 129),
    ("ordered_vjp", "float32"): (10, 13, 129, 130, 257, 513, 1025, 2047, 2052), ("ordered_vjp", "float64"): (10, 11, 65, 66, 129, 257, 513, 1023, 1026),
    ("simplex_vjp", "float32"): (79, 81, 500, 2017, 1055, 1056, 1057, 10242), ("simplex_vjp", "float64"): (79, 81, 250, 1009, 543, 544, 545, 5122),
}
TALLEST = {"float32": 10242, "float64": 5122}          # the tallest height any case runs: one row into TABLE = false of the transform


def form_heights(entry, dtname, inverse):
    """the heights of the forms test: lo and hi of every RANGES row that is served (the open last row: its lo), and EXTRA"""
    hs = set()
    for lo, hi, k in RANGES[(entry, dtname, bool(inverse))]:
        if k[0] != "refused":
            hs |= {lo, hi} if hi < SCAN_MAX else {lo}
    hs |= set(EXTRA.get((entry, dtname, bool(inverse)), ())) | set(EXTRA.get((entry, dtname), ()))
    return tuple(sorted(h for h in hs if h <= TALLEST[dtname]))


def edge_batches(fm):
    """1, group − 1, group, group + 1 of the family's column group (the chunk walkers: also 3)"""
    g = fm["group"]
    return tuple(sorted(({1, g - 1, g, g + 1} | ({3} if fm.family.startswith("chunk") else set())) - {0}))


# ------------------------------------------------------------------ draws
def _keep(*arrs):
    for a in arrs:
        if a is not None:
            a.setflags(write=False)
    return arrs


def _col(a, dt):
    return np.asfortranarray(np.asarray(a).astype(dt))


@functools.lru_cache(maxsize=None)
def draw(kind, dtname, inverse, K, batch):
    """the input of a transform, (rows_in, batch), rounded to the type, column-major, read-only"""
    dt = np.dtype(dtname)
    r = rng_for("seq", kind, dtname, bool(inverse), K, batch)
    if kind == "ordered":
        y = _col(0.7 * r.normal(size=(K, batch)), dt)
        if not inverse:
            return _keep(y)[0]
        return _keep(_col(ordered_ref(y, False)[0], dt))[0]
    if inverse:
        return _keep(_col(r.normal(-3.0, 0.5, size=(K - 1, batch)), dt))[0]
    x = np.empty((K, batch))
    if K == 2:                                   # ½·Dirichlet(5·1_1) is the single point ½ (image 0, no scale): x_1 = ½·U(0.1, 0.9), the last stick >= 0.55
        x[0] = 0.5 * r.uniform(0.1, 0.9, size=batch)
        x[1] = 1.0 - x[0]
        return _keep(_col(x, dt))[0]
    x[:K - 1] = 0.5 * r.dirichlet(np.full(K - 1, 5.0), size=batch).T
    x[K - 1] = 0.5
    return _keep(_col(x, dt))[0]


@functools.lru_cache(maxsize=None)
def draw_bar(kind, dtname, inverse, K, batch):
    """(out_bar (rows_out, batch), ladj_bar (batch,)): standard normal, rounded to the type"""
    dt = np.dtype(dtname)
    r = rng_for("seq_bar", kind, dtname, bool(inverse), K, batch)
    _, ro = rows_io(kind, K, inverse)
    return _keep(_col(r.normal(size=(ro, batch)), dt), r.normal(size=batch).astype(dt))


def tiled_index(D, batch):
    """column s of a tiled batch holds distinct column s % D"""
    return np.arange(batch, dtype=np.int64) % D


# ------------------------------------------------------------------ Float64 references
def ordered_ref(a, inverse):
    """ordered.jl:36-49 (forward), :64-77 (inverse), :80 and interface.jl:276-281 for the log-det; the row loop in the reference's order,
    vectorised over the batch -> (out, ladj (batch,), floor (batch,)): floor = the largest |term| of the column's log-det sum, which is
    Σ y_i over rows 2 … and can cancel."""
    a = np.asarray(a, np.float64)
    out = np.empty_like(a)
    out[0] = a[0]
    n = a.shape[0]
    if not inverse:
        for i in range(1, n):
            out[i] = out[i - 1] + np.exp(a[i])
        terms = a[1:]
        ladj = terms.sum(axis=0) if n > 1 else np.zeros(a.shape[1])
    else:
        for i in range(1, n):
            out[i] = np.log(a[i] - a[i - 1])
        terms = out[1:]
        ladj = -terms.sum(axis=0) if n > 1 else np.zeros(a.shape[1])
    floor = np.abs(terms).max(axis=0) if n > 1 else np.zeros(a.shape[1])
    return out, ladj, floor


def _logit(z):
    return np.log(z) - np.log1p(-z)


def _simplex_lp(x, eps):
    """lp of simplex.jl:122-138 per column and the largest |term| of its sum"""
    K = x.shape[0]
    z = x[0]
    t = np.log(np.maximum(z, eps)) + np.log(np.maximum(1 - z, eps))
    lp, floor = t.copy(), np.abs(t)
    s = np.zeros(x.shape[1])
    for k in range(1, K - 1):
        s = s + x[k - 1]
        m = np.maximum(1 - s, eps)
        z = x[k] / m
        t = np.log(np.maximum(z, eps)) + np.log(np.maximum(1 - z, eps)) + np.log(m)
        lp += t
        floor = np.maximum(floor, np.abs(t))
    return lp, floor


def simplex_ref(a, inverse, eps):
    """simplex.jl:47-64 (forward: x[K] -> y[K−1], log-det −lp(x)), :102-120 (inverse: y[K−1] -> x[K], log-det +lp(x)), :122-138; the
    row loop in the reference's order, vectorised over the batch; ε a parameter (the Float32 kernels use eps(Float32) by definition)
    -> (out, ladj, floor)"""
    a = np.asarray(a, np.float64)
    N = a.shape[1]
    if not inverse:
        K = a.shape[0]
        y = np.empty((K - 1, N))
        y[0] = _logit(a[0] * (1 - 2 * eps) + eps) + np.log(float(K - 1))
        s = np.zeros(N)
        for k in range(1, K - 1):
            s = s + a[k - 1]
            z = (a[k] + eps) * (1 - 2 * eps) / ((1 + eps) - s)
            y[k] = _logit(z) + np.log(float(K - k - 1))
        lp, floor = _simplex_lp(a, eps)
        return y, -lp, floor
    K = a.shape[0] + 1
    x = np.empty((K, N))
    z = 1 / (1 + np.exp(-(a[0] - np.log(float(K - 1)))))
    x[0] = np.clip((z - eps) / (1 - 2 * eps), 0, 1)
    s = np.zeros(N)
    for k in range(1, K - 1):
        z = 1 / (1 + np.exp(-(a[k] - np.log(float(K - k - 1)))))
        s = s + x[k - 1]
        x[k] = np.clip(((1 + eps) - s) / (1 - 2 * eps) * z - eps, 0, 1)
    s = s + x[K - 2]
    x[K - 1] = np.clip(1 - s, 0, 1)
    lp, floor = _simplex_lp(x, eps)
    return x, lp, floor


def eps_of(dt):
    return float(np.finfo(np.dtype(dt)).eps)


@functools.lru_cache(maxsize=None)
def ref(kind, dtname, inverse, K, batch):
    """(out, ladj, floor) of `draw(kind, dtname, inverse, K, batch)` in Float64 with ε of the type, computed once"""
    a = draw(kind, dtname, inverse, K, batch)
    return _keep(*(ordered_ref(a, inverse) if kind == "ordered" else simplex_ref(a, inverse, eps_of(dtname))))


@functools.lru_cache(maxsize=None)
def ref_vjp(kind, dtname, inverse, K, batch, with_l=True):
    """the Float64 pullback (oracle.ordered_vjp / oracle.simplex_vjp(eps=)) of draw / draw_bar, computed once"""
    from oracle import oracle

    a = np.asarray(draw(kind, dtname, inverse, K, batch), np.float64)
    g, l = draw_bar(kind, dtname, inverse, K, batch)
    g, l = np.asarray(g, np.float64), (np.asarray(l, np.float64) if with_l else None)
    if kind == "ordered":
        out = oracle.ordered_vjp(a, g, l, inverse=bool(inverse))
    else:
        out = oracle.simplex_vjp(a, g, l, inverse=bool(inverse), eps=eps_of(dtname))
    return _keep(np.asarray(out, np.float64))[0]


# ------------------------------------------------------------------ the case tables of the other sections
# (b) alignment: whole-pack heights, one or two per family (K and K − 1 whole packs for the Simplex); offsets in elements
ALIGN_KS = {("transform", "float32"): (8, 24, 25, 32, 256, 257, 1088, 1089), ("transform", "float64"): (8, 12, 13, 16, 256, 257, 544, 545),
            ("ordered_vjp", "float32"): (8, 63, 64, 2052), ("ordered_vjp", "float64"): (8, 63, 64, 1026),
            ("simplex_vjp", "float32"): (8, 24, 25, 32, 256, 257, 1056, 1057), ("simplex_vjp", "float64"): (8, 12, 13, 16, 256, 257, 544, 545)}
OFFSETS = {"float32": (1, 2), "float64": (1,)}


def align_ks(entry, dtname):
    return ALIGN_KS[("transform" if entry in TRANSFORMS else entry, dtname)]


def offset_patterns(entry, off):
    """(off_in, off_out | off_in_bar, off_out_bar): each pointer alone, and all of them"""
    if entry in TRANSFORMS:
        return ((off, 0, 0), (0, off, 0), (off, off, 0))
    return ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off))


# (c) leading dimensions: a wave-kernel height, the last one before `chunk_min`, the first of the chunk walker, one more; batch 67
LD_KS = {("ordered", "float32"): (24, 199, 200, 257), ("simplex", "float32"): (24, 100, 195, 196, 200, 201),
         ("ordered", "float64"): (12, 99, 100, 129), ("simplex", "float64"): (12, 50, 97, 98, 100, 101)}
LD_BATCH = 67


def ld_variants(dt, ri, ro):
    """(ld_in, ld_out): only `in` strided, only `out`, both — with whole-pack and with odd leading dimensions"""
    V = vw(dt)
    wp = lambda r: (r + V - 1) // V * V + V
    odd = lambda r: (r | 1) + 2
    return ((wp(ri), ro), (ri, wp(ro)), (wp(ri), wp(ro)), (odd(ri), ro), (ri, odd(ro)), (odd(ri), odd(ro)), (wp(ri), odd(ro)))


# (d) loop trips of the tall kernels: CPS = 2 (Simplex inverse, Float32: 4) keeps every buffer under 70 MB; a whole-pack and an odd height
TRIP_D = 37
TRIPS = [("ordered", "float32", False, 708), ("ordered", "float32", False, 707), ("ordered", "float32", True, 708), ("ordered", "float32", True, 707),
         ("ordered", "float64", False, 356), ("ordered", "float64", False, 355), ("ordered", "float64", True, 356), ("ordered", "float64", True, 355),
         ("simplex", "float32", False, 708), ("simplex", "float32", False, 707), ("simplex", "float64", False, 356), ("simplex", "float64", False, 355),
         ("simplex", "float32", True, 388), ("simplex", "float32", True, 389),
         ("simplex_vjp", "float32", False, 708), ("simplex_vjp", "float32", False, 707), ("simplex_vjp", "float32", True, 708), ("simplex_vjp", "float32", True, 707),
         ("simplex_vjp", "float64", False, 356), ("simplex_vjp", "float64", False, 355), ("simplex_vjp", "float64", True, 356), ("simplex_vjp", "float64", True, 355)]
TRIP3 = ("ordered", "float32", False, 676)
ORDERED_TALL_TRIP_K = {"float32": 2052, "float64": 1026}


def trip_batch(CPS, nsteps=2):
    """nsteps·4096 sets, one more full set and one column: the last wave walks a full set and then a ragged one"""
    return nsteps * 4096 * CPS + CPS + 1


# (f) aliasing
ALIAS_IN_KS = {("ordered_vjp", "float32"): (3, 7, 8, 64, 301, 2048, 2049, 2052), ("ordered_vjp", "float64"): (3, 4, 8, 64, 301, 1024, 1025, 1026),
               ("simplex_vjp", "float32"): (5, 8, 24, 32, 256, 257, 1056), ("simplex_vjp", "float64"): (5, 8, 12, 16, 256, 257, 544)}
ALIAS_OUT_BAR_SERVED = {"float32": (3, 8, 64, 301, 2048), "float64": (3, 8, 64, 301, 1024)}       # bjx_ordered_vjp; the last: the tallest served
ALIAS_OUT_BAR_REFUSED = {"float32": 2049, "float64": 1025}

# (g) the 2 GiB range of one buffer descriptor: 64 · ld · sizeof(T) < 2³¹
LD_REFUSED = {"float32": 1 << 23, "float64": 1 << 22}
