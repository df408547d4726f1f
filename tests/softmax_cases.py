"""Case table, reference, checker and route restatement for csrc/softmax.hip: ``pthip_softmax``, ``pthip_logsumexp_rows``,
``pthip_logsumexp_cols`` and ``pthip_softmax_cols``.

Pure NumPy: imported by tests/test_gpu_tiers_softmax.py (GPU), tests/_softmax_tiers_worker.py (device runners and the child
process of the switch tests) and tests/test_softmax_cases.py (the CPU self-test of table, checker and routes).

Layout.  Every operand is seen as slices reduced over axis 1: a row matrix is ``(rows, cols)``, a column operand is
``(batch, R, C)``.  ``n`` is the reduced extent.

Reference.  In ``np.longdouble`` for float64 operands and in float64 for float32 operands (``blas_cases.hp_type``), the
stabilised definition: ``m = max``, ``sh = 0 if isinf(m) else m``, ``s = sum exp(x - sh)``; softmax ``exp(x - m) / s``,
log-softmax ``(x - m) - log s``, log-sum-exp ``log s + sh``.  Non-finite slices are stated by rule, not computed: an
all ``-inf`` slice gives LSE ``-inf`` and an all-NaN (log-)softmax; a NaN anywhere makes everything NaN; a ``+inf`` entry
gives LSE ``+inf`` and an all-NaN softmax, and in log-softmax NaN at the ``+inf`` entry and ``-inf`` or NaN elsewhere
(scipy's ``log_softmax`` and the ``(x - max) - log(sum)`` graph differ there).

Bound.  ``u`` the unit roundoff of the operand type, ``ua = 2^-53`` that of the accumulator, ``d = x - m``, ``c_exp`` /
``c_log`` the ulp allowance of one transcendental call (1 for the file's own fp64 exp, csrc/exp_device.h; 2 for the
device library's ``exp``, ``expf``, ``logf`` and ``log``), ``lv`` the number of merge levels a partial state passes
(each multiplies the partial sum by one more ``exp``).  No further factor:

    softmax:          |err| <= (|d| u + c_exp u + n ua + 3 u + lv c_exp u) * want + (c_exp + 1) * eta
    LSE, log-softmax: |err| <= (c_exp u + n ua + u + lv c_exp u) + c_log u |log s| + u (|m| + |want|)

``3 u``: the sum rounded to T, the reciprocal, the product.  ``eta`` is the smallest subnormal of the operand type: a
result below the normal range is rounded to a multiple of ``eta`` when the exp is scaled (c_exp ulps of a subnormal are
c_exp * eta) and once more by the product, and no relative bound can hold there; it is 5e-324 / 1.4e-45, invisible for
any normal result.  Where an entry is ``-inf`` the softmax is exactly 0 and the log-softmax exactly ``-inf``.

Leaks.  The operand sits in a NaN-filled parent (in front of its first and behind its last element) and every output
between sentinel bytes with NaN bits in between (tests/_softmax_tiers_worker.py), so a read past either end of the
matrix shows up as NaN and a write out of range as a changed sentinel.  A read past the end of one row is the first
element of the next: the generators below make that visible.

Inputs.  ``flat``: uniform in [-0.45 c, c], c in {1, 7/8, 3/4} by slice, so every element carries at least 1 / (e^2 n) of
its sum and neighbouring slices have different maxima; the minimum (-1 and -1/2 in turn) sits at the last valid position
and at the last position of the first pack, wave-row and visit.  ``ramp``: an ascending ramp over [-800, 0] (fp64) / [-110, 0] (fp32)
with the maximum at the last position (every earlier partial state is rescaled), planted values whose ``exp(x - m)`` is
subnormal, just above and just below the flush threshold, and ``-inf`` entries.  ``shifted``: ``flat + 1e6`` / ``+ 1e3``.
"""
import hashlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from blas_cases import DTYPES, hp_type, unit_roundoff, vec_elems  # noqa: F401

GENS = ("flat", "ramp", "shifted")
UA = 2.0 ** -53
NUM_CU = 256
BLOCK = 256
SM_PER_CU, LSE_WAVE_PER_CU, LSE_ROWS_PER_CU = 3, 3, 8
COL_PER_CU_ONE, COL_PER_CU_MANY = 2, 8
STREAM_U = 4


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------
# Python restatement of the host dispatch of csrc/softmax.hip (softmax_typed, lse_rows_typed, col_geometry,
# colstat_typed).  ``aligned``: x and (where the entry point looks at it) out sit on 16-byte boundaries.
# ---------------------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "kernel VPL V G nwaves levels", defaults=(0, 0, 0, 0, 0))


def _nwaves(rows, per_cu):
    return min(ceil_div(rows, 4), NUM_CU * per_cu) * 4


def softmax_route(dt, rows, cols, aligned, per_cu=SM_PER_CU):
    """kernel of ``pthip_softmax``: small (V = 1: 16-byte staging on) / block / reg (VPL, V) / wave"""
    VW = vec_elems(dt)
    if cols <= 16:
        return Route("small", 16, 1 if aligned else 0)
    if rows < 2 * NUM_CU and cols >= 4096:
        return Route("block")
    nw = _nwaves(rows, per_cu)
    if cols % VW == 0 and aligned:
        for vpl in (2, 8, 16):
            if cols <= 64 * vpl * VW:
                return Route("reg", vpl, VW, 0, nw)
    for vpl in (4, 16, 32):
        if cols <= 64 * vpl:
            return Route("reg", vpl, 1, 0, nw)
    return Route("wave", 0, 0, 0, nw)


def lse_small_lds(dt, cols):
    return BLOCK * (cols | 1) * np.dtype(dt).itemsize


def lse_rows_route(dt, rows, cols, aligned, wave_per_cu=LSE_WAVE_PER_CU, rows_per_cu=LSE_ROWS_PER_CU):
    """kernel of ``pthip_logsumexp_rows``: small (VPL = MAXC) / wave (VPL, V) / stream (V, G)"""
    VW = vec_elems(dt)
    if cols <= 32:
        return Route("small", 8 if cols <= 8 else 16 if cols <= 16 else 32, 1)
    packs = cols % VW == 0 and aligned
    nw = _nwaves(rows, wave_per_cu)
    if packs:
        for vpl in (2, 4, 8, 16):
            if cols <= 64 * vpl * VW:
                return Route("wave", vpl, VW, 0, nw)
    else:
        for vpl in (4, 16):
            if cols <= 64 * vpl:
                return Route("wave", vpl, 1, 0, nw)
    V = VW if packs else 1
    G = ceil_div(cols, 64 * V * STREAM_U)
    # every visit rescales the lane's sum once, the butterfly at the end of the row once more
    return Route("stream", STREAM_U, V, G, _nwaves(rows, rows_per_cu), G + 1)


ColGeom = namedtuple("ColGeom", "V TX TY ctiles rows_per nsplit L")


def col_pack_width(dt, C, aligned):
    VW = vec_elems(dt)
    return VW if (C % VW == 0 and aligned) else 1


def col_geometry(dt, batch, R, C, aligned, per_cu=None):
    V = col_pack_width(dt, C, aligned)
    CP = C // V
    if CP <= BLOCK:
        TX, TY, ctiles = CP, BLOCK // CP, 1
    else:
        TX, TY, ctiles = 64, BLOCK // 64, ceil_div(CP, 64)
    if not per_cu:
        per_cu = COL_PER_CU_MANY if ctiles > 1 else COL_PER_CU_ONE
    want = ceil_div(NUM_CU * per_cu, ctiles * batch)
    want = min(want, ceil_div(R, TY * 16))
    want = min(max(want, 1), 4096)
    rows_per = ceil_div(R, want)
    nsplit = ceil_div(R, rows_per)
    L = 64
    while L > 1 and (batch * C * L > 32768 or L > nsplit):
        L >>= 1
    return ColGeom(V, TX, TY, ctiles, rows_per, nsplit, L)


def col_visit_u(dt, V):
    """packs per visit of col_lse_partial_kernel"""
    return 8 if (V == 1 or np.dtype(dt).itemsize == 8) else 4


def col_levels(dt, g):
    """merge levels of a column sum: the visits of a row lane, the LDS tree over row lanes, the splits a finish lane
    folds, the butterfly over finish lanes"""
    visits = ceil_div(ceil_div(g.rows_per, g.TY), col_visit_u(dt, g.V))
    tree = int(np.ceil(np.log2(g.TY))) if g.TY > 1 else 0
    return visits + tree + ceil_div(g.nsplit, g.L) + int(np.log2(g.L))


def colstat_workspace(dt, batch, R, C, per_cu=None):
    """``pthip_colstat_workspace`` restated: the larger of the two pack widths' needs"""
    most = 0
    for al in (False, True):
        g = col_geometry(dt, batch, R, C, al, per_cu)
        most = max(most, batch * g.nsplit * C * 16 + batch * C * 16)
    return most + 256


def staging_magic(cols):
    return ((1 << 20) + cols - 1) // cols


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    entry: str   # "softmax" | "lse_rows" | "cols"
    name: str
    shape: tuple  # (rows, cols) | (batch, R, C)
    only: str = ""   # restricted to one dtype where the other reaches nothing new at that size
    note: str = ""

    @property
    def n(self):
        return self.shape[1]

    @property
    def nslices(self):
        return self.shape[0] if len(self.shape) == 2 else self.shape[0] * self.shape[2]


def _rc(entry, pairs, only="", note=""):
    return tuple(Case(entry, f"{r}x{c}", (r, c), only, note) for r, c in pairs)


SOFTMAX_CASES = (
    # thread per row: every width class against a full, a partial and a one-row last workgroup
    _rc("softmax", [(r, c) for c in (1, 2, 3, 15, 16) for r in (1, 255, 256, 257, 513)])
    # every softmax_wave_reg_kernel<VPL, V> at its upper edge and one step above the edge below (5 rows: a partial workgroup)
    + _rc("softmax", [(5, c) for c in (17, 18, 20, 255, 256, 257, 258, 512, 516, 1023, 1024, 1025, 1026, 2047, 2048, 2052)])
    + _rc("softmax", [(1, 18), (1, 20), (1, 257), (1, 2049)], note="one row")
    + _rc("softmax", [(512, 4096)], only="float32", note="reg<16, 4> at its edge: 512 rows keep it off the block kernel")
    # wave kernel
    + _rc("softmax", [(5, 2049), (5, 2050)])
    + _rc("softmax", [(512, 4100)], only="float32")
    + _rc("softmax", [(512, 4097)], note="512 rows keep 4097 columns off the block kernel")
    # workgroup per row
    + _rc("softmax", [(r, c) for r in (1, 3, 511) for c in (4096, 4097)])
    # nwaves + 1 rows: wave 0 takes a second row and the prefetch behind it clamps to the last row
    + _rc("softmax", [(3073, c) for c in (17, 18, 20, 257, 258)])
    # 2 * nwaves + 6: wave 0 finishes a row from each buffer and then a third
    + _rc("softmax", [(6150, c) for c in (17, 18, 20, 258)])
)
# PTHIP_SOFTMAX_WG_PER_CU=1: 1024 waves, 2051 = 2 * 1024 + 3 rows for the wide tiers
SOFTMAX_CHILD_CASES = _rc("softmax", [(2051, 1025), (2051, 1026), (2051, 2049)]) + _rc("softmax", [(2051, 2052)], only="float32")

LSE_ROWS_CASES = (
    _rc("lse_rows", [(r, c) for c in (1, 8, 9, 16, 17, 24, 31, 32) for r in (1, 256, 257)])
    + _rc("lse_rows", [(70001, c) for c in (1, 8, 9, 16, 17, 24, 31, 32)], note="274 workgroups")
    # every lse_rows_wave_kernel<VPL, V> at both edges
    + _rc("lse_rows", [(5, c) for c in (33, 34, 36, 255, 256, 257, 258, 512, 514, 516, 1023, 1024, 1026, 1028, 2048, 2052, 4096)])
    + _rc("lse_rows", [(1, 34), (3073, 33), (3073, 36), (6150, 258)])
    # stream kernel (U = 4): V = 1 from 1025 columns, V = VW past 64 * 16 * VW.  Exactly G * 64 * V * U columns, one
    # over, one lane of the last visit live; G odd and even.
    + _rc("lse_rows", [(5, c) for c in (1025, 1279, 1280, 1281, 1537)], note="V = 1: G = 5, 5, 5, 6, 7 (1280: behind a misaligned pointer)")
    + _rc("lse_rows", [(5, c) for c in (2050, 2560, 2562, 3072, 3074)], only="float64", note="V = 2: G = 5, 5, 6, 6, 7")
    + _rc("lse_rows", [(5, c) for c in (4100, 5120, 5124, 6144, 6148)], only="float32", note="V = 4: G = 5, 5, 6, 6, 7")
    + _rc("lse_rows", [(1, 1281), (8195, 1025)], only="float32", note="8192 waves: wave 0..2 walk to a second row")
)
# PTHIP_LSE_WAVE_WG_PER_CU=1 / PTHIP_LSE_ROWS_WG_PER_CU=1: 1024 waves, 2051 rows
LSE_WAVE_CHILD_CASES = _rc("lse_rows", [(2051, 257), (2051, 1024), (2051, 1026)])
LSE_STREAM_CHILD_CASES = (_rc("lse_rows", [(2051, 1025), (2051, 1281)]) + _rc("lse_rows", [(2051, 2562)], only="float64")
                          + _rc("lse_rows", [(2051, 4100)], only="float32"))
LSE_SMALL_CHILD_CASES = _rc("lse_rows", [(257, 8), (257, 9), (513, 24), (257, 31), (257, 32)])


def _col(pairs, only="", note=""):
    return tuple(Case("cols", f"{b}x{r}x{c}", (b, r, c), only, note) for b, r, c in pairs)


COL_CASES = (
    # one tile: TX dividing 256 or not, TY = 1, R below TY, R = 2
    _col([(1, 2, 2), (1, 2, 16), (1, 300, 8), (1, 700, 10), (1, 700, 14), (3, 257, 7), (1, 130, 100), (1, 130, 200), (1, 37, 256), (1, 40, 129),
          (1, 9, 5), (2, 33, 512), (1, 3, 1), (1, 1000, 1)])
    # several tiles: a multiple of 64 packs and a partial last tile
    + _col([(1, 67, 1024), (1, 130, 257), (1, 33, 1025), (3, 100, 514), (1, 2, 2050), (1, 67, 1028), (1, 33, 2048)])
    # the last split short, shorter than TY; a visit count ending in each buffer; nsplit = 1, <= L, > L; L cut by ncols
    + _col([(1, 4099, 5), (1, 20001, 10), (1, 4100, 128), (1, 259, 2050), (3, 1000, 3), (1, 100, 600), (1, 1025, 100)])
)
# PTHIP_COL_WG_PER_CU=8 on one tile: nsplit = 1025 > 8 * 64, the finish loop runs three times
COL_CHILD_CASES = _col([(1, 16400, 255), (1, 4099, 5), (1, 130, 257)])

NONFINITE_CASES = (
    Case("softmax", "nf_small", (12, 5)), Case("softmax", "nf_reg", (12, 100)), Case("softmax", "nf_wave", (12, 2050)),
    Case("softmax", "nf_block", (12, 4096)),
    Case("lse_rows", "nf_small", (12, 9)), Case("lse_rows", "nf_wave", (12, 100)), Case("lse_rows", "nf_stream1", (12, 1025)),
    Case("lse_rows", "nf_streamV", (12, 4100)),
    Case("cols", "nf_tile1", (1, 40, 12)), Case("cols", "nf_tile1_split", (1, 700, 12)), Case("cols", "nf_tiled", (1, 40, 1030)),
)
# one flat case per kernel family, run twice
DETERMINISM_CASES = (
    Case("softmax", "det", (257, 10)), Case("softmax", "det", (300, 258)), Case("softmax", "det", (7, 2050)), Case("softmax", "det", (3, 4097)),
    Case("lse_rows", "det", (257, 9)), Case("lse_rows", "det", (300, 258)), Case("lse_rows", "det", (7, 5124)),
    Case("cols", "det", (1, 4099, 10)), Case("cols", "det", (1, 1031, 2050)),
)

ALL_CASES = SOFTMAX_CASES + LSE_ROWS_CASES + COL_CASES
CHILD_CASES = SOFTMAX_CHILD_CASES + LSE_WAVE_CHILD_CASES + LSE_STREAM_CHILD_CASES + LSE_SMALL_CHILD_CASES + COL_CHILD_CASES


def dtypes_of(case):
    return tuple(dt for dt in DTYPES if case.only in ("", dt))


def whats(case):
    """what is computed per entry: (entry point, LOG) pairs named"""
    return {"softmax": ("softmax", "log_softmax"), "lse_rows": ("lse",), "cols": ("lse", "softmax", "log_softmax")}[case.entry]


MISALIGNMENTS = ("x", "out", "both")


def misalignment(case, index):
    """which pointer sits one element into its 16-byte-aligned parent in the misaligned run of a case: x, out or both in
    turn over the table (x where the entry point looks at nothing else)"""
    return "x" if case.entry == "lse_rows" else MISALIGNMENTS[index % 3]


def route_aligned(case, what, mis):
    """does the dispatch see aligned pointers for this run?"""
    if mis == "aligned":
        return True
    if what == "lse" or (case.entry == "lse_rows"):
        return mis == "out"  # out is never tested there
    return False


def route_of(case, dt, what, mis, **kw):
    al = route_aligned(case, what, mis)
    if case.entry == "softmax":
        return softmax_route(dt, *case.shape, al, **kw)
    if case.entry == "lse_rows":
        return lse_rows_route(dt, *case.shape, al, **kw)
    return col_geometry(dt, *case.shape, al, **kw)


def tier_name(case, dt, r, what):
    """the kernel instance a run reaches, as the profile names it"""
    if case.entry == "cols":
        return f"col_{'lse' if what == 'lse' else what}<{dt}, V={r.V}, {'one tile' if r.ctiles == 1 else 'tiled'}>"
    k = {"softmax": "softmax", "lse_rows": "lse_rows"}[case.entry]
    log = ", LOG" if what == "log_softmax" else ""
    if r.kernel == "reg" or (case.entry == "lse_rows" and r.kernel == "wave"):
        return f"{k}_{'wave_reg' if case.entry == 'softmax' else 'wave'}<{dt}{log}, {r.VPL}, {r.V}>"
    if r.kernel == "stream":
        return f"{k}_stream<{dt}, V={r.V}>"
    if r.kernel == "small":
        return f"{k}_small<{dt}{log}, {r.VPL}>"
    return f"{k}_{r.kernel}<{dt}{log}>"


def c_exp_of(case, dt, r):
    """ulp allowance of one exp call in the kernel a run reaches: csrc/exp_device.h's own fp64 exp is held to 1 ulp;
    softmax_wave_kernel and softmax_block_kernel call the device library's ``exp``; ``expf`` everywhere in float32"""
    if np.dtype(dt) == np.float32:
        return 2.0
    if case.entry == "softmax" and r.kernel in ("wave", "block"):
        return 2.0
    return 1.0


C_LOG = 2.0


def levels_of(case, dt, r):
    return col_levels(dt, r) if case.entry == "cols" else r.levels


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def plant_positions(dt, n, extra=()):
    """where the slice minimum of ``flat`` goes: the last valid position; the last position of the first 16-byte pack, of
    the first row of packs a wave reads (V = 1 and V = VW) and of the first visit of the stream kernel; ``extra``"""
    VW = vec_elems(dt)
    cand = {n - 1, VW - 1, 63, 64 * VW - 1, 64 * STREAM_U - 1, 64 * STREAM_U * VW - 1, *extra}
    return sorted(p for p in cand if 1 <= p < n)


def _col_extra(case, dt):
    """column operands: the last row of the first and second split, the last row of the first visit"""
    out = set()
    for al in (True, False):
        g = col_geometry(dt, *case.shape, al)
        out |= {g.rows_per - 1, 2 * g.rows_per - 1, g.TY * col_visit_u(dt, g.V) - 1, g.TY - 1}
    return out


RAMP_LO = {"float64": -800.0, "float32": -110.0}
# exp(x - m): subnormal, subnormal next to the flush threshold, below it (exactly 0)
RAMP_PLANT = {"float64": (-730.0, -744.9, -745.5), "float32": (-95.0, -103.5, -104.5)}
SHIFT = {"float64": 1.0e6, "float32": 1.0e3}


def slices(case, dt, gen):
    """(nslices, n) values in ``dt``: slice k is row k of a row matrix, column (b, c) = divmod(k, C) of a column operand"""
    dt = np.dtype(dt)
    N, n = case.nslices, case.n
    rng = np.random.default_rng([GENS.index(gen), N, n, dt.itemsize])
    k = np.arange(N)
    if gen in ("flat", "shifted"):
        S = rng.uniform(-0.45, 1.0, (N, n)) * (1.0 - (k % 3) / 8.0)[:, None]
        if n >= 2:  # (the minimum alternates between -1 and -1/2, so the same position of the next slice holds another value)
            S[:, plant_positions(dt, n, _col_extra(case, dt) if case.entry == "cols" else ())] = (-1.0 + 0.5 * (k % 2))[:, None]
        if gen == "shifted":
            S = S.astype(dt) + dt.type(SHIFT[dt.name])
        return S.astype(dt)
    lo = RAMP_LO[dt.name]
    mk = -0.5 * (k % 7)
    base = lo * (1.0 - np.arange(n) / (n - 1)) if n > 1 else np.zeros(1)
    S = base[None, :] - rng.uniform(0.0, 0.25, (N, n))
    S[:, n - 1] = 0.0
    if n >= 8:
        for j, v in enumerate(RAMP_PLANT[dt.name]):
            S[:, 1 + j] = v
        S[:, n // 3] = -np.inf
        S[::2, 0] = -np.inf
    return (S + mk[:, None]).astype(dt)


def arrange(case, S):
    """the operand as the entry point takes it"""
    if case.entry != "cols":
        return S
    b, R, Cc = case.shape
    return np.ascontiguousarray(S.reshape(b, Cc, R).transpose(0, 2, 1))


def values(case, dt, gen):
    return arrange(case, slices(case, dt, gen))


def embed(x, off):
    """(parent, index of the first element): ``x`` contiguous behind ``4 * VW + off`` NaNs, 8 NaNs behind it"""
    lead = 4 * vec_elems(x.dtype) + off
    parent = np.full(lead + x.size + 8, np.nan, dtype=x.dtype)
    parent[lead:lead + x.size] = x.reshape(-1)
    return parent, lead


# ---------------------------------------------------------------------------------------------------------------
# reference and checker
# ---------------------------------------------------------------------------------------------------------------
class Stats:
    """per-slice high-precision statistics of an operand (reduced over axis 1), computed once and shared"""

    def __init__(self, x):
        self.dt = x.dtype
        H = hp_type(x.dtype)
        self.nan = np.isnan(x).any(axis=1, keepdims=True)
        self.pinf = (x == np.inf).any(axis=1, keepdims=True) & ~self.nan
        self.ninf = (x == -np.inf).all(axis=1, keepdims=True)
        self.special = self.nan | self.pinf | self.ninf
        xh = np.where(self.special, H(0), x.astype(H))
        self.x, self.xh = x, xh
        self.m = xh.max(axis=1, keepdims=True)
        self.d = xh - self.m
        self.e = np.exp(self.d)
        self.s = self.e.sum(axis=1, keepdims=True)
        self.logs = np.log(self.s)
        self.n = x.shape[1]


@dataclass
class Expect:
    want: np.ndarray
    bound: np.ndarray
    must_nan: np.ndarray
    ninf_or_nan: np.ndarray


def expect(st, what, dt, c_exp, levels=0):
    """(want, bound, rule masks) of ``what`` in {"lse", "softmax", "log_softmax"}; ``lse`` has axis 1 removed"""
    H = hp_type(dt)
    u, ua = H(unit_roundoff(dt)), H(UA)
    eta = H(np.finfo(dt).smallest_subnormal)
    rel_s = c_exp * u + st.n * ua + levels * c_exp * u
    if what == "lse":
        want = st.logs + st.m
        bound = (rel_s + u) + C_LOG * u * np.abs(st.logs) + u * (np.abs(st.m) + np.abs(want))
        want = np.where(st.pinf, H(np.inf), np.where(st.ninf, H(-np.inf), want))
        sq = lambda a: a[:, 0]  # noqa: E731
        return Expect(sq(want), sq(bound), sq(st.nan), sq(np.zeros_like(st.nan)))
    shape = st.x.shape
    lowest = np.broadcast_to(st.x == -np.inf, shape) & ~st.special
    if what == "softmax":
        want = st.e / st.s
        with np.errstate(invalid="ignore"):
            bound = (np.abs(st.d) * u + rel_s + 3 * u) * want + (c_exp + 1) * eta
        want = np.where(lowest, H(0), want)
        bound = np.where(lowest, H(0), bound)
        return Expect(want, bound, np.broadcast_to(st.special, shape), np.zeros(shape, bool))
    want = st.d - st.logs
    with np.errstate(invalid="ignore"):
        bound = (rel_s + u) + C_LOG * u * np.abs(st.logs) + u * (np.abs(st.m) + np.abs(want))
    bound = np.where(lowest, H(0), np.broadcast_to(bound, shape))
    pinf_here = np.broadcast_to(st.pinf, shape)
    at_inf = pinf_here & (st.x == np.inf)
    must_nan = np.broadcast_to(st.nan | st.ninf, shape) | at_inf
    return Expect(want, bound, must_nan, pinf_here & ~at_inf)


def check(got, ex, dt, what=""):
    """Assert the rules on non-finite slices, exact values where the reference is infinite or the bound 0, and
    ``|got - want| <= bound`` elsewhere (a NaN fails).  Returns the worst ratio of error to bound."""
    got = np.asarray(got)
    assert got.dtype == np.dtype(dt), f"{what}: dtype {got.dtype}, expected {dt}"
    assert got.shape == ex.want.shape, f"{what}: shape {got.shape}, expected {ex.want.shape}"
    if got.size == 0:
        return 0.0
    gh = got.astype(ex.want.dtype)
    gnan = np.isnan(got)
    ruled = ex.must_nan | ex.ninf_or_nan
    exact = ~ruled & (~np.isfinite(ex.want) | (ex.bound == 0))
    with np.errstate(invalid="ignore"):
        err = np.abs(gh - ex.want)
        ok = np.where(ex.must_nan, gnan, np.where(ex.ninf_or_nan, gnan | (got == -np.inf), np.where(exact, gh == ex.want, err <= ex.bound)))
    free = ~ruled & ~exact
    if not np.all(ok):
        idx = tuple(int(v) for v in np.argwhere(~ok)[0])
        rule = "NaN" if ex.must_nan[idx] else "-inf or NaN" if ex.ninf_or_nan[idx] else repr(ex.want[idx])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {got.size} elements outside the bound; first at {idx}: got {got[idx]!r}, "
                             f"want {rule}, |err| {err[idx]!r} > bound {ex.bound[idx]!r}; worst |err|/bound {_ratio(err, ex.bound, free):.3g}")
    return _ratio(err, ex.bound, free)


def _ratio(err, bound, free):
    sel = free & (bound > 0)
    if not np.any(sel):
        return 0.0
    r = err[sel] / bound[sel]
    return float("inf") if not np.all(np.isfinite(r)) else float(np.max(r))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------
# non-finite plants: slice index -> what is planted; every other slice must come out bit-identical to the clean call
# ---------------------------------------------------------------------------------------------------------------
def plant_nonfinite(case, S):
    """a copy of the (nslices, n) values with: slice 1 all -inf; +inf first in slice 3, last in slice 5; NaN last in slice 7;
    -inf entries inside slice 8; NaN in the last position of the last slice (the element every clamped load of a padding
    lane, of a row past the split and of a prefetch past the last row re-reads).  Returns (values, planted slices)."""
    N, n = S.shape
    assert N >= 12
    P = S.copy()
    P[1, :] = -np.inf
    P[3, 0] = np.inf
    P[5, n - 1] = np.inf
    P[7, n - 1] = np.nan
    P[8, 0] = -np.inf
    P[8, n // 2] = -np.inf
    P[N - 1, n - 1] = np.nan
    return P, (1, 3, 5, 7, 8, N - 1)
