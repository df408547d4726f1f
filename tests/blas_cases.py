"""Case table, reference and checker for the dense BLAS tier (csrc/gemm.hip, csrc/gemm_skinny.hip, csrc/gemv.hip).

Pure NumPy: imported by tests/test_gpu_tiers_blas.py (GPU), tests/_blas_tiers_worker.py (the child process of the
switch tests) and tests/test_blas_cases.py (the CPU self-test of the checker).

Reference.  ``alpha * (A @ B) + beta * C`` with ``alpha`` and ``beta`` first rounded to the operand dtype (the library
casts them with ``(T)alpha``), computed in float64 for float32 operands and in ``np.longdouble`` for float64 operands (a
64-bit mantissa on x86-64: 2^-11 of a double ulp per operation).

Bound.  With ``u = eps / 2`` every summation order of a length-K dot product, in FMAs or in mul + add, satisfies
``|err| <= gamma_K * sum |a||b|``; the alpha multiply and the ``beta * C`` update add three roundings.  The checker
requires, elementwise and with no further factor,

    |got - want| <= (K + 4) * u * (|alpha| * (|A| @ |B|) + |beta| * |C|)

and ``got == 0`` exactly where that bound is 0 (K = 0 with beta = 0).  A split-K product is a summation order like any
other (slab sums of k_s terms, then s - 1 additions: k_s + s - 1 <= K), so the slabs of ``pthip_gemm_partials`` added in
ascending order meet the same bound.  Gemv: K is N.  ``pthip_gemv_finish``: K is nparts, over |part|.  Ger: three
roundings over ``|A| + |alpha x y|``.  Inputs are standard normal: nothing underflows.

Leaks.  Every operand is a strided view into a parent whose other elements (pitch padding, the gap in front of the first
element, the tail, the elements a stride skips) are NaN, so an out-of-range element that enters a sum shows up as NaN,
which no bound admits.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

DTYPES = ("float64", "float32")
ALPHA, BETA = -0.75, 1.25


def unit_roundoff(dt):
    return float(np.finfo(dt).eps) / 2.0


def hp_type(dt):
    return np.float64 if np.dtype(dt) == np.float32 else np.longdouble


def vec_elems(dt):
    """elements of a 16-byte vector: the alignment unit of the staging paths"""
    return 16 // np.dtype(dt).itemsize


# ---------------------------------------------------------------------------------------------------------------
# Python restatement of the dispatch of csrc/gemm.hip (split_plan / launch), used to keep the table honest on the CPU.
# The GPU test asserts the same routes from what the library reports (pthip_gemm_nslabs, pthip_launch_count).
# ---------------------------------------------------------------------------------------------------------------
NUM_CU = 256


def split_plan(batch, M, N, K, cap=64, mink=64, wgs=256):
    tiles = -(-M // 128) * -(-N // 128) * batch
    nsplit = 1
    if tiles < 128 and K >= 128:
        nsplit = -(-wgs // tiles)
        nsplit = min(nsplit, K // mink, cap)
        nsplit = max(nsplit, 1)
    kchunk = -(-K // nsplit)
    kchunk = max(-(-kchunk // 16) * 16, 16)
    nsplit = max(-(-K // kchunk), 1)
    return nsplit, kchunk


def plan_route(dt, batch, M, N, K, vec=True):
    """(branch, nslabs, launches) of pthip_gemm for a shape that csrc/gemm_skinny.hip does not take"""
    nsplit, kchunk = split_plan(batch, M, N, K)
    tiles = -(-M // 128) * -(-N // 128) * batch
    skinny = M <= 64
    if skinny:
        if nsplit > 1:
            return "skinny_split", nsplit, 2
        nk = -(-K // 16)
        return ("skinny_short" if nk <= 4 else "skinny_long"), 1, 1
    if np.dtype(dt) == np.float64:
        t64 = -(-M // 64) * -(-N // 64) * batch
        if (nsplit > 1 or tiles < NUM_CU) and M > 64 and t64 >= 128:
            return "t64", nsplit, 1
        return ("split", nsplit, 2) if nsplit > 1 else ("plain", 1, 1)
    if nsplit > 1:
        return "split", nsplit, 2
    if M % 256 == 0 and N % 256 == 0 and K % 16 == 0 and K >= 16 and vec:
        return "s256", 1, 1
    if tiles > 2 * NUM_CU:
        return "persistent", 1, 1
    return "plain", 1, 1


@dataclass(frozen=True)
class GemmRow:
    name: str
    batch: int
    M: int
    N: int
    K: int
    f64: str  # branch taken by float64 operands
    f32: str  # branch taken by float32 operands
    note: str = ""

    def branch(self, dt):
        return self.f64 if np.dtype(dt) == np.float64 else self.f32

    @property
    def shape(self):
        return self.batch, self.M, self.N, self.K


# (the fp64 kernel has no "all loads up front" path: its skinny rows run the K loop; "skinny_short" / "skinny_long" there
# name the same K extents)
GEMM_ROWS = (
    GemmRow("skinny_short", 1, 33, 150, 21, "skinny_short", "skinny_short"),
    GemmRow("skinny_one", 1, 1, 1, 1, "skinny_short", "skinny_short"),
    GemmRow("skinny_long", 1, 33, 150, 100, "skinny_long", "skinny_long"),
    GemmRow("skinny_split_4steps", 1, 64, 130, 128, "skinny_split", "skinny_split", "2 slabs of 64 = 4 steps each"),
    GemmRow("skinny_split_ragged", 1, 64, 130, 300, "skinny_split", "skinny_split", "4 slabs of 80, last 60"),
    GemmRow("skinny_split_52", 1, 17, 40, 4100, "skinny_split", "skinny_split", "52 slabs of 80, last 20"),
    GemmRow("skinny_split_m1", 1, 1, 200, 129, "skinny_split", "skinny_split", "2 slabs of 80, last 49"),
    GemmRow("plain", 1, 130, 135, 50, "plain", "plain"),
    GemmRow("plain_col", 1, 65, 1, 1, "plain", "plain"),
    GemmRow("split", 1, 130, 135, 300, "split", "split", "4 slabs of 80, last 60"),
    GemmRow("split_ragged", 1, 129, 257, 131, "split", "split", "2 slabs of 80, last 51"),
    GemmRow("t64_batched", 15, 129, 150, 37, "t64", "plain"),
    GemmRow("t64_square", 1, 705, 705, 21, "t64", "plain"),
    GemmRow("t64_for_split", 15, 129, 150, 200, "t64", "split", "nslabs = 3; float64 takes 64 x 64 tiles in one launch"),
    GemmRow("remap_on", 264, 65, 20, 40, "plain", "plain", "264 tiles: total % 8 == 0"),
    GemmRow("remap_off", 261, 65, 20, 40, "plain", "plain", "261 tiles: total % 8 != 0"),
    GemmRow("persistent", 520, 65, 70, 40, "plain", "persistent", "K not a multiple of 32"),
    GemmRow("persistent_k33", 513, 129, 1, 33, "plain", "persistent", "two K steps, the second has one column"),
    GemmRow("persistent_k17", 515, 65, 33, 17, "plain", "persistent", "one K step: the next tile's prefetch sits behind it"),
    GemmRow("persistent_interior", 129, 129, 129, 33, "plain", "persistent",
            "a full 128 x 128 tile per item: the vector loads and the unconditional stores of an interior tile without C"),
    GemmRow("s256", 2, 256, 512, 48, "plain", "s256"),
    GemmRow("k0_skinny", 3, 64, 129, 0, "skinny_short", "skinny_short", "K = 0: beta * C"),
    GemmRow("k0", 1, 130, 135, 0, "plain", "plain", "K = 0: beta * C"),
)
GEMM_BY_NAME = {r.name: r for r in GEMM_ROWS}
SPLIT_BRANCHES = ("skinny_split", "split")
# pthip_gemm_partials: every row whose plan has slabs, and one without
PARTIALS_ROWS = tuple(r.name for r in GEMM_ROWS if split_plan(*r.shape)[0] > 1) + ("plain",)
# csrc/gemm_skinny.hip takes these unbatched shapes (M >= 8192 with N <= 16; K >= 8192 with A a transposed view): the
# rows PTHIP_GEMM_SKINNY=0 sends back to the MFMA kernels.  (name, M, N, K, A transposed)
LONG_ROWS = (("long_fwd", 8192, 5, 37, False), ("long_bwd", 33, 5, 8200, True))


# ---------------------------------------------------------------------------------------------------------------
# operands: strided views into NaN-filled parents
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Operand:
    """``parent`` (1-D, NaN outside the view) with element (b, i, j) at ``off + b*sb + i*s0 + j*s1``"""
    parent: np.ndarray
    off: int
    sb: int
    s0: int
    s1: int
    shape: tuple

    def view(self):
        it = self.parent.itemsize
        return np.lib.stride_tricks.as_strided(self.parent[self.off:], self.shape, (self.sb * it, self.s0 * it, self.s1 * it), writeable=False)


ALIGNED = dict(ptr=0, pitch="aligned", bstride="aligned")


def embed(vals, trans=False, ptr=0, pitch="aligned", bstride="aligned", bcast=None):
    """Place ``vals`` (batch, R, C) into a NaN parent.

    trans: stored C x R (the operand is a transposed view: s0 == 1).  ptr: elements the first element sits behind a
    16-byte boundary (0 aligned, 1 off by one).  pitch: "aligned" (a multiple of the 16-byte vector, with padding),
    "odd", or "tight" (no padding).  bstride: "aligned", "odd" or "zero" (one shared item: ``vals`` has batch 1 and
    the view repeats it).  bcast: "row" / "col" = a (batch, 1, C) / (batch, R, 1) operand passed with a 0 stride.
    """
    vals = np.asarray(vals)
    dt = vals.dtype
    vn = vec_elems(dt)
    nb, R, Cc = vals.shape
    rows, cols = (Cc, R) if trans else (R, Cc)
    if pitch == "aligned":
        p = -(-cols // vn) * vn + vn
    elif pitch == "odd":
        p = cols + 1 if (cols + 1) % 2 else cols + 2
    else:
        p = cols
    item = rows * p
    if bstride == "zero":
        assert nb == 1
        sb = 0
    elif bstride == "odd":
        sb = item + 2 * vn + 1
        sb += 1 - sb % 2
    else:
        sb = -(-item // vn) * vn + 2 * vn
    off = 4 * vn + ptr
    parent = np.full(off + (nb - 1) * sb + item + 7, np.nan, dtype=dt)
    s0, s1 = (1, p) if trans else (p, 1)
    op = Operand(parent, off, sb, s0, s1, (nb, R, Cc))
    it = dt.itemsize
    np.lib.stride_tricks.as_strided(parent[off:], (nb, R, Cc), (sb * it, s0 * it, s1 * it))[...] = vals
    if bcast == "row":
        assert R == 1
        op.s0 = 0
    elif bcast == "col":
        assert Cc == 1
        op.s1 = 0
    return op


def embed_vec(vals, stride=1, ptr=0):
    """1-D ``vals`` with element i at ``off + i*stride`` of a NaN parent (stride may be negative)"""
    vals = np.asarray(vals)
    vn = vec_elems(vals.dtype)
    n = len(vals)
    span = (n - 1) * abs(stride) + 1 if n else 0
    lead = 4 * vn + ptr
    parent = np.full(lead + span + 7, np.nan, dtype=vals.dtype)
    off = lead + (span - 1 if stride < 0 and n else 0)
    if n:
        parent[off + stride * np.arange(n)] = vals
    return parent, off


# ---------------------------------------------------------------------------------------------------------------
# reference and checker
# ---------------------------------------------------------------------------------------------------------------
def rounded(x, dt):
    return float(np.dtype(dt).type(x))


def hp_matmul(A, B):
    """``np.matmul`` of (batch, M, K) @ (batch, K, N) in a type without a BLAS (long double): the batch items, or the
    row blocks of a single item, go to a few threads (the inner loops release the interpreter lock)"""
    nb = max(A.shape[0], B.shape[0])
    work = nb * A.shape[1] * A.shape[2] * B.shape[2]
    nt = min(8, os.cpu_count() or 1)
    if work < 2 * 10 ** 6 or nt < 2:
        return np.matmul(A, B)
    out = np.empty((nb, A.shape[1], B.shape[2]), dtype=np.result_type(A, B))
    if nb > 1:
        A, B = np.broadcast_to(A, (nb,) + A.shape[1:]), np.broadcast_to(B, (nb,) + B.shape[1:])
        cuts = np.linspace(0, nb, min(nt, nb) + 1).astype(int)
        jobs = [(slice(a, b), slice(None)) for a, b in zip(cuts[:-1], cuts[1:])]
    else:
        cuts = np.linspace(0, A.shape[1], min(nt, A.shape[1]) + 1).astype(int)
        jobs = [(slice(None), slice(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]

    def one(j):
        sb, sm = j
        np.matmul(A[sb, sm], B[sb], out=out[sb, sm])

    with ThreadPoolExecutor(len(jobs)) as ex:
        list(ex.map(one, jobs))
    return out


class GemmData:
    """Operand values of one (row, dtype) and their high-precision products, computed once and shared."""

    def __init__(self, row, dt, seed=0):
        self.row, self.dt = row, np.dtype(dt)
        nb, M, N, K = row.shape
        rng = np.random.default_rng([seed, nb, M, N, K])
        self.A = rng.standard_normal((nb, M, K)).astype(dt)
        self.B = rng.standard_normal((nb, K, N)).astype(dt)
        self.C = rng.standard_normal((nb, M, N)).astype(dt)
        self._prod = {}

    def products(self, share_a=False, share_b=False):
        """(A @ B, |A| @ |B|) in the high-precision type; a shared operand is batch item 0 for every item"""
        key = (share_a, share_b)
        if key not in self._prod:
            H = hp_type(self.dt)
            A = (self.A[:1] if share_a else self.A).astype(H)
            B = (self.B[:1] if share_b else self.B).astype(H)
            self._prod[key] = (hp_matmul(A, B), hp_matmul(np.abs(A), np.abs(B)))
        return self._prod[key]

    def expect(self, alpha, beta, C=None, share_a=False, share_b=False):
        """(want, bound) for ``alpha * A @ B + beta * C``; C broadcastable to (batch, M, N), ignored when beta == 0"""
        H = hp_type(self.dt)
        P, Pabs = (np.broadcast_to(v, self.C.shape) for v in self.products(share_a, share_b))
        a, b = H(rounded(alpha, self.dt)), H(rounded(beta, self.dt))
        want, mag = a * P, abs(a) * Pabs
        if b != 0:
            Ch = np.broadcast_to(np.asarray(C).astype(H), P.shape)
            want, mag = want + b * Ch, mag + abs(b) * np.abs(Ch)
        return want, (self.row.K + 4) * H(unit_roundoff(self.dt)) * mag


def gemv_expect(A, x, alpha, beta, y, dt):
    """(want, bound) of ``alpha * A @ x + beta * y`` (y ignored when beta == 0); K is N"""
    H = hp_type(dt)
    Ah, xh = np.asarray(A).astype(H), np.asarray(x).astype(H)
    a, b = H(rounded(alpha, dt)), H(rounded(beta, dt))
    want, mag = a * (Ah @ xh), abs(a) * (np.abs(Ah) @ np.abs(xh))
    if b != 0:
        yh = np.asarray(y).astype(H)
        want, mag = want + b * yh, mag + abs(b) * np.abs(yh)
    return want, (Ah.shape[1] + 4) * H(unit_roundoff(dt)) * mag


def finish_expect(part, alpha, beta, y, dt):
    """(want, bound) of ``alpha * sum_p part[p] + beta * y``; K is nparts, over |part|"""
    H = hp_type(dt)
    ph = np.asarray(part).astype(H)
    a, b = H(rounded(alpha, dt)), H(rounded(beta, dt))
    want, mag = a * ph.sum(axis=0), abs(a) * np.abs(ph).sum(axis=0)
    if b != 0:
        yh = np.asarray(y).astype(H)
        want, mag = want + b * yh, mag + abs(b) * np.abs(yh)
    return want, (ph.shape[0] + 4) * H(unit_roundoff(dt)) * mag


def ger_expect(A, x, y, alpha, dt):
    """(want, bound) of ``A + alpha * x y^T``: three roundings over |A| + |alpha x y|"""
    H = hp_type(dt)
    Ah, xh, yh = (np.asarray(v).astype(H) for v in (A, x, y))
    a = H(rounded(alpha, dt))
    upd = a * np.outer(xh, yh)
    return Ah + upd, 3 * H(unit_roundoff(dt)) * (np.abs(Ah) + np.abs(upd))


def _ratio(err, bound):
    pos = bound > 0
    if not np.all(np.isfinite(err)):
        return float("inf")
    return float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements with bound > 0 (inf for a NaN or an inf in ``got``)"""
    got, want = np.asarray(got), np.asarray(want)
    return _ratio(np.abs(got.astype(want.dtype) - want), bound) if got.size else 0.0


def check(got, want, bound, dt, what=""):
    """Assert ``|got - want| <= bound`` elementwise (a NaN fails), exact zeros where the bound is 0.  Returns the worst
    ratio of error to bound."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.dtype(dt), f"{what}: dtype {got.dtype}, expected {dt}"
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(want.dtype) - want)
    ok = err <= bound  # False for NaN
    ok &= (bound != 0) | (got == 0)
    if not np.all(ok):
        idx = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {got.size} elements outside the bound; first at {idx}: got {got[idx]!r}, "
                             f"want {want[idx]!r}, |err| {err[idx]!r} > bound {bound[idx]!r}; worst |err|/bound {_ratio(err, bound):.3g}")
    return _ratio(err, bound)


# ---------------------------------------------------------------------------------------------------------------
# Gemv cases (csrc/gemv.hip): kind "row" (sA1 == 1), "col" (sA0 == 1), "gen" (neither)
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemvCase:
    name: str
    M: int
    N: int
    kind: str = "row"
    sx: int = 1
    a_ptr: int = 0       # A's first element: elements behind a 16-byte boundary
    a_pitch: str = "aligned"
    x_ptr: int = 0
    strides: tuple = ()  # kind "gen" / the N = 1 row: (row step, column step) of the slice A = P[::r, ::c]
    launches: int = 1
    only: str = ""       # restricted to one dtype where the threshold is in bytes
    note: str = ""


GEMV_CASES = (
    GemvCase("row_vec_xlds", 37, 64),
    GemvCase("row_vec_direct_f64", 5, 520, only="float64", note="x over 4 KB: read through the caches"),
    GemvCase("row_vec_direct", 5, 1032, note="x over 4 KB in both dtypes"),
    GemvCase("row_scalar_xlds", 9, 67),
    GemvCase("row_scalar_direct_f64", 5, 521, only="float64"),
    GemvCase("row_scalar_direct", 5, 1033),
    GemvCase("row_odd_pitch", 6, 64, a_pitch="odd", note="N a multiple of the vector, the pitch not"),
    GemvCase("row_ptr_off", 6, 64, a_ptr=1),
    GemvCase("row_x_misaligned", 5, 1032, x_ptr=1, note="long x behind a misaligned pointer: staged in LDS"),
    GemvCase("row_sx2", 3, 1000, sx=2, note="x staged in LDS although long"),
    GemvCase("row_sx3_f64", 3, 8200, sx=3, only="float64", note="over 64 KB: neither staged nor vector"),
    GemvCase("row_sx3_f32", 3, 16400, sx=3, only="float32", note="over 64 KB: neither staged nor vector"),
    GemvCase("row_sx_neg", 7, 50, sx=-1),
    GemvCase("row_4rows_6", 16387, 6, note="four rows per wave, M % 4 == 3"),
    GemvCase("row_4rows_7", 16387, 7),
    GemvCase("row_4rows_8", 16387, 8),
    GemvCase("row_n0", 5, 0, note="beta * y"),
    GemvCase("row_n1_strided", 7, 1, strides=(3, 5), note="N = 1, sA1 != 1"),
    GemvCase("row_m1", 1, 300),
    GemvCase("col_vec_f64", 130, 1000, kind="col", launches=2),
    GemvCase("col_vec", 132, 1000, kind="col", launches=2),
    GemvCase("col_scalar", 131, 77, kind="col", launches=2),
    GemvCase("col_ptr_off", 130, 1000, kind="col", a_ptr=1, launches=2),
    GemvCase("col_one_block", 4, 50, kind="col", launches=2),
    GemvCase("col_many_parts", 4, 70000, kind="col", launches=2, note="274 partial rows"),
    GemvCase("col_sx_neg", 66, 300, kind="col", sx=-1, launches=2),
    GemvCase("generic", 9, 70, kind="gen", strides=(2, 3)),
)
GEMV_BY_NAME = {c.name: c for c in GEMV_CASES}


@dataclass
class GemvData:
    case: GemvCase
    dt: np.dtype
    A: np.ndarray = field(default=None)
    x: np.ndarray = field(default=None)
    y: np.ndarray = field(default=None)
    a_parent: np.ndarray = field(default=None)
    a_off: int = 0
    sA0: int = 0
    sA1: int = 0
    x_parent: np.ndarray = field(default=None)
    x_off: int = 0


def gemv_data(case, dt):
    dt = np.dtype(dt)
    M, N = case.M, case.N
    rng = np.random.default_rng([7, M, N, abs(case.sx)])
    d = GemvData(case, dt)
    d.A = rng.standard_normal((M, N)).astype(dt)
    d.x = rng.standard_normal(N).astype(dt)
    d.y = rng.standard_normal(M).astype(dt)
    if case.strides:
        r, c = case.strides
        vn = vec_elems(dt)
        pitch = N * c + 3
        off = 4 * vn
        d.a_parent = np.full(off + M * r * pitch + 7, np.nan, dtype=dt)
        np.lib.stride_tricks.as_strided(d.a_parent[off:], (M, N), (r * pitch * dt.itemsize, c * dt.itemsize))[...] = d.A
        d.a_off, d.sA0, d.sA1 = off, r * pitch, c
    else:
        op = embed(d.A[None], trans=(case.kind == "col"), ptr=case.a_ptr, pitch=case.a_pitch)
        d.a_parent, d.a_off, d.sA0, d.sA1 = op.parent, op.off, op.s0, op.s1
    d.x_parent, d.x_off = embed_vec(d.x, case.sx, case.x_ptr)
    return d
