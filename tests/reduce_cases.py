"""Case table, plan restatement, generators, reference and bound for csrc/reduce.hip (``pthip_reduce``).

Pure NumPy: imported by tests/test_gpu_tiers_reduce.py (GPU) and tests/test_reduce_cases.py (the CPU self-test of the
table, the restated plan and the generators).

View.  ``out[a, b] = reduce_r x[off + a sA + r sR + b sB]`` over a flat parent buffer; ``Row.strides()`` gives the element
strides and the offset of a layout, ``build`` the parent.  Every element of the parent the view does not name (the lead, the
tail, the gaps of a padded or strided row) holds NaN (floats) or 77 (integers), so a read outside the view changes the
answer.

Plan.  ``make_plan`` restates the host function of the same name: the stage-1 kernel (contig with 64- or 256-lane groups,
or strided), ``nsplit``, ``chunk``, the stage-2 group and the number of launches.  Seven routes: contig-64 and contig-256,
each in one and two stages; strided in one and two stages; the two-stage contig route whose finisher runs 256 lanes
(``nsplit >= 512``).

Reference.  Add: the exact sum (``math.fsum`` of the operands, which every float type converts to float64 exactly),
rounded once.  Mul: the product in ``np.longdouble`` (its own error, ``R 2^-64``, is 2^-11 of the float64 bound).  Integer
triples wrap: ``np.add.reduce`` / ``np.multiply.reduce`` with ``dtype=acc`` and the wrap-around cast to out, bit-exact.
Max / Min / And / Or / Xor: NumPy's reduction in the type the kernel computes in, bit-exact.

Bound (floats), with ``u`` the unit roundoff, ``gamma_k(u) = k u / (1 - k u)`` and ``d`` the number of additions an
element passes through on its route (``depth``: the lane's accumulator, the two joins of the four accumulators, the six
butterfly levels, the four LDS slots of a 256-lane group, and the same again for stage 2).  No tuned factor:

    Add:  |err| <= gamma_d(u_acc) sum|x| + u_out |exact|
    Mul:  |err| <= gamma_{R+d}(u_acc) |exact| + u_out |exact|

Generators.  ``ints``: small integers (every route is bit-exact, a dropped or doubled element changes the answer);
``cancel``: a third of the row large, a third its negation, a third small, shuffled, so ``sum|x| / |sum x|`` is ~1e6 and a
float32 accumulator is told from a float64 one; ``flat``: standard normal; ``wide`` (integers): the full range, so sums
wrap; ``pm`` / ``prod`` / ``odd`` for products: signs and a few twos (exact), factors ``exp(+-s)`` with the product kept in
the normal range of out, odd integers (a wrapped product of evens is 0).

Empty last split.  With ``R = nsplit c + k`` (``1 <= k <= nsplit``) the chunk is ``c + 1`` and the last split is empty when
``k <= nsplit - c - 1``, so ``nsplit >= c + 2``; the plans keep ``c >= 64`` (strided) or ``c >= 512`` (contig, at most 2048
splits: ``c >= 512`` again there).  Strided: ``want = ceil(512 / blocks)`` is first above 65 at 7 blocks of outputs (74
splits), and R = 74 * 64 + 1 = 4737 is the shortest row that allows 74 splits: (1, 4737, 1537), row ``strided_empty_split``
(73 * 65 = 4745 >= 4737).  Contig: the 64-lane group has at most 4 splits (R < 2048) of ``c >= 500``, the 256-lane group
``c >= 2048 (nsplit - 1) / nsplit`` and at most 2048 splits, so ``nsplit >= c + 2`` never holds: no contig shape has an empty split
(``find_empty_split`` searches both kernels and agrees).
"""
import functools
import math
import re
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

NUM_CU = 256
BLOCK = 256
OPS = {"Add": 0, "Mul": 1, "Max": 2, "Min": 3, "And": 4, "Or": 5, "Xor": 6}
FLOATS = ("float64", "float32", "float16")
POISON_INT = 77
LEAD = 16  # elements in front of the view: a whole number of 16-byte vectors for every type


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "route group nsplit chunk g2 launches")


def make_plan(A, R, B, sR, sB):
    n_out = A * B
    target = NUM_CU * 8
    contig = (sR in (1, -1) or B == 1) and not (sB == 1 and B >= 64 and sR != 1)
    if R <= 32 and n_out >= 256:
        contig = False
    if contig:
        group = 256 if R >= 2048 else 64
        want = ceil_div(target, n_out or 1)
        nsplit = min(max(want, 1), ceil_div(R, group * 8))
        nsplit = min(max(nsplit, 1), 2048)
    else:
        group = 1
        blocks = ceil_div(n_out, BLOCK)
        want = ceil_div(target // 4, blocks or 1)
        nsplit = min(max(want, 1), ceil_div(R, 64))
        nsplit = min(max(nsplit, 1), 1024)
    chunk = max(ceil_div(R, nsplit), 1)
    route = f"contig-{group}" if contig else "strided"
    g2 = 0 if nsplit == 1 else (256 if nsplit >= 512 else 64) if contig else 1
    return Plan(route, group, nsplit, chunk, g2, 0 if n_out == 0 else 1 if nsplit == 1 else 2)


def route_name(p):
    """one of the seven routes"""
    if p.nsplit == 1:
        return f"{p.route} one-stage"
    return f"{p.route} two-stage" + (", 256-lane finisher" if p.g2 == 256 else "")


ROUTES = ("contig-64 one-stage", "contig-64 two-stage", "contig-256 one-stage", "contig-256 two-stage", "strided one-stage",
          "strided two-stage", "contig-256 two-stage, 256-lane finisher")


def reduce_workspace(acc, A, R, B):
    """``pthip_reduce_workspace`` restated"""
    n_out = A * B
    if n_out == 0 or R == 0:
        return 0
    ns = min(2048, ceil_div(R, 64))
    return 0 if ns <= 1 else n_out * ns * np.dtype(acc).itemsize


def _depth_one(length, group):
    """additions an element of a run of ``length`` passes through in one launch: the lane's accumulator 0 takes every
    fourth of its elements and up to three left over, then two joins, then the lanes"""
    per = ceil_div(length, group)
    d = per // 4 + per % 4 + 2
    if group > 1:
        d += 6 + (4 if group == 256 else 0)
    return d


def depth(p, R):
    d = _depth_one(min(p.chunk, R), p.group)
    if p.nsplit > 1:
        d += _depth_one(p.nsplit, p.g2)
    return d


def gamma(k, u):
    return k * u / (1 - k * u)


def find_empty_split(limit=1 << 13):
    """the smallest (A, R, B) per kernel whose last split is empty, or None; contig is searched as a full reduction and
    rows of few outputs (where nsplit is largest), strided over whole blocks of outputs"""
    found = {}
    for kind, shapes in (("contig", [(a, 1, 1, 1) for a in (1, 2, 3, 4, 8)]), ("strided", [(1, 256 * k + 1, 256 * k + 1, 1) for k in range(8)])):
        for A, B, sR, sB in shapes:
            for R in range(1, limit if kind == "strided" else 1 << 22, 1 if kind == "strided" else 257):
                p = make_plan(A, R, B, sR, sB)
                if (p.nsplit - 1) * p.chunk >= R and p.nsplit > 1:
                    if kind not in found or R * A * B < np.prod(found[kind]):
                        found[kind] = (A, R, B)
                    break
    return found


# ---------------------------------------------------------------------------------------------------------------
# dtype triples: the tables of dispatch_types / dispatch_minmax / dispatch_bool, in the order of the file
# ---------------------------------------------------------------------------------------------------------------
_NP = {"F64": "float64", "F32": "float32", "F16": "float16", "I64": "int64", "I32": "int32", "I16": "int16", "I8": "int8", "U64": "uint64",
       "U32": "uint32", "U16": "uint16", "U8": "uint8", "BOOL": "bool"}


def _t(s):
    return tuple(tuple(_NP[c] for c in tri.split()) for tri in s.split(","))


TYPES_TRIPLES = _t("F64 F64 F64,F32 F64 F32,F64 F64 F32,F32 F64 F64,F32 F32 F32,F16 F32 F16,F16 F32 F32,I64 I64 I64,I32 I64 I64,I16 I64 I64,"
                   "I8 I64 I64,BOOL I64 I64,U8 I64 I64,I32 I64 I32,I16 I64 I16,I8 I64 I8,U64 U64 U64,U32 U64 U64,U16 U64 U64,U8 U64 U64,"
                   "U32 U64 U32,U16 U64 U16,U8 U64 U8,I32 I32 I32,I16 I16 I16,I8 I8 I8,U8 U8 U8,I64 I64 I32,I64 I64 I16,I64 I64 I8,"
                   "U64 U64 U32,U64 U64 U16,U64 U64 U8,F32 F32 F16")
MINMAX_TRIPLES = _t("F64 F64 F64,F32 F32 F32,F32 F64 F32,F16 F16 F16,F16 F32 F16,F64 F64 F32,I64 I64 I32,I64 I64 I16,I64 I64 I8,U64 U64 U32,"
                    "U64 U64 U16,U64 U64 U8,F32 F32 F16,I64 I64 I64,I32 I32 I32,I16 I16 I16,I8 I8 I8,U64 U64 U64,U32 U32 U32,U16 U16 U16,U8 U8 U8")
BOOL_TRIPLES = _t("BOOL BOOL BOOL,I64 I64 I64,I32 I32 I32,I16 I16 I16,I8 I8 I8,U8 U8 U8,U16 U16 U16,U32 U32 U32,U64 U64 U64")
TABLE_OF = {"Add": TYPES_TRIPLES, "Mul": TYPES_TRIPLES, "Max": MINMAX_TRIPLES, "Min": MINMAX_TRIPLES, "And": BOOL_TRIPLES, "Or": BOOL_TRIPLES,
            "Xor": BOOL_TRIPLES}
# the accumulator type two lines of dispatch_minmax compute in, whatever the graph names
MINMAX_COMPUTES_IN = {("float32", "float64", "float32"): "float32", ("float16", "float32", "float16"): "float16"}

# the families that run the whole route table: name -> {op: triple}
_same = lambda t: (t, t, t)  # noqa: E731
FAMILIES = {
    "f64": {**dict.fromkeys(("Add", "Mul", "Max", "Min"), _same("float64"))},
    "f32_f64": {**dict.fromkeys(("Add", "Mul", "Max", "Min"), ("float32", "float64", "float32"))},
    "f32": {**dict.fromkeys(("Add", "Mul", "Max", "Min"), _same("float32"))},
    "i32": {**dict.fromkeys(("Add", "Mul"), ("int32", "int64", "int64")), **dict.fromkeys(("Max", "Min", "And", "Or", "Xor"), _same("int32"))},
    "u8": {**dict.fromkeys(("Add", "Mul"), ("uint8", "uint64", "uint64")), **dict.fromkeys(("Max", "Min", "And", "Or", "Xor"), _same("uint8"))},
    # (bool Max / Min go through Or / And)
    "bool": {**dict.fromkeys(("Add", "Mul"), ("bool", "int64", "int64")), **dict.fromkeys(("Max", "Min", "And", "Or", "Xor"), _same("bool"))},
    "f16": {**dict.fromkeys(("Add", "Mul"), ("float16", "float32", "float16")), **dict.fromkeys(("Max", "Min"), _same("float16"))},
}


def other_runs():
    """(op, triple) of every table line no family runs"""
    full = {(op, tri) for fam in FAMILIES.values() for op, tri in fam.items()}
    return [(op, tri) for op in OPS for tri in TABLE_OF[op] if (op, tri) not in full]


def parse_dispatch(src):
    """{function: [(in, acc, out)]} as csrc/reduce.hip lists them"""
    out = {}
    for fn in ("dispatch_types", "dispatch_minmax", "dispatch_bool"):
        body = src[src.index(f"int {fn}("):]
        body = body[:body.index("return pthip::set_error")]
        tri = [tuple(_NP[c] for c in m) for m in re.findall(r"PTHIP_CASE\(PTHIP_(\w+), PTHIP_(\w+), PTHIP_(\w+),", body)]
        tri += [(_NP[m],) * 3 for m in re.findall(r"case PTHIP_(\w+): PTHIP_RUN", body)]
        if fn == "dispatch_bool":
            tri += [("bool",) * 3] + [(_NP[m],) * 3 for m in re.findall(r"\n  CASE\(PTHIP_(\w+),", body)]
        out[fn] = tri
    return out


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Row:
    name: str
    A: int
    R: int
    B: int
    layout: str = "c"   # c: contiguous (A, R, B) | pad: rows 7 elements apart | rev: sR = -1 | step3: sR = 3 | hankel: sR = -1, sB = 1
    note: str = ""

    @property
    def n_out(self):
        return self.A * self.B

    def strides(self):
        """(sA, sR, sB, offset of x[0, 0, 0])"""
        A, R, B = self.A, self.R, self.B
        if self.layout == "c":
            return R * B, B, 1, 0
        if self.layout == "pad":
            return R * B + 7, B, 1, 0
        if self.layout == "rev":
            assert B == 1
            return R, -1, 1, max(R - 1, 0)
        if self.layout == "step3":
            assert B == 1
            return 3 * R + 2, 3, 1, 0
        assert self.layout == "hankel"
        return R + B - 1, -1, 1, R - 1

    def plan(self):
        sA, sR, sB, _ = self.strides()
        return make_plan(self.A, self.R, self.B, sR, sB)

    def index(self):
        return _index(self)


@functools.lru_cache(maxsize=2)
def _index(row):
    sA, sR, sB, off = row.strides()
    a, r, b = np.ix_(np.arange(row.A), np.arange(row.R), np.arange(row.B))
    return off + a * sA + r * sR + b * sB


ROWS = (
    # R around the 4 x GROUP unroll of the 64-lane group and the group switch; 3 outputs: the block's fourth group is inactive
    tuple(Row(f"rows3_R{R}", 3, R, 1) for R in (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048))
    + (
        Row("full_R1", 1, 1, 1), Row("full_R0", 1, 0, 1),
        Row("contig64_two", 3, 1000, 1, note="2 splits of 500, 6 groups: two inactive"),
        Row("contig64_two_5", 5, 1537, 1, note="4 splits, 20 groups"),
        Row("contig64_one_many", 2050, 600, 1, note="want = 1: one stage although R > 512; 2050 groups, the last block half empty"),
        Row("contig256_one", 3, 2048, 1), Row("contig256_two", 1, 4097, 1, note="3 splits of 1366"),
        Row("contig256_two_3", 3, 6145, 1, note="4 splits, 12 blocks"),
        Row("finisher256", 1, 511 * 2048 + 1, 1, note="512 splits: the stage-2 group is 256 lanes"),
        Row("finisher256_2", 2, 511 * 2048 + 1, 1, note="512 splits per output"),
        # strided: column sums, blocks of outputs around 256
        Row("strided_one_255", 1, 40, 255), Row("strided_one_256", 1, 64, 256), Row("strided_one_257", 1, 7, 257),
        Row("strided_two_255", 1, 100, 255), Row("strided_two_256", 1, 130, 256), Row("strided_two_257", 1, 129, 257),
        Row("strided_mid", 4, 70, 5, note="a middle axis: 20 outputs, 2 splits"),
        Row("strided_R0", 1, 0, 300), Row("strided_R1", 2, 1, 150),
        Row("strided_empty_split", 1, 4737, 1537, note="74 splits of 65: the last one is empty"),
        # tiny rows: thread per output from 256 outputs on, R <= 32
        Row("tiny_255x32", 255, 32, 1), Row("tiny_256x32", 256, 32, 1), Row("tiny_256x33", 256, 33, 1), Row("tiny_257x3", 257, 3, 1),
        Row("tiny_255x33", 255, 33, 1),
        # sB = 1 with sR = -1 on both sides of the contig exclusion
        Row("hankel_63", 2, 90, 63, "hankel"), Row("hankel_64", 2, 90, 64, "hankel"),
        Row("rev", 2, 1000, 1, "rev", note="base at the last element"), Row("rev_4097", 1, 4097, 1, "rev"),
        Row("step3", 3, 300, 1, "step3"), Row("step3_two", 2, 1100, 1, "step3"),
        Row("padded", 5, 100, 1, "pad"), Row("padded_two", 3, 1000, 1, "pad"), Row("padded_cols", 2, 130, 40, "pad"),
    )
)
BY_NAME = {r.name: r for r in ROWS}
# every other triple runs on these two
OTHER_ROWS = ("contig64_two", "strided_two_257")
# NaN is planted at every split boundary where the splits are few
PLANT_ROWS = ("rows3_R257", "contig64_two", "contig256_two", "strided_two_257", "strided_mid", "rev", "padded_cols", "finisher256")


# ---------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------
def gens_for(op, tin, row):
    """the generators a run of ``op`` on ``row`` uses (``cancel`` from 63 elements on, and not where a layout overlaps
    itself: a row there is not what was generated)"""
    k = np.dtype(tin).kind
    if op == "Add":
        return (("ints", "cancel", "flat") if row.R >= 63 and row.layout != "hankel" else ("ints", "flat")) if k == "f" else ("ints",) if k == "b" else ("ints", "wide")
    if op == "Mul":
        return ("pm", "prod") if k == "f" else ("ints",) if k == "b" else ("odd",)
    if op in ("Max", "Min"):
        return ("flat",) if k == "f" else ("ints",) if k == "b" else ("wide",)
    return ("sparse",)


CANCEL_EXP = {"float64": 20, "float32": 20, "float16": 9}


def generate(row, op, gen, tin, tout):
    """(A, R, B) values in ``tin``"""
    dt = np.dtype(tin)
    shape = (row.A, row.R, row.B)
    R = row.R
    rng = np.random.default_rng([list(OPS).index(op), sum(map(ord, gen)), row.A, R, row.B, dt.itemsize, dt.kind == "u"])
    if dt.kind == "b":
        p = {"And": 1 - 1.0 / max(R, 1), "Min": 1 - 1.0 / max(R, 1), "Mul": 1 - 1.0 / max(R, 1), "Or": 1.0 / max(R, 1), "Max": 1.0 / max(R, 1)}.get(op, 0.5)
        return rng.random(shape) < p
    if gen == "ints":
        return rng.integers(0 if dt.kind == "u" else -2, 5 if dt.kind == "u" else 3, shape).astype(dt)
    if gen == "flat":
        return rng.standard_normal(shape).astype(dt)
    if gen == "cancel":
        q = R // 3
        big = (rng.uniform(0.5, 1.0, (row.A, q, row.B)) * 2.0 ** CANCEL_EXP[dt.name]).astype(dt)
        X = rng.uniform(-1, 1, shape).astype(dt)
        X[:, :q], X[:, q:2 * q] = big, -big
        return X[:, rng.permutation(R)]
    if gen in ("wide", "odd", "sparse"):
        info = np.iinfo(dt)
        X = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
        if gen == "odd":
            return X | dt.type(1)
        if gen == "sparse":  # a bit set (Or) or cleared (And) about twice per row
            if op == "Xor":
                return X
            X = np.where(rng.random(shape) < 2.0 / max(R, 1), X, dt.type(0))
            return ~X if op == "And" else X
        return X
    if gen == "pm":
        X = np.where(rng.random(shape) < 0.5, 1.0, -1.0)
        X[:, :min(R, 10)] *= 2.0
        return X[:, rng.permutation(R)].astype(dt)
    assert gen == "prod"
    # log|product| is a walk of R steps uniform in [-s, s]: 2 standard deviations of it stay inside half the
    # normal range of out (the factors are rounded to tin afterwards; at float16 that bends the walk by less than R 2^-22)
    half_range = 0.5 * math.log(float(np.finfo(tout).max))
    s = min(0.5, half_range / 2 * math.sqrt(3.0 / max(R, 1)))
    X = np.exp(rng.uniform(-s, s, shape)) * np.where(rng.random(shape) < 0.5, 1.0, -1.0)
    return X.astype(dt)


def poison(dt):
    dt = np.dtype(dt)
    return dt.type(np.nan) if dt.kind == "f" else dt.type(True) if dt.kind == "b" else dt.type(POISON_INT)


def build(row, X0, off=0):
    """(parent, element index of x[0, 0, 0], the view as the kernel sees it): ``LEAD + off`` poisoned elements in front,
    8 behind, every gap poisoned.  Where a layout overlaps itself (hankel) the view is re-read from the parent."""
    idx = row.index()
    size = int(idx.max()) + 1 if idx.size else max(row.strides()[3] + 1, 1)
    assert idx.size == 0 or idx.min() >= 0
    lead = LEAD + off
    parent = np.full(lead + size + 8, poison(X0.dtype), dtype=X0.dtype)
    parent[lead + idx] = X0
    return parent, lead + row.strides()[3], parent[lead + idx]


# ---------------------------------------------------------------------------------------------------------------
# reference, bound, checker
# ---------------------------------------------------------------------------------------------------------------
def unit_roundoff(dt):
    return float(np.finfo(dt).eps) / 2.0


def computes_in(op, tri):
    return MINMAX_COMPUTES_IN.get(tri, tri[1]) if op in ("Max", "Min") else tri[1]


def np_reduce(op, X, tri):
    """the bit-exact reference of everything but a float Add / Mul: NumPy's reduction in the accumulator type, then the
    cast to out (wrap-around for integers)"""
    acc = np.dtype(computes_in(op, tri))
    uf = {"Add": np.add, "Mul": np.multiply, "Max": np.maximum, "Min": np.minimum, "And": np.bitwise_and, "Or": np.bitwise_or, "Xor": np.bitwise_xor}[op]
    if acc.kind == "b":
        uf = {"And": np.logical_and, "Min": np.logical_and, "Or": np.logical_or, "Max": np.logical_or, "Xor": np.logical_xor}[op]
    with np.errstate(all="ignore"):
        return uf.reduce(X.astype(acc), axis=1, dtype=acc).astype(tri[2])


def float_expect(op, X, tri, plan):
    """(want in long double, bound in long double) of a float Add / Mul over axis 1 of the (A, R, B) view"""
    L = np.longdouble
    A, R, B = X.shape
    ua, uo = unit_roundoff(tri[1]), unit_roundoff(tri[2])
    d = depth(plan, R)
    X64 = X.astype(np.float64)
    if op == "Add":
        Xt = np.ascontiguousarray(X64.transpose(0, 2, 1))
        want = np.array([[math.fsum(Xt[a, b]) for b in range(B)] for a in range(A)], dtype=np.float64).reshape(A, B).astype(L)
        mag = np.abs(X64).astype(L).sum(axis=1)
        return want, L(gamma(d, ua)) * mag + L(uo) * np.abs(want)
    want = np.multiply.reduce(X.astype(L), axis=1) if R else np.ones((A, B), L)
    return want, (L(gamma(R + d, ua)) + L(uo)) * np.abs(want)


def check_float(got, want, bound, what=""):
    """``|got - want| <= bound`` everywhere (a NaN fails); the worst ratio"""
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(np.longdouble) - want)
    ok = err <= bound
    if not np.all(ok):
        i = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {got.size} outputs outside the bound; first at {i}: got {got[i]!r}, want {want[i]!r}, "
                             f"|err| {err[i]!r} > bound {bound[i]!r}")
    sel = bound > 0
    return float(np.max(err[sel] / bound[sel])) if np.any(sel) else 0.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}") if a.dtype.kind != "b" else a.view(np.uint8)


def check_exact(got, want, what=""):
    """bit-identical, except that any NaN stands for any NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape}, expected {want.dtype}{want.shape}"
    same = bits(got) == bits(want)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    if not np.all(same):
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {got.size} outputs differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


def is_exact(op, gen, tri):
    """is this run held bit-exact (everything but a float Add / Mul on rounded data)?"""
    return op not in ("Add", "Mul") or np.dtype(tri[0]).kind != "f" or gen in ("ints", "pm")


def plant_positions(row, cap=8):
    """where a NaN goes along r: first, last, and both sides of every split boundary (of the first and the last split only
    where there are more than ``cap``)"""
    p = row.plan()
    cuts = range(1, p.nsplit) if p.nsplit <= cap else (1, p.nsplit - 1)
    pos = {0, row.R - 1}
    for s in cuts:
        pos |= {s * p.chunk - 1, s * p.chunk}
    return sorted(q for q in pos if 0 <= q < row.R)
