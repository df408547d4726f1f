"""Scalar graph of a fused ``Elemwise``/``Composite`` → device statements for gfx950.

The reference emits the fused body with ``Composite.c_code_template``
(pytensor/scalar/basic.py:4111-4170) by concatenating each scalar op's ``c_code``
statement.  Here the same SSA walk emits a device expression per scalar op (same formulas
as the reference ``c_code`` strings, cited below): ``emit_body``.  The helpers those
expressions call are real headers under ``csrc/`` (``scalar_device.h`` and one
``special_*.h`` per family of long special functions), spliced into a generated kernel as
text by ``prelude_for``; the host accuracy tests compile the same files.

The kernel generators that wrap these statements in a loop live in the sibling modules
``codegen`` (flat / multi-flat / N-d), ``codegen_tile``, ``codegen_gchain``,
``codegen_dotew`` and ``codegen_tail``.
"""

from __future__ import annotations

import functools
import math
import os

import numpy as np

CTYPE = {
    "float64": "double",
    "float32": "float",
    "int64": "long long",
    "int32": "int",
    "int16": "short",
    "int8": "signed char",
    "uint8": "unsigned char",
    "uint16": "unsigned short",
    "uint32": "unsigned int",
    "uint64": "unsigned long long",
    # storage type with per-op rounding: every SSA temporary of dtype float16 is a `_Float16`, so
    # +,-,*,/ are IEEE half operations and libm-style ops are evaluated in float and rounded —
    # what NumPy does for float16 scalars (the reference has no C code for float16:
    # Elemwise runs `perform`, tensor/elemwise.py:755-823)
    "float16": "_Float16",
    "bool": "bool",
}

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


@functools.lru_cache(maxsize=None)
def device_header(name: str) -> str:
    """``csrc/<name>`` as the text a generated kernel carries (hiprtc sees one translation unit: no ``#pragma once``)."""
    with open(os.path.join(_CSRC, name), encoding="utf-8") as f:
        return f.read().replace("#pragma once", "")


# ---- incomplete gamma / beta: emitted only into kernels that use them ----


def _gamma_tables():
    """log(i!) and log(Gamma(i+1/2)) by the running products of the reference's support code
    (scalar/c_code/gamma.c:62-80; the last half-integer slot stays 0 there)."""
    logfs = [0.0] * 171
    loghs = [0.0] * 171
    x = 1.0
    for i in range(2, 171):
        x *= i
        logfs[i] = math.log(x)
    x = 1.77245385090551602729816748334
    loghs[0] = 0.5 * 1.14472988584940017414342735135
    for i in range(1, 170):
        x *= i - 0.5
        loghs[i] = math.log(x)
    return logfs, loghs


def _c_table(name, vals):
    return f"static __device__ const double {name}[{len(vals)}] = {{" + ", ".join(repr(float(v)) for v in vals) + "};\n"


@functools.lru_cache(maxsize=None)
def gamma_tables_src() -> str:
    """The ``pt_g_logfs`` / ``pt_g_loghs`` tables that ``csrc/special_gammainc.h`` reads, as device text."""
    logfs, loghs = _gamma_tables()
    return _c_table("pt_g_logfs", logfs) + _c_table("pt_g_loghs", loghs)


_OPTIONAL_HELPERS = {"NdtriExp": ("ndtriexp",), "GammaInc": ("gammainc",), "GammaIncC": ("gammainc",), "BetaInc": ("betainc",), "PolyGamma": ("polygamma",),
                     "GammaIncInv": ("gammainc", "gammaincinv"), "GammaIncCInv": ("gammainc", "gammaincinv"),
                     "BetaIncInv": ("betainc", "betaincinv"),
                     "Jv": ("bessel",), "Ive": ("bessel",), "Kve": ("bessel",), "Owens_t": ("owens_t",)}
_OPTIONAL_ORDER = ("gammainc", "betainc", "polygamma", "ndtriexp", "gammaincinv", "betaincinv", "bessel", "owens_t")
# the helpers are headers under csrc/ (the host accuracy tests compile the same text)
_OPTIONAL_FILES = {"gammainc": "special_gammainc.h", "betainc": "special_betainc.h", "polygamma": "special_polygamma.h", "ndtriexp": "special_ndtri_exp.h",
                   "gammaincinv": "special_gammaincinv.h", "betaincinv": "special_betaincinv.h", "bessel": "special_bessel.h", "owens_t": "special_owens_t.h"}


def _optional_src(key: str) -> str:
    src = device_header(_OPTIONAL_FILES[key])
    return gamma_tables_src() + src if key == "gammainc" else src


def prelude_for(*bodies) -> str:
    """``csrc/scalar_device.h`` plus the long helpers only the given scalar bodies need."""
    want = {k for b in bodies if b for op in body_ops(b) if op in _OPTIONAL_HELPERS for k in _OPTIONAL_HELPERS[op]}
    return device_header("scalar_device.h") + "".join(_optional_src(k) for k in _OPTIONAL_ORDER if k in want)


def body_ops(body: dict):
    """every scalar op name of a body, the inner bodies of its ``ScalarLoop`` nodes included"""
    for n in body["body"]:
        if n["op"] == "ScalarLoop":
            yield from body_ops(n["loop"]["body"])
        elif n["op"] != "LoopOut":
            yield n["op"]



class ScalarCodegenError(NotImplementedError):
    pass


def _lit(value, dtype: str) -> str:
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = float.fromhex(value) if isinstance(value, str) else float(value)
        if np.isnan(v):
            return "__builtin_nan(\"\")" if dt == np.float64 else "__builtin_nanf(\"\")"
        if np.isinf(v):
            s = "__builtin_huge_val()" if dt == np.float64 else "__builtin_huge_valf()"
            return s if v > 0 else f"(-{s})"
        if dt == np.float64:
            return f"{v.hex()}"  # C++17 hex float literal: bit exact
        return f"{float(np.float32(v)).hex()}f"
    if dt.kind == "b":
        return "true" if value else "false"
    v = int(value)
    if dt == np.uint64:
        return f"({v}ULL)"
    if dt == np.int64:
        return f"({v}LL)" if v != -(2**63) else "(-9223372036854775807LL - 1)"
    return f"(({CTYPE[str(dt)]}){v})"


def _is_float(dt):
    return np.dtype(dt).kind == "f"


def _is_int(dt):
    return np.dtype(dt).kind in "iu"


def _f(name64, name32=None):
    """libm-style unary: computed in the *output* dtype (upgrade_to_float ops)."""
    name32 = name32 or name64 + "f"

    def gen(args, in_dts, out_dt):
        ct = CTYPE[out_dt]
        fn = name64 if out_dt == "float64" else name32
        return f"{fn}(({ct}){args[0]})"

    return gen


def _chain(op):
    def gen(args, in_dts, out_dt):
        ct = CTYPE[out_dt]
        if out_dt == "bool":
            sym = {"+": "||", "*": "&&"}[op]
            return "(" + f" {sym} ".join(f"(bool){a}" for a in args) + ")"
        return "(" + f" {op} ".join(f"({ct}){a}" for a in args) + ")"

    return gen


def _binop_upcast(op):
    def gen(args, in_dts, out_dt):
        ct = CTYPE[out_dt]
        return f"(({ct}){args[0]} {op} ({ct}){args[1]})"

    return gen


def _cmp(op):
    def gen(args, in_dts, out_dt):
        # compare in the common type of the operands (C usual arithmetic conversions
        # differ from NumPy only for mixed signed/unsigned, which we upcast explicitly)
        common = str(np.result_type(*[np.dtype(d) for d in in_dts]))
        ct = CTYPE.get(common, "double")
        return f"(({ct}){args[0]} {op} ({ct}){args[1]})"

    return gen


def _bitop(op, boolop):
    def gen(args, in_dts, out_dt):
        if out_dt == "bool":
            return "(" + f" {boolop} ".join(f"(bool){a}" for a in args) + ")"
        ct = CTYPE[out_dt]
        return "(" + f" {op} ".join(f"({ct}){a}" for a in args) + ")"

    return gen


def _truediv(args, in_dts, out_dt):
    # TrueDiv.c_code (scalar/basic.py:1968+): discrete/discrete → (double)x / y
    ct = CTYPE[out_dt]
    return f"(({ct}){args[0]} / ({ct}){args[1]})"


def _intdiv(args, in_dts, out_dt):
    ct = CTYPE[out_dt]
    fn = "pt_intdiv_f" if _is_float(out_dt) else "pt_intdiv_i"
    return f"{fn}(({ct}){args[0]}, ({ct}){args[1]})"


def _mod(args, in_dts, out_dt):
    ct = CTYPE[out_dt]
    fn = "pt_mod_f" if _is_float(out_dt) else "pt_mod_i"
    return f"{fn}(({ct}){args[0]}, ({ct}){args[1]})"


def _pow(args, in_dts, out_dt):
    # Pow.c_code (scalar/basic.py:2250+): pow(x, y); integer outputs are cast back
    # (pt_pow: the library's pow with the exactly representable cases made exact — an integer power must not truncate
    #  6858.999999999999; float32 through the double: the rounded double is libm's powf value)
    return f"({CTYPE[out_dt]})pt_pow((double){args[0]}, (double){args[1]})"


def _abs(args, in_dts, out_dt):
    dt = in_dts[0]
    if _is_float(dt):
        return f"fabs({args[0]})" if dt == "float64" else f"fabsf({args[0]})"
    if dt in ("uint8", "uint16", "uint32", "uint64", "bool"):
        return args[0]
    return f"(({args[0]}) < 0 ? -({args[0]}) : ({args[0]}))"


def _switch(args, in_dts, out_dt):
    ct = CTYPE[out_dt]
    return f"(({args[0]}) ? ({ct}){args[1]} : ({ct}){args[2]})"


def _clip(args, in_dts, out_dt):
    ct = CTYPE[out_dt]
    x, lo, hi = (f"({ct}){a}" for a in args)
    return f"({x} < {lo} ? {lo} : ({x} > {hi} ? {hi} : {x}))"


def _cast(args, in_dts, out_dt):
    # Cast.c_code (scalar/basic.py:2435+)
    if out_dt == "bool":
        return f"(({args[0]}) ? true : false)"
    return f"({CTYPE[out_dt]}){args[0]}"


def _maxmin(fn):
    def gen(args, in_dts, out_dt):
        ct = CTYPE[out_dt]
        e = f"({ct}){args[0]}"
        for a in args[1:]:
            e = f"{fn}({e}, ({ct}){a})"
        return e

    return gen


def _isnan(args, in_dts, out_dt):
    return f"isnan({args[0]})" if _is_float(in_dts[0]) else "false"


def _isinf(args, in_dts, out_dt):
    return f"isinf({args[0]})" if _is_float(in_dts[0]) else "false"


def _invert(args, in_dts, out_dt):
    return f"(!{args[0]})" if out_dt == "bool" else f"(({CTYPE[out_dt]})~{args[0]})"


def _helper(fn):
    def gen(args, in_dts, out_dt):
        ct = CTYPE[out_dt]
        return f"{fn}(" + ", ".join(f"({ct}){a}" for a in args) + ")"

    return gen


_FAST_LOG = os.environ.get("PTHIP_FAST_LOG", "1") != "0"  # diagnostic: 0 = the device library's log / log1p

# op name (reference ScalarOp class) → expression generator
SCALAR_EXPR = {
    "Add": _chain("+"),  # scalar/basic.py:1835 Add.c_code
    "Mul": _chain("*"),  # 1876
    "Sub": _binop_upcast("-"),  # 1937
    "TrueDiv": _truediv,  # 1968
    "IntDiv": _intdiv,
    "Mod": _mod,
    "Pow": _pow,  # 2250
    "Neg": lambda a, i, o: f"(-({CTYPE[o]}){a[0]})",
    "Abs": _abs,  # 2524
    "Sign": _helper("pt_sign"),  # 2575
    "Sqr": _helper("pt_sqr"),  # 3202
    "Sqrt": _f("sqrt"),  # 3231
    "Exp": _f("pt_exp" if os.environ.get("PTHIP_FAST_EXP", "1") != "0" else "exp", "expf"),  # 3085
    "Exp2": _f("exp2"),
    "Expm1": _f("expm1"),
    "Log": _f("pt_log" if _FAST_LOG else "log", "logf"),  # 2907
    "Log2": _f("log2"),
    "Log10": _f("log10"),
    "Log1p": _f("pt_log1p" if _FAST_LOG else "log1p", "log1pf"),  # 3042
    "Sin": _f("sin"),
    "Cos": _f("cos"),
    "Tan": _f("tan"),
    "ArcSin": _f("asin"),
    "ArcCos": _f("acos"),
    "ArcTan": _f("atan"),
    "ArcTan2": lambda a, i, o: (
        f"{'atan2' if o == 'float64' else 'atan2f'}(({CTYPE[o]}){a[0]}, ({CTYPE[o]}){a[1]})"
    ),
    "Sinh": _f("sinh"),
    "Cosh": _f("cosh"),
    "Tanh": _f("pt_tanh" if os.environ.get("PTHIP_FAST_TANH", "1") != "0" else "tanh", "tanhf"),  # 3702
    "ArcSinh": _f("asinh"),
    "ArcCosh": _f("acosh"),
    "ArcTanh": _f("atanh"),
    "Sigmoid": _helper("pt_sigmoid"),  # scalar/math.py:1187-1198
    "Softplus": _helper("pt_softplus"),  # scalar/math.py:1250-1277
    "Log1mexp": _helper("pt_log1mexp"),  # scalar/math.py:1295+
    "Erf": _f("erf"),  # scalar/math.py:55
    "Erfc": _f("erfc"),  # 91
    "Erfinv": _f("erfinv"),
    "Erfcinv": _f("erfcinv"),
    "Erfcx": _f("erfcx"),
    "GammaLn": _f("lgamma"),  # scalar/math.py:363
    "Gamma": _f("tgamma"),
    "Psi": _helper("pt_psi"),  # scalar/math.py:403
    "TriGamma": _helper("pt_trigamma"),  # scalar/math.py:502
    "GammaInc": _helper("pt_gammainc"),  # scalar/math.py:627
    "GammaIncC": _helper("pt_gammaincc"),  # scalar/math.py:674
    "BetaInc": _helper("pt_betainc"),  # scalar/math.py:1342
    "PolyGamma": _helper("pt_polygamma"),  # scalar/math.py:595 (scipy.special.polygamma)
    "NdtriExp": _helper("pt_ndtri_exp"),  # scalar/math.py:271 (scipy.special.ndtri_exp)
    "GammaIncInv": _helper("pt_gammaincinv"),  # scipy.special.gammaincinv
    "GammaIncCInv": _helper("pt_gammainccinv"),  # scipy.special.gammainccinv
    "BetaIncInv": _helper("pt_betaincinv"),  # scipy.special.betaincinv
    # Bessel functions: J0/J1.c_code call libm's j0/j1 in double (scalar/math.py:1011-1064);
    # I0/I1 have no C code, the reference evaluates scipy.special.i0/i1 (1066-1110)
    "J0": lambda a, i, o: f"({CTYPE[o]})j0((double){a[0]})",
    "J1": lambda a, i, o: f"({CTYPE[o]})j1((double){a[0]})",
    "I0": lambda a, i, o: f"({CTYPE[o]})cyl_bessel_i0((double){a[0]})",
    "I1": lambda a, i, o: f"({CTYPE[o]})cyl_bessel_i1((double){a[0]})",
    # real-order Bessel functions and Owen's T: the reference evaluates scipy.special.jv / ive / kve / owens_t
    # (scalar/math.py); fp64 helpers of csrc/special_bessel.h and csrc/special_owens_t.h, rounded for float32
    "Jv": _helper("pt_jv"),
    "Ive": _helper("pt_ive"),
    "Kve": _helper("pt_kve"),
    "Owens_t": _helper("pt_owens_t"),
    "Reciprocal": lambda a, i, o: f"(({CTYPE[o]})1 / ({CTYPE[o]}){a[0]})",
    "Maximum": _maxmin("pt_max"),  # 1744
    "Minimum": _maxmin("pt_min"),  # 1790
    "ScalarMaximum": _maxmin("pt_max"),
    "ScalarMinimum": _maxmin("pt_min"),
    "EQ": _cmp("=="),  # 1411-1530
    "NEQ": _cmp("!="),
    "LT": _cmp("<"),
    "GT": _cmp(">"),
    "LE": _cmp("<="),
    "GE": _cmp(">="),
    "AND": _bitop("&", "&&"),
    "OR": _bitop("|", "||"),
    "XOR": _bitop("^", "!="),
    "Invert": _invert,
    "IsNan": _isnan,
    "IsInf": _isinf,
    "Switch": _switch,  # 1588
    "Clip": _clip,  # 2335
    "Identity": lambda a, i, o: f"({CTYPE[o]}){a[0]}",
    "Second": lambda a, i, o: f"({CTYPE[o]}){a[1]}",
    "Floor": _f("floor"),
    "Ceil": _f("ceil"),
    "Trunc": _f("trunc"),
    "RoundHalfToEven": _helper("pt_rint_even"),
    "RoundHalfAwayFromZero": _f("round"),
    "Cast": _cast,  # 2435
    "Deg2Rad": lambda a, i, o: f"(({CTYPE[o]}){a[0]} * ({CTYPE[o]})0.017453292519943295)",
    "Rad2Deg": lambda a, i, o: f"(({CTYPE[o]}){a[0]} * ({CTYPE[o]})57.29577951308232)",
}


def supported(body: dict) -> bool:
    def dtypes(b):
        yield from b["in_dtypes"] + b["out_dtypes"]
        for n in b["body"]:
            if n["op"] == "ScalarLoop":
                yield from dtypes(n["loop"]["body"])

    return all(op in SCALAR_EXPR for op in body_ops(body)) and all(d in CTYPE for d in dtypes(body))


_SHARE_SIG_SP = os.environ.get("PTHIP_SHARE_SIG_SP", "1") != "0"
_EMIT_CTX = {"share_recip": False}  # set by flat_kernel_source for bodies all of whose outputs are summed


def emit_body(body: dict, in_names, out_names, indent="      ", tp="t") -> str:
    """SSA statements computing ``out_names`` from ``in_names`` (one element).  ``tp`` prefixes
    the temporaries (the inner body of a loop lives in a nested scope with its own prefix)."""
    lines = []
    tdt = []

    def ref(r):
        if r[0] == "i":
            return in_names[r[1]], body["in_dtypes"][r[1]]
        if r[0] == "t":
            return f"{tp}{r[1]}", tdt[r[1]]
        return _lit(r[1], r[2]), r[2]

    # sigmoid and softplus of the same float64 operand: one shared evaluation (pt_sig_sp)
    shared = {}
    if _SHARE_SIG_SP:
        by_arg = {}
        for k, n in enumerate(body["body"]):
            if n["op"] in ("Sigmoid", "Softplus") and n["dtype"] == "float64" and len(n["in"]) == 1 and n["in"][0][0] in ("i", "t"):
                src_dt = body["in_dtypes"][n["in"][0][1]] if n["in"][0][0] == "i" else body["body"][n["in"][0][1]]["dtype"]
                if src_dt == "float64":
                    by_arg.setdefault((n["in"][0][0], n["in"][0][1]), {}).setdefault(n["op"], k)
        for d in by_arg.values():
            if len(d) == 2:
                first = min(d.values())
                for op, k in d.items():
                    shared[k] = (first, "sg" if op == "Sigmoid" else "sp")
    recip = {}  # TrueDiv node -> first node of its denominator group
    if _EMIT_CTX["share_recip"]:
        by_den = {}
        for k, n in enumerate(body["body"]):
            if n["op"] == "TrueDiv" and n["dtype"] == "float64" and len(n["in"]) == 2 and n["in"][1][0] in ("i", "t"):
                den = n["in"][1]
                den_dt = body["in_dtypes"][den[1]] if den[0] == "i" else body["body"][den[1]]["dtype"]
                num = n["in"][0]
                num_dt = (body["in_dtypes"][num[1]] if num[0] == "i" else body["body"][num[1]]["dtype"]) if num[0] in ("i", "t") else num[2]
                if den_dt == "float64" and num_dt == "float64":
                    by_den.setdefault((den[0], den[1]), []).append(k)
        for ks in by_den.values():
            if len(ks) >= 2:
                for k in ks:
                    recip[k] = ks[0]
    for k, n in enumerate(body["body"]):
        ct = CTYPE[n["dtype"]]
        if k in recip:
            first = recip[k]
            if k == first:
                den, _ = ref(n["in"][1])
                lines.append(f"{indent}const double {tp}{first}_rcp = 1.0 / (double){den};")
            num, _ = ref(n["in"][0])
            lines.append(f"{indent}const {ct} {tp}{k} = ({ct})((double){num} * {tp}{first}_rcp);")
            tdt.append(n["dtype"])
            continue
        if k in shared:
            first, which = shared[k]
            if k == first:
                arg, _ = ref(n["in"][0])
                lines.append(f"{indent}double {tp}{first}_sg, {tp}{first}_sp; pt_sig_sp((double){arg}, {tp}{first}_sg, {tp}{first}_sp);")
            lines.append(f"{indent}const {ct} {tp}{k} = {tp}{first}_{which};")
            tdt.append(n["dtype"])
            continue
        if n["op"] == "ScalarLoop":
            lines.append(_emit_loop(n, [ref(r) for r in n["in"]], f"{tp}{k}_", indent))
            lines.append(f"{indent}const {ct} {tp}{k} = {tp}{k}_s0;")
        elif n["op"] == "LoopOut":
            assert n["in"][0][0] == "t" and body["body"][n["in"][0][1]]["op"] == "ScalarLoop"
            loop = body["body"][n["in"][0][1]]["loop"]
            which = "done" if (loop["is_while"] and n["k"] == loop["n_state"]) else f"s{n['k']}"
            lines.append(f"{indent}const {ct} {tp}{k} = ({ct}){tp}{n['in'][0][1]}_{which};")
        else:
            gen = SCALAR_EXPR.get(n["op"])
            if gen is None:
                raise ScalarCodegenError(f"no device expression for scalar op {n['op']}")
            pairs = [ref(r) for r in n["in"]]
            odt = n["dtype"]
            if odt == "float16" or any(p[1] == "float16" for p in pairs):
                # half is a storage type: operands widen to float, the op runs in float and the
                # assignment below rounds to half — bit-identical to IEEE half +,-,*,/ (float has
                # 24 >= 2*11+2 significand bits, so the double rounding is innocuous) and what
                # NumPy does for every float16 ufunc
                pairs = [(f"(float){a}", "float32") if d == "float16" else (a, d) for a, d in pairs]
                odt = "float32" if odt == "float16" else odt
            expr = gen([p[0] for p in pairs], [p[1] for p in pairs], odt)
            lines.append(f"{indent}const {ct} {tp}{k} = ({ct})({expr});")
        tdt.append(n["dtype"])
    for name, r, dt in zip(out_names, body["outs"], body["out_dtypes"]):
        e, _ = ref(r)
        lines.append(f"{indent}{name} = ({CTYPE[dt]})({e});")
    return "\n".join(lines)


def _emit_loop(n: dict, pairs, P: str, indent: str) -> str:
    """``ScalarLoop.c_code_template`` (pytensor/scalar/loop.py:181-290) restated: carried
    copies of the initial states, ``for (i < n_steps)`` around the inner body, the carries
    overwritten after the whole body ran, ``until`` starting true and breaking after the update."""
    loop = n["loop"]
    inner = loop["body"]
    S = loop["n_state"]
    L = []
    for j in range(S):
        ct = CTYPE[inner["in_dtypes"][j]]
        L.append(f"{indent}{ct} {P}s{j} = ({ct})({pairs[1 + j][0]});")
    names = [f"{P}s{j}" for j in range(S)]
    for j in range(S, len(inner["in_dtypes"])):
        ct = CTYPE[inner["in_dtypes"][j]]
        L.append(f"{indent}const {ct} {P}c{j} = ({ct})({pairs[1 + j][0]});")
        names.append(f"{P}c{j}")
    if loop["is_while"]:
        L.append(f"{indent}bool {P}done = true;")
    L.append(f"{indent}for (long long {P}it = 0, {P}n = (long long)({pairs[0][0]}); {P}it < {P}n; ++{P}it) {{")
    ind2 = indent + "  "
    outs = []
    for j, dt in enumerate(inner["out_dtypes"]):
        L.append(f"{ind2}{CTYPE[dt]} {P}n{j};")
        outs.append(f"{P}n{j}")
    L.append(emit_body(inner, names, outs, ind2, tp=P + "t"))
    for j in range(S):
        L.append(f"{ind2}{P}s{j} = {P}n{j};")
    if loop["is_while"]:
        L.append(f"{ind2}{P}done = {P}n{S};")
        L.append(f"{ind2}if ({P}done) break;")
    L.append(f"{indent}}}")
    return "\n".join(L)
