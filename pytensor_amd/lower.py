"""Lower a rewritten PyTensor ``FunctionGraph`` to the portable IR (``pytensor_amd.ir``).

This is the ``hip_funcify`` of the backend — the analogue of
``pytorch_funcify`` (pytensor/link/pytorch/dispatch/basic.py:45-68) and of
``fgraph_to_python`` (pytensor/link/utils.py:677-828) — except that instead of
emitting Python source it records, per ``Apply`` node in toposort order, the
reference ``Op`` class name and its ``__props__`` so the executor / oracle can
interpret them without PyTensor.

Needs PyTensor importable.  Ops without a device lowering raise
``NotImplementedError`` at compile time.  Only with ``PTHIP_ALLOW_HOST_PERFORM=1``
do they lower to a ``HostPerform`` node carrying the live ``Op`` (not serialisable;
D2H → ``Op.perform`` → H2D, like numba's object-mode fallback,
pytensor/link/numba/dispatch/basic.py:228-263) — never on the measured paths.
"""

from __future__ import annotations

from functools import singledispatch

import numpy as np

from pytensor.compile.ops import DeepCopyOp, TypeCastingOp, ViewOp
from pytensor.graph.basic import Constant
from pytensor.raise_op import CheckAndRaise
from pytensor.scalar.basic import Cast, Composite, ScalarOp, ScalarType
from pytensor.scalar.loop import ScalarLoop
from pytensor.scan.op import Scan
from pytensor.tensor.basic import (
    Alloc,
    AllocEmpty,
    ExtractDiag,
    Join,
    MakeVector,
    ScalarFromTensor,
    Split,
    TensorFromScalar,
)
from pytensor.tensor.blas import BatchedDot, Dot22, Dot22Scalar, Gemm, Gemv, Ger
from pytensor.tensor.blockwise import Blockwise
from pytensor.tensor.elemwise import CAReduce, DimShuffle, Elemwise
from pytensor.tensor.linalg.decomposition.cholesky import Cholesky
from pytensor.tensor.linalg.solvers.psd import CholeskySolve
from pytensor.tensor.linalg.solvers.triangular import SolveTriangular
from pytensor.tensor.math import Dot
from pytensor.tensor.shape import Reshape, Shape, Shape_i, SpecifyShape
from pytensor.tensor.subtensor import (
    AdvancedIncSubtensor,
    AdvancedSubtensor,
    IncSubtensor,
    Subtensor,
)
from pytensor.tensor.random.op import RandomVariable
from pytensor.tensor.random.type import RandomType
from pytensor.tensor.type import TensorType
from pytensor.sparse.type import SparseTensorType
from pytensor.tensor.type_other import NoneTypeT, SliceType

from pytensor_amd.ir import Graph


# ---------------------------------------------------------------------------
# scalar graphs (Composite bodies)
# ---------------------------------------------------------------------------

def _scalar_op_name(op) -> str:
    return type(op).__name__


def lower_scalar_op(op: ScalarOp, in_dtypes, out_dtypes) -> dict:
    """Scalar op, ``Composite`` or ``ScalarLoop`` → SSA body.

    Follows the walk of ``Composite.c_code_template``
    (pytensor/scalar/basic.py:4111-4170): inner nodes in toposort order,
    constants inlined as literals.
    refs: ["i", k] input k · ["t", k] k-th body value · ["c", value, dtype] literal.

    A ``ScalarLoop`` (pytensor/scalar/loop.py:10; the gradients of the incomplete gamma / beta
    functions and of hyp2f1 are built from it) becomes one body node carrying its inner SSA
    body under ``"loop"``, followed by one ``LoopOut`` node per output selecting a final state
    (or the ``until`` flag).
    """
    if isinstance(op, Composite):
        return _lower_scalar_fgraph(op.fgraph, in_dtypes, out_dtypes)
    args = [["i", k] for k in range(len(in_dtypes))]
    if isinstance(op, ScalarLoop):
        body = []
        outs = _append_loop(body, op, args, out_dtypes)
        return {"in_dtypes": list(in_dtypes), "out_dtypes": list(out_dtypes), "body": body, "outs": outs}
    if len(out_dtypes) != 1:
        raise NotImplementedError(f"multi-output scalar op {op}")
    return {
        "in_dtypes": list(in_dtypes),
        "out_dtypes": list(out_dtypes),
        "body": [_scalar_node(op, args, out_dtypes[0])],
        "outs": [["t", 0]],
    }


def _append_loop(body, op, args, out_dtypes):
    """append the loop node and its ``LoopOut`` selectors to ``body``; returns the output refs"""
    n_state = len(op.outputs) - (1 if op.is_while else 0)
    inner = _lower_scalar_fgraph(op.fgraph, [i.type.dtype for i in op.fgraph.inputs], [o.type.dtype for o in op.fgraph.outputs])
    k = len(body)
    body.append({"op": "ScalarLoop", "in": args, "dtype": str(out_dtypes[0]),
                 "loop": {"n_state": n_state, "is_while": bool(op.is_while), "body": inner}})
    refs = []
    for j, dt in enumerate(out_dtypes):
        body.append({"op": "LoopOut", "in": [["t", k]], "dtype": str(dt), "k": j})
        refs.append(["t", len(body) - 1])
    return refs


def _lower_scalar_fgraph(fg, in_dtypes, out_dtypes) -> dict:
    ref = {}
    for k, v in enumerate(fg.inputs):
        ref[v] = ["i", k]
    body = []
    for node in fg.toposort():
        args = []
        for inp in node.inputs:
            if inp in ref:
                args.append(ref[inp])
            elif isinstance(inp, Constant):
                args.append(_const_ref(inp))
            else:  # pragma: no cover
                raise NotImplementedError(f"dangling scalar input {inp}")
        if isinstance(node.op, Composite):  # nested composite: flatten
            sub = lower_scalar_op(
                node.op,
                [i.type.dtype for i in node.inputs],
                [o.type.dtype for o in node.outputs],
            )
            base = len(body)

            def fix(r, base=base, args=args):
                if r[0] == "i":
                    return args[r[1]]
                if r[0] == "t":
                    return ["t", base + r[1]]
                return r

            for sn in sub["body"]:
                body.append({**sn, "in": [fix(r) for r in sn["in"]]})
            for out, r in zip(node.outputs, sub["outs"]):
                ref[out] = fix(r)
            continue
        if isinstance(node.op, ScalarLoop):
            for out, r in zip(node.outputs, _append_loop(body, node.op, args, [o.type.dtype for o in node.outputs])):
                ref[out] = r
            continue
        if len(node.outputs) != 1:
            raise NotImplementedError(f"multi-output scalar op {node.op}")
        body.append(_scalar_node(node.op, args, node.outputs[0].type.dtype))
        ref[node.outputs[0]] = ["t", len(body) - 1]
    outs = []
    for o in fg.outputs:
        if o in ref:
            outs.append(ref[o])
        elif isinstance(o, Constant):
            outs.append(_const_ref(o))
        else:  # pragma: no cover
            raise NotImplementedError
    return {"in_dtypes": list(in_dtypes), "out_dtypes": list(out_dtypes), "body": body, "outs": outs}


def _const_ref(c: Constant):
    data = np.asarray(c.data)
    dt = str(data.dtype)
    if data.dtype.kind == "f":
        return ["c", float(data).hex(), dt]
    if data.dtype.kind == "b":
        return ["c", int(bool(data)), dt]
    return ["c", int(data), dt]


def _scalar_node(op: ScalarOp, args, out_dtype) -> dict:
    d = {"op": _scalar_op_name(op), "in": args, "dtype": str(out_dtype)}
    return d


# ---------------------------------------------------------------------------
# tensor ops
# ---------------------------------------------------------------------------

def _jsonable(v):
    if isinstance(v, (bool, int, float, str, type(None))):
        return v
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.bool_,)):
        return bool(v)
    if isinstance(v, (tuple, list)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.dtype):
        return str(v)
    if isinstance(v, slice):
        return v
    raise NotImplementedError(f"prop {v!r} ({type(v)})")


@singledispatch
def hip_funcify(op, node, ctx):
    """Return ``(op_name, params)`` for ``op`` or ``None`` for the host fallback."""
    return None


def _props(op):
    return {k: _jsonable(v) for k, v in op._props_dict().items()}


@hip_funcify.register(Elemwise)
def _(op, node, ctx):
    body = lower_scalar_op(
        op.scalar_op,
        [i.type.dtype for i in node.inputs],
        [o.type.dtype for o in node.outputs],
    )
    _require_device_body(body, op)
    return "Elemwise", {"scalar": body}


def _require_device_body(body, op):
    """fail at compile time, not at the first call: every scalar op and dtype of the fused body
    must have a device expression (codegen_scalar.SCALAR_EXPR)"""
    from pytensor_amd import codegen_scalar

    if not codegen_scalar.supported(body):
        missing = sorted({o for o in codegen_scalar.body_ops(body) if o not in codegen_scalar.SCALAR_EXPR})
        dts = sorted({d for d in body["in_dtypes"] + body["out_dtypes"] if d not in codegen_scalar.CTYPE})
        what = ", ".join([*(f"scalar op {m}" for m in missing), *(f"dtype {d}" for d in dts)]) or "an inner loop dtype"
        raise NotImplementedError(f"hip linker: no device code for {what} (in {op})")


@hip_funcify.register(ScalarOp)
def _(op, node, ctx):
    # a ScalarOp applied directly to ScalarType variables (between ScalarFromTensor and
    # TensorFromScalar): the same scalar graph on 0-d values
    body = lower_scalar_op(op, [i.type.dtype for i in node.inputs], [o.type.dtype for o in node.outputs])
    _require_device_body(body, op)
    return "Elemwise", {"scalar": body}


@hip_funcify.register(CAReduce)
def _(op, node, ctx):
    # Sum/Prod/Max/Min/All/Any are subclasses (pytensor/tensor/math.py:3498...)
    axis = op.axis
    if axis is None:
        axis = tuple(range(node.inputs[0].type.ndim))
    acc = getattr(op, "acc_dtype", None)
    in_dtype = node.inputs[0].type.dtype
    out_dtype = node.outputs[0].type.dtype
    acc_dtype = op._acc_dtype(in_dtype) if hasattr(op, "_acc_dtype") else (acc or out_dtype)
    return "CAReduce", {
        "scalar_op": _scalar_op_name(op.scalar_op),
        "axis": [int(a) for a in axis],
        "acc_dtype": str(acc_dtype),
        "dtype": str(out_dtype),
    }


@hip_funcify.register(DimShuffle)
def _(op, node, ctx):
    return "DimShuffle", {"new_order": [("x" if o == "x" else int(o)) for o in op.new_order]}


for _cls in (Dot22, Dot22Scalar, BatchedDot, Dot, Shape, Reshape, ScalarFromTensor,
             TensorFromScalar, ViewOp, DeepCopyOp, SpecifyShape, Alloc):
    @hip_funcify.register(_cls)
    def _(op, node, ctx, _name=_cls.__name__):
        return _name, {}


def _register_sort():
    from pytensor.tensor.sort import ArgSortOp, SortOp

    @hip_funcify.register(SortOp)
    def _(op, node, ctx):
        return "SortOp", {"kind": str(op.kind)}

    @hip_funcify.register(ArgSortOp)
    def _(op, node, ctx):
        return "ArgSortOp", {"kind": str(op.kind), "dtype": str(node.outputs[0].type.dtype)}


_register_sort()


def _register_nonzero():
    from pytensor.tensor.basic import Nonzero

    @hip_funcify.register(Nonzero)
    def _(op, node, ctx):
        return "Nonzero", {}


_register_nonzero()


@hip_funcify.register(Split)
def _(op, node, ctx):
    return "Split", {"len_splits": int(op.len_splits), "axis": int(op.axis)}


@hip_funcify.register(TypeCastingOp)
def _(op, node, ctx):
    return "ViewOp", {}


def _register_extra_ops():
    # ops next to the hot path that model graphs routinely carry along (index helpers, scans)
    from pytensor.tensor.basic import ARange, Eye
    from pytensor.tensor.extra_ops import CumOp
    from pytensor.tensor.math import Argmax

    @hip_funcify.register(ARange)
    @hip_funcify.register(Eye)
    def _(op, node, ctx):
        return type(op).__name__, {"dtype": str(op.dtype)}

    @hip_funcify.register(CumOp)
    def _(op, node, ctx):
        return "CumOp", {"axis": int(op.axis), "mode": str(op.mode)}

    @hip_funcify.register(Argmax)
    def _(op, node, ctx):
        axis = op.axis if op.axis is not None else tuple(range(node.inputs[0].type.ndim))
        return "Argmax", {"axis": [int(a) for a in axis]}

    # general dense solves on LU with partial pivoting (csrc/lu.hip)
    from pytensor.tensor.linalg.inverse import MatrixInverse
    from pytensor.tensor.linalg.solvers.general import Solve
    from pytensor.tensor.linalg.summary import Det, SLogDet

    @hip_funcify.register(Solve)
    def _(op, node, ctx):
        # "sym"/"her" (real dtypes: the same thing) run on the general LU — LAPACK's sysv
        # (Bunch-Kaufman) is a different but equally backward-stable factorisation
        if op.assume_a not in ("gen", "pos", "sym", "her", "tridiagonal", "banded"):
            return None
        return "Solve", {"assume_a": str(op.assume_a), "lower": bool(op.lower), "b_ndim": int(op.b_ndim)}

    @hip_funcify.register(Det)
    @hip_funcify.register(SLogDet)
    @hip_funcify.register(MatrixInverse)
    def _(op, node, ctx):
        return type(op).__name__, {}

    from pytensor.tensor.linalg.decomposition.lu import LUFactor, PivotToPermutations

    @hip_funcify.register(LUFactor)
    def _(op, node, ctx):
        return "LUFactor", {}

    @hip_funcify.register(PivotToPermutations)
    def _(op, node, ctx):
        return "PivotToPermutations", {"inverse": bool(op.inverse)}

    from pytensor.tensor.linalg.decomposition.eigen import Eigh, Eigvalsh

    @hip_funcify.register(Eigh)
    def _(op, node, ctx):
        # one input: the standard problem; two: A v = w B v (dispatch/lu.py::_eigh_generalised)
        return "Eigh", {"lower": bool(op.lower)}

    @hip_funcify.register(Eigvalsh)
    def _(op, node, ctx):
        return "Eigvalsh", {"lower": bool(op.lower)}

    # dense decompositions of the correct-first tier (csrc/decomp.hip, dispatch/decomp.py)
    from pytensor.tensor.linalg.constructors import BlockDiagonal
    from pytensor.tensor.linalg.decomposition.qr import QR
    from pytensor.tensor.linalg.decomposition.svd import SVD
    from pytensor.tensor.linalg.inverse import MatrixPinv, TensorInv
    from pytensor.tensor.linalg.solvers.lstsq import Lstsq, TensorSolve
    from pytensor.tensor.linalg.solvers.tridiagonal import LUFactorTridiagonal, SolveLUFactorTridiagonal

    from pytensor.tensor.linalg.products import Expm

    @hip_funcify.register(Expm)
    def _(op, node, ctx):
        return "Expm", {}

    @hip_funcify.register(QR)
    def _(op, node, ctx):
        if op.pivoting:
            # geqp3: one more output, the int32 permutation, last.  The key is emitted only when true: unpivoted
            # nodes keep exactly the params they always had
            return "QR", {"mode": str(op.mode), "pivoting": True}
        return "QR", {"mode": str(op.mode)}

    @hip_funcify.register(SVD)
    def _(op, node, ctx):
        return "SVD", {"full_matrices": bool(op.full_matrices), "compute_uv": bool(op.compute_uv)}

    @hip_funcify.register(MatrixPinv)
    def _(op, node, ctx):
        return "MatrixPinv", {"hermitian": bool(op.hermitian)}

    @hip_funcify.register(Lstsq)
    def _(op, node, ctx):
        return "Lstsq", {}

    @hip_funcify.register(TensorInv)
    def _(op, node, ctx):
        return "TensorInv", {"ind": int(op.ind)}

    @hip_funcify.register(TensorSolve)
    def _(op, node, ctx):
        return "TensorSolve", {"axes": None if op.axes is None else [int(a) for a in op.axes]}

    @hip_funcify.register(LUFactorTridiagonal)
    def _(op, node, ctx):
        return "LUFactorTridiagonal", {}

    @hip_funcify.register(SolveLUFactorTridiagonal)
    def _(op, node, ctx):
        return "SolveLUFactorTridiagonal", {"b_ndim": int(op.b_ndim), "transposed": bool(op.transposed)}

    @hip_funcify.register(BlockDiagonal)
    def _(op, node, ctx):
        if node is None:
            return None  # (as the core of a Blockwise the output dtype is not known here)
        return "BlockDiagonal", {"dtype": str(node.outputs[0].type.dtype)}

    # kept whole (HipLinker excludes the reference's inline_symbolic_for_fusion): one kernel
    from pytensor.tensor.special import LogSoftmax, Softmax

    @hip_funcify.register(Softmax)
    @hip_funcify.register(LogSoftmax)
    def _(op, node, ctx):
        nd = node.inputs[0].type.ndim
        axis = tuple(range(nd)) if op.axis is None else tuple(int(a) % nd for a in op.axis)
        return "Softmax", {"axis": sorted(axis), "log": isinstance(op, LogSoftmax)}


_register_extra_ops()


def _register_collective():
    # the one explicit collective (pytensor_amd/collective.py; north_star: RCCL over xGMI)
    from pytensor_amd.collective import AllReduce

    @hip_funcify.register(AllReduce)
    def _(op, node, ctx):
        return "AllReduce", {"op": str(op.op)}


_register_collective()


@hip_funcify.register(Gemm)
@hip_funcify.register(Gemv)
@hip_funcify.register(Ger)
def _(op, node, ctx):
    return type(op).__name__, {}


@hip_funcify.register(AllocEmpty)
@hip_funcify.register(MakeVector)
def _(op, node, ctx):
    return type(op).__name__, {"dtype": str(node.outputs[0].type.dtype)}


@hip_funcify.register(Join)
def _(op, node, ctx):
    return "Join", {"axis": int(op.axis)}


@hip_funcify.register(Shape_i)
def _(op, node, ctx):
    return "Shape_i", {"i": int(op.i)}


@hip_funcify.register(ExtractDiag)
def _(op, node, ctx):
    return "ExtractDiag", {"offset": int(op.offset), "axis1": int(op.axis1), "axis2": int(op.axis2)}


@hip_funcify.register(CheckAndRaise)
def _(op, node, ctx):
    return "CheckAndRaise", {"msg": str(op.msg), "exc_type": op.exc_type.__name__}


@hip_funcify.register(Cholesky)
def _(op, node, ctx):
    return "Cholesky", {"lower": bool(op.lower)}


@hip_funcify.register(SolveTriangular)
def _(op, node, ctx):
    return "SolveTriangular", {
        "lower": bool(op.lower),
        "unit_diagonal": bool(op.unit_diagonal),
        "b_ndim": int(op.b_ndim),
    }


@hip_funcify.register(CholeskySolve)
def _(op, node, ctx):
    return "CholeskySolve", {"lower": bool(op.lower), "b_ndim": int(op.b_ndim)}


@hip_funcify.register(Blockwise)
def _(op, node, ctx):
    # (lowerings that look at the Apply node — output dtypes — get the core node the Blockwise itself
    #  builds for shape inference, blockwise.py `_create_dummy_core_node`)
    try:
        core_node = op._create_dummy_core_node(node.inputs) if node is not None else None
    except Exception:  # noqa: BLE001
        core_node = None
    core = hip_funcify(op.core_op, core_node, ctx)
    # (batched kernels exist for the linalg family; any other lowered core op runs as a host loop
    #  over the batch of single-item device calls — dispatch/linalg.py::_blockwise_loop)
    # (a vectorised Scan — `vectorize_graph` of a graph holding a Scan — also runs as that host loop: one device
    #  Scan per batch item, Blockwise.perform's gufunc semantics, pytensor/tensor/blockwise.py:542)
    if core is None or core[0] in ("Blockwise", "HostPerform"):
        return None
    name, params = core
    if name == "SolveSylvester":  # (the dummy core node has fresh inputs: look at the batched ones)
        params = {**params, "b_is_a_t": sylvester_b_is_a_t(node)}
    if core is _INLINE:
        # the core op is an OpFromGraph without a kernel of its own (AllocDiag in the Cholesky pullback,
        # ...): its inner graph, lowered once, is what the host loop runs per batch item
        params = {"inner": lower_fgraph(op.core_op.fgraph, name="blockwise_inner")}
    return "Blockwise", {"core_op": name, "core_params": params, "signature": op.signature}


def _idx_list(idx_list):
    out = []
    for e in idx_list:
        if isinstance(e, slice):
            out.append(slice(e.start, e.stop, e.step))
        elif isinstance(e, (int, np.integer)):
            out.append(int(e))
        else:  # pragma: no cover
            raise NotImplementedError(f"idx_list entry {e!r}")
    return out


@hip_funcify.register(Subtensor)
def _(op, node, ctx):
    return "Subtensor", {"idx_list": _idx_list(op.idx_list)}


@hip_funcify.register(IncSubtensor)
def _(op, node, ctx):
    return "IncSubtensor", {
        "idx_list": _idx_list(op.idx_list),
        "set_instead_of_inc": bool(op.set_instead_of_inc),
    }


@hip_funcify.register(AdvancedSubtensor)
def _(op, node, ctx):
    return "AdvancedSubtensor", {"idx_list": _idx_list(op.idx_list)}


@hip_funcify.register(AdvancedIncSubtensor)
def _(op, node, ctx):
    return "AdvancedIncSubtensor", {
        "idx_list": _idx_list(op.idx_list),
        "set_instead_of_inc": bool(op.set_instead_of_inc),
        "ignore_duplicates": bool(op.ignore_duplicates),
    }


@hip_funcify.register(Scan)
def _(op, node, ctx):
    info = op.info
    inner = lower_fgraph(op.fgraph, name="scan_inner")
    # (a generator used inside the loop is an untraced sit-sot state or a non-sequence of the Scan,
    #  scan/op.py:211 `ScanInfo.n_untraced_sit_sot`: the step driver hands the `RngState` of step t
    #  to step t+1 like any other untraced value, dispatch/scan.py)
    return "Scan", {
        "info": {
            "n_seqs": info.n_seqs,
            "mit_mot_in_slices": _jsonable(info.mit_mot_in_slices),
            "mit_mot_out_slices": _jsonable(info.mit_mot_out_slices),
            "mit_sot_in_slices": _jsonable(info.mit_sot_in_slices),
            "sit_sot_in_slices": _jsonable(info.sit_sot_in_slices),
            "n_nit_sot": info.n_nit_sot,
            "n_untraced_sit_sot": info.n_untraced_sit_sot,
            "n_non_seqs": info.n_non_seqs,
            "as_while": bool(info.as_while),
        },
        "inner": inner,
    }


# ---------------------------------------------------------------------------
# graph
# ---------------------------------------------------------------------------

def _var_spec(v):
    t = v.type
    if isinstance(t, SparseTensorType):  # (a TensorType subclass: checked first)
        _check_sparse_type(t)
        return str(t.dtype), tuple(t.shape), "sparse"
    if isinstance(t, TensorType):
        return str(t.dtype), tuple(t.shape), "tensor"
    if isinstance(t, ScalarType):
        return str(t.dtype), (), "scalar"
    if isinstance(t, SliceType):
        return "object", (), "slice"
    if isinstance(t, NoneTypeT):
        return "object", (), "none"
    if isinstance(t, RandomType):
        return "object", (), "rng"
    raise NotImplementedError(f"unsupported variable type {t!r} for the hip linker")


_INLINE = ("__inline__", {})


@hip_funcify.register(RandomVariable)
def _(op, node, ctx):
    # inputs (rng, size, *dist_params) -> outputs (advanced rng, draws), random/op.py make_node;
    # samplers and their stream: csrc/random.hip, pytensor_amd/rng.py
    from pytensor_amd.dispatch.random import DISTRIBUTIONS, STRUCTURED

    name = str(op.name)
    if name not in DISTRIBUTIONS and name not in STRUCTURED:
        return None
    params = {
        "name": name,
        "dtype": str(node.outputs[1].type.dtype),
        "size_is_none": isinstance(node.inputs[1].type, NoneTypeT),
    }
    if name == "multivariate_normal":
        params["method"] = str(getattr(op, "method", "cholesky"))
    if name in ("permutation", "choice_without_replacement"):
        # rng.permutation / rng.choice have no batch dimensions (the reference loops over them on the host)
        core = int(op.ndims_params[0])
        if node.inputs[2].type.ndim != core or not params["size_is_none"]:
            return None
        params["ndims_params"] = [int(v) for v in op.ndims_params]
    return "RandomVariable", params


def _register_misc():
    # index / layout / signal ops of the widening tier (dispatch/misc.py)
    from pytensor.tensor.extra_ops import (
        Bartlett,
        CpuContiguous,
        FillDiagonal,
        FillDiagonalOffset,
        RavelMultiIndex,
        Repeat,
        SearchsortedOp,
        Unique,
        UnravelIndex,
    )
    from pytensor.tensor.linalg.decomposition.lu import LU
    from pytensor.tensor.reshape import JoinDims, SplitDims
    from pytensor.tensor.basic import Choose, PermuteRowElements
    from pytensor.tensor.signal.conv import Convolve1d, Convolve2d

    @hip_funcify.register(Choose)
    def _(op, node, ctx):
        if node is not None and not isinstance(node.inputs[1].type, TensorType):
            return None  # (typed-list choices)
        return "Choose", {"mode": str(op.mode)}

    @hip_funcify.register(PermuteRowElements)
    def _(op, node, ctx):
        return "PermuteRowElements", {"inverse": bool(op.inverse)}

    for cls in (Bartlett, CpuContiguous, FillDiagonal, FillDiagonalOffset, Convolve1d, Convolve2d):
        hip_funcify.register(cls)(lambda op, node, ctx: (type(op).__name__, {}))

    @hip_funcify.register(JoinDims)
    def _(op, node, ctx):
        return "JoinDims", {"start_axis": int(op.start_axis), "n_axes": int(op.n_axes)}

    @hip_funcify.register(SplitDims)
    def _(op, node, ctx):
        return "SplitDims", {"axis": int(op.axis)}

    @hip_funcify.register(SearchsortedOp)
    def _(op, node, ctx):
        return "SearchsortedOp", {"side": str(op.side)}

    @hip_funcify.register(Repeat)
    def _(op, node, ctx):
        return "Repeat", {"axis": int(op.axis)}

    @hip_funcify.register(UnravelIndex)
    def _(op, node, ctx):
        return "UnravelIndex", {"order": str(op.order)}

    @hip_funcify.register(RavelMultiIndex)
    def _(op, node, ctx):
        return "RavelMultiIndex", {"mode": str(op.mode), "order": str(op.order)}

    @hip_funcify.register(Unique)
    def _(op, node, ctx):
        return "Unique", {"return_index": bool(op.return_index), "return_inverse": bool(op.return_inverse),
                          "return_counts": bool(op.return_counts), "axis": None if op.axis is None else int(op.axis)}

    @hip_funcify.register(LU)
    def _(op, node, ctx):
        return "LU", {"permute_l": bool(op.permute_l), "p_indices": bool(op.p_indices)}


_register_misc()


def _register_fft():
    from pytensor.tensor.fft import IRFFTOp, RFFTOp

    @hip_funcify.register(RFFTOp)
    def _(op, node, ctx):
        return "RFFTOp", {}

    @hip_funcify.register(IRFFTOp)
    def _(op, node, ctx):
        return "IRFFTOp", {}


_register_fft()


def _register_ifelse():
    from pytensor.ifelse import IfElse

    @hip_funcify.register(IfElse)
    def _(op, node, ctx):
        # inputs (condition, n_outs "then" values, n_outs "else" values); lazily evaluated
        return "IfElse", {"n_outs": int(op.n_outs)}


_register_ifelse()


def sylvester_b_is_a_t(node) -> bool:
    """Whether the operands (A, B, C) of a SolveSylvester (or its Blockwise) node have B = A^T: one of A, B is a
    DimShuffle of the other that swaps the last two axes and keeps the leading ones (solve_continuous_lyapunov passes
    (A, A^T); the bilinear solve_discrete_lyapunov, after the rewrites, (B^T, B))."""
    from pytensor.tensor.elemwise import DimShuffle

    if node is None or len(node.inputs) != 3:
        return False

    def is_t(x, y):
        o = x.owner
        if o is None or not isinstance(o.op, DimShuffle) or o.inputs[0] is not y:
            return False
        nd = y.type.ndim
        return nd >= 2 and tuple(o.op.new_order) == (*range(nd - 2), nd - 1, nd - 2)

    a, b = node.inputs[0], node.inputs[1]
    return is_t(a, b) or is_t(b, a)


def _register_ofg():
    from pytensor.compile.builders import OpFromGraph
    from pytensor.tensor.linalg.solvers.linear_control import SolveDiscreteARE, SolveSylvester

    @hip_funcify.register(SolveSylvester)
    def _(op, node, ctx):
        # (its inner graph is Schur + TRSYL, which have no lowering: the equation is solved directly.  b_is_a_t: the
        #  Lyapunov case B = A^T, which the Bartels-Stewart tier solves with one Schur form, dispatch/decomp.py)
        return "SolveSylvester", {"b_is_a_t": sylvester_b_is_a_t(node)}

    @hip_funcify.register(SolveDiscreteARE)
    def _(op, node, ctx):
        # (its inner graph is QR + QZ(sort="iuc"), which has no lowering: the stabilising solution is computed
        #  by the doubling algorithm instead, dispatch/riccati.py)
        return "SolveDiscreteARE", {}

    @hip_funcify.register(OpFromGraph)
    def _(op, node, ctx):
        # OpFromGraph / SymbolicOp without a kernel of its own (AllocDiag, KroneckerProduct, user
        # OpFromGraphs, ...): the reference runs the inner function from ``perform``
        # (compile/builders.py); here the inner graph is lowered in place.  Ops registered on
        # their own class (Softmax, LogSoftmax) take precedence in the dispatch.
        return _INLINE


_register_ofg()


_SPARSE_DTYPES = ("float32", "float64")


def _check_sparse_type(t):
    """csr / csc of float32 / float64 only (indices and indptr are int32, as CSM requires)"""
    if t.format not in ("csr", "csc"):
        raise NotImplementedError(f"hip linker: sparse format {t.format!r} is not supported (only csr and csc)")
    if str(t.dtype) not in _SPARSE_DTYPES:
        raise NotImplementedError(f"hip linker: sparse dtype {t.dtype} is not supported (only float32 and float64)")


def _register_sparse():
    # pytensor.sparse csr / csc: kernels in csrc/sparse.hip, handlers in dispatch/sparse.py.
    # `mode="hip"` excludes the `cxx_only` rewrites (HipLinker.incompatible_rewrites), so the C-only
    # specialisations (MulSDCSR, StructuredDotCSR, AddSD_ccode, ...) never reach the lowering.
    import pytensor.sparse.basic as sb
    import pytensor.sparse.math as sm

    def _is_sparse(v):
        from pytensor.sparse.type import SparseTensorType

        return isinstance(v.type, SparseTensorType)

    for cls in (sb.CSMProperties, sb.CSMGrad, sb.DenseFromSparse, sm.StructuredDotGradCSR,
                sm.StructuredDotGradCSC, sm.SamplingDot, sm.SparseDenseMultiply, sm.SparseDenseVectorMultiply,
                sm.AddSD, sm.StructuredAddSV, sb.ColScaleCSC, sb.RowScaleCSC):
        hip_funcify.register(cls)(lambda op, node, ctx: (type(op).__name__, {}))

    @hip_funcify.register(sb.CSM)
    def _(op, node, ctx):
        return "CSM", {"format": str(op.format)}

    @hip_funcify.register(sb.SparseFromDense)
    def _(op, node, ctx):
        return "SparseFromDense", {"format": str(op.format)}

    @hip_funcify.register(sb.Transpose)
    def _(op, node, ctx):
        return "SparseTranspose", {}

    @hip_funcify.register(sb.Cast)
    def _(op, node, ctx):
        return "SparseCast", {"out_type": str(op.out_type)}

    @hip_funcify.register(sm.SpSum)
    def _(op, node, ctx):
        return "SpSum", {"axis": None if op.axis is None else int(op.axis)}

    def _dense_and_sparse(op, node):
        if node is not None and all(_is_sparse(v) for v in node.inputs):
            raise NotImplementedError(f"hip linker: {type(op).__name__} of two sparse operands (sparse x sparse) is not lowered")

    @hip_funcify.register(sm.Dot)
    def _(op, node, ctx):
        _dense_and_sparse(op, node)
        return "SparseDot", {}

    @hip_funcify.register(sm.TrueDot)
    def _(op, node, ctx):
        _dense_and_sparse(op, node)
        if node is not None and not _is_sparse(node.inputs[0]):
            raise NotImplementedError("hip linker: TrueDot with a dense left operand is not lowered")
        return "TrueDot", {}

    @hip_funcify.register(sm.StructuredDot)
    def _(op, node, ctx):
        _dense_and_sparse(op, node)
        return "StructuredDot", {}

    refused = [sm.AddSS, sm.AddSSData, sm.SparseSparseMultiply, sm.Usmm, sb.GetItemList, sb.GetItemListGrad, sb.GetItem2Lists,
               sb.GetItem2ListsGrad, sb.GetItem2d, sb.GetItemScalar, sb.HStack, sb.VStack, sb.ConstructSparseFromList,
               sb.Remove0, sb.EnsureSortedIndices, sb.Diag]
    refused += [getattr(sm, n) for n in dir(sm) if n.endswith(("SS", "SD")) and n.startswith(
        ("Equal", "NotEqual", "LessThan", "GreaterThan", "LessEqual", "GreaterEqual"))]

    def _refuse(op, node, ctx):
        raise NotImplementedError(f"hip linker: the sparse op {type(op).__name__} is not lowered (DESIGN §7)")

    for cls in refused:
        hip_funcify.register(cls)(_refuse)


_register_sparse()


def lower_fgraph(fgraph, name="graph", allow_host_fallback=False) -> Graph:
    g = Graph(name=name)

    def getter(scope):
        def get(v):
            if v in scope:
                return scope[v]
            dtype, shape, kind = _var_spec(v)
            const = None
            if isinstance(v, Constant):
                if kind in ("tensor", "scalar"):
                    const = np.asarray(v.data)
                    shape = const.shape
                elif kind == "slice":
                    const = v.data
                elif kind == "sparse":
                    const = v.data  # (scipy csr_matrix / csc_matrix; ir.encode_sparse)
                    shape = const.shape
            fmt = v.type.format if kind == "sparse" else None
            i = g.new_var(dtype, shape, kind=kind, const=const, name=getattr(v, "name", None), format=fmt)
            scope[v] = i
            return i

        return get

    def lower_nodes(fg, scope):
        get = getter(scope)
        for node in fg.toposort():
            lowered = hip_funcify(node.op, node, g)
            if lowered is _INLINE:
                # a fresh scope per application: the (interned) inner variables of one op are
                # shared by every node that applies it
                inner = node.op.fgraph
                iscope = {iv: get(ov) for iv, ov in zip(inner.inputs, node.inputs)}
                lower_nodes(inner, iscope)
                iget = getter(iscope)
                for ov, iv in zip(node.outputs, inner.outputs):
                    scope[ov] = iget(iv)
                continue
            ins = [get(v) for v in node.inputs]
            outs = [get(v) for v in node.outputs]
            if lowered is None:
                if not allow_host_fallback:
                    raise NotImplementedError(
                        f"hip linker: no device lowering for {node.op} (set PTHIP_ALLOW_HOST_PERFORM=1 to run it "
                        "through Op.perform on the host)"
                    )
                g.add_node("HostPerform", {"op": node.op, "node": node, "name": str(node.op)}, ins, outs)
            else:
                g.add_node(lowered[0], lowered[1], ins, outs)

    top = {}
    get = getter(top)
    g.inputs = [get(v) for v in fgraph.inputs]
    lower_nodes(fgraph, top)
    g.outputs = [get(v) for v in fgraph.outputs]
    return g
