"""CPU: pytensor.sparse csr / csc under ``mode="hip"`` — what is lowered, what is refused, and sparse constants in the IR.

Compiles only (no GPU needed): the lowered IR is read from ``f.maker.linker.last_ir`` as in tests/test_lowering.py.
"""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

import make_ref

pytestmark = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")

FORMATS = ("csr", "csc")
DTYPES = ("float32", "float64")


@pytest.fixture(scope="module")
def pt():
    make_ref.activate()
    import pytensor
    import pytensor.sparse as ps
    import pytensor.tensor as ptt

    import pytensor_amd

    pytensor_amd.register()
    return pytensor, ptt, ps


def _ops(f):
    g = f.maker.linker.last_ir
    ops = [n.op for n in g.nodes]
    assert "HostPerform" not in ops
    return ops


def _graphs(pytensor, ptt, ps, fmt, dt):
    """name -> (inputs, outputs, the IR op the graph must contain)"""
    import pytensor.sparse.basic as sb
    import pytensor.sparse.math as sm

    x = ps.matrix(fmt, "x", dtype=dt)
    b = ptt.matrix("b", dtype=dt)
    v = ptt.vector("v", dtype=dt)
    d = ptt.vector("d", dtype=dt)
    ind, ptr, shp = ptt.ivector("i"), ptt.ivector("p"), ptt.ivector("s")
    m = sb.CSM(fmt)(d, ind, ptr, shp)
    g = {
        "CSMProperties": ([x], list(sb.csm_properties(x)[:3]), "CSMProperties"),
        "CSM": ([d, ind, ptr, shp], m, "CSM"),
        "CSMGrad": ([d, ind, ptr, shp, b], pytensor.grad(ps.structured_dot(m, b).sum(), d), "CSMGrad"),
        "Cast": ([x], sb.cast(x, "float64" if dt == "float32" else "float32"), "SparseCast"),
        "Transpose": ([x], ps.transpose(x), "SparseTranspose"),
        "DenseFromSparse": ([x], ps.dense_from_sparse(x), "DenseFromSparse"),
        "SparseFromDense": ([b], sb.SparseFromDense(fmt)(b), "SparseFromDense"),
        "StructuredDot": ([x, b], ps.structured_dot(x, b), "StructuredDot"),
        "Dot_sd": ([x, b], sm.dot(x, b), "SparseDot"),
        "Dot_ds": ([b, x], sm.dot(b, x), "SparseDot"),
        "TrueDot": ([x, b], sm.true_dot(x, b), "TrueDot"),
        "StructuredDotGrad": ([x, b], pytensor.grad(ps.structured_dot(x, b).sum(), x),
                              "StructuredDotGradCSR" if fmt == "csr" else "StructuredDotGradCSC"),
        "SamplingDot": ([b, x], sm.sampling_dot(b, b, x), "SamplingDot"),
        "SpSum_None": ([x], sm.sp_sum(x), "SpSum"),
        "SpSum_0": ([x], sm.sp_sum(x, 0), "SpSum"),
        "SpSum_1": ([x], sm.sp_sum(x, 1), "SpSum"),
        "SpSum_grad_sparse": ([x], pytensor.grad(sm.sp_sum(x, 0, sparse_grad=True).sum(), x), "CSM"),
        "SpSum_grad_dense": ([x], pytensor.grad(sm.sp_sum(x, 1, sparse_grad=False).sum(), x), "SparseFromDense"),
        "SparseDenseMultiply": ([x, b], sm.mul_s_d(x, b), "SparseDenseMultiply"),
        "SparseDenseVectorMultiply": ([x, v], sm.mul_s_v(x, v), "SparseDenseVectorMultiply"),
        "AddSD": ([x, b], sm.add_s_d(x, b), "AddSD"),
        "StructuredAddSV": ([x, v], sm.structured_add_s_v(x, v), "StructuredAddSV"),
    }
    if fmt == "csc":
        g["ColScaleCSC"] = ([x, v], sb.ColScaleCSC()(x, v), "ColScaleCSC")
        g["RowScaleCSC"] = ([x, v], sb.RowScaleCSC()(x, v), "RowScaleCSC")
    return g


CASES = ["CSMProperties", "CSM", "CSMGrad", "Cast", "Transpose", "DenseFromSparse", "SparseFromDense", "StructuredDot",
         "Dot_sd", "Dot_ds", "TrueDot", "StructuredDotGrad", "SamplingDot", "SpSum_None", "SpSum_0", "SpSum_1",
         "SpSum_grad_sparse", "SpSum_grad_dense", "SparseDenseMultiply", "SparseDenseVectorMultiply", "AddSD",
         "StructuredAddSV", "ColScaleCSC", "RowScaleCSC"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", CASES)
def test_sparse_op_lowers(pt, case, fmt, dt):
    pytensor, ptt, ps = pt
    g = _graphs(pytensor, ptt, ps, fmt, dt)
    if case not in g:
        pytest.skip(f"{case} takes a csc operand only")
    ins, outs, op = g[case]
    f = pytensor.function(ins, outs, mode="hip", on_unused_input="ignore")
    ops = _ops(f)
    assert op in ops, ops
    v = f.maker.linker.last_ir.vars
    sparse = [x for x in v.values() if x.kind == "sparse"]
    assert all(x.format in FORMATS and x.dtype in DTYPES for x in sparse)


@pytest.mark.parametrize("fmt", FORMATS)
def test_structured_unary_is_one_elemwise_on_data(pt, fmt):
    pytensor, ptt, ps = pt
    x = ps.matrix(fmt, "x", dtype="float64")
    f = pytensor.function([x], ps.structured_exp(x), mode="hip")
    assert _ops(f) == ["CSMProperties", "Elemwise", "CSM"]
    g = f.maker.linker.last_ir
    props, ew, csm = g.nodes
    assert ew.inputs == [props.outputs[0]] and csm.inputs[0] == ew.outputs[0]
    assert csm.inputs[1:3] == props.outputs[1:3]  # the structure passes through, no copy


def test_sparse_var_kind_and_format_in_ir(pt):
    pytensor, ptt, ps = pt
    x = ps.csc_matrix("x", dtype="float32")
    f = pytensor.function([x], ps.transpose(x), mode="hip")
    g = f.maker.linker.last_ir
    vi, vo = g.vars[g.inputs[0]], g.vars[g.outputs[0]]
    assert (vi.kind, vi.format, vi.dtype) == ("sparse", "csc", "float32")
    assert (vo.kind, vo.format) == ("sparse", "csr")


def _refused(pytensor, ptt, ps):
    import pytensor.sparse.basic as sb
    import pytensor.sparse.math as sm

    x, y = ps.csr_dmatrix("x"), ps.csr_dmatrix("y")
    b = ptt.dmatrix("b")
    return {
        "AddSS": ([x, y], sm.add_s_s(x, y)),
        "SparseSparseMultiply": ([x, y], sm.mul_s_s(x, y)),
        "StructuredDot": ([x, y], sm.structured_dot(x, y)),
        "Dot": ([x, y], sm.dot(x, y)),
        "EqualSD": ([x, b], sm.equal_s_d(x, b)),
        "LessThanSS": ([x, y], sm.less_than_s_s(x, y)),
        "GetItem2d": ([x], x[1:3, 0:2]),
        "GetItemScalar": ([x], x[1, 2]),
        "HStack": ([x, y], sb.hstack([x, y])),
        "VStack": ([x, y], sb.vstack([x, y])),
        "Remove0": ([x], sb.Remove0()(x)),
        "EnsureSortedIndices": ([x], sb.ensure_sorted_indices(x)),
        "Diag": ([x], sb.diag(x)),
    }


@pytest.mark.parametrize("name", ["AddSS", "SparseSparseMultiply", "StructuredDot", "Dot", "EqualSD", "LessThanSS", "GetItem2d",
                                  "GetItemScalar", "HStack", "VStack", "Remove0", "EnsureSortedIndices", "Diag"])
def test_refused_sparse_ops_name_themselves(pt, name):
    pytensor, ptt, ps = pt
    ins, outs = _refused(pytensor, ptt, ps)[name]
    with pytest.raises(NotImplementedError, match=name):
        pytensor.function(ins, outs, mode="hip")


@pytest.mark.parametrize("dtype", ["int32", "complex128"])
def test_unsupported_sparse_dtype_is_named(pt, dtype):
    pytensor, ptt, ps = pt
    x = ps.csr_matrix("x", dtype=dtype)
    with pytest.raises(NotImplementedError, match=dtype):
        pytensor.function([x], ps.transpose(x), mode="hip")


def test_bsr_is_refused(pt):
    pytensor, ptt, ps = pt
    x = ps.bsr_matrix("x", dtype="float64")
    with pytest.raises(NotImplementedError, match="bsr"):
        pytensor.function([x], x, mode="hip")


def _with_unsorted_duplicates(fmt):
    # structure as given: unsorted indices and a duplicate entry must survive unchanged
    data = np.array([1.5, -2.0, 3.25, 0.5, 7.0])
    indices = np.array([2, 0, 2, 1, 0], dtype=np.int32)
    indptr = np.array([0, 3, 3, 5], dtype=np.int32)
    cls = sp.csr_matrix if fmt == "csr" else sp.csc_matrix
    return cls((data, indices, indptr), shape=(3, 4) if fmt == "csr" else (4, 3))


@pytest.mark.parametrize("fmt", FORMATS)
def test_sparse_constant_ir_round_trip(pt, fmt):
    pytensor, ptt, ps = pt
    from pytensor_amd.ir import Graph

    W = _with_unsorted_duplicates(fmt)
    b = ptt.dmatrix("b")
    f = pytensor.function([b], ps.structured_dot(ps.as_sparse_variable(W), b), mode="hip")
    g = f.maker.linker.last_ir
    g2 = Graph.from_json(g.to_json())
    (c,) = [v for v in g.vars.values() if v.kind == "sparse" and v.const is not None]
    c2 = g2.vars[c.id]
    assert (c2.kind, c2.format, c2.dtype) == ("sparse", fmt, "float64")
    assert c2.const.format == fmt and c2.const.shape == W.shape
    for a in ("data", "indices", "indptr"):
        np.testing.assert_array_equal(getattr(c2.const, a), getattr(W, a))
        assert getattr(c2.const, a).dtype == getattr(W, a).dtype
    assert [n.op for n in g2.nodes] == [n.op for n in g.nodes]


def test_function_with_sparse_constant_pickles(pt):
    pytensor, ptt, ps = pt
    W = _with_unsorted_duplicates("csr")
    b = ptt.dmatrix("b")
    f = pytensor.function([b], ps.structured_dot(ps.as_sparse_variable(W), b), mode="hip")
    f2 = pickle.loads(pickle.dumps(f))
    g = f2.maker.linker.last_ir
    (c,) = [v for v in g.vars.values() if v.kind == "sparse" and v.const is not None]
    np.testing.assert_array_equal(c.const.indices, W.indices)
    np.testing.assert_array_equal(c.const.data, W.data)
    assert "StructuredDot" in [n.op for n in g.nodes]


def test_car_logp_grad_lowers_without_host_perform(pt):
    pytensor, ptt, ps = pt
    import pytensor.sparse.math as sm

    W = sp.random(60, 60, density=0.08, format="csr", random_state=0)
    W = ((W + W.T) > 0).astype("float64").tocsr()
    Wc = ps.as_sparse_variable(W)
    phi = ptt.dvector("phi")
    tau, alpha = ptt.dscalar("tau"), ptt.dscalar("alpha")
    D = sm.sp_sum(Wc, axis=0)
    Wphi = ps.structured_dot(Wc, phi[:, None])[:, 0]
    delta = phi * D - alpha * Wphi
    logp = -0.5 * tau * (phi * delta).sum() + 0.5 * tau * ps.dot(delta[None, :], Wc)[0].sum()
    f = pytensor.function([phi, tau, alpha], [logp, *pytensor.grad(logp, [phi, tau, alpha])], mode="hip")
    ops = _ops(f)
    assert "StructuredDot" in ops or "SparseDot" in ops
    g = f.maker.linker.last_ir
    assert all(g.vars[i].kind == "tensor" for i in g.inputs)  # W is a constant, not an input
