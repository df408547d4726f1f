"""pytensor.sparse csr / csc matrices (csrc/sparse.hip).

A sparse value is a :class:`~pytensor_amd.device.DeviceSparse`: the three CSR arrays of the matrix (csr) or of
its transpose (csc — scipy's csc arrays are exactly those), so every kernel works on one stored CSR matrix
("major" rows, "minor" columns) and a csc operand is handled by reading the product the other way round.
When a kernel needs the CSR of the other orientation (``_flipped``) it is built by the stable counting sort
of ``pthip_csr_transpose`` — once per constant (kept in the constant's ``cache``), once per call otherwise.

Structure-preserving ops return the input's ``indices`` / ``indptr`` arrays themselves, as the reference's
``perform`` does (sparse/basic.py, sparse/math.py).
"""

from __future__ import annotations

import numpy as np

from pytensor_amd import ffi
from pytensor_amd.device import DeviceArray, DeviceSparse, copy_into
from pytensor_amd.dispatch import handler
from pytensor_amd.executor import HostValue

_LONG_ROW = 1024  # csrc/sparse.hip kLongRow


def _code(dt):
    return ffi.np_dtype_code(dt)


def _dev(env, v) -> DeviceArray:
    return env.to_device(v).contiguous()


def _lanes(nnz, rows):
    mean = nnz / max(rows, 1)
    return 1 if mean <= 6 else 4 if mean <= 24 else 16 if mean <= 96 else 64


def _flipped(env, s: DeviceSparse) -> DeviceSparse:
    """the same logical matrix in the other format (its stored CSR is the transpose of ``s``'s)"""
    f = s.cache.get("flip")
    if f is None:
        rows, n, nnz = s.major, s.minor, s.nnz
        data = DeviceArray.empty((nnz,), s.dtype)
        ind = DeviceArray.empty((nnz,), "int32")
        ptr = DeviceArray.empty((n + 1,), "int32")
        ffi.check(env.lib.pthip_csr_transpose(_code(s.dtype), rows, n, nnz, s.data.ptr, s.indices.ptr, s.indptr.ptr,
                                              data.ptr, ind.ptr, ptr.ptr))
        f = DeviceSparse(data, ind, ptr, s.shape, "csc" if s.format == "csr" else "csr")
        s.cache["flip"] = f
    return f


def _csr_of(env, s: DeviceSparse, transposed: bool) -> DeviceSparse:
    """a DeviceSparse whose stored CSR is the CSR of ``s`` (or of ``s.T`` when ``transposed``)"""
    want = "csc" if transposed else "csr"
    return s if s.format == want else _flipped(env, s)


def _spmm(env, m: DeviceSparse, B, sb0, sb1, k, out, so0, so1):
    """out[r, j] = sum over the stored row r of m of data * B[col, j] (B None: the row sums)"""
    rows, n, nnz = m.major, m.minor, m.nnz
    has_long = 1 if (m.max_row is None or m.max_row > _LONG_ROW) else 0
    ffi.check(env.lib.pthip_csr_spmm(_code(m.dtype), rows, n, k, nnz, m.data.ptr, m.indices.ptr, m.indptr.ptr,
                                     None if B is None else B.ptr, sb0, sb1, out.ptr, so0, so1, _lanes(nnz, rows), has_long))


def _check(cond, node, what):
    # (the kernels index by these extents: a mismatch is refused before anything is launched)
    if not cond:
        raise ValueError(f"hip linker: {node.op}: {what}")


def _require_dtype(node, *vals):
    dts = {str(v.dtype) for v in vals}
    if len(dts) != 1:
        raise NotImplementedError(f"hip linker: {node.op} with mixed dtypes {sorted(dts)}")


def sparse_times_dense(env, s: DeviceSparse, b: DeviceArray, transposed=False) -> DeviceArray:
    """op(S) @ b, op = identity or transpose; b 1-d or 2-d, result of b's rank"""
    m = _csr_of(env, s, transposed)
    if b.shape[0] != m.minor:
        raise ValueError(f"hip linker: sparse product: shapes {s.shape[::-1] if transposed else s.shape} and {b.shape} not aligned")
    if b.ndim == 1:
        out = DeviceArray.empty((m.major,), s.dtype)
        _spmm(env, m, b, b.strides[0], 0, 1, out, 1, 0)
        return out
    k = b.shape[1]
    out = DeviceArray.empty((m.major, k), s.dtype)
    _spmm(env, m, b, b.strides[0], b.strides[1], k, out, k, 1)
    return out


def dense_times_sparse(env, x: DeviceArray, s: DeviceSparse) -> DeviceArray:
    """x @ S = (S.T @ x.T).T, written straight into the result's layout"""
    m = _csr_of(env, s, True)  # the CSR of S.T: rows = columns of S
    if x.shape[-1] != s.shape[0]:
        raise ValueError(f"hip linker: sparse product: shapes {x.shape} and {s.shape} not aligned")
    if x.ndim == 1:
        out = DeviceArray.empty((m.major,), s.dtype)
        _spmm(env, m, x, x.strides[0], 0, 1, out, 1, 0)
        return out
    p = x.shape[0]
    out = DeviceArray.empty((p, m.major), s.dtype)
    _spmm(env, m, x, x.strides[1], x.strides[0], p, out, 1, m.major)
    return out


def _like(s: DeviceSparse, data: DeviceArray, format=None, shape=None) -> DeviceSparse:
    r = DeviceSparse(data, s.indices, s.indptr, shape or s.shape, format or s.format, s.max_row)
    return r


def _gather(env, s: DeviceSparse, op, V: DeviceArray, s_row, s_col) -> DeviceArray:
    """out[e] = data[e] (op 0: *, 1: +) V[row(e) * s_row + col(e) * s_col] in logical rows / columns"""
    s_major, s_minor = (s_row, s_col) if s.format == "csr" else (s_col, s_row)
    out = DeviceArray.empty((s.nnz,), s.dtype)
    ffi.check(env.lib.pthip_csr_gather(_code(s.dtype), op, s.major, s.minor, s.nnz, s.data.ptr, s.indices.ptr, s.indptr.ptr,
                                       V.ptr, s_major, s_minor, out.ptr))
    return out


def _todense_into(env, s: DeviceSparse, out: DeviceArray, accumulate):
    so0, so1 = out.strides if s.format == "csr" else out.strides[::-1]
    ffi.check(env.lib.pthip_csr_todense(_code(s.dtype), s.major, s.minor, s.nnz, s.data.ptr, s.indices.ptr, s.indptr.ptr,
                                        out.ptr, so0, so1, int(accumulate)))


def from_dense(env, x: DeviceArray, format) -> DeviceSparse:
    """SparseFromDense: the non-zeros of x (NaN included, as scipy keeps them), sorted indices"""
    m, n = x.shape
    rows, cols, s0, s1 = (m, n, x.strides[0], x.strides[1]) if format == "csr" else (n, m, x.strides[1], x.strides[0])
    code = _code(x.dtype)
    ptr = DeviceArray.empty((rows + 1,), "int32")
    ffi.check(env.lib.pthip_csr_fromdense_count(code, rows, cols, x.ptr, s0, s1, ptr.ptr))
    nnz = int(np.asarray(env.to_host(ptr.view((1,), (1,), rows)))[0])  # (the one host read, as Nonzero does)
    data = DeviceArray.empty((nnz,), x.dtype)
    ind = DeviceArray.empty((nnz,), "int32")
    ffi.check(env.lib.pthip_csr_fromdense_fill(code, rows, cols, x.ptr, s0, s1, ptr.ptr, data.ptr, ind.ptr))
    return DeviceSparse(data, ind, ptr, (m, n), format)


# ---------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------

@handler("CSMProperties")
def csm_properties(node, inputs, env):
    (s,) = inputs
    return [s.data, s.indices, s.indptr, HostValue(np.array(s.shape, dtype="int32"))]


@handler("CSM")
def csm(node, inputs, env):
    data, ind, ptr, shape = inputs
    shp = [int(v) for v in np.asarray(env.to_host(shape)).ravel()]
    fmt = node.params["format"]
    _check(len(shp) == 2 and min(shp) >= 0, node, f"shape {shp}")
    data, ind, ptr = _dev(env, data), _dev(env, ind), _dev(env, ptr)
    major = shp[0] if fmt == "csr" else shp[1]
    _check(ptr.shape == (major + 1,), node, f"indptr of length {ptr.shape} for {major} {'rows' if fmt == 'csr' else 'columns'}")
    _check(ind.shape == data.shape, node, f"indices {ind.shape} and data {data.shape} differ in length")
    return [DeviceSparse(data, ind, ptr, shp, fmt)]


@handler("CSMGrad")
def csm_grad(node, inputs, env):
    x_data, x_ind, x_ptr, _x_shape, g_data, g_ind, g_ptr, _g_shape = inputs
    x_ind, x_ptr, g_data, g_ind, g_ptr = (_dev(env, v) for v in (x_ind, x_ptr, g_data, g_ind, g_ptr))
    _check(g_ptr.shape == x_ptr.shape and g_ind.shape == g_data.shape and x_ind.shape == x_data.shape, node, "structures differ in size")
    out = DeviceArray.empty((x_data.shape[0],), g_data.dtype)
    ffi.check(env.lib.pthip_csr_csm_grad(_code(g_data.dtype), x_ptr.shape[0] - 1, x_ind.shape[0], x_ind.ptr, x_ptr.ptr,
                                         g_data.shape[0], g_data.ptr, g_ind.ptr, g_ptr.ptr, out.ptr))
    return [out]


@handler("SparseTranspose")
def transpose(node, inputs, env):
    (s,) = inputs
    r = DeviceSparse(s.data, s.indices, s.indptr, s.shape[::-1], "csc" if s.format == "csr" else "csr", s.max_row)
    f = s.cache.get("flip")
    if f is not None:  # (the transpose of a flipped constant is the flip of its transpose)
        r.cache["flip"] = DeviceSparse(f.data, f.indices, f.indptr, s.shape[::-1], s.format, f.max_row)
    return [r]


@handler("SparseCast")
def cast(node, inputs, env):
    (s,) = inputs
    dt = node.params["out_type"]
    if str(s.dtype) == dt:
        return [s]
    from pytensor_amd.dispatch.elemwise import _cast

    return [_like(s, _cast(env, s.data.contiguous(), dt))]


@handler("DenseFromSparse")
def dense_from_sparse(node, inputs, env):
    (s,) = inputs
    out = DeviceArray.empty(s.shape, s.dtype)
    _todense_into(env, s, out, accumulate=False)
    return [out]


@handler("SparseFromDense")
def sparse_from_dense(node, inputs, env):
    (x,) = inputs
    return [from_dense(env, _dev(env, x), node.params["format"])]


# ---------------------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------------------

@handler("StructuredDot")
def structured_dot(node, inputs, env):
    a, b = inputs
    b = _dev(env, b)
    _require_dtype(node, a, b)
    return [sparse_times_dense(env, a, b)]


@handler("SparseDot")
def sparse_dot(node, inputs, env):
    x, y = inputs
    if isinstance(x, DeviceSparse):
        y = _dev(env, y)
        _require_dtype(node, x, y)
        return [sparse_times_dense(env, x, y)]
    x = _dev(env, x)
    _require_dtype(node, x, y)
    return [dense_times_sparse(env, x, y)]


@handler("TrueDot")
def true_dot(node, inputs, env):
    x, y = inputs
    y = _dev(env, y)
    _require_dtype(node, x, y)
    d = sparse_times_dense(env, x, y)
    if d.ndim == 1:
        d = d.view((d.shape[0], 1), (1, 1))
    return [from_dense(env, d, x.format)]


def _sddmm(env, node, ind, ptr, P, Q, k, data=None):
    """out[e] = (data[e]) * <P[major(e), :], Q[minor(e), :]>"""
    out = DeviceArray.empty((ind.shape[0],), P.dtype)
    ffi.check(env.lib.pthip_csr_sddmm(_code(P.dtype), ptr.shape[0] - 1, Q.shape[0], k, ind.shape[0],
                                      None if data is None else data.ptr, ind.ptr, ptr.ptr,
                                      P.ptr, P.strides[0], P.strides[1], Q.ptr, Q.strides[0], Q.strides[1], out.ptr))
    return out


@handler("StructuredDotGradCSR", "StructuredDotGradCSC")
def structured_dot_grad(node, inputs, env):
    # g_a_data[e] = <g_ab[row(e), :], b[col(e), :]> over the structure of a (sparse/math.py StructuredDotGradCSR)
    ind, ptr, b, g = (_dev(env, v) for v in inputs)
    _require_dtype(node, b, g)
    _check(b.ndim == 2 and g.ndim == 2 and b.shape[1] == g.shape[1], node, f"operands {b.shape} and {g.shape}")
    major = (g if node.op == "StructuredDotGradCSR" else b).shape[0]
    _check(ptr.shape == (major + 1,), node, f"indptr of length {ptr.shape} for {major} rows")
    if node.op == "StructuredDotGradCSR":
        return [_sddmm(env, node, ind, ptr, g, b, b.shape[1])]
    return [_sddmm(env, node, ind, ptr, b, g, b.shape[1])]


@handler("SamplingDot")
def sampling_dot(node, inputs, env):
    # p .* (x @ y.T) on the structure of p (sparse/math.py SamplingDot)
    x, y, p = inputs
    x, y = _dev(env, x), _dev(env, y)
    _require_dtype(node, x, y, p)
    _check(x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1] and (x.shape[0], y.shape[0]) == p.shape, node,
           f"operands {x.shape}, {y.shape} and pattern {p.shape}")
    P, Q = (x, y) if p.format == "csr" else (y, x)
    return [_like(p, _sddmm(env, node, p.indices, p.indptr, P, Q, x.shape[1], data=p.data))]


@handler("SpSum")
def sp_sum(node, inputs, env):
    (s,) = inputs
    axis = node.params["axis"]
    if axis is None:
        from pytensor_amd.dispatch.elemwise import device_reduce

        d = s.data.contiguous()
        if d.shape[0] == 0:
            out = DeviceArray.empty((), s.dtype)
            ffi.check(env.lib.pthip_memset(out.ptr, 0, out.nbytes))
            return [out]
        return [device_reduce(env, "Add", d, 1, d.shape[0], 1, 0, 1, 0, str(s.dtype), str(s.dtype), ())]
    m = _csr_of(env, s, transposed=(axis == 0))  # axis 1: row sums of S; axis 0: row sums of S.T
    out = DeviceArray.empty((m.major,), s.dtype)
    _spmm(env, m, None, 0, 0, 1, out, 1, 0)
    return [out]


# ---------------------------------------------------------------------------------------------------------
# structure-preserving gathers
# ---------------------------------------------------------------------------------------------------------

@handler("SparseDenseMultiply")
def mul_s_d(node, inputs, env):
    s, y = inputs
    y = env.to_device(y)
    _require_dtype(node, s, y)
    if y.ndim == 0:
        return [_like(s, _gather(env, s, 0, y, 0, 0))]
    _check(y.shape == s.shape, node, f"shapes {s.shape} and {y.shape}")
    return [_like(s, _gather(env, s, 0, y, y.strides[0], y.strides[1]))]


@handler("SparseDenseVectorMultiply")
def mul_s_v(node, inputs, env):
    s, v = inputs
    v = env.to_device(v)
    _require_dtype(node, s, v)
    _check(v.shape == (s.shape[1],), node, f"matrix {s.shape} and vector {v.shape}")
    return [_like(s, _gather(env, s, 0, v, 0, v.strides[0]))]


@handler("StructuredAddSV")
def structured_add_s_v(node, inputs, env):
    s, v = inputs
    v = env.to_device(v)
    _require_dtype(node, s, v)
    _check(v.shape == (s.shape[1],), node, f"matrix {s.shape} and vector {v.shape}")
    return [_like(s, _gather(env, s, 1, v, 0, v.strides[0]))]


@handler("ColScaleCSC")
def col_scale_csc(node, inputs, env):
    s, v = inputs
    v = env.to_device(v)
    _require_dtype(node, s, v)
    _check(v.shape == (s.shape[1],), node, f"matrix {s.shape} and vector {v.shape}")
    return [_like(s, _gather(env, s, 0, v, 0, v.strides[0]))]


@handler("RowScaleCSC")
def row_scale_csc(node, inputs, env):
    s, v = inputs
    v = env.to_device(v)
    _require_dtype(node, s, v)
    _check(v.shape == (s.shape[0],), node, f"matrix {s.shape} and vector {v.shape}")
    return [_like(s, _gather(env, s, 0, v, v.strides[0], 0))]


@handler("AddSD")
def add_s_d(node, inputs, env):
    s, y = inputs
    y = env.to_device(y)
    _require_dtype(node, s, y)
    _check(y.shape == s.shape, node, f"shapes {s.shape} and {y.shape}")
    out = DeviceArray.empty(s.shape, s.dtype)
    copy_into(out, y)
    _todense_into(env, s, out, accumulate=True)
    return [out]
