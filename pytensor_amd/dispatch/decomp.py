"""Dense decompositions and what is composed from them: ``QR``, ``SVD``, ``MatrixPinv``, ``Lstsq``,
the tridiagonal LU pair, ``Eigvalsh``, ``TensorInv`` / ``TensorSolve``, ``BlockDiagonal``.

Reference: linalg/decomposition/qr.py:20 (perform 153-221: geqrf + orgqr), decomposition/svd.py:19
(np.linalg.svd), inverse.py:14 ``MatrixPinv`` (np.linalg.pinv), 169 ``TensorInv``,
solvers/lstsq.py:10 ``Lstsq`` (np.linalg.lstsq), 39 ``TensorSolve``, solvers/tridiagonal.py:18, 92
(gttrf / gttrs), decomposition/eigen.py:363 ``Eigvalsh``, constructors.py:52 ``BlockDiagonal``
(scipy.linalg.block_diag).  Kernels: csrc/decomp.hip (correct-first tier).
Leading batch dimensions arrive through ``Blockwise``: ``QR`` (pivoted or not), ``SVD`` and ``MatrixPinv`` take the
whole stack — ``svd_tier``: one launch of csrc/svd_batched.hip up to max(m, n) = 64, the kernels of the single matrix
launched once each over the stack above it, and beyond min(m, n) = 2048 the whole-chip block Jacobi tier
(``pthip_svd_block``, csrc/eigh.hip), which a single matrix of that size takes as well; dispatch/linalg.py loops the
items of the other ops here.
"""

from __future__ import annotations

import numpy as np

from pytensor_amd import ffi
from pytensor_amd.device import DeviceArray, contiguous_strides, copy_into
from pytensor_amd.dispatch import handler
from pytensor_amd.dispatch.linalg import _dt, _require_float
from pytensor_amd.executor import HostValue


def _cs(shape):
    return contiguous_strides(tuple(shape))


def _reshape(x: DeviceArray, shape) -> DeviceArray:
    x = x.contiguous()
    return x.view(tuple(shape), _cs(shape))


def _t(x: DeviceArray) -> DeviceArray:
    """transposed view of a matrix"""
    return x.view((x.shape[1], x.shape[0]), (x.strides[1], x.strides[0]))


def _matrix(env, v, what):
    from pytensor_amd.dispatch.linalg import _lapack_operands

    (x,) = _lapack_operands(env, what, v)
    if x.ndim != 2:
        # (np.linalg raises LinAlgError: "%d-dimensional array given. Array must be two-dimensional")
        raise np.linalg.LinAlgError(f"{what}: {x.ndim}-dimensional array given. Array must be two-dimensional")
    return x


# ---- QR -------------------------------------------------------------------------------------------
def geqrf_device(env, x: DeviceArray):
    """(packed factors, tau) — LAPACK's geqrf on a copy of ``x`` (..., m, n), the leading batch dimensions flattened
    into one launch like ``geqp3_device``; tau (..., min(m, n))"""
    *lead, m, n = x.shape
    nb = int(np.prod(lead)) if lead else 1
    qr = x.contiguous_copy()
    tau = DeviceArray.empty((*lead, min(m, n)), x.dtype)
    ffi.check(env.lib.pthip_geqrf(_dt(x), nb, m, n, qr.ptr, tau.ptr))
    return qr, tau


QR_LDS_MAX = 160 * 1024 - 12 * 1024  # (csrc/decomp.hip)


def geqp3_lds_fits(m: int, n: int, itemsize: int) -> bool:
    """Whether ``pthip_geqp3`` keeps an m x n matrix in LDS (beside the two norm vectors and the permutation) or
    leaves it in global memory: the bound of csrc/decomp.hip ``geqp3_typed``, for tests and tools that want to sit
    on either side of it.  (``PTHIP_QR_NO_LDS`` forces the global form whatever this says.)"""
    return m <= 512 and m * n * itemsize + n * (2 * itemsize + 4) <= QR_LDS_MAX


def geqp3_device(env, x: DeviceArray):
    """(packed factors, tau, jpvt) — LAPACK's geqp3 on a copy of ``x`` (..., m, n): A P = Q R with the leading batch
    dimensions flattened into one launch; jpvt (..., n) int32, 0-based.  A broadcast (stride-0) operand is
    materialised by the copy."""
    *lead, m, n = x.shape
    nb = int(np.prod(lead)) if lead else 1
    qr = x.contiguous_copy()
    tau = DeviceArray.empty((*lead, min(m, n)), x.dtype)
    jpvt = DeviceArray.empty((*lead, n), np.dtype("int32"))
    ffi.check(env.lib.pthip_geqp3(_dt(x), nb, m, n, qr.ptr, tau.ptr, jpvt.ptr))
    return qr, tau, jpvt


def orgqr_device(env, qr: DeviceArray, tau: DeviceArray, ncols: int) -> DeviceArray:
    """Q (..., m, ncols) of the packed factors ``qr`` (..., m, n) and ``tau`` (..., k): one launch for the stack"""
    *lead, m, n = qr.shape
    nb = int(np.prod(lead)) if lead else 1
    q = DeviceArray.empty((*lead, m, ncols), qr.dtype)
    ffi.check(env.lib.pthip_orgqr(_dt(qr), nb, m, ncols, tau.shape[-1], qr.ptr, n, m * n, tau.ptr, q.ptr))
    return q


def _triu(env, qr: DeviceArray, rows: int, lower=False, unit=False) -> DeviceArray:
    *lead, m, n = qr.shape
    nb = int(np.prod(lead)) if lead else 1
    r = DeviceArray.empty((*lead, rows, n), qr.dtype)
    ffi.check(env.lib.pthip_triu(_dt(qr), nb, rows, n, qr.ptr, n, m * n, r.ptr, int(lower), int(unit)))
    return r


def _geqp3_empty(m: int, n: int, dtype) -> None:
    """An empty operand launches nothing; what happens instead is whatever the reference's ``QR.perform`` does with
    it, which is LAPACK's own argument check.  SciPy 1.15: n = 0 returns (empty factors, an empty permutation, and
    for mode "full" the m x m identity — the code below gives exactly that), while m = 0 with n > 0 raises f2py's
    ``_flapack.error`` ("(lwork>=n||lwork==-1) failed for 1st keyword lwork: dgeqp3:lwork=0": the workspace query
    answers 0).  That class has no public name, so the same two calls are made here on an empty host array of the
    operand's shape — no device data is read — and raise it, type and message, themselves."""
    import scipy.linalg

    a = np.empty((m, n), dtype=dtype)
    (geqp3,) = scipy.linalg.get_lapack_funcs(("geqp3",), (a,))
    *_, work, _info = geqp3(a, lwork=-1)
    geqp3(a, lwork=work.item())


@handler("QR")
def qr_op(node, inputs, env):
    """``QR.perform``.  The operand may carry leading batch dimensions (``Blockwise`` hands the whole stack over:
    every kernel takes a batch count); with ``pivoting`` (geqp3) the permutation is the last output."""
    from pytensor_amd.dispatch.linalg import _lapack_operands

    mode = node.params["mode"]
    pivoting = bool(node.params.get("pivoting", False))
    (x,) = _lapack_operands(env, "QR", inputs[0])
    if x.ndim < 2:
        raise np.linalg.LinAlgError(f"QR: {x.ndim}-dimensional array given. Array must be at least two-dimensional")
    m, n = x.shape[-2:]
    if pivoting:
        if m == 0 or n == 0:
            _geqp3_empty(m, n, x.dtype)
        qr, tau, jpvt = geqp3_device(env, x)
        P = [jpvt]
    else:
        qr, tau = geqrf_device(env, x)
        P = []
    # perform 171-174: economic / raw keep the leading n rows of R when m >= n
    R = _triu(env, qr, m if (mode not in ("economic", "raw") or m < n) else n)
    if mode == "r":
        return [R, *P]
    if mode == "raw":
        return [qr, tau, R, *P]
    if m < n:
        Q = orgqr_device(env, qr, tau, m)
    elif mode == "economic":
        Q = orgqr_device(env, qr, tau, n)
    else:
        Q = orgqr_device(env, qr, tau, m)
    return [Q, R, *P]


# ---- SVD ------------------------------------------------------------------------------------------
def svd_device(env, x: DeviceArray, full_matrices: bool, compute_uv: bool):
    """(U, S, Vt) or S alone.  One-sided Jacobi on the rows of the wide orientation of ``x``
    (csrc/decomp.hip); the tall factor's null / complementary directions are completed from a
    Householder Q, which LAPACK leaves just as arbitrary."""
    if x.ndim > 2:
        return _svd_stack(env, x, full_matrices, compute_uv)
    m, n = x.shape
    if min(m, n) > SVD_ROWS_MAX:  # (read at call time)
        return _svd_block(env, x, full_matrices, compute_uv)
    tall = m >= n
    X = (_t(x).contiguous_copy() if tall else x.contiguous_copy())  # r x c, r <= c
    r, c = X.shape
    dt = x.dtype
    S = DeviceArray.empty((r,), dt)
    if r == 0:
        if not compute_uv:
            return [S]
        eye = lambda k: env.to_device(HostValue(np.eye(k, dtype=dt)))
        if full_matrices:
            return [eye(m), S, eye(n)]
        return [DeviceArray.empty((m, 0), dt), S, DeviceArray.empty((0, n), dt)]
    work = DeviceArray.empty((r, r), dt) if compute_uv else DeviceArray.empty((1,), dt)
    Wt = DeviceArray.empty((r, c), dt) if compute_uv else work
    Pt = DeviceArray.empty((r, r), dt) if compute_uv else work
    ffi.check(env.lib.pthip_svd_rows(_dt(x), 1, r, c, int(compute_uv), X.ptr, work.ptr, S.ptr, Wt.ptr, Pt.ptr))
    env.keepalive.extend((X, work))
    if not compute_uv:
        return [S]
    # completion: Householder Q of Wt^T (c x r); its column i replaces a null row i, its columns
    # r.. (full_matrices) span the complement
    rows = c if full_matrices else r
    qr, tau = geqrf_device(env, _t(Wt))
    Q = orgqr_device(env, qr, tau, rows)
    if rows == r:
        big = Wt
    else:
        big = DeviceArray.empty((rows, c), dt)
        copy_into(big.view((r, c), _cs((r, c))), Wt)
    ffi.check(env.lib.pthip_fill_null_rows(_dt(x), 1, rows, c, big.ptr, S.ptr, r, Q.ptr, rows))
    env.keepalive.extend((Q, qr, tau))
    if tall:  # x^T = P S Wt  ->  x = Wt^T S P^T
        return [_t(big).contiguous(), S, Pt]
    return [_t(Pt).contiguous(), S, big]


SVD_WAVE_MAX = 64  # max(m, n) of the one-launch tier (csrc/svd_batched.hip)
SVD_ROWS_MAX = 2048  # min(m, n) of pthip_svd_rows
PINV_RCOND = 1e-15  # np.linalg.pinv's default


def svd_tier(m: int, n: int, nb: int):
    """The tier that takes a stack of ``nb`` m x n matrices, from the shapes alone: "wave" (one lane group per matrix,
    one launch) up to max(m, n) = 64, "rows" (one ``pthip_svd_rows`` workgroup per matrix, the batch in grid.x, and the
    batched completion) above that up to min(m, n) = 2048, "block" (``pthip_svd_block``: the whole chip on one matrix
    at a time, the items walked inside the call) beyond."""
    if max(m, n) <= SVD_WAVE_MAX:
        return "wave"
    if min(m, n) <= SVD_ROWS_MAX:
        return "rows"
    return "block"


def _svd_block(env, x: DeviceArray, full_matrices: bool, compute_uv: bool):
    """``svd_device`` on the block tier, a matrix or a stack (..., m, n) with m, n >= 1: the wide-orientation copy, one
    ``pthip_svd_block`` call (it completes its own factors) and the factors in ``svd_device``'s layout.  The tier
    reads the device once per sweep, so it cannot be part of a frozen plan."""
    if env.exe._capturing:
        raise ffi.HipError("data-dependent host read inside a frozen (hipGraph) plan")
    *lead, m, n = x.shape
    nb = int(np.prod(lead)) if lead else 1
    tall = m >= n
    X = (_tb(x) if tall else x).contiguous_copy()  # (..., r, c), r <= c
    r, c = X.shape[-2:]
    dt = x.dtype
    S = DeviceArray.empty((*lead, r), dt)
    if not compute_uv:
        ffi.check(env.lib.pthip_svd_block(_dt(x), nb, r, c, 0, r, X.ptr, S.ptr, None, None))
        env.keepalive.append(X)
        return [S]
    rows = c if full_matrices else r
    Wt = DeviceArray.empty((*lead, rows, c), dt)
    Pt = DeviceArray.empty((*lead, r, r), dt)
    ffi.check(env.lib.pthip_svd_block(_dt(x), nb, r, c, 1, rows, X.ptr, S.ptr, Wt.ptr, Pt.ptr))
    env.keepalive.append(X)
    if tall:  # x^T = P S Wt  ->  x = Wt^T S P^T
        return [_tb(Wt).contiguous(), S, Pt]
    return [_tb(Pt).contiguous(), S, Wt]


def _tb(x: DeviceArray) -> DeviceArray:
    """the stack with its two core dimensions swapped (a view)"""
    return x.view((*x.shape[:-2], x.shape[-1], x.shape[-2]), (*x.strides[:-2], x.strides[-1], x.strides[-2]))


def gesvj_device(env, x: DeviceArray, job: int, rcond: float = 0.0):
    """``pthip_gesvj_batched`` on a stack (..., m, n) of the wave tier.  job 0: [S]; 1 / 2: [U, S, Vt] economic / full;
    3: [pinv].  Leading dimensions reach the kernel as one batch stride where they fold (a broadcast or strided stack
    included: nothing is copied); the dimensions that do not fold are walked here, one launch per outer index."""
    from pytensor_amd.dispatch.lu import _batch_strides, _collapse_batch

    *lead, m, n = x.shape
    lead = tuple(lead)
    k, dt = min(m, n), x.dtype
    if job == 3:
        outs = [DeviceArray.empty((*lead, n, m), dt)]
        slots = [None, None, None, outs[0]]
    else:
        S = DeviceArray.empty((*lead, k), dt)
        U = DeviceArray.empty((*lead, m, m if job == 2 else k), dt) if job else None
        Vt = DeviceArray.empty((*lead, n if job == 2 else k, n), dt) if job else None
        outs = [U, S, Vt] if job else [S]
        slots = [U, S, Vt, None]
    per = [0 if o is None else int(np.prod(o.shape[len(lead):])) * o.itemsize for o in slots]
    outer, inner, st = _collapse_batch(lead, _batch_strides(x, 2, lead))
    for f, idx in enumerate(np.ndindex(*[s for s, _ in outer])):
        off = sum(i * sts[0] for i, (_, sts) in zip(idx, outer))
        ptrs = [None if o is None else o.ptr + f * inner * p for o, p in zip(slots, per)]
        ffi.check(env.lib.pthip_gesvj_batched(_dt(x), inner, m, n, job, x.ptr + off * x.itemsize, st[0], x.strides[-2], x.strides[-1],
                                              float(rcond), *ptrs))
    return outs


def _svd_stack(env, x: DeviceArray, full_matrices: bool, compute_uv: bool):
    """``svd_device`` of a stack (..., m, n): the wave tier in one launch; above it the kernels of the single matrix,
    each launched once over the whole stack (transposed copy, svd_rows, transposed copy, geqrf, orgqr, fill_null_rows,
    a transposed copy of the result) — a launch count that does not depend on the batch."""
    *lead, m, n = x.shape
    nb = int(np.prod(lead)) if lead else 1
    k, dt = min(m, n), x.dtype
    if nb == 0 or k == 0:
        S = DeviceArray.empty((*lead, k), dt)
        if not compute_uv:
            return [S]
        um, vn = (m, n) if full_matrices else (k, k)
        # (k = 0 with full_matrices: the identities np.linalg.svd returns)
        eye = lambda s: env.to_device(HostValue(np.ascontiguousarray(np.broadcast_to(np.eye(s, dtype=dt), (*lead, s, s)))))
        U = eye(m) if (full_matrices and nb and m) else DeviceArray.empty((*lead, m, um), dt)
        Vt = eye(n) if (full_matrices and nb and n) else DeviceArray.empty((*lead, vn, n), dt)
        return [U, S, Vt]
    tier = svd_tier(m, n, nb)
    if tier == "wave":
        return gesvj_device(env, x, (2 if full_matrices else 1) if compute_uv else 0)
    if tier == "block":
        return _svd_block(env, x, full_matrices, compute_uv)
    tall = m >= n
    X = (_tb(x) if tall else x).contiguous_copy()  # (..., r, c), r <= c
    r, c = X.shape[-2:]
    S = DeviceArray.empty((*lead, r), dt)
    work = DeviceArray.empty((nb, r, r), dt) if compute_uv else DeviceArray.empty((1,), dt)
    Wt = DeviceArray.empty((*lead, r, c), dt) if compute_uv else work
    Pt = DeviceArray.empty((*lead, r, r), dt) if compute_uv else work
    ffi.check(env.lib.pthip_svd_rows(_dt(x), nb, r, c, int(compute_uv), X.ptr, work.ptr, S.ptr, Wt.ptr, Pt.ptr))
    env.keepalive.extend((X, work))
    if not compute_uv:
        return [S]
    rows = c if full_matrices else r
    qr, tau = geqrf_device(env, _tb(Wt))
    Q = orgqr_device(env, qr, tau, rows)
    if rows == r:
        big = Wt
    else:
        big = DeviceArray.empty((*lead, rows, c), dt)
        copy_into(big.view((*lead, r, c), big.strides), Wt)
    ffi.check(env.lib.pthip_fill_null_rows(_dt(x), nb, rows, c, big.ptr, S.ptr, r, Q.ptr, rows))
    env.keepalive.extend((Q, qr, tau))
    if tall:  # x^T = P S Wt  ->  x = Wt^T S P^T
        return [_tb(big).contiguous(), S, Pt]
    return [_tb(Pt).contiguous(), S, big]


def _stack_operand(env, v, what):
    from pytensor_amd.dispatch.linalg import _lapack_operands

    (x,) = _lapack_operands(env, what, v)
    if x.ndim < 2:
        raise np.linalg.LinAlgError(f"{what}: {x.ndim}-dimensional array given. Array must be at least two-dimensional")
    return x


def svd_stack_op(node, inputs, env):
    """``Blockwise(SVD)``: the whole stack in one call"""
    x = _stack_operand(env, inputs[0], "SVD")
    return svd_device(env, x, bool(node.params["full_matrices"]), bool(node.params["compute_uv"]))


def pinv_stack_op(node, inputs, env):
    """``Blockwise(MatrixPinv)``: job 3 of the wave tier in one launch; above it the batched SVD, the cut-off as one
    elementwise launch and two batched GEMMs"""
    x = _stack_operand(env, inputs[0], "MatrixPinv")
    *lead, m, n = x.shape
    nb = int(np.prod(lead)) if lead else 1
    if nb == 0 or m == 0 or n == 0:
        return [DeviceArray.empty((*lead, n, m), x.dtype)]
    if x.ndim == 2 or svd_tier(m, n, nb) != "wave":
        U, S, Vt = svd_device(env, x, False, True)
        rcond = env.to_device(HostValue(np.asarray([PINV_RCOND], dtype=x.dtype)))
        if x.ndim == 2:
            return [_pinv_apply(env, U, S, Vt, rcond)]
        return [_pinv_apply_stack(env, U, S, Vt, rcond)]
    return gesvj_device(env, x, 3, PINV_RCOND)


def _pinv_apply_stack(env, U, S, Vt, rcond_dev):
    """``_pinv_apply`` for a stack: U (..., m, k), S (..., k), Vt (..., k, n) -> (..., n, m); three launches whatever
    the batch"""
    from pytensor_amd.dispatch.blas import gemm_device
    from pytensor_amd.dispatch.elemwise import launch_elemwise

    *lead, m, k = U.shape
    n = Vt.shape[-1]
    nb = int(np.prod(lead)) if lead else 1
    dt = str(S.dtype)
    U, S, Vt = (_reshape(a, (nb, *a.shape[len(lead):])) for a in (U, S, Vt))
    body = {"in_dtypes": [dt, dt, dt], "out_dtypes": [dt],
            "body": [{"op": "Mul", "in": [["i", 1], ["i", 2]], "dtype": dt},
                     {"op": "GT", "in": [["i", 0], ["t", 0]], "dtype": "bool"},
                     {"op": "Reciprocal", "in": [["i", 0]], "dtype": dt},
                     {"op": "Switch", "in": [["t", 1], ["t", 2], ["c", 0.0, dt]], "dtype": dt}],
            "outs": [["t", 3]]}
    (sinv,), _, _ = launch_elemwise(body, [S, S.view((nb, k), (k, 0)), rcond_dev.view((nb, k), (0, 0))], (nb, k), [dt], None, env)
    scale = {"in_dtypes": [dt, dt], "out_dtypes": [dt], "body": [{"op": "Mul", "in": [["i", 0], ["i", 1]], "dtype": dt}], "outs": [["t", 0]]}
    Ut = U.view((nb, k, m), (m * k, 1, k))
    (scaled,), _, _ = launch_elemwise(scale, [Ut, sinv.view((nb, k, m), (k, 1, 0))], (nb, k, m), [dt], None, env)
    out = gemm_device(env, 1.0, Vt.view((nb, n, k), (k * n, 1, n)), scaled, batch=True)
    return out.view((*lead, n, m), _cs((*lead, n, m)))


@handler("SVD")
def svd_op(node, inputs, env):
    x = _matrix(env, inputs[0], "SVD")
    return svd_device(env, x, bool(node.params["full_matrices"]), bool(node.params["compute_uv"]))


def _pinv_apply(env, U, S, Vt, rcond_dev, rhs=None):
    """Vt^T diag(1/s where s > rcond * s_max) U^T [rhs]  (np.linalg.pinv / the minimum-norm lstsq)"""
    from pytensor_amd.dispatch.blas import gemm_device
    from pytensor_amd.dispatch.elemwise import launch_elemwise

    dt = str(S.dtype)
    k = S.shape[0]
    # sinv_i = s_i > rcond * s_0 ? 1 / s_i : 0   (s is descending: s_0 is the maximum)
    body = {"in_dtypes": [dt, dt, dt], "out_dtypes": [dt],
            "body": [{"op": "Mul", "in": [["i", 1], ["i", 2]], "dtype": dt},
                     {"op": "GT", "in": [["i", 0], ["t", 0]], "dtype": "bool"},
                     {"op": "Reciprocal", "in": [["i", 0]], "dtype": dt},
                     {"op": "Switch", "in": [["t", 1], ["t", 2], ["c", 0.0, dt]], "dtype": dt}],
            "outs": [["t", 3]]}
    s0 = S.view((k,), (0,))
    (sinv,), _, _ = launch_elemwise(body, [S, s0, rcond_dev.view((k,), (0,))], (k,), [dt], None, env)
    right = _t(U) if rhs is None else gemm_device(env, 1.0, _t(U), rhs)  # k x m  |  k x nrhs
    cols = right.shape[1]
    scale = {"in_dtypes": [dt, dt], "out_dtypes": [dt], "body": [{"op": "Mul", "in": [["i", 0], ["i", 1]], "dtype": dt}], "outs": [["t", 0]]}
    (scaled,), _, _ = launch_elemwise(scale, [right, sinv.view((k, cols), (1, 0))], (k, cols), [dt], None, env)
    return gemm_device(env, 1.0, _t(Vt), scaled)


@handler("MatrixPinv")
def matrix_pinv(node, inputs, env):
    x = _matrix(env, inputs[0], "MatrixPinv")
    m, n = x.shape
    if m == 0 or n == 0:
        return [DeviceArray.empty((n, m), x.dtype)]
    U, S, Vt = svd_device(env, x, False, True)
    rcond = env.to_device(HostValue(np.asarray([1e-15], dtype=x.dtype)))  # np.linalg.pinv's default
    return [_pinv_apply(env, U, S, Vt, rcond)]


@handler("Lstsq")
def lstsq(node, inputs, env):
    """np.linalg.lstsq(x, y, rcond) -> (solution, residuals, rank, singular values): the minimum-norm
    solution through the SVD as gelsd computes it; ``rank`` decides the shape of ``residuals`` (one
    host read, like every data-dependent shape)."""
    from pytensor_amd.dispatch.blas import gemm_device
    from pytensor_amd.dispatch.elemwise import _cast, launch_elemwise

    a = _matrix(env, inputs[0], "Lstsq")
    b = env.to_device(inputs[1])
    rc = np.asarray(env.to_host(inputs[2]))
    m, n = a.shape
    if b.shape[0] != m:
        raise np.linalg.LinAlgError("Incompatible dimensions")
    dt = np.dtype(a.dtype)
    if np.dtype(b.dtype) != dt:
        b = _cast(env, b.contiguous(), dt)
    eps = float(np.finfo(dt).eps)
    rcond = eps * max(m, n) if rc.dtype == object or rc.size == 0 else float(rc)
    if rcond <= 0 or rcond >= 1:
        rcond = eps  # LAPACK gelsd -> dlalsd: "IF( (RCOND.LE.ZERO) .OR. (RCOND.GE.ONE) ) RCND = EPS"
    b2 = b if b.ndim == 2 else b.view((m, 1), (b.strides[0], 0))
    U, S, Vt = svd_device(env, a, False, True)
    s_host = np.asarray(env.to_host(S))
    rank = int((s_host > rcond * (s_host[0] if s_host.size else 0.0)).sum())
    x = _pinv_apply(env, U, S, Vt, env.to_device(HostValue(np.asarray([rcond], dtype=dt))), rhs=b2.contiguous())
    nrhs = b2.shape[1]
    if rank == n and m > n:
        res = gemm_device(env, -1.0, a, x, 1.0, b2.contiguous())  # b - a x
        sq = {"in_dtypes": [str(dt)], "out_dtypes": [str(dt)], "body": [{"op": "Sqr", "in": [["i", 0]], "dtype": str(dt)}], "outs": [["t", 0]]}
        (r2,), _, _ = launch_elemwise(sq, [res], (m, nrhs), [str(dt)], None, env)
        resid = _column_sums(env, r2)
    else:
        resid = DeviceArray.empty((0,), dt)
    xs = x if b.ndim == 2 else x.view((n,), (x.strides[0],))
    f64 = np.dtype("float64")
    up = lambda v: v if np.dtype(v.dtype) == f64 else _cast(env, v.contiguous(), f64)  # Lstsq.make_node: d-typed outputs
    return [up(xs), up(resid), HostValue(np.asarray(rank, dtype="int32")), up(S)]


def _column_sums(env, x: DeviceArray) -> DeviceArray:
    """sum over axis 0 of a contiguous matrix, as ones^T x on the GEMM path"""
    from pytensor_amd.dispatch.blas import gemm_device

    m, n = x.shape
    ones = env.to_device(HostValue(np.ones((1, m), dtype=x.dtype)))
    return gemm_device(env, 1.0, ones, x).view((n,), (1,))


# ---- tridiagonal LU -------------------------------------------------------------------------------
def gttrf_device(env, dl, d, du):
    n = d.shape[0]
    if dl.shape[0] != max(n - 1, 0) or du.shape[0] != max(n - 1, 0):
        raise ValueError("LUFactorTridiagonal: diagonals of inconsistent lengths")
    dl, d, du = (v.contiguous_copy() for v in (dl, d, du))
    du2 = DeviceArray.empty((max(n - 2, 0),), d.dtype)
    ipiv = DeviceArray.empty((n,), "int32")
    ffi.check(env.lib.pthip_gttrf(_dt(d), 1, n, dl.ptr, d.ptr, du.ptr, du2.ptr, ipiv.ptr))
    return dl, d, du, du2, ipiv


def gttrs_device(env, dl, d, du, du2, ipiv, b, transposed):
    n = d.shape[0]
    if b.shape[0] != n:
        raise ValueError(f"SolveLUFactorTridiagonal: b has {b.shape[0]} rows, the system {n}")
    out = b.contiguous_copy()
    nrhs = out.size // n if n else 0
    ffi.check(env.lib.pthip_gttrs(_dt(d), 1, n, nrhs, int(transposed), dl.contiguous().ptr, d.contiguous().ptr, du.contiguous().ptr,
                                  du2.contiguous().ptr, ipiv.contiguous().ptr, out.ptr))
    return out


def _same_float(env, vals, what):
    from pytensor_amd.dispatch.linalg import _lapack_operands

    return _lapack_operands(env, what, *vals)


@handler("LUFactorTridiagonal")
def lu_factor_tridiagonal(node, inputs, env):
    dl, d, du = _same_float(env, inputs, "LUFactorTridiagonal")
    return list(gttrf_device(env, dl, d, du))


@handler("SolveLUFactorTridiagonal")
def solve_lu_factor_tridiagonal(node, inputs, env):
    dl, d, du, du2, b = _same_float(env, [inputs[0], inputs[1], inputs[2], inputs[3], inputs[5]], "SolveLUFactorTridiagonal")
    ipiv = env.to_device(inputs[4])
    if str(ipiv.dtype) != "int32":
        from pytensor_amd.dispatch.elemwise import _cast

        ipiv = _cast(env, ipiv.contiguous(), "int32")
    return [gttrs_device(env, dl, d, du, du2, ipiv, b, bool(node.params["transposed"]))]


def solve_tridiagonal(env, A: DeviceArray, b: DeviceArray, b_ndim: int) -> DeviceArray:
    """``Solve(assume_a="tridiagonal")`` (scipy.linalg.solve -> gttrf + gttrs on the three diagonals
    of ``A``; everything else in ``A`` is ignored, as scipy ignores it)"""
    n = A.shape[-1]
    if A.ndim != 2 or b.ndim != b_ndim:
        # batched (Blockwise; reference tests/tensor/rewriting/linalg/test_solvers.py): the (small) batch on the host, like
        # dispatch/lu.solve_general — each item is a factorisation and a solve launch
        from pytensor_amd.device import contiguous_strides, copy_into
        from pytensor_amd.dispatch.lu import _batchify

        bshape = tuple(np.broadcast_shapes(A.shape[:-2], b.shape[: b.ndim - b_ndim]))
        core_b = b.shape[b.ndim - b_ndim:]
        Ab, bbm = _batchify(A, 2, bshape), _batchify(b, b_ndim, bshape)
        out = DeviceArray.empty((*bshape, *core_b), b.dtype)
        step = int(np.prod(core_b)) if core_b else 1
        for k in range(Ab.shape[0]):
            xk = solve_tridiagonal(env, Ab.view((n, n), (n, 1), k * n * n), bbm.view(core_b, contiguous_strides(core_b), k * step), b_ndim)
            copy_into(out.view(core_b, contiguous_strides(core_b), k * step), xk)
        return out
    diag = lambda off: A.view((max(n - abs(off), 0),), (A.strides[0] + A.strides[1],), (-off) * A.strides[0] if off < 0 else off * A.strides[1])
    f = gttrf_device(env, diag(-1), diag(0), diag(1))
    return gttrs_device(env, *f, b, False)


# ---- composed from existing device ops ----------------------------------------------------------------
@handler("Eigvalsh")
def eigvalsh(node, inputs, env):
    from pytensor_amd.dispatch.lu import eigh

    ins = [i for i in inputs if not (isinstance(i, HostValue) and i.a.dtype == object)]
    fake = type("_N", (), {"params": {"lower": bool(node.params["lower"])}})
    return [eigh(fake, ins, env)[0]]


@handler("TensorInv")
def tensor_inv(node, inputs, env):
    from pytensor_amd.dispatch.lu import matrix_inverse

    a = env.to_device(inputs[0])
    ind = int(node.params["ind"])
    if ind <= 0:
        raise ValueError("Invalid ind argument.")
    old = tuple(a.shape)
    inv_shape = old[ind:] + old[:ind]
    prod = int(np.prod(old[ind:])) if old[ind:] else 1
    a2 = _reshape(a, (prod, a.size // prod if prod else 0))
    if a2.shape[0] != a2.shape[1]:
        raise np.linalg.LinAlgError("Last 2 dimensions of the array must be square")
    fake = type("_N", (), {"params": {}})
    (ia,) = matrix_inverse(fake, [a2], env)
    return [_reshape(ia, inv_shape)]


@handler("TensorSolve")
def tensor_solve(node, inputs, env):
    from pytensor_amd.dispatch.lu import solve_general

    a, b = _same_float(env, inputs, "TensorSolve")
    axes = node.params.get("axes")
    an = a.ndim
    if axes is not None:
        order = list(range(an))
        for k in axes:
            order.remove(k)
            order.insert(an, k)
        a = a.view([a.shape[d] for d in order], [a.strides[d] for d in order])
    old = tuple(a.shape[-(an - b.ndim):]) if an > b.ndim else ()
    prod = int(np.prod(old)) if old else 1
    if a.size != prod * prod:
        raise np.linalg.LinAlgError("Input arrays must satisfy the requirement prod(a.shape[b.ndim:]) == prod(a.shape[:b.ndim])")
    x = solve_general(env, _reshape(a, (prod, prod)), _reshape(b, (prod,)), 1)
    return [_reshape(x, old)]


@handler("BlockDiagonal")
def block_diagonal(node, inputs, env):
    from pytensor_amd.dispatch.elemwise import _cast

    out_dt = np.dtype(node.params["dtype"])
    mats = [env.to_device(i) for i in inputs]
    rows = sum(m.shape[0] for m in mats)
    cols = sum(m.shape[1] for m in mats)
    out = DeviceArray.empty((rows, cols), out_dt)
    if out.size:
        ffi.check(env.lib.pthip_memset(out.ptr, 0, out.nbytes))
    r0 = c0 = 0
    for m in mats:
        if m.size:
            src = m if np.dtype(m.dtype) == out_dt else _cast(env, m.contiguous(), out_dt)
            copy_into(out.view(m.shape, (cols, 1), r0 * cols + c0), src)
        r0 += m.shape[0]
        c0 += m.shape[1]
    return [out]


# ---- matrix exponential ---------------------------------------------------------------------------
_PADE13 = (64764752532480000.0, 32382376266240000.0, 7771770303897600.0, 1187353796428800.0, 129060195264000.0, 10559470521600.0,
           670442572800.0, 33522128640.0, 1323241920.0, 40840800.0, 960960.0, 16380.0, 182.0, 1.0)
_THETA13 = 5.371920351148152  # Higham (2005), Table 2.3: ||A||_1 up to which the [13/13] Pade approximant is exact to fp64


@handler("Expm")
def expm(node, inputs, env):
    """``Expm`` (linalg/products.py:13; perform = scipy.linalg.expm): scaling and squaring with the
    [13/13] Pade approximant (Higham 2005, the algorithm scipy's expm descends from) out of device
    GEMMs, fused linear combinations and one LU solve.  The scaling power is chosen from ||A||_1 (one
    host read of n column sums).  scipy additionally picks lower Pade orders for small norms; both are
    backward stable to unit roundoff."""
    from pytensor_amd.dispatch.blas import gemm_device
    from pytensor_amd.dispatch.lu import solve_general

    A = _matrix(env, inputs[0], "Expm")
    n = A.shape[0]
    if A.shape[1] != n:
        raise ValueError("expected a square matrix")
    if n == 0:
        return [DeviceArray.empty((0, 0), A.dtype)]
    dt = str(A.dtype)
    A = A.contiguous()
    absA = _ew1(env, [{"op": "Abs", "in": [["i", 0]], "dtype": dt}], [A], [dt], dt, (n, n))
    norm1 = float(np.asarray(env.to_host(_column_sums(env, absA))).max())
    if not np.isfinite(norm1):
        return [env.to_device(HostValue(np.full((n, n), np.nan, dtype=A.dtype)))]
    s = max(0, int(np.ceil(np.log2(norm1 / _THETA13)))) if norm1 > _THETA13 else 0
    if s:
        A = _ew1(env, [{"op": "Mul", "in": [["i", 0], ["c", float(2.0 ** -s).hex(), dt]], "dtype": dt}], [A], [dt], dt, (n, n))
    eye = DeviceArray.empty((n, n), A.dtype)
    ffi.check(env.lib.pthip_eye(ffi.np_dtype_code(A.dtype), n, n, 0, eye.ptr))
    b = _PADE13
    A2 = gemm_device(env, 1.0, A, A)
    A4 = gemm_device(env, 1.0, A2, A2)
    A6 = gemm_device(env, 1.0, A4, A2)

    def comb(coefs, mats):
        ops, acc = [], None
        for k, c in enumerate(coefs):
            ops.append({"op": "Mul", "in": [["i", k], ["c", float(c).hex(), dt]], "dtype": dt})
            if acc is not None:
                ops.append({"op": "Add", "in": [acc, ["t", len(ops) - 1]], "dtype": dt})
            acc = ["t", len(ops) - 1]
        return _ew1(env, ops, mats, [dt] * len(mats), dt, (n, n))

    W1 = comb((b[13], b[11], b[9]), [A6, A4, A2])
    W2 = comb((b[7], b[5], b[3], b[1]), [A6, A4, A2, eye])
    Z1 = comb((b[12], b[10], b[8]), [A6, A4, A2])
    Z2 = comb((b[6], b[4], b[2], b[0]), [A6, A4, A2, eye])
    W = gemm_device(env, 1.0, A6, W1, 1.0, W2)  # A6 W1 + W2
    U = gemm_device(env, 1.0, A, W)
    V = gemm_device(env, 1.0, A6, Z1, 1.0, Z2)
    P = comb((1.0, 1.0), [V, U])
    Q = comb((1.0, -1.0), [V, U])
    X = solve_general(env, Q, P, 2)
    for _ in range(s):
        X = gemm_device(env, 1.0, X, X)
    return [X]


def _ew1(env, body_ops, ins, in_dtypes, out_dtype, shape):
    from pytensor_amd.dispatch.elemwise import launch_elemwise

    body = {"in_dtypes": list(in_dtypes), "out_dtypes": [out_dtype], "body": body_ops, "outs": [["t", len(body_ops) - 1]]}
    (out,), _, _ = launch_elemwise(body, ins, tuple(shape), [out_dtype], None, env)
    return out


# ---- Sylvester equation -----------------------------------------------------------------------------
MAX_SYLVESTER = 4096  # m * n: the Kronecker system is (m n) x (m n)
MAX_SYLVESTER_SCHUR = 1024  # m and n of the Bartels-Stewart tier (csrc/sylvester.hip SYL_MAX_N)


def sylvester_tier(m: int, n: int):
    """The tier that solves an m x n Sylvester equation: "kronecker" up to m n = 4096, "schur" (Bartels-Stewart)
    above that up to m, n <= 1024, None (refused) beyond."""
    if m * n <= MAX_SYLVESTER:
        return "kronecker"
    if max(m, n) <= MAX_SYLVESTER_SCHUR:
        return "schur"
    return None


def _sylvester_refused(m, n):
    return NotImplementedError(f"hip linker: SolveSylvester with m = {m}, n = {n} (device tiers: m*n <= {MAX_SYLVESTER} "
                               f"Kronecker, m, n <= {MAX_SYLVESTER_SCHUR} Bartels-Stewart)")


def solve_sylvester_schur(env, A, B, C, b_is_a_t=False, out_dtype=None):
    """X (*batch, m, n) with A X + X B = C for operands with broadcastable leading batch dims, by Bartels-Stewart
    (csrc/sylvester.hip): real Schur forms A = U R U^T, B = V S V^T in one launch (one workgroup per form), F = U^T C V
    on the GEMM, R Y + Y S = F in a second launch, X = U Y V^T on the GEMM; fp64 throughout, X in ``out_dtype``
    (default: the operands' working type).  ``b_is_a_t``: B = A^T, so only A is factored and R Y + Y R^T = U^T C U
    is solved.  An item whose A or B holds a non-finite value, or whose QR iteration reached its cap, is all NaN.
    No host read."""
    from pytensor_amd.dispatch.blas import gemm_device
    from pytensor_amd.dispatch.elemwise import _cast
    from pytensor_amd.dispatch.linalg import _batchify, _lapack_operands

    A, B, C = _lapack_operands(env, "SolveSylvester", A, B, C)
    m, n = A.shape[-1], B.shape[-1]
    if A.shape[-2:] != (m, m) or B.shape[-2:] != (n, n) or C.shape[-2:] != (m, n):
        raise ValueError(f"SolveSylvester: incompatible shapes {A.shape}, {B.shape}, {C.shape}")
    if b_is_a_t and m != n:
        raise ValueError(f"SolveSylvester: B = A^T needs square operands of one size, got m = {m}, n = {n}")
    bshape = tuple(np.broadcast_shapes(A.shape[:-2], B.shape[:-2], C.shape[:-2]))
    nb = int(np.prod(bshape)) if bshape else 1
    out = DeviceArray.empty((*bshape, m, n), out_dtype or A.dtype)
    if nb == 0 or m * n == 0:
        return out
    if max(m, n) > MAX_SYLVESTER_SCHUR:
        raise _sylvester_refused(m, n)
    f64 = "float64"
    Ab = _batchify(A, 2, bshape)
    Bb = None if b_is_a_t else _batchify(B, 2, bshape)
    Cb = _batchify(C, 2, bshape)
    if str(Cb.dtype) != f64:
        Cb = _cast(env, Cb, f64)
    ws_bytes = int(env.lib.pthip_sylvester_workspace(nb, m, n, int(b_is_a_t)))
    ws = DeviceArray.empty(((ws_bytes + 7) // 8,), f64)
    env.timed(f"real_schur_{A.dtype}_{m}x{n}_b{nb}", lambda: ffi.check(env.lib.pthip_real_schur(
        _dt(Ab), nb, m, n, int(b_is_a_t), Ab.ptr, None if Bb is None else Bb.ptr, ws.ptr, ws_bytes)))
    # the orthogonal factors, stored transposed (csrc/schur_device.h): U(i, j) = Zt[j, i]; workspace layout in pthip.h
    U = ws.view((nb, m, m), (2 * m * m, 1, m), m * m)
    V = U if b_is_a_t else ws.view((nb, n, n), (2 * n * n, 1, n), 2 * nb * m * m + n * n)
    tr = lambda x: x.view(x.shape, (x.strides[0], x.strides[2], x.strides[1]), 0)
    F = gemm_device(env, 1.0, gemm_device(env, 1.0, tr(U), Cb, batch=True), V, batch=True)  # U^T C V
    env.timed(f"trsyl_{m}x{n}_b{nb}", lambda: ffi.check(env.lib.pthip_trsyl(nb, m, n, int(b_is_a_t), F.ptr, ws.ptr, ws_bytes)))
    X = gemm_device(env, 1.0, gemm_device(env, 1.0, U, F, batch=True), tr(V), batch=True)  # U Y V^T
    env.keepalive.extend((ws, F, Ab, Cb) + (() if Bb is None else (Bb,)))
    if np.dtype(out.dtype) != np.dtype(f64):
        X = _cast(env, X, out.dtype)
    return X.view(out.shape, contiguous_strides(out.shape))


@handler("SolveSylvester")
def solve_sylvester(node, inputs, env):
    """``A X + X B = C`` (linalg/solvers/linear_control.py:117 ``SolveSylvester``; the reference builds
    it from real Schur forms and LAPACK ``trsyl``).  Two tiers (DESIGN §4 "Sylvester / Lyapunov"):

    - m n <= 4096: the linear system it is, (A (x) I_n + I_m (x) B^T) vec(X) = vec(C) with row-major vec,
      assembled by one generated kernel and handed to the LU solver — O((m n)^3);
    - m, n <= 1024 above that: Bartels-Stewart (``solve_sylvester_schur``), O(m^3 + n^3), with one Schur form
      when B = A^T (the ``b_is_a_t`` param of the lowering).

    Both give the unique solution whenever the spectra of A and -B are disjoint."""
    from pytensor_amd.dispatch.lu import solve_general
    from pytensor_amd.dispatch.riccati import out_dtype

    A, B, Cm = _same_float(env, inputs, "SolveSylvester")
    m, n = A.shape[0], B.shape[0]
    if A.shape != (m, m) or B.shape != (n, n) or Cm.shape != (m, n):
        raise ValueError(f"SolveSylvester: incompatible shapes {A.shape}, {B.shape}, {Cm.shape}")
    if m * n == 0:
        return [DeviceArray.empty((m, n), A.dtype)]
    tier = sylvester_tier(m, n)
    if tier is None:
        raise _sylvester_refused(m, n)
    if tier == "schur":
        return [solve_sylvester_schur(env, A, B, Cm, bool(node.params.get("b_is_a_t", False)), out_dtype(env, node))]
    dt = str(A.dtype)
    eye = lambda k: env.to_device(HostValue(np.eye(k, dtype=A.dtype)))
    Im, In = eye(m), eye(n)
    shape = (m, n, m, n)  # K[(i, j), (k, l)] = A[i, k] d_jl + d_ik B[l, j]
    ops = [{"op": "Mul", "in": [["i", 0], ["i", 1]], "dtype": dt}, {"op": "Mul", "in": [["i", 2], ["i", 3]], "dtype": dt},
           {"op": "Add", "in": [["t", 0], ["t", 1]], "dtype": dt}]
    K = _ew1(env, ops, [A.view(shape, (A.strides[0], 0, A.strides[1], 0)), In.view(shape, (0, In.strides[0], 0, In.strides[1])),
                        Im.view(shape, (Im.strides[0], 0, Im.strides[1], 0)), B.view(shape, (0, B.strides[1], 0, B.strides[0]))],
             [dt] * 4, dt, shape)
    mn = m * n
    x = solve_general(env, K.view((mn, mn), (mn, 1)), _reshape(Cm, (mn,)), 1)
    return [x.view((m, n), (n, 1))]
