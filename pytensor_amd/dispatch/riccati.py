"""``SolveDiscreteARE`` and its ``Blockwise`` batch: the stabilising solution of the discrete algebraic
Riccati equation A^T X A - X - A^T X B (R + B^T X B)^-1 B^T X A + Q = 0.

Reference: linalg/solvers/linear_control.py ``SolveDiscreteARE`` (an OpFromGraph over the QR-compressed
extended pencil and ``QZ(sort="iuc")``, symmetrised, NaN when U00^T U10 is not symmetric) and its pullback
``_lop_solve_discrete_are``, which is built from ops that lower already.  Here X is computed by the
structure-preserving doubling algorithm (csrc/riccati.hip, DESIGN §4 "Riccati"):

- m <= 64 and n <= m (n = 0, no input, is the Stein equation X = A^T X A + Q): one launch for the whole batch, one workgroup per item, the iteration in fp64
  on the device (``pthip_dare``);
- m <= 1024: the composed tier, ``COMPOSED_STEPS`` doubling steps out of the device GEMM and LU solve,
  then ``pthip_dare_finish`` applies the convergence test on the device.  No host read, so a graph that
  holds it still freezes into a replayable plan.  A batch loops its items.

Failure (no convergence within the cap, a non-finite value, a zero pivot in R or W) is an all-NaN X.
"""

from __future__ import annotations

import numpy as np

from pytensor_amd import ffi
from pytensor_amd.device import DeviceArray, contiguous_strides, copy_into
from pytensor_amd.dispatch import handler
from pytensor_amd.dispatch.linalg import _batchify, _lapack_operands

MAX_SINGLE_LAUNCH = 64  # m of the one-kernel tier (csrc/riccati.hip DARE_MAX_M)
MAX_DARE = 1024  # m of the composed tier
COMPOSED_STEPS = 48  # = DARE_MAX_STEPS of the one-kernel tier


def _check_shapes(A, B, Q, R):
    m, n = B.shape[-2], B.shape[-1]
    if A.shape[-2:] != (m, m) or Q.shape[-2:] != (m, m) or R.shape[-2:] != (n, n):
        raise ValueError(f"SolveDiscreteARE: incompatible shapes {A.shape}, {B.shape}, {Q.shape}, {R.shape} "
                         "(expected (m, m), (m, n), (m, m), (n, n))")
    return m, n


def dare_device(env, A, B, Q, R, out_dtype=None, with_steps=False):
    """X (*batch, m, m) for operands with broadcastable leading batch dims, in ``out_dtype`` (default: their
    LAPACK working type; the reference's graph gives float64 for float32 operands).  ``with_steps``: also the
    int32 (*batch,) doubling step counts of the one-kernel tier (-1 where it failed; None from the
    composed tier)."""
    A, B, Q, R = _lapack_operands(env, "SolveDiscreteARE", A, B, Q, R)
    m, n = _check_shapes(A, B, Q, R)
    bshape = tuple(np.broadcast_shapes(A.shape[:-2], B.shape[:-2], Q.shape[:-2], R.shape[:-2]))
    nb = int(np.prod(bshape)) if bshape else 1
    out_shape = (*bshape, m, m)
    out = DeviceArray.empty(out_shape, out_dtype or A.dtype)
    if m == 0 or nb == 0:
        return (out, None) if with_steps else out
    if m > MAX_DARE:
        raise NotImplementedError(f"hip linker: SolveDiscreteARE with m = {m} (device tiers up to m = {MAX_DARE})")
    Ab, Bb, Qb, Rb = (_batchify(x, 2, bshape) for x in (A, B, Q, R))
    ob = out.view((nb, m, m), contiguous_strides((nb, m, m)))
    steps = None
    if m <= MAX_SINGLE_LAUNCH and n <= m:
        ws_bytes = int(env.lib.pthip_dare_workspace(nb, m, n))
        ws = DeviceArray.empty((ws_bytes,), "uint8") if ws_bytes else None
        steps = DeviceArray.empty((nb,), "int32")
        env.timed(f"dare_{A.dtype}_{m}x{n}_b{nb}", lambda: ffi.check(env.lib.pthip_dare(
            ffi.np_dtype_code(A.dtype), ffi.np_dtype_code(out.dtype), nb, m, n, Ab.ptr, Bb.ptr, Qb.ptr, Rb.ptr, ob.ptr, steps.ptr,
            ws.ptr if ws is not None else None, ws_bytes)))
    else:
        for k in range(nb):
            item = lambda x, r, c: x.view((r, c), (c, 1), k * r * c)
            _dare_composed(env, item(Ab, m, m), item(Bb, m, n), item(Qb, m, m), item(Rb, n, n), item(ob, m, m))
    steps = steps.view(bshape, contiguous_strides(bshape)) if steps is not None else None
    return (out, steps) if with_steps else out


def _dare_composed(env, A, B, Q, R, X):
    """One DARE (m > 64 or n > m) into X from device GEMMs, LU solves and one fused add per step, in fp64.
    A fixed ``COMPOSED_STEPS`` steps: once converged Ak underflows to 0 and further steps leave G and H
    unchanged, so no host read decides when to stop."""
    from pytensor_amd.dispatch.blas import gemm_device
    from pytensor_amd.dispatch.decomp import _ew1, _t
    from pytensor_amd.dispatch.elemwise import _cast
    from pytensor_amd.dispatch.lu import solve_general

    f64 = "float64"
    A, B, Q, R = (x if str(x.dtype) == f64 else _cast(env, x, f64) for x in (A, B, Q, R))
    m, n = B.shape
    eye = DeviceArray.empty((m, m), f64)
    ffi.check(env.lib.pthip_eye(ffi.np_dtype_code(f64), m, m, 0, eye.ptr))
    flag = DeviceArray.empty((1,), "int32")  # (a non-finite R or W: the LU kernels never see it, X is NaN)
    if n:
        R = R.contiguous_copy()
        ffi.check(env.lib.pthip_dare_guard(n, R.ptr, flag.ptr, 1))
        Z = solve_general(env, R, _t(B).contiguous_copy(), 2)  # R^-1 B^T
        G = gemm_device(env, 1.0, B, Z)
    else:  # (no input: G0 = 0, the Stein equation X = A^T X A + Q)
        G = DeviceArray.empty((m, m), f64)
        ffi.check(env.lib.pthip_eye(ffi.np_dtype_code(f64), m, m, m, G.ptr))  # (the diagonal m places up: all zero)
        ffi.check(env.lib.pthip_dare_guard(m, G.ptr, flag.ptr, 1))  # (finite: only clears the flag)
    H, Ak = Q, A
    add = [{"op": "Add", "in": [["i", 0], ["i", 1]], "dtype": f64}]
    rhs = DeviceArray.empty((m, 2 * m), f64)
    left, right = rhs.view((m, m), (2 * m, 1)), rhs.view((m, m), (2 * m, 1), m)
    dH = None
    for _ in range(COMPOSED_STEPS):
        W = gemm_device(env, 1.0, G, H, 1.0, eye)  # I + G H
        ffi.check(env.lib.pthip_dare_guard(m, W.ptr, flag.ptr, 0))
        copy_into(left, Ak)
        copy_into(right, G)
        Y = solve_general(env, W, rhs, 2)  # [W^-1 A | W^-1 G]
        Y1 = Y.view((m, m), Y.strides)
        Y2 = Y.view((m, m), Y.strides, m * Y.strides[1])
        T = gemm_device(env, 1.0, Ak, Y2)
        G = gemm_device(env, 1.0, T, _t(Ak), 1.0, G)  # G + A W^-1 G A^T
        S = gemm_device(env, 1.0, H, Y1)
        dH = gemm_device(env, 1.0, _t(Ak), S)  # A^T H W^-1 A
        H = _ew1(env, add, [H, dH], [f64, f64], f64, (m, m))
        Ak = gemm_device(env, 1.0, Ak, Y1)  # A W^-1 A
    ffi.check(env.lib.pthip_dare_finish(ffi.np_dtype_code(X.dtype), m, H.ptr, dH.ptr, A.contiguous().ptr, Ak.ptr, flag.ptr, X.ptr))


@handler("SolveDiscreteARE")
def solve_discrete_are(node, inputs, env):
    A, B, Q, R = (env.to_device(i) for i in inputs)
    for x, what in ((A, "A"), (B, "B"), (Q, "Q"), (R, "R")):
        if x.ndim != 2:
            raise ValueError(f"SolveDiscreteARE: {what} must be a matrix, got {x.ndim} dimensions")
    return [dare_device(env, A, B, Q, R, out_dtype(env, node))]


def out_dtype(env, node):
    v = node.outputs[0]
    return str(env.graph.vars[v].dtype) if v in env.graph.vars else None
