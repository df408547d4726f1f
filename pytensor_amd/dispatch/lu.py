"""General dense solves on LU with partial pivoting: ``Solve`` (gen / pos / banded), ``Det``, ``SLogDet``,
``MatrixInverse`` and their ``Blockwise`` batching.

Reference: pytensor/tensor/linalg/solvers/general.py:17 ``Solve`` (perform 62-75:
``scipy.linalg.solve``; a singular system NaN-fills), linalg/summary.py:34 ``Det`` /
84 ``SLogDet`` (``np.linalg.det`` / ``slogdet``), linalg/inverse.py:87 ``MatrixInverse``
(``np.linalg.inv``: LinAlgError when singular).  SURVEY §8f row 3.
"""

from __future__ import annotations

import numpy as np

from pytensor_amd import ffi
from pytensor_amd.device import DeviceArray, contiguous_strides
from pytensor_amd.dispatch import handler
from pytensor_amd.dispatch.linalg import _batchify, _dt, _require_float, cho_solve_device, cholesky_device, trsm_device


def getrf_device(env, a: DeviceArray, flag_singular=False):
    """(LU, perm, sign, logabsdet) of a (..., n, n) array; batch dims flattened."""
    from pytensor_amd.dispatch.linalg import _lapack_operands

    (a,) = _lapack_operands(env, "LU", a)
    n = a.shape[-1]
    if a.shape[-2] != n:
        raise ValueError("expected a square matrix")
    bshape = a.shape[:-2]
    ab = _batchify(a, 2, bshape)
    nb = ab.shape[0]
    LU = DeviceArray.empty((nb, n, n), a.dtype)
    perm = DeviceArray.empty((nb, n), "int64")
    sign = DeviceArray.empty((nb,), a.dtype)
    logabs = DeviceArray.empty((nb,), a.dtype)
    if nb and n:
        ffi.check(env.lib.pthip_getrf(_dt(a), nb, n, ab.ptr, LU.ptr, perm.ptr, sign.ptr, logabs.ptr, int(flag_singular)))
    elif nb:  # 0 x 0: det = 1
        from pytensor_amd.executor import HostValue

        sign = env.to_device(HostValue(np.ones((nb,), dtype=a.dtype)))
        logabs = env.to_device(HostValue(np.zeros((nb,), dtype=a.dtype)))
    return LU, perm, sign, logabs, bshape


def _permute_rows(env, b: DeviceArray, perm: DeviceArray) -> DeviceArray:
    """b[perm] along axis 0 of a contiguous (n, nrhs) / (n,) array (P applied to the rhs)."""
    bc = b.contiguous()
    inner = int(np.prod(bc.shape[1:])) if bc.ndim > 1 else 1
    out = DeviceArray.empty(bc.shape, bc.dtype)
    if out.size:
        ffi.check(env.lib.pthip_take_rows(bc.itemsize, perm.size, inner, bc.ptr, bc.shape[0], inner, perm.ptr, out.ptr))
    return out


WAVE_MAX_N = 64  # csrc/lu_batched.hip: one lane per row, the row in registers


def solve_tier(n: int, nb: int) -> str:
    """How a general solve / inverse of ``nb`` systems of order ``n`` runs:

    ``"wave"``      n <= 64, any ``nb`` (the unbatched solve of a Scan step included): one launch of
                    ``pthip_gesv_batched`` factors, permutes and substitutes for the whole batch.
    ``"composed"``  n > 64, two items or more: ``pthip_getrf`` with ``batch = nb``, one batched row gather
                    (``pthip_laswp_batched``) and two batched ``pthip_trsm`` — four calls whatever ``nb`` is.  Up
                    to the one-workgroup LDS bound of getrf (n <= ~140 fp64 / ~200 fp32) those are four launches;
                    beyond it ``getrf_typed`` walks the matrices inside the call (the blocked factorisation keeps
                    the whole device busy with one matrix), and that stays.
    ``"loop"``      n > 64 and at most one item: nothing to batch, the per-item sequence."""
    if n <= WAVE_MAX_N:
        return "wave"
    return "composed" if nb >= 2 else "loop"


def _batch_strides(x: DeviceArray, core_ndim: int, bshape):
    """Element strides of ``x``'s leading dims broadcast to ``bshape`` (0 along a broadcast dim)."""
    lead = x.shape[: x.ndim - core_ndim]
    pad = len(bshape) - len(lead)
    return (0,) * pad + tuple(0 if s == 1 else st for s, st in zip(lead, x.strides[: len(lead)]))


def _collapse_batch(bshape, *stride_sets):
    """Fold the batch dims, innermost first, into one count with ONE stride per operand — what a kernel that takes
    a batch stride can walk by itself.  Returns (outer, inner, strides): ``outer`` lists the (size, stride per
    operand) of the leading dims that do not fold (the caller loops them), ``inner`` the folded count."""
    dims = [(s, [ss[d] for ss in stride_sets]) for d, s in enumerate(bshape) if s != 1]
    inner, st = 1, [0] * len(stride_sets)
    while dims:
        s, sts = dims[-1]
        if inner > 1 and any(a != b * inner for a, b in zip(sts, st)):
            break
        if inner == 1:
            st = list(sts)
        inner *= s
        dims.pop()
    return dims, inner, st


def _gesv_wave(env, A: DeviceArray, b, b_ndim: int, out: DeviceArray, bshape, flag_singular: bool):
    """``out`` (contiguous, (*bshape, *core)) = A^-1 b (``b`` None: the inverse) through pthip_gesv_batched.
    Broadcast and strided batch dims go to the kernel as strides; dims that do not fold into one stride (``A``
    (5,1,n,n) against ``b`` (1,7,n,k)) are walked here, one launch per outer index, and nothing is copied."""
    n = A.shape[-1]
    nrhs = n if b is None else (1 if b_ndim == 1 else b.shape[-1])
    sets = [_batch_strides(A, 2, bshape)]
    if b is not None:
        core_b = b.shape[b.ndim - b_ndim :]
        # (the stride of a core dim of length 1 is never read: it forces no copy)
        if any(s != 1 and st != c for s, st, c in zip(core_b, b.strides[b.ndim - b_ndim :], contiguous_strides(core_b))):
            b = b.contiguous()
        sets.append(_batch_strides(b, b_ndim, bshape))
    outer, inner, st = _collapse_batch(bshape, *sets)
    isz, per = A.itemsize, n * nrhs
    for f, idx in enumerate(np.ndindex(*[s for s, _ in outer])):
        offs = [sum(i * sts[k] for i, (_, sts) in zip(idx, outer)) for k in range(len(sets))]
        ffi.check(env.lib.pthip_gesv_batched(
            _dt(A), inner, n, nrhs, A.ptr + offs[0] * isz, st[0], A.strides[-2], A.strides[-1],
            None if b is None else b.ptr + offs[1] * isz, 0 if b is None else st[1], out.ptr + f * inner * per * isz,
            int(flag_singular)))


def _solve_composed(env, A: DeviceArray, b, b_ndim: int, out: DeviceArray, bshape, flag_singular: bool):
    """The composed tier: batched getrf, one batched row gather, two batched triangular solves.  A matrix shared
    by the whole batch is factored once and handed on with a batch stride of 0."""
    n = A.shape[-1]
    nb = int(np.prod(bshape))
    nrhs = n if b is None else (1 if b_ndim == 1 else b.shape[-1])
    shared = int(np.prod(A.shape[:-2])) == 1
    LU, perm, _, _, _ = getrf_device(env, A.view((n, n), A.strides[-2:]) if shared else _batchify(A, 2, bshape).view((nb, n, n), (n * n, n, 1)),
                                     flag_singular=flag_singular)
    sTb = 0 if shared else n * n
    bptr, sBb = None, 0
    if b is not None:
        if int(np.prod(b.shape[: b.ndim - b_ndim])) == 1:
            bm = b.contiguous()
        else:
            bm, sBb = _batchify(b, b_ndim, bshape), n * nrhs
        bptr = bm.ptr
    pb = DeviceArray.empty((nb, n, nrhs), A.dtype)
    y = DeviceArray.empty((nb, n, nrhs), A.dtype)
    ffi.check(env.lib.pthip_laswp_batched(_dt(A), nb, n, nrhs, bptr, sBb, perm.ptr, 0 if shared else n, pb.ptr))
    ffi.check(env.lib.pthip_trsm(_dt(A), 1, 0, 1, nb, n, nrhs, LU.ptr, sTb, n, 1, pb.ptr, n * nrhs, y.ptr))
    ffi.check(env.lib.pthip_trsm(_dt(A), 0, 0, 0, nb, n, nrhs, LU.ptr, sTb, n, 1, y.ptr, n * nrhs, out.ptr))


def solve_general(env, A: DeviceArray, b: DeviceArray, b_ndim: int) -> DeviceArray:
    """x = A^-1 b through P A = L U, by the tier ``solve_tier`` names.  A singular U has a zero pivot, which every
    tier turns into the reference's NaN fill of that item."""
    n = A.shape[-1]
    if A.shape[-2] != n:
        raise ValueError("Solve: expected a square matrix")
    if b.shape[b.ndim - b_ndim] != n:
        raise ValueError(f"Solve: incompatible shapes {A.shape} and {b.shape}")
    if str(b.dtype) != str(A.dtype):
        raise TypeError("Solve: dtype mismatch")
    bA, bb = A.shape[:-2], b.shape[: b.ndim - b_ndim]
    bshape = tuple(np.broadcast_shapes(bA, bb))
    core_b = b.shape[b.ndim - b_ndim :]
    nb = int(np.prod(bshape)) if bshape else 1
    tier = solve_tier(n, nb)
    if tier != "loop":
        out = DeviceArray.empty((*bshape, *core_b), b.dtype)
        if out.size:
            (_gesv_wave if tier == "wave" else _solve_composed)(env, A, b, b_ndim, out, bshape, False)
        return out
    if A.ndim == 2 and b.ndim == b_ndim:
        LU, perm, _, _, _ = getrf_device(env, A)
        lu = LU.view((n, n), (n, 1))
        pb = _permute_rows(env, b, perm.view((n,), (1,)))
        y = trsm_device(env, lu, pb, True, True, b_ndim)
        return trsm_device(env, lu, y, False, False, b_ndim)
    # (at most one item behind leading dims of length 1 — or none at all)
    Ab = _batchify(A, 2, bshape)
    bbm = _batchify(b, b_ndim, bshape)
    out = DeviceArray.empty((*bshape, *core_b), b.dtype)
    step = int(np.prod(core_b)) if core_b else 1
    for k in range(Ab.shape[0]):
        Ak = Ab.view((n, n), (n, 1), k * n * n)
        bk = bbm.view(core_b, contiguous_strides(core_b), k * step)
        xk = solve_general(env, Ak, bk, b_ndim)
        from pytensor_amd.device import copy_into

        copy_into(out.view(core_b, contiguous_strides(core_b), k * step), xk)
    return out


def banded_tier(n: int, nb: int) -> str:
    """How ``Solve(assume_a="banded")`` of ``nb`` systems of order ``n`` runs, from the shapes alone (the bandwidths
    are data and never reach the host):

    ``"wave"``  n <= 64: the one-launch dense tier of ``solve_tier`` — one launch and the same n^2 read as a band
                scan; partial pivoting on the dense rows picks gbsv's pivots (what lies outside the band is zero).
    ``"band"``  n > 64, any ``nb``: ``pthip_band_scan`` then ``pthip_gbsv_batched`` (csrc/gbsv.hip), two launches."""
    return "wave" if n <= WAVE_MAX_N else "band"


def _gbsv(env, A: DeviceArray, b: DeviceArray, b_ndim: int, out: DeviceArray, bshape):
    """``out`` (contiguous, (*bshape, *core)) = A^-1 b through the band kernels.  The batch dims go to the kernels
    as strides, as in ``_gesv_wave``: nothing is copied, a matrix shared by the batch (stride 0) is scanned once, and
    dims that do not fold into one stride are walked here."""
    n = A.shape[-1]
    nrhs = 1 if b_ndim == 1 else b.shape[-1]
    core_b = b.shape[b.ndim - b_ndim :]
    if any(s != 1 and st != c for s, st, c in zip(core_b, b.strides[b.ndim - b_ndim :], contiguous_strides(core_b))):
        b = b.contiguous()
    outer, inner, st = _collapse_batch(bshape, _batch_strides(A, 2, bshape), _batch_strides(b, b_ndim, bshape))
    isz, per = A.itemsize, n * nrhs
    scanned = 1 if st[0] == 0 else inner
    band = DeviceArray.empty((scanned, 2), "int32")
    # a band that does not fit the LDS works in a dense slab per item: what the LU copy of the general path costs
    ws_bytes = int(env.lib.pthip_gbsv_workspace(_dt(A), inner, n))
    ws = DeviceArray.empty((ws_bytes,), "uint8") if ws_bytes else None
    for f, idx in enumerate(np.ndindex(*[s for s, _ in outer])):
        offs = [sum(i * sts[k] for i, (_, sts) in zip(idx, outer)) for k in range(2)]
        ffi.check(env.lib.pthip_band_scan(_dt(A), scanned, n, A.ptr + offs[0] * isz, st[0], A.strides[-2], A.strides[-1], band.ptr))
        ffi.check(env.lib.pthip_gbsv_batched(
            _dt(A), inner, n, nrhs, A.ptr + offs[0] * isz, st[0], A.strides[-2], A.strides[-1], b.ptr + offs[1] * isz, st[1],
            out.ptr + f * inner * per * isz, band.ptr, None if ws is None else ws.ptr, ws_bytes))


def solve_banded(env, A: DeviceArray, b: DeviceArray, b_ndim: int) -> DeviceArray:
    """x = A^-1 b with each item's bandwidths found from its data, by the tier ``banded_tier`` names.  ``lower`` plays
    no part (scipy ignores it); a zero or NaN pivot NaN-fills the item, as in ``solve_general``."""
    n = A.shape[-1]
    if A.shape[-2] != n:
        raise ValueError("Solve: expected a square matrix")
    if b.shape[b.ndim - b_ndim] != n:
        raise ValueError(f"Solve: incompatible shapes {A.shape} and {b.shape}")
    if str(b.dtype) != str(A.dtype):
        raise TypeError("Solve: dtype mismatch")
    bshape = tuple(np.broadcast_shapes(A.shape[:-2], b.shape[: b.ndim - b_ndim]))
    nb = int(np.prod(bshape)) if bshape else 1
    out = DeviceArray.empty((*bshape, *b.shape[b.ndim - b_ndim :]), b.dtype)
    if out.size:
        if banded_tier(n, nb) == "wave":
            _gesv_wave(env, A, b, b_ndim, out, bshape, False)
        else:
            _gbsv(env, A, b, b_ndim, out, bshape)
    return out


def _solve(env, p, A, b):
    from pytensor_amd.dispatch.linalg import _lapack_operands

    A, b = _lapack_operands(env, "Solve", A, b)  # (integer / float16 operands: LAPACK's working type)
    assume = p["assume_a"]
    if assume == "pos":
        # scipy posv reads the triangle named by `lower` (default: upper)
        c = cholesky_device(env, A, bool(p["lower"]))
        return cho_solve_device(env, c, b, bool(p["lower"]), p["b_ndim"])
    if assume in ("gen", "sym", "her"):
        if assume != "gen":
            # scipy sysv reads only the triangle named by `lower`
            A = _symmetrize(env, A, bool(p["lower"]))
        return solve_general(env, A, b, p["b_ndim"])
    if assume == "tridiagonal":
        from pytensor_amd.dispatch.decomp import solve_tridiagonal

        return solve_tridiagonal(env, A, b, p["b_ndim"])
    if assume == "banded":
        return solve_banded(env, A, b, p["b_ndim"])
    raise NotImplementedError(f"hip linker: Solve(assume_a={assume!r}) is not lowered")


def lu_factor_device(env, a: DeviceArray):
    """``LUFactor`` (linalg/decomposition/lu.py:239; perform 279-299: scipy ``getrf``): the packed
    factors and LAPACK's 0-based interchange vector (int32); an exactly zero pivot NaN-fills LU.
    Leading dims are a batch (``Blockwise``).  What the reference's decomposition-reuse rewrites
    (rewriting/linalg/solvers.py:615-632) factor once for several ``Solve`` nodes."""
    LU, perm, _, _, bshape = getrf_device(env, a)
    nb, n = perm.shape
    piv = DeviceArray.empty((nb, n), "int32")
    if nb and n:
        ffi.check(env.lib.pthip_lu_factor_finish(_dt(a), nb, n, LU.ptr, perm.ptr, piv.ptr))
    return (LU.view((*bshape, n, n), contiguous_strides((*bshape, n, n))),
            piv.view((*bshape, n), contiguous_strides((*bshape, n))))


@handler("LUFactor")
def lu_factor(node, inputs, env):
    return list(lu_factor_device(env, env.to_device(inputs[0])))


@handler("PivotToPermutations")
def pivot_to_permutations(node, inputs, env):
    """lu.py:206-231: the permutation (or its inverse) LAPACK's sequential row interchanges amount to."""
    piv = env.to_device(inputs[0])
    if piv.dtype.kind not in "iu" or piv.itemsize not in (4, 8):
        raise TypeError(f"PivotToPermutations: integer pivots expected, got {piv.dtype}")
    n = piv.shape[-1]
    bshape = piv.shape[:-1]
    pc = piv.contiguous()
    nb = int(np.prod(bshape)) if bshape else 1
    out = DeviceArray.empty(piv.shape, "int64")
    if nb and n:
        ffi.check(env.lib.pthip_pivots_to_perm(pc.itemsize, int(bool(node.params["inverse"])), nb, n, pc.ptr, out.ptr))
    return [out]


@handler("Solve")
def solve(node, inputs, env):
    A, b = (env.to_device(i) for i in inputs)
    return [_solve(env, node.params, A, b)]


def _det(env, x):
    LU, perm, sign, logabs, bshape = getrf_device(env, x)
    return sign, logabs, bshape


@handler("Det")
def det(node, inputs, env):
    from pytensor_amd.dispatch.elemwise import launch_elemwise

    sign, logabs, bshape = _det(env, env.to_device(inputs[0]))
    dt = str(sign.dtype)
    # det = sign * exp(log|det|): how np.linalg.det finishes too (umath_linalg det_from_slogdet)
    body = {
        "in_dtypes": [dt, dt], "out_dtypes": [dt],
        "body": [{"op": "Exp", "in": [["i", 1]], "dtype": dt}, {"op": "Mul", "in": [["i", 0], ["t", 0]], "dtype": dt}],
        "outs": [["t", 1]],
    }
    outs, _, _ = launch_elemwise(body, [sign, logabs], sign.shape, [dt], None, env)
    return [outs[0].view(bshape, contiguous_strides(bshape))]


@handler("SLogDet")
def slogdet(node, inputs, env):
    sign, logabs, bshape = _det(env, env.to_device(inputs[0]))
    return [sign.view(bshape, contiguous_strides(bshape)), logabs.view(bshape, contiguous_strides(bshape))]


@handler("MatrixInverse")
def matrix_inverse(node, inputs, env):
    """``np.linalg.inv`` of a (..., n, n) stack (LinAlgError when an item is singular), by the tiers of
    ``solve_tier`` with the identity as the right-hand side (generated on the device)."""
    x = env.to_device(inputs[0])
    n = x.shape[-1]
    if x.ndim < 2 or x.shape[-2] != n:
        raise ValueError("MatrixInverse: expected square matrices")
    bshape = x.shape[:-2]
    nb = int(np.prod(bshape)) if bshape else 1
    tier = solve_tier(n, nb)
    if tier != "loop":
        out = DeviceArray.empty(x.shape, x.dtype)
        if out.size:
            (_gesv_wave if tier == "wave" else _solve_composed)(env, x, None, 2, out, bshape, True)
        return [out]
    if nb == 0:
        return [DeviceArray.empty(x.shape, x.dtype)]
    LU, perm, _, _, _ = getrf_device(env, x.view((n, n), x.strides[-2:]), flag_singular=True)  # np.linalg.inv raises when singular
    lu = LU.view((n, n), (n, 1))
    pb = DeviceArray.empty((n, n), x.dtype)  # P * I, built on the device (no upload per call)
    ffi.check(env.lib.pthip_permuted_identity(_dt(x), n, perm.ptr, pb.ptr))
    y = trsm_device(env, lu, pb, True, True, 2)
    return [trsm_device(env, lu, y, False, False, 2).view(x.shape, contiguous_strides(x.shape))]


@handler("Eigh")
def eigh(node, inputs, env):
    """``Eigh`` of the standard problem (linalg/decomposition/eigen.py:102; perform 177-195):
    eigenvalues ascending, eigenvectors as columns, the chosen triangle only (csrc/eigh.hip).
    Leading dims are a batch (``Blockwise``)."""
    if len(inputs) == 2:
        return _eigh_generalised(node, inputs, env)
    from pytensor_amd.dispatch.linalg import _lapack_operands

    (a,) = _lapack_operands(env, "Eigh", inputs[0])
    n = a.shape[-1]
    if a.shape[-2] != n:
        raise ValueError("Eigh: expected a square matrix")
    bshape = a.shape[:-2]
    ab = _batchify(a, 2, bshape)
    nb = ab.shape[0]
    w = DeviceArray.empty((nb, n), a.dtype)
    v = DeviceArray.empty((nb, n, n), a.dtype)
    if nb and n:
        ffi.check(env.lib.pthip_eigh(_dt(a), nb, n, int(node.params["lower"]), ab.ptr, w.ptr, v.ptr))
    return [w.view((*bshape, n), contiguous_strides((*bshape, n))), v.view((*bshape, n, n), contiguous_strides((*bshape, n, n)))]



def _symmetrize(env, x: DeviceArray, lower: bool) -> DeviceArray:
    n = x.shape[-1]
    bshape = x.shape[:-2]
    xb = _batchify(x, 2, bshape)
    out = DeviceArray.empty(xb.shape, x.dtype)
    if out.size:
        ffi.check(env.lib.pthip_symmetrize(_dt(x), xb.shape[0], n, int(lower), xb.ptr, out.ptr))
    return out.view((*bshape, n, n), contiguous_strides((*bshape, n, n)))


def _eigh_generalised(node, inputs, env):
    """``A v = w B v`` (Eigh with two inputs; perform = ``scipy.linalg.eigh(a, b, lower=)``, LAPACK
    sygvd): the same reduction LAPACK's ``sygst`` does, out of kernels that exist — ``B = L L^T``
    (potrf), ``C = L^-1 A L^-T`` (two multi-rhs triangular solves), the standard problem for C
    (Jacobi), ``v = L^-T y``.  Eigenvectors come out B-orthonormal (``v^T B v = I``) like scipy's.  Every one of
    those kernels takes a batch, so leading dims are a batch here too (``Blockwise``)."""
    from pytensor_amd.dispatch.linalg import _lapack_operands

    a, b = _lapack_operands(env, "Eigh", *inputs)
    n = a.shape[-1]
    if a.shape[-2] != n or b.shape[-2:] != (n, n):
        raise ValueError(f"Eigh: incompatible shapes {a.shape} and {b.shape}")
    lower = bool(node.params["lower"])
    A = _symmetrize(env, a, lower)
    B = _symmetrize(env, b, lower)
    L = cholesky_device(env, B, True)
    Y = trsm_device(env, L, A, True, False, 2)  # L Y = A  (leading dims: a batch, broadcast by the solve)
    Yt = Y.view(Y.shape, (*Y.strides[:-2], Y.strides[-1], Y.strides[-2])).contiguous()
    Cm = trsm_device(env, L, Yt, True, False, 2)  # L C = Y^T  ->  C = L^-1 A L^-T (symmetric)
    fake = type("_N", (), {"params": {"lower": True}})
    w, y = eigh(fake, [Cm], env)
    v = trsm_device(env, L, y, True, False, 2, trans=True)  # L^T v = y
    return [w, v]
