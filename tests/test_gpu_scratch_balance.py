"""GPU: every library function that takes scratch from the pool gives all of it back (csrc/scratch.h), and a launch
behind the cached LDS opt-in (csrc/common.h ``lds_opt_in``) still succeeds.

Each case calls a C-ABI entry on ``DeviceArray`` operands twice in one process (the second call goes through the cached
opt-in), checks both results against NumPy / SciPy at the bar of the path's own test, drops the operands and asserts
that ``bytes_in_use`` of ``pthip_pool_stats`` is what it was before the call.  The pool's cached blocks are released
before each call (``pthip_pool_trim``), so every block the call takes is a device allocation: ``n_device_allocs`` has
to rise by more than the number of operand and output arrays, which shows that the shape did reach a scratch path.

Shapes: the smallest that reach the scratch path, by the dispatch conditions of the sources.
  trsm_blocked     float64 n = 160, 64 right-hand sides: n (n|1) 8 > 160 KB - 256, no LDS kernel; nrhs > 16
  trsv_dag         the same matrix, 4 right-hand sides: nrhs <= 16
  chol (dag)       float64 n = 142: n (n|1) 8 > 160 KB - 2560 (tests/test_gpu_chol_blocked.py starts there)
  getrf_reg        float64 n = 64: n <= 128, the register kernel with its staged multipliers
  getrf_blocked2   float64 n = 141: n (n|1) 8 > 160 KB - 8192 (tests/test_gpu_lu_blocked.py starts there)
  eigh, A and V in scratch   float64 n = 141: beyond the one-sided kernel (n (n|1) 8 > 152 KB), not above EIGH_BLOCK_MIN
  eigh_block_jacobi          float64 n = 161 > EIGH_BLOCK_MIN = 160
  svd_block        float64 65 x 130, full matrices: svd_block_item, then svd_block_complete for rows 65 .. 129
  sort             float64, one row of 4097 > TILE = 4096
  nonzero          1000 mask bytes (any n > 0)
  exclusive_scan   1000 counts (any n > 0)
  csr_transpose    a 37 x 53 matrix with 300 stored entries (any nnz > 0)
  csr_fromdense_count   a 37 x 53 dense matrix (any rows > 0)
  gemm split-K     float64 130 x 135 x 300, row "split" of tests/blas_cases.py
  gemm_skinny slabs     float64 A^T B with 8192 rows, A 8192 x 5, B 8192 x 3: K >= 8192, M <= 512, N <= 16
  trsm_lds         float64 n = 80 then n = 120, 32 right-hand sides: 51 840 then 116 160 bytes of LDS, both above 48 KB —
                   the grant of the first call does not cover the second ("grants only grow")
  join_probe       pthip_join_probe, 256 iterations as in tests/test_gpu_plan.py: its 1 MB buffer
Three drivers are selected by environment switches that are read once per process; the same check runs in a fresh child
process with the switch set, as tests/test_gpu_lu_blocked.py and tests/test_gpu_chol_blocked.py do:
  getrf_blocked    PTHIP_LU_PANEL=v1, float64 n = 141
  chol_blocked     PTHIP_CHOL=steps, float64 n = 142 (the launch-per-step form)
  getrf, global memory   PTHIP_LU_UNBLOCKED=1, float64 n = 141: the one-workgroup kernel with the matrix in scratch
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def _pool(hip):
    """(bytes in use, device allocations so far)"""
    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    hip.check(hip.lib().pthip_pool_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, c.value


ARRAYS_MADE = [0]  # device arrays the running case has created (each is one pool block)


def _dev(*arrays):
    from pytensor_amd.device import DeviceArray

    ARRAYS_MADE[0] += len(arrays)
    return [DeviceArray.from_host(np.ascontiguousarray(a)) for a in arrays]


def _empty(shape, dtype):
    from pytensor_amd.device import DeviceArray

    ARRAYS_MADE[0] += 1
    return DeviceArray.empty(shape, dtype)


EPS = float(np.finfo("float64").eps)


def _tri(n, seed):
    rng = np.random.default_rng(seed)
    T = np.tril(rng.normal(size=(n, n)) / np.sqrt(n))
    T[np.diag_indices(n)] = 1.0 + rng.uniform(0.5, 1.5, n)
    return T


def _trsm(hip, n, nrhs):
    T = _tri(n, n)
    b = np.random.default_rng(n + nrhs).normal(size=(n, nrhs))
    dT, db = _dev(T, b)
    out = _empty(b.shape, b.dtype)
    hip.check(hip.lib().pthip_trsm(hip.np_dtype_code(b.dtype), 1, 0, 0, 1, n, nrhs, dT.ptr, n * n, n, 1, db.ptr, n * nrhs, out.ptr))
    x = out.to_host()
    # (tests/test_gpu_trsm_blocked.py: row-wise backward bound of substitution, c = 8)
    assert (np.abs(T @ x - b) <= 8.0 * n * EPS * (np.abs(T) @ np.abs(x))).all()


def _spd(n, seed):
    A = np.random.default_rng(seed).normal(size=(n, n + 8))
    return A @ A.T / n + np.eye(n)


def _potrf(hip, n):
    S = _spd(n, n)
    (dS,) = _dev(S)
    out = _empty(S.shape, S.dtype)
    hip.check(hip.lib().pthip_potrf(hip.np_dtype_code(S.dtype), 1, 1, n, dS.ptr, out.ptr))
    L = out.to_host()
    assert not np.triu(L, 1).any()
    # (tests/test_gpu_chol_blocked.py: C = 4)
    assert (np.abs(L @ L.T - S) <= 4.0 * n * EPS * (np.abs(L) @ np.abs(L).T)).all()


def _getrf(hip, n):
    import scipy.linalg

    A = np.random.default_rng(n).normal(size=(n, n))
    (dA,) = _dev(A)
    LU, perm, sign, logabs = _empty(A.shape, A.dtype), _empty((1, n), "int64"), _empty((1,), A.dtype), _empty((1,), A.dtype)
    hip.check(hip.lib().pthip_getrf(hip.np_dtype_code(A.dtype), 1, n, dA.ptr, LU.ptr, perm.ptr, sign.ptr, logabs.ptr, 0))
    LU, perm = LU.to_host(), perm.to_host()[0]
    _, piv = scipy.linalg.lu_factor(A)
    pref = np.arange(n)
    for k, p in enumerate(piv):
        pref[[k, p]] = pref[[p, k]]
    np.testing.assert_array_equal(perm, pref)
    L, U = np.tril(LU, -1) + np.eye(n), np.triu(LU)
    # (tests/test_gpu_lu_blocked.py: c = 4)
    assert (np.abs(L @ U - A[perm]) <= 4.0 * n * EPS * (np.abs(L) @ np.abs(U))).all()


def _eigh(hip, n):
    M = np.random.default_rng(100 + n).normal(size=(n, n))
    S = (M + M.T) / 2
    (dS,) = _dev(S)
    w, v = _empty((1, n), S.dtype), _empty((1, n, n), S.dtype)
    hip.check(hip.lib().pthip_eigh(hip.np_dtype_code(S.dtype), 1, n, 1, dS.ptr, w.ptr, v.ptr))
    w, V = w.to_host()[0], v.to_host()[0]
    st = ctypes.c_int(-1)
    hip.check(hip.lib().pthip_check_status(ctypes.byref(st)))
    assert st.value == 0
    wr = np.linalg.eigvalsh(S)
    scale = max(1.0, float(np.abs(wr).max()))
    # (tests/test_gpu_parity.py test_eigh_block_jacobi_beyond_one_cu: tol = 1e-12, times scale times n)
    np.testing.assert_allclose(w, wr, rtol=0, atol=1e-12 * scale * n)
    assert np.abs(S @ V - V * w).max() <= 1e-12 * scale * n
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-12 * n


def _svd_block(hip, r, c):
    x = np.random.default_rng(r + c).normal(size=(1, r, c))
    (X,) = _dev(x)
    S, Wt, Pt = _empty((1, r), x.dtype), _empty((1, c, c), x.dtype), _empty((1, r, r), x.dtype)
    hip.check(hip.lib().pthip_svd_block(hip.np_dtype_code(x.dtype), 1, r, c, 1, c, X.ptr, S.ptr, Wt.ptr, Pt.ptr))
    s, W, P = S.to_host()[0], Wt.to_host()[0], Pt.to_host()[0]
    s_ref = np.linalg.svd(x[0], compute_uv=False)
    # (tests/test_gpu_svd_block.py: TOL = 1e-12 for float64, relative to the largest singular value)
    assert np.abs(s - s_ref).max() <= 1e-12 * s_ref.max()
    assert np.abs(P.T @ (s[:, None] * W[:r]) - x[0]).max() <= 1e-12 * max(r, c) * s_ref.max()
    assert np.abs(W @ W.T - np.eye(c)).max() <= 1e-12 * c


def _sort(hip, n):
    x = np.random.default_rng(n).normal(size=(1, n))
    (dx,) = _dev(x)
    vals, idx = _empty(x.shape, x.dtype), _empty(x.shape, "int64")
    hip.check(hip.lib().pthip_sort(hip.np_dtype_code(x.dtype), 1, n, dx.ptr, vals.ptr, idx.ptr))
    np.testing.assert_array_equal(vals.to_host(), np.sort(x, axis=1))
    np.testing.assert_array_equal(idx.to_host(), np.argsort(x, axis=1, kind="stable"))


def _nonzero(hip, n):
    mask = (np.random.default_rng(n).uniform(size=n) < 0.3).astype("uint8")
    (dm,) = _dev(mask)
    idx, count = _empty((n,), "int64"), _empty((1,), "int64")
    hip.check(hip.lib().pthip_nonzero(n, dm.ptr, idx.ptr, count.ptr))
    k = int(count.to_host()[0])
    np.testing.assert_array_equal(idx.to_host()[:k], np.flatnonzero(mask))


def _scan(hip, n):
    c = np.random.default_rng(n).integers(0, 9, size=n).astype("int32")
    (dc,) = _dev(c)
    out = _empty((n + 1,), "int32")
    hip.check(hip.lib().pthip_exclusive_scan_i32(n, dc.ptr, out.ptr))
    np.testing.assert_array_equal(out.to_host(), np.concatenate([[0], np.cumsum(c)]))


def _sparse_case():
    import scipy.sparse as sp

    rng = np.random.default_rng(7)
    dense = np.zeros((37, 53))
    flat = rng.choice(37 * 53, size=300, replace=False)
    dense.flat[flat] = rng.normal(size=300)
    return dense, sp.csr_matrix(dense)


def _csr_transpose(hip):
    _, A = _sparse_case()
    m, n = A.shape
    d, i, p = _dev(A.data, A.indices.astype("int32"), A.indptr.astype("int32"))
    od, oi, op = _empty((A.nnz,), A.dtype), _empty((A.nnz,), "int32"), _empty((n + 1,), "int32")
    hip.check(hip.lib().pthip_csr_transpose(hip.np_dtype_code(A.dtype), m, n, A.nnz, d.ptr, i.ptr, p.ptr, od.ptr, oi.ptr, op.ptr))
    C = A.tocsc()
    np.testing.assert_array_equal(od.to_host(), C.data)
    np.testing.assert_array_equal(oi.to_host(), C.indices)
    np.testing.assert_array_equal(op.to_host(), C.indptr)


def _fromdense_count(hip):
    dense, A = _sparse_case()
    m, n = dense.shape
    (dx,) = _dev(dense)
    indptr = _empty((m + 1,), "int32")
    hip.check(hip.lib().pthip_csr_fromdense_count(hip.np_dtype_code(dense.dtype), m, n, dx.ptr, n, 1, indptr.ptr))
    np.testing.assert_array_equal(indptr.to_host(), A.indptr)


def _gemm(hip, A, pA, sA, B, M, N, K):
    """out = A @ B for device operands given as (pointer, element strides); the bar of tests/test_gpu_gemm_skinny.py"""
    (dB,) = _dev(B)
    out = _empty((M, N), "float64")
    hip.check(hip.lib().pthip_gemm(hip.np_dtype_code(np.dtype("float64")), 1, M, N, K, 1.0, pA, 0, sA[0], sA[1], dB.ptr, 0, N, 1, 0.0, None, 0, 0, 0,
                                   out.ptr))
    want = A @ B
    bound = 1e-12 * np.abs(want) + 8.0 * EPS * (np.abs(A) @ np.abs(B))
    assert (np.abs(out.to_host() - want) <= bound).all()


def _gemm_split(hip):
    rng = np.random.default_rng(3)
    A, B = rng.normal(size=(130, 300)), rng.normal(size=(300, 135))
    (dA,) = _dev(A)
    _gemm(hip, A, dA.ptr, (300, 1), B, 130, 135, 300)


def _gemm_skinny(hip):
    rng = np.random.default_rng(4)
    X, B = rng.normal(size=(8192, 5)), rng.normal(size=(8192, 3))
    (dX,) = _dev(X)
    _gemm(hip, X.T, dX.ptr, (1, 5), B, 5, 3, 8192)  # (A is the transposed view of the row-major 8192 x 5 array)


def _join_probe(hip):
    bad = ctypes.c_int(-1)
    had = os.environ.get("PTHIP_NO_STREAM_PRIORITY")
    os.environ["PTHIP_NO_STREAM_PRIORITY"] = "1"  # (if this call is the one that creates stream 1: at the default priority)
    try:
        hip.check(hip.lib().pthip_join_probe(256, ctypes.byref(bad)))
    finally:
        if had is None:
            del os.environ["PTHIP_NO_STREAM_PRIORITY"]
        else:
            os.environ["PTHIP_NO_STREAM_PRIORITY"] = had
    assert bad.value == 0


CASES = {
    "trsm_blocked": lambda hip: _trsm(hip, 160, 64),
    "trsv_dag": lambda hip: _trsm(hip, 160, 4),
    "chol_dag": lambda hip: _potrf(hip, 142),
    "getrf_reg": lambda hip: _getrf(hip, 64),
    "getrf_blocked2": lambda hip: _getrf(hip, 141),
    "eigh_scratch": lambda hip: _eigh(hip, 141),
    "eigh_block_jacobi": lambda hip: _eigh(hip, 161),
    "svd_block": lambda hip: _svd_block(hip, 65, 130),
    "sort": lambda hip: _sort(hip, 4097),
    "nonzero": lambda hip: _nonzero(hip, 1000),
    "exclusive_scan": lambda hip: _scan(hip, 1000),
    "csr_transpose": _csr_transpose,
    "csr_fromdense_count": _fromdense_count,
    "gemm_split": _gemm_split,
    "gemm_skinny": _gemm_skinny,
    "join_probe": _join_probe,
}
# (name, switch, value, case): the case run in a child process with the switch set
ENV_CASES = [("getrf_blocked", "PTHIP_LU_PANEL", "v1", "getrf_blocked2"), ("chol_steps", "PTHIP_CHOL", "steps", "chol_dag"),
             ("getrf_global", "PTHIP_LU_UNBLOCKED", "1", "getrf_blocked2")]


def balance(hip, case, takes_scratch=True):
    """run ``case`` twice: the pool is back where it was after each run, and each run took scratch"""
    for _ in range(2):
        hip.check(hip.lib().pthip_pool_trim())
        ARRAYS_MADE[0] = 0
        in_use, allocs = _pool(hip)
        case(hip)
        hip.check(hip.lib().pthip_synchronize())
        in_use_after, allocs_after = _pool(hip)
        assert in_use_after == in_use
        if takes_scratch:
            assert allocs_after - allocs > ARRAYS_MADE[0], "the call took no scratch: the shape did not reach the path"


@pytest.mark.parametrize("name", list(CASES))
def test_scratch_goes_back_to_the_pool(hip, name):
    balance(hip, CASES[name])


@pytest.mark.parametrize("name,switch,value,case", ENV_CASES, ids=[c[0] for c in ENV_CASES])
def test_scratch_goes_back_to_the_pool_in_the_switched_drivers(hip, name, switch, value, case):
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys\n"
        f"sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]\n"
        "from pytensor_amd import ffi\n"
        "import test_gpu_scratch_balance as t\n"
        "ffi.init(0)\n"
        f"t.balance(ffi, t.CASES[{case!r}])\n"
        "print('ok')\n"
    )
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{switch: value}), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_lds_grant_grows_with_the_need(hip):
    """trsm_lds_kernel asks for its own need at every call: a smaller matrix first, then one the first grant does not
    cover, then the smaller one again (already covered)"""
    for n in (80, 120, 80):
        balance(hip, lambda hip: _trsm(hip, n, 32), takes_scratch=False)
