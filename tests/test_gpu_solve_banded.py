"""GPU: ``Solve(assume_a="banded")`` — the band scan and the banded LU of csrc/gbsv.hip behind
``dispatch/lu.py::solve_banded``, the dense one-launch tier it uses up to n = 64, and the C ABI called directly at
the sizes the dispatcher never sends to the band kernels.

The yardstick is ``np.linalg.solve`` on the host in float64.  The bar of every comparison, per item:
``max|x - x_ref| <= tol * max|x_ref|`` with tol = 1e-12 (float64) / 1e-5 (float32), the project's parity tolerances.
The inputs (``banded_input``) keep cond(A) <= 100 (float64) / 10 (float32), which the tests assert and never repair;
swapping adjacent rows makes every second pivot a genuine interchange.
"""
import numpy as np
import pytest
import scipy.linalg

from test_gpu_solve_batched import assert_bar, one_node
from test_solve_banded_lowering import banded_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def solve_exe(dtype, a_nd, b_nd, b_ndim, **kw):
    from pytensor_amd.executor import HipExecutable

    p = {"assume_a": "banded", "lower": False, "b_ndim": b_ndim}
    out_nd = max(a_nd - 2, b_nd - b_ndim) + b_ndim
    if a_nd == 2 and b_nd == b_ndim:
        g = one_node("Solve", p, [(dtype, 2), (dtype, b_nd)], [(dtype, out_nd)])
    else:
        sig = "(m,m),(m)->(m)" if b_ndim == 1 else "(m,m),(m,k)->(m,k)"
        g = one_node("Blockwise", {"core_op": "Solve", "core_params": p, "signature": sig}, [(dtype, a_nd), (dtype, b_nd)], [(dtype, out_nd)])
    return HipExecutable(g, **kw)


def inputs(n, band, rhs, batch, dtype, seed=0):
    """(A, b, reference, b_ndim): A of ``dtype`` with the condition bound asserted, the reference in float64"""
    rng = np.random.default_rng(seed)
    kl0, ku0 = (n, n) if band == "full" else band
    A = banded_input(n, kl0, ku0, rng, batch=batch).astype(dtype)
    cond = np.linalg.cond(A.astype("float64")).max()
    assert cond <= (100 if dtype == "float64" else 10), (n, band, dtype, cond)
    b_ndim = 1 if rhs == "vec" else 2
    b = rng.standard_normal((batch, n) if rhs == "vec" else (batch, n, rhs)).astype(dtype)
    return A, b, reference(A, b, b_ndim), b_ndim


def reference(A, b, b_ndim):
    A64, b64 = A.astype("float64"), b.astype("float64")
    return np.linalg.solve(A64, b64[..., None])[..., 0] if b_ndim == 1 else np.linalg.solve(A64, b64)


# (n, band before the row swaps, right-hand sides, batch, dtype): every n with every band, and each kind of right-hand
# side, batch size and dtype spread over them — pruned from the full product
PARITY = [
    (65, (0, 0), "vec", 67, "float64"), (65, (1, 1), 1, 2, "float32"), (65, (2, 0), 3, 1, "float64"), (65, (0, 3), 9, 2, "float32"),
    (65, (7, 5), "vec", 1, "float32"), (65, (40, 40), 3, 2, "float64"), (65, "full", 1, 67, "float32"),
    (130, (0, 0), 9, 1, "float32"), (130, (1, 1), "vec", 67, "float64"), (130, (2, 0), 1, 2, "float32"), (130, (0, 3), 3, 2, "float64"),
    (130, (7, 5), 9, 67, "float64"), (130, (40, 40), "vec", 2, "float32"), (130, "full", 3, 1, "float64"),
    (300, (0, 0), 1, 2, "float64"), (300, (1, 1), 9, 1, "float64"), (300, (2, 0), "vec", 2, "float32"), (300, (0, 3), 1, 1, "float32"),
    (300, (7, 5), 3, 2, "float32"), (300, (40, 40), 9, 2, "float64"), (300, "full", "vec", 1, "float64"), (300, "full", 3, 2, "float32"),
    # the band (2, 2) keeps the rows a step touches in registers while 3 * nrhs <= 64 going down and 5 * nrhs <= 64 coming
    # back: both in registers, the last count that is, down only, neither, and more columns than a wave has lanes
    (130, (1, 1), 12, 2, "float64"), (130, (1, 1), 13, 1, "float32"), (130, (1, 1), 21, 2, "float64"), (130, (1, 1), 22, 1, "float64"),
    (65, (1, 1), 70, 2, "float64"),
]


@pytest.mark.parametrize("n,band,rhs,batch,dtype", PARITY)
def test_parity(hip, n, band, rhs, batch, dtype):
    A, b, ref, b_ndim = inputs(n, band, rhs, batch, dtype)
    (x,) = solve_exe(dtype, 3, 1 + b_ndim, b_ndim)(A, b)
    assert_bar(x, ref, dtype, f"banded n={n} band={band} rhs={rhs} batch={batch}")
    if batch == 1:  # the unbatched node takes the same kernels
        (x1,) = solve_exe(dtype, 2, b_ndim, b_ndim)(A[0], b[0])
        assert np.array_equal(x1, x[0])


@pytest.mark.parametrize("band,where", [((40, 40), "the global workspace"), ((1, 1), "LDS")])
def test_band_beyond_the_lds_and_inside_it(hip, band, where):
    """float64, n = 1025: the working band of (41, 41) is 124 rows x 1025 x 8 B = 1.0 MB and goes through the
    workspace accessor; (2, 2) at the same n stays in LDS"""
    n = 1025
    A, b, ref, _ = inputs(n, band, "vec", 1, "float64")
    kl, ku = scipy.linalg.bandwidth(A[0])
    assert ((2 * kl + ku + 1) * n * 8 > 160 * 1024) == (where != "LDS")
    (x,) = solve_exe("float64", 3, 2, 1)(A, b)
    assert_bar(x, ref, "float64", f"n={n} band={band}: {where}")


def _abi_solve(hip, A, b):
    """pthip_band_scan + pthip_gbsv_batched on a contiguous stack; returns (x, the bandwidths the scan found)"""
    from pytensor_amd.device import DeviceArray

    lib = hip.lib()
    batch, n, nrhs = b.shape
    dt = hip.np_dtype_code(A.dtype)
    dA, dB = DeviceArray.from_host(A), DeviceArray.from_host(b)
    X, band = DeviceArray.empty(b.shape, b.dtype), DeviceArray.empty((batch, 2), "int32")
    wsb = int(lib.pthip_gbsv_workspace(dt, batch, n))
    ws = DeviceArray.empty((wsb,), "uint8") if wsb else None
    hip.check(lib.pthip_band_scan(dt, batch, n, dA.ptr, n * n, n, 1, band.ptr))
    hip.check(lib.pthip_gbsv_batched(dt, batch, n, nrhs, dA.ptr, n * n, n, 1, dB.ptr, n * nrhs, X.ptr, band.ptr, None if ws is None else ws.ptr, wsb))
    return X.to_host(), band.to_host()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_c_abi_at_the_sizes_below_the_band_tier(hip, n, dtype):
    for band in [(0, 0), (1, 1), (2, 0), (0, 3)]:
        A, b, ref, _ = inputs(n, band, 3, 5, dtype, seed=n)
        x, found = _abi_solve(hip, A, b)
        assert [tuple(f) for f in found] == [scipy.linalg.bandwidth(a) for a in A], (n, band)
        assert_bar(x, ref, dtype, f"C ABI n={n} band={band}")


def test_band_scan_follows_scipy(hip):
    """exact zeros bound the band: a NaN counts as an entry, -0.0 does not; several workgroups per item, both the
    16-byte and the element-wise loads, and a transposed view"""
    from pytensor_amd.device import DeviceArray

    lib = hip.lib()
    rng = np.random.default_rng(5)
    for dtype in ("float64", "float32"):
        for n in (4, 130, 300, 301):
            A = np.stack([np.eye(n), banded_input(n, 3, 1, rng), banded_input(n, 0, 7, rng), rng.standard_normal((n, n)), np.zeros((n, n))]).astype(dtype)
            A[0, 3, 0], A[0, 0, 3] = np.nan, -0.0
            A[2, n - 1, 1] = 1e-30
            want = [scipy.linalg.bandwidth(a) for a in A]
            assert want[0] == (3, 0) and want[2][0] == n - 2 and want[4] == (0, 0)
            dA, band = DeviceArray.from_host(A), DeviceArray.empty((len(A), 2), "int32")
            hip.check(lib.pthip_band_scan(hip.np_dtype_code(dtype), len(A), n, dA.ptr, n * n, n, 1, band.ptr))
            assert [tuple(f) for f in band.to_host()] == want, (dtype, n)
            hip.check(lib.pthip_band_scan(hip.np_dtype_code(dtype), len(A), n, dA.ptr, n * n, 1, n, band.ptr))  # A.mT
            assert [tuple(f) for f in band.to_host()] == [(u, l) for l, u in want], (dtype, n)


def test_mixed_bandwidths_in_one_batch(hip):
    n = 130
    rng = np.random.default_rng(11)
    bands = [(0, 0), (n, n), (1, 1), (7, 5), (40, 40), (2, 0), (0, 3)]
    A = np.stack([np.diag(1.0 + rng.random(n))] + [banded_input(n, kl, ku, rng) for kl, ku in bands[1:]])
    # a lower and an upper triangular band (kl or ku exactly zero): the same inputs with the row swaps undone
    unswapped = np.stack([banded_input(n, 2, 0, rng), banded_input(n, 0, 3, rng)])
    unswapped[:, : n - n % 2] = unswapped[:, : n - n % 2].reshape(2, -1, 2, n)[:, :, ::-1].reshape(2, -1, n)
    assert scipy.linalg.bandwidth(unswapped[0]) == (2, 0) and scipy.linalg.bandwidth(unswapped[1]) == (0, 3)
    A = np.concatenate([A, unswapped])
    bands += [(2, 0), (0, 3)]
    assert np.linalg.cond(A).max() <= 100
    b = rng.standard_normal((len(bands), n, 3))
    (x,) = solve_exe("float64", 3, 3, 2)(A, b)
    assert_bar(x, np.linalg.solve(A, b), "float64", "mixed bandwidths")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pivoting_is_real(hip, dtype):
    n, batch = 130, 67
    A, b, ref, _ = inputs(n, (2, 2), 3, batch, dtype, seed=3)
    # (without row interchanges every second pivot is ~0.01 against a column maximum of ~1)
    assert np.median(np.abs(np.diagonal(A, axis1=1, axis2=2)) / np.abs(A).max(axis=1)) < 0.1
    (x,) = solve_exe(dtype, 3, 3, 2)(A, b)
    assert_bar(x, ref, dtype, "pivot n=130")


def test_singular_and_nan_items_stay_isolated(hip):
    n, batch = 130, 9
    A, b, _, _ = inputs(n, (3, 1), "vec", batch, "float64", seed=7)
    A = A.copy()
    zero_row, zero_pivot, nan_item, wide_zero_row = 0, 4, 6, 8
    A[zero_row, 17, :] = 0.0  # an exactly zero row
    # rows 0 and 1 equal, their leading 2.0 the pivot of column 0: the multiplier is exactly 1, row 1 becomes exactly zero
    A[zero_pivot, 1, :] = A[zero_pivot, 0, :]
    A[zero_pivot, :2, 0] = 2.0
    A[nan_item, 41, 40] = np.nan
    A[wide_zero_row] = banded_input(n, 40, 40, np.random.default_rng(8))  # (the four-wave path)
    A[wide_zero_row, n - 1, :] = 0.0
    (x,) = solve_exe("float64", 3, 2, 1)(A, b)
    dead = np.zeros(batch, bool)
    dead[[zero_row, zero_pivot, nan_item, wide_zero_row]] = True
    assert np.isnan(x[dead]).all()
    assert_bar(x[~dead], reference(A[~dead], b[~dead], 1), "float64", "isolation")


@pytest.fixture(scope="module")
def pt(hip):
    from e2e_util import activate

    pytensor = activate()
    import pytensor.tensor as ptt

    return pytensor, ptt


def test_strided_and_broadcast_operands_match_the_contiguous_case(hip, pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve

    n = 130
    A, b, _, _ = inputs(n, (3, 1), 2, 5, "float64", seed=2)
    A2, A3, b2, b3 = ptt.dmatrix("A2"), ptt.dtensor3("A3"), ptt.dmatrix("b2"), ptt.dtensor3("b3")
    plain = pytensor.function([A3, b3], solve(A3, b3, assume_a="banded"), mode="hip")
    # a transposed view of the stack
    At = np.ascontiguousarray(A.transpose(0, 2, 1))
    assert np.linalg.cond(At).max() <= 100
    xt = pytensor.function([A3, b3], solve(A3.transpose(0, 2, 1), b3, assume_a="banded"), mode="hip")(A, b)
    assert_bar(xt, np.linalg.solve(At, b), "float64", "transposed view")
    assert np.array_equal(xt, plain(At, b))
    # one matrix against a stack of right-hand sides, and a stack of matrices against one block
    xa = pytensor.function([A2, b3], solve(A2, b3, assume_a="banded"), mode="hip")(A[0], b)
    assert_bar(xa, np.linalg.solve(A[0], b), "float64", "A (n,n), b (5,n,2)")
    assert np.array_equal(xa, plain(np.ascontiguousarray(np.broadcast_to(A[0], A.shape)), b))
    xb = pytensor.function([A3, b2], solve(A3, b2, assume_a="banded"), mode="hip")(A, b[0])
    assert_bar(xb, np.linalg.solve(A, b[0]), "float64", "A (5,n,n), b (n,2)")
    assert np.array_equal(xb, plain(A, np.ascontiguousarray(np.broadcast_to(b[0], b.shape))))


def test_frozen_plan_reads_the_band_on_every_replay(hip):
    """a plan captured with one bandwidth replays with others: the band is found on the device at every call"""
    n = 130
    exe = solve_exe("float64", 2, 1, 1, auto_freeze=True)
    rng = np.random.default_rng(4)
    calls = [(1, 1)] * 3 + [(7, 5), None, (40, 40), (1, 1)]
    for c, band in enumerate(calls):
        A = np.diag(1.0 + rng.random(n)) if band is None else banded_input(n, *band, rng)
        assert np.linalg.cond(A) <= 100
        b = rng.standard_normal(n)
        (x,) = exe(A, b)
        assert_bar(x[None], np.linalg.solve(A, b)[None], "float64", f"call {c}, band {band}")
        if c == 2:
            assert exe._auto_plan is not None, exe.stats
    assert exe.stats["capture_failures"] == 0 and exe.stats["replays"] >= len(calls) - 2, exe.stats


def test_end_to_end_solve_and_gradient_against_the_c_linker(hip, pt):
    pytensor, ptt = pt
    import e2e_util as E
    from pytensor.tensor.linalg import solve

    n = 130
    rng = np.random.default_rng(6)
    Av, bv = banded_input(n, 3, 2, rng), rng.standard_normal(n)
    assert np.linalg.cond(Av) <= 100
    A, b = ptt.dmatrix("A"), ptt.dvector("b")
    x = solve(A, b, assume_a="banded")
    outs = [x, *pytensor.grad((x**2).sum(), [A, b])]
    f_hip = pytensor.function([A, b], outs, mode="hip")
    want = pytensor.function([A, b], outs, mode=E.reference_mode())(Av, bv)
    for c in range(3):  # eager, capture, replay
        got = f_hip(Av, bv)
        for name, g, w in zip(("x", "dA", "db"), got, want):
            assert_bar(g[None], np.asarray(w)[None], "float64", f"{name}, call {c} (hip vs {E.reference_mode_name()})")
    assert E.hip_executable(f_hip).stats["capture_failures"] == 0
