"""GPU: ``SolveSylvester`` above the Kronecker tier (Bartels-Stewart, csrc/sylvester.hip) against SciPy at run time
and against the reference's C linker for gradients; the Lyapunov solves that reach it (one Schur form); batches;
failure as all-NaN; eager / captured / replayed bits and plan freezing."""
import numpy as np
import pytest

from e2e_util import activate, assert_close, have_gpu, hip_executable, reference_mode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    pytensor = activate()
    if not have_gpu():
        pytest.skip("no GPU")
    import pytensor.tensor as pt

    fns = {}

    def sylv(dtype="float64", batched=False):
        key = (dtype, batched)
        if key not in fns:
            from pytensor.tensor.linalg import solve_sylvester

            mk = pt.tensor3 if batched else pt.matrix
            A, B, C = (mk(nm, dtype=dtype) for nm in "ABC")
            fns[key] = pytensor.function([A, B, C], solve_sylvester(A, B, C), mode="hip")
        return fns[key]

    return pytensor, pt, sylv


def _problem(m, n, seed):
    """well-separated spectra: eig(A) in Re > 1, eig(-B) in Re < -1"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(m, m)) / np.sqrt(m) + 3.0 * np.eye(m)
    B = rng.normal(size=(n, n)) / np.sqrt(n) + 3.0 * np.eye(n)
    C = rng.normal(size=(m, n))
    return A, B, C


def _rel_residual(A, B, C, X):
    return np.linalg.norm(A @ X + X @ B - C) / (np.linalg.norm(A) * np.linalg.norm(X) + np.linalg.norm(X) * np.linalg.norm(B) + np.linalg.norm(C))


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def _direct(env_, A, B, C, b_is_a_t=False):
    """the device path called on its own (any m, n up to 1024, below the Kronecker bound too)"""
    from pytensor_amd.dispatch.decomp import solve_sylvester_schur

    return _run_device(lambda e, a, b, c: solve_sylvester_schur(e, a, b, c, b_is_a_t), A, B, C)


def _run_device(fn, *arrs):
    from pytensor_amd import ffi
    from pytensor_amd.device import DeviceArray

    class _Env:
        lib = ffi.lib()
        keepalive = []

        @staticmethod
        def to_device(v):
            return v if isinstance(v, DeviceArray) else DeviceArray.from_host(np.asarray(v))

        @staticmethod
        def timed(name, f):
            f()

    out = fn(_Env, *(DeviceArray.from_host(np.ascontiguousarray(a)) for a in arrs))
    return out.to_host()


@pytest.mark.parametrize("mn", [(65, 65), (70, 90), (300, 20), (20, 300), (128, 128)])
def test_solve_sylvester_fp64(env, mn):
    import scipy.linalg as sl

    _, _, sylv = env
    A, B, C = _problem(*mn, seed=mn[0] * 7 + mn[1])
    X = sylv()(A, B, C)
    assert X.dtype == np.float64 and X.shape == mn
    assert _rel_residual(A, B, C, X) <= 1e-12
    assert _rel(X, sl.solve_sylvester(A, B, C)) <= 1e-10


def test_solve_sylvester_1024(env):
    _, _, sylv = env
    A, B, C = _problem(1024, 1024, seed=11)
    X = sylv()(A, B, C)
    assert _rel_residual(A, B, C, X) <= 1e-12


def test_fp32_operands(env):
    """computed in fp64 on the rounded operands, returned in the node's dtype"""
    import scipy.linalg as sl

    _, _, sylv = env
    A, B, C = (x.astype(np.float32) for x in _problem(80, 70, seed=3))
    X = sylv("float32")(A, B, C)
    want = sl.solve_sylvester(*(x.astype(np.float64) for x in (A, B, C)))
    assert X.dtype == np.float32
    assert _rel(X.astype(np.float64), want) <= 1e-5


def test_strided_and_transposed_operands(env):
    import scipy.linalg as sl

    pytensor, pt, _ = env
    from pytensor.tensor.linalg import solve_sylvester

    A, B, C = _problem(70, 80, seed=5)
    a, b, c = pt.dmatrix("a"), pt.dmatrix("b"), pt.dmatrix("c")
    f = pytensor.function([a, b, c], solve_sylvester(a.T, b[::2], c.T), mode="hip")
    Bbig = np.zeros((160, 80))
    Bbig[::2] = B
    X = f(np.ascontiguousarray(A.T), Bbig, np.ascontiguousarray(C.T))
    assert _rel(X, sl.solve_sylvester(A, B, C)) <= 1e-10


def test_broadcast_batch_matches_single_calls(env):
    """one batched call: items agree with single calls within 1e-13, bit for bit here (same kernels, same GEMM
    shapes except the batch count)"""
    _, _, sylv = env
    items = [_problem(66, 66, seed=40 + k) for k in range(3)]
    A = np.stack([it[0] for it in items])
    B = items[0][1][None]  # broadcast over the batch
    C = np.stack([it[2] for it in items])
    Xb = sylv("float64", batched=True)(A, B, C)
    assert Xb.shape == (3, 66, 66)
    for k in range(3):
        X1 = sylv()(A[k], B[0], C[k])
        assert _rel(Xb[k], X1) <= 1e-13
        assert np.array_equal(Xb[k], X1), k


def test_continuous_lyapunov(env):
    import scipy.linalg as sl

    pytensor, pt, _ = env
    from pytensor.tensor.linalg import solve_continuous_lyapunov

    rng = np.random.default_rng(8)
    A = rng.normal(size=(100, 100)) / 10.0 - 2.0 * np.eye(100)
    Q = rng.normal(size=(100, 100))
    a, q = pt.dmatrix("a"), pt.dmatrix("q")
    f = pytensor.function([a, q], solve_continuous_lyapunov(a, q), mode="hip")
    X = f(A, Q)
    assert _rel(X, sl.solve_continuous_lyapunov(A, Q)) <= 1e-10
    # the one-Schur path agrees with the two-Schur path
    X2 = _direct(None, A, A.T, Q, b_is_a_t=False)
    assert _rel(X, X2) <= 1e-12


def _seasonal(s, phi=0.6):
    """state transition of a structural model with a dummy seasonal of period s and an AR(1) level: s states"""
    T = np.zeros((s, s))
    T[0, 0] = phi
    T[1, 1:] = -1.0
    T[2:, 1:-1] += np.eye(s - 2)
    return T


def test_bilinear_discrete_lyapunov_seasonal(env):
    import scipy.linalg as sl

    pytensor, pt, _ = env
    from pytensor.tensor.linalg import solve_discrete_lyapunov

    A = 0.98 * _seasonal(100)
    Q = np.eye(100)
    a, q = pt.dmatrix("a"), pt.dmatrix("q")
    f = pytensor.function([a, q], solve_discrete_lyapunov(a, q, method="bilinear"), mode="hip")
    X = f(A, Q)
    want = sl.solve_discrete_lyapunov(A, Q)
    assert _rel(X, want) <= 1e-8
    assert np.linalg.norm(A @ X @ A.T - X + Q) / np.linalg.norm(X) <= 1e-10


@pytest.mark.parametrize("n", [8, 33, 64])
def test_direct_call_matches_kronecker_tier(env, n):
    _, _, sylv = env
    A, B, C = _problem(n, n, seed=n)
    X_kron = sylv()(A, B, C)  # (m n <= 4096: the Kronecker tier)
    X_bs = _direct(None, A, B, C)
    assert _rel(X_bs, X_kron) <= 1e-10


def test_nan_operand_gives_all_nan(env):
    _, _, sylv = env
    A, B, C = _problem(70, 70, seed=2)
    for which in range(2):
        ops = [A.copy(), B.copy(), C]
        ops[which][3, 5] = np.nan
        X = sylv()(*ops)
        assert X.shape == (70, 70) and np.all(np.isnan(X))


def test_eager_captured_replayed_identical_bits_and_freeze(env):
    pytensor, pt, _ = env
    from pytensor.tensor.linalg import solve_sylvester

    A, B, C = _problem(80, 72, seed=9)
    a, b, c = pt.dmatrix("a"), pt.dmatrix("b"), pt.dmatrix("c")
    X = solve_sylvester(a, b, c)
    f = pytensor.function([a, b, c], [X, X.sum()], mode="hip")
    outs = [[np.array(o, copy=True) for o in f(A, B, C)] for _ in range(3)]
    for o in outs[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(outs[0], o))
    assert hip_executable(f)._auto_plan is not None


def test_gradient_matches_c_linker(env):
    pytensor, pt, _ = env
    from pytensor.tensor.linalg import solve_sylvester

    A, B, C = _problem(80, 70, seed=21)
    W = np.random.default_rng(22).normal(size=(80, 70))
    a, b, c, w = (pt.dmatrix(nm) for nm in "abcw")
    cost = (solve_sylvester(a, b, c) * w).sum()
    outs = [cost, *pytensor.grad(cost, [a, b, c])]
    got = pytensor.function([a, b, c, w], outs, mode="hip")(A, B, C, W)
    want = pytensor.function([a, b, c, w], outs, mode=reference_mode())(A, B, C, W)
    for g, r, k in zip(got, want, ["cost", "gA", "gB", "gC"]):
        assert_close(g, r, k, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("m", [70, 100])
def test_dare_value_and_gradient_matches_c_linker(env, m):
    """the DARE's pullback solves a bilinear discrete Lyapunov equation of size m: above m = 64 it reaches this tier"""
    pytensor, pt, _ = env
    from pytensor.tensor.linalg import solve_discrete_are

    rng = np.random.default_rng(m)
    A = 0.9 * rng.normal(size=(m, m)) / np.sqrt(m)
    Bm = rng.normal(size=(m, 2))
    Q, R = np.eye(m), np.eye(2)
    Wt = rng.normal(size=(m, m))
    ins = [pt.dmatrix(nm) for nm in "ABQR"]
    w = pt.dmatrix("W")
    cost = (solve_discrete_are(*ins) * w).sum()
    outs = [cost, *pytensor.grad(cost, ins)]
    vals = [A, Bm, Q, R, Wt]
    got = pytensor.function([*ins, w], outs, mode="hip")(*vals)
    want = pytensor.function([*ins, w], outs, mode=reference_mode())(*vals)
    for g, r, k in zip(got, want, ["cost", "gA", "gB", "gQ", "gR"]):
        assert_close(g, r, f"m = {m}: {k}", rtol=1e-7, atol=1e-9)
