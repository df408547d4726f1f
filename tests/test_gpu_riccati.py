"""GPU: ``solve_discrete_are`` under ``mode="hip"`` against the reference: fixtures of its own graph, its gradient and
a steady-state Kalman log-likelihood under its C linker (tests/golden/riccati/, tools/make_riccati_fixtures.py)."""
import json
import os

import numpy as np
import pytest

import riccati_cases as rc
from e2e_util import activate, assert_close, have_gpu, hip_executable

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "riccati")
CASES = json.load(open(os.path.join(GOLDEN, "cases.json")))["cases"]
# where the reference has a finite solution and the device returns NaN: R singular, or (A, Q^1/2) not
# detectable although (A, B) is stabilisable
DEVICE_NAN = ("singular_r", "undetectable_scalar", "undetectable_2x2")
FINITE = [c["name"] for c in CASES if not c["reference_all_nan"] and c["kind"] not in DEVICE_NAN]
META = {c["name"]: c for c in CASES}
F64_RTOL = 1e-10


@pytest.fixture(scope="module")
def env():
    pytensor = activate()
    if not have_gpu():
        pytest.skip("no GPU")
    import pytensor.tensor as pt
    from pytensor.tensor.linalg import solve_discrete_are

    fns = {}

    def dare(dtype, batched=False):
        key = (dtype, batched)
        if key not in fns:
            mk = (lambda nm: pt.tensor3(nm, dtype=dtype)) if batched else (lambda nm: pt.matrix(nm, dtype=dtype))
            ins = [mk(nm) for nm in "ABQR"]
            fns[key] = pytensor.function(ins, solve_discrete_are(*ins), mode="hip")
        return fns[key]

    return pytensor, pt, solve_discrete_are, dare


def _load(name):
    return rc.case_inputs(META[name]), np.load(os.path.join(GOLDEN, name + ".npz"))


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("name", FINITE)
def test_fixture_fp64(env, name):
    _, _, _, dare = env
    (A, B, Q, R), z = _load(name)
    X = dare("float64")(A, B, Q, R)
    assert X.dtype == np.float64 and X.shape == z["X"].shape
    assert np.all(np.isfinite(X))
    assert _rel(X, z["X"]) <= F64_RTOL, (name, _rel(X, z["X"]))


def test_reference_problem_residual(env):
    """the reference's own eval_fun: A^T X A - X - A^T X B (R + B^T X B)^-1 B^T X A + Q ~ 0 within 1e-12"""
    _, _, _, dare = env
    (a, b, q, r), _ = _load("reference")
    x = dare("float64")(a, b, q, r)
    res = a.T @ x @ a - x - (a.T @ x @ b) @ np.linalg.solve(r + b.T @ x @ b, b.T) @ x @ a + q
    np.testing.assert_allclose(res, 0.0, atol=1e-12)


@pytest.mark.parametrize("name", ["reference", "random_5x3", "random_14x1"])
def test_fixture_fp32(env, name):
    """float32 operands: iterated in fp64, returned as float64 like the reference's graph"""
    _, _, _, dare = env
    (A, B, Q, R), z = _load(name)
    X = dare("float32")(*(x.astype(np.float32) for x in (A, B, Q, R)))
    assert X.dtype == z["X32"].dtype
    # (the reference's own float32 answer is off its float64 one by up to 1.2e-4 on the near-marginal
    #  random_14x1, closed-loop spectral radius 0.976: the bar is 1e-4 or twice that distance, whichever is larger)
    ref_err = _rel(z["X32"], z["X"])
    assert _rel(X, z["X32"]) <= max(1e-4, 2 * ref_err)
    # (the iteration runs in fp64 on the rounded operands: closer to the float64 solution than the reference is)
    assert _rel(X, z["X"]) <= max(1e-4, ref_err)


@pytest.mark.parametrize("name", ["unstabilizable", *DEVICE_NAN])
def test_failure_is_all_nan(env, name):
    _, _, _, dare = env
    (A, B, Q, R), z = _load(name)
    # (the reference has no solution for the unstabilisable pair; for the others its solution is finite and the
    #  device's NaN is the documented difference)
    assert META[name]["reference_all_nan"] == (name == "unstabilizable")
    X = dare("float64")(A, B, Q, R)
    assert X.shape == A.shape and np.all(np.isnan(X)), X


def test_composed_tier_failure_is_all_nan(env):
    """m > 64: the same semantics from the composed tier (unstabilisable mode in a 70-state system)"""
    _, _, _, dare = env
    A = np.diag(np.r_[1.5, np.full(69, 0.5)])
    B = np.zeros((70, 1))
    B[1:, 0] = 1.0
    X = dare("float64")(A, B, np.eye(70), np.eye(1))
    assert np.all(np.isnan(X))


def test_empty(env):
    _, _, _, dare = env
    X = dare("float64")(np.zeros((0, 0)), np.zeros((0, 2)), np.zeros((0, 0)), np.eye(2))
    assert X.shape == (0, 0) and X.dtype == np.float64


def test_strided_operands(env):
    """transposed / sliced operands reach the kernel as their values"""
    pytensor, pt, solve_discrete_are, _ = env
    (A, B, Q, R), z = _load("random_5x3")
    a, b, q, r = (pt.dmatrix(nm) for nm in "ABQR")
    f = pytensor.function([a, b, q, r], solve_discrete_are(a.T, b[::2], q.T, r.T), mode="hip")
    Bbig = np.zeros((10, 3))
    Bbig[::2] = B
    X = f(np.ascontiguousarray(A.T), Bbig, np.ascontiguousarray(Q.T), np.ascontiguousarray(R.T))
    assert _rel(X, z["X"]) <= F64_RTOL


def test_batch_of_5_matches_single_bitwise(env):
    """the reference's batched test problem: one launch, every item bit-identical to its own solve"""
    _, _, _, dare = env
    (a, b, q, r), z = _load("reference")
    Xb = dare("float64", batched=True)(*(np.stack([x] * 5) for x in (a, b, q, r)))
    X1 = dare("float64")(a, b, q, r)
    assert Xb.shape == (5, 2, 2)
    for k in range(5):
        assert np.array_equal(Xb[k], X1)
    assert _rel(X1, z["X"]) <= F64_RTOL


def test_batch_of_64_matches_single_bitwise(env):
    _, _, _, dare = env
    items = [rc.random_case(10, 2, 7000 + k) for k in range(64)]
    Xb = dare("float64", batched=True)(*(np.stack([it[j] for it in items]) for j in range(4)))
    f1 = dare("float64")
    for k, it in enumerate(items):
        X1 = f1(*it)
        assert np.array_equal(Xb[k], X1), k
    import scipy.linalg as sl

    assert _rel(Xb[3], sl.solve_discrete_are(*items[3])) <= F64_RTOL


def _three_calls(f, vals):
    """eager, capture and replay calls: identical bits"""
    outs = [[np.array(o, copy=True) for o in f(*vals)] for _ in range(3)]
    for o in outs[1:]:
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(outs[0], o))
    return outs[0]


@pytest.mark.parametrize("m", [2, 10, 40])
def test_gradient_matches_c_linker(env, m):
    """the reference's pullback, lowered as it is, against its values under the C linker"""
    pytensor, pt, solve_discrete_are, _ = env
    z = np.load(os.path.join(GOLDEN, f"grad_m{m}.npz"))
    ins = [pt.dmatrix(nm) for nm in "ABQR"]
    W = pt.dmatrix("W")
    cost = rc.gradient_cost(pt, solve_discrete_are(*ins), W)
    f = pytensor.function([*ins, W], [cost, *pytensor.grad(cost, ins)], mode="hip")
    got = _three_calls(f, [z[k] for k in "ABQRW"])
    for g, k in zip(got, ["cost", "gA", "gB", "gQ", "gR"]):
        assert_close(g, z[k], f"m = {m}: {k}", rtol=1e-7, atol=1e-9)


def test_gradient_at_a_failed_dare_is_nan(env):
    """X is all NaN at the unstabilisable pair: the pullback (whose symmetric solve factors R + B^T X B) gives NaN
    gradients, not a fault"""
    pytensor, pt, solve_discrete_are, _ = env
    (A, B, Q, R), _ = _load("unstabilizable")
    ins = [pt.dmatrix(nm) for nm in "ABQR"]
    X = solve_discrete_are(*ins)
    f = pytensor.function(ins, pytensor.grad((X ** 2).sum(), ins), mode="hip")
    for g in f(A, B, Q, R):
        assert np.all(np.isnan(g))


def test_kalman_steady_state_logp_and_grad(env):
    """the seasonal model's steady-state Kalman log-likelihood (DARE covariance, Scan over 96 observations) and its
    gradient against the reference's C linker"""
    pytensor, pt, solve_discrete_are, _ = env
    z = np.load(os.path.join(GOLDEN, "kalman.npz"))
    ins, logp = rc.kalman_graph(pt, solve_discrete_are, pytensor.scan)
    f = pytensor.function(ins, [logp, pytensor.grad(logp, ins[0])], mode="hip")
    assert "HostPerform" not in [n.op for n in f.maker.linker.last_ir.nodes]
    lp, g = _three_calls(f, [z["log_sd"], z["y"]])
    assert_close(lp, z["logp"], "logp", rtol=1e-9, atol=1e-10)
    assert_close(g, z["grad"], "grad", rtol=1e-9, atol=1e-10)


def test_composed_tier_stein_equation(env):
    """n = 0 above m = 64: X = A^T X A + Q"""
    import scipy.linalg as sl

    _, _, _, dare = env
    A = 0.8 * np.random.default_rng(4).normal(size=(70, 70)) / np.sqrt(70)
    X = dare("float64")(A, np.zeros((70, 0)), np.eye(70), np.zeros((0, 0)))
    assert _rel(X, sl.solve_discrete_lyapunov(A.T, np.eye(70))) <= F64_RTOL


def test_eager_captured_replayed_identical_bits(env):
    """three calls of one compiled function (eager, capture, replay) give the same bits, both tiers"""
    _, _, _, dare = env
    for name in ("random_32x3", "random_65x1"):
        (A, B, Q, R), z = _load(name)
        f = dare("float64")
        outs = [f(A, B, Q, R).copy() for _ in range(3)]
        assert all(np.array_equal(outs[0], o) for o in outs[1:]), name
        assert _rel(outs[0], z["X"]) <= F64_RTOL


def test_graph_with_dare_freezes(env):
    """no host read in either tier: a graph holding the DARE freezes into a replayable plan"""
    pytensor, pt, solve_discrete_are, _ = env
    for name in ("random_14x3", "random_65x3"):
        (A, B, Q, R), z = _load(name)
        ins = [pt.dmatrix(nm) for nm in "ABQR"]
        X = solve_discrete_are(*ins)
        f = pytensor.function(ins, [X, X.sum()], mode="hip")
        Xg, _ = _three_calls(f, [A, B, Q, R])
        assert hip_executable(f)._auto_plan is not None, name
        assert _rel(Xg, z["X"]) <= F64_RTOL
