"""GPU: column-pivoted QR (``QR(pivoting=True)``, csrc/decomp.hip ``geqp3_kernel``) against the call the reference
makes: LAPACK ``geqp3`` (+ ``orgqr``) on the host, assembled into the op's outputs as ``QR.perform`` does.

Pivots are compared only where they are well defined.  From the reference's R, at step k the candidates' residual
norms are ``c_j = ||R[k:K, j]||`` (j >= k) and ``gap_k = (c_k - max_{j>k} c_j) / c_k``; every parity case asserts
``min_k gap_k >= 4 sqrt(eps)`` (6e-8 in float64, 1.4e-3 in float32: sqrt(eps) is the accuracy to which LAPACK's own
downdated norms are guaranteed).  Then ``jpvt`` must be equal element for element and every other output entry by
entry within

    float64: |a - b| <= 1e-13 max|x| max(m, n) + 1e-11 |b|      (the bar of test_gpu_decomp.test_qr_matches_lapack)
    float32: |a - b| <= 1e-6  max|x| max(m, n) + 1e-4  |b|

The worst ``|a - b| / bar`` of each case is printed.  Every case, compared or not, must satisfy the invariants of
``check_invariants``.

Input families (all deterministic in their seed):

``gauss(m, n, dtype, seed)``     standard normal; float64 only (its gaps, >= 1e-5 at these shapes, are below the
                                 float32 condition).
``graded(m, n, dtype, seed)``    ``x[:, perm] = Q0 @ R0`` with Q0 an orthonormal m x K basis, R0 upper trapezoidal
                                 K x n with diagonal +-d_k, d_k = 1000^(-k/(K-1)), and entries above the diagonal
                                 uniform in +-0.1 d_i by row, perm a random permutation: the pivot order is perm by
                                 construction, and the dynamic range of 1000 stays above float32 rounding.
``parallel(m, pairs, seed)``     float64; from an orthonormal m x 2 pairs basis Q the columns ``u = 1.37^i Q[:, 2i]``
                                 and ``0.9 u + 1e-7 (1 + 1e-3 i) Q[:, 2i+1]``, permuted: every second pivot depends
                                 on a norm that dropped by seven orders of magnitude in one step, so the
                                 recomputation branch of the downdating decides it.  Only ``jpvt`` and the invariants
                                 are checked: the small pivots are ill-conditioned (entries differ by about 1e-8).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

from pytensor_amd.ir import Graph

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

MODES = ("full", "economic", "r", "raw")
SIGNATURE = {"full": "(m,n)->(m,m),(m,n),(n)", "economic": "(m,n)->(m,k),(k,n),(n)", "r": "(m,n)->(m,n),(n)",
             "raw": "(m,n)->(n,m),(k),(m,n),(n)"}
BAR = {"float64": (1e-13, 1e-11), "float32": (1e-6, 1e-4)}
INVARIANT_TOL = {"float64": lambda m, n: 1e-13 * max(m, n), "float32": lambda m, n: 1e-5}


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def one_node(op, params, in_specs, out_specs):
    g = Graph(name=f"one_{op}")
    ins = [g.new_var(dt, (None,) * nd) for dt, nd in in_specs]
    outs = [g.new_var(dt, (None,) * nd) for dt, nd in out_specs]
    g.add_node(op, params, ins, outs)
    g.inputs, g.outputs = ins, outs
    return g


@functools.lru_cache(maxsize=None)
def qr_exe(mode, dtype, lead=0, in_dtype=None):
    """the executable of one pivoted QR node (``lead`` = 0) or of its Blockwise over ``lead`` batch dimensions"""
    from pytensor_amd.executor import HipExecutable

    mat, vec, piv = (dtype, 2 + lead), (dtype, 1 + lead), ("int32", 1 + lead)
    outs = {"full": [mat, mat, piv], "economic": [mat, mat, piv], "r": [mat, piv], "raw": [mat, vec, mat, piv]}[mode]
    params = {"mode": mode, "pivoting": True}
    ins = [(in_dtype or dtype, 2 + lead)]
    if lead == 0:
        return HipExecutable(one_node("QR", params, ins, outs))
    return HipExecutable(one_node("Blockwise", {"core_op": "QR", "core_params": params, "signature": SIGNATURE[mode]}, ins, outs))


# ---- inputs ---------------------------------------------------------------------------------------
def gauss(m, n, dtype, seed):
    return np.random.default_rng(seed).standard_normal((m, n)).astype(dtype)


def graded(m, n, dtype, seed):
    rng = np.random.default_rng(seed)
    K = min(m, n)
    d = 1000.0 ** (-np.arange(K) / max(K - 1, 1))
    R0 = np.triu(rng.uniform(-0.1, 0.1, size=(K, n)) * d[:, None], 1)
    R0[np.arange(K), np.arange(K)] = d * rng.choice([-1.0, 1.0], size=K)
    Q0, _ = np.linalg.qr(rng.standard_normal((m, K)))
    perm = rng.permutation(n)
    x = np.empty((m, n))
    x[:, perm] = Q0 @ R0
    return x.astype(dtype)


def parallel(m, pairs, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((m, 2 * pairs)))
    cols = []
    for i in range(pairs):
        u = 1.37**i * Q[:, 2 * i]
        cols += [u, 0.9 * u + 1e-7 * (1 + 1e-3 * i) * Q[:, 2 * i + 1]]
    return np.stack(cols, axis=1)[:, rng.permutation(2 * pairs)].copy()


FAMILY = {"gauss": gauss, "graded": graded}


# ---- the reference: the LAPACK calls of QR.perform, assembled as it assembles them ------------------
def _with_lwork(fn, *args, **kw):
    *_, work, _info = fn(*args, lwork=-1, **kw)
    return fn(*args, lwork=work.item(), **kw)


def lapack_factor(x):
    (geqp3,) = scipy.linalg.get_lapack_funcs(("geqp3",), (x,))
    qr, jpvt, tau, *_ = _with_lwork(geqp3, x)
    return qr, tau, (jpvt - 1).astype("int32")  # (1-based in LAPACK)


def lapack_outputs(x, mode, factor=None):
    M, N = x.shape
    qr, tau, jpvt = factor if factor is not None else lapack_factor(x)
    R = np.triu(qr) if (mode not in ("economic", "raw") or M < N) else np.triu(qr[:N, :])
    if mode == "r":
        return [R, jpvt]
    if mode == "raw":
        return [qr, tau, R, jpvt]
    (orgqr,) = scipy.linalg.get_lapack_funcs(("orgqr",), (qr,))
    if M < N:
        Q, _work, _info = _with_lwork(orgqr, qr[:, :M].copy(), tau)
    elif mode == "economic":
        Q, _work, _info = _with_lwork(orgqr, qr.copy(), tau)
    else:
        qqr = np.zeros((M, M), dtype=qr.dtype)
        qqr[:, :N] = qr
        Q, _work, _info = _with_lwork(orgqr, qqr, tau)
    return [Q, R, jpvt]


@functools.lru_cache(maxsize=None)
def case(family, m, n, dtype):
    """(x, LAPACK's factorisation of it): computed once, shared and read-only"""
    x = FAMILY[family](m, n, dtype, m + n)
    fac = lapack_factor(x)
    for a in (x, *fac):
        a.setflags(write=False)
    return x, fac


def min_gap(R):
    """min over the steps k of (c_k - max_{j>k} c_j) / c_k, c_j = ||R[k:K, j]||, from a (reference) R"""
    K, n = min(R.shape), R.shape[1]
    R = np.asarray(R[:K], dtype="float64")
    c = np.sqrt(np.cumsum((R * R)[::-1], axis=0)[::-1])  # c[k, j] = ||R[k:K, j]||
    gaps = [(c[k, k] - c[k, k + 1:].max()) / c[k, k] for k in range(K) if k + 1 < n]
    return min(gaps) if gaps else np.inf


def sqrt_eps(dtype):
    return float(np.sqrt(np.finfo(dtype).eps))


def worst_ratio(got, want, x):
    """max over the floating outputs of |a - b| / bar; the permutation must be equal"""
    ca, cr = BAR[str(x.dtype)]
    scale = float(np.abs(x).max()) if x.size else 0.0
    worst = 0.0
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if b.dtype.kind == "i":
            assert np.array_equal(a, b), (k, a, b)
        elif b.size:
            bar = ca * scale * max(x.shape) + cr * np.abs(b.astype("float64"))
            worst = max(worst, float((np.abs(a.astype("float64") - b.astype("float64")) / bar).max()))
    return worst


def check_invariants(x, outs, mode):
    m, n = x.shape
    K = min(m, n)
    dtype = str(np.result_type(x.dtype, "float32")) if x.dtype.kind == "f" else "float64"
    jpvt = outs[-1]
    assert jpvt.dtype == np.int32 and jpvt.shape == (n,)
    assert np.array_equal(np.sort(jpvt), np.arange(n)), jpvt
    R = outs[{"full": 1, "economic": 1, "r": 0, "raw": 2}[mode]].astype("float64")
    assert np.array_equal(R, np.triu(R))
    tol = INVARIANT_TOL[dtype](m, n)
    scale = float(np.abs(x).max()) if x.size else 0.0
    if mode in ("full", "economic"):
        Q = outs[0].astype("float64")
        assert np.abs(Q.T @ Q - np.eye(Q.shape[1])).max(initial=0.0) <= tol
        assert np.abs(Q @ R - x[:, jpvt]).max(initial=0.0) <= tol * scale
    # the pivoting property: R[k,k]^2 >= (1 - delta) sum_{i=k..min(j,K-1)} R[i,j]^2 for all j > k
    delta = 4 * sqrt_eps(dtype)
    S = np.cumsum((R[:K] * R[:K])[::-1], axis=0)[::-1]
    d2 = np.diag(R[:K, :K]) ** 2
    later = np.arange(n)[None, :] > np.arange(K)[:, None]
    bad = later & ~(d2[:, None] >= (1 - delta) * S)
    assert not bad.any(), (np.argwhere(bad)[:5], d2[:5])


# ---- parity with LAPACK ---------------------------------------------------------------------------
def lds_edge(dtype):
    """the largest square shape the LDS form takes (136 in float64, 193 in float32)"""
    from pytensor_amd.dispatch.decomp import geqp3_lds_fits

    item = np.dtype(dtype).itemsize
    n = max(k for k in range(1, 513) if geqp3_lds_fits(k, k, item))
    assert geqp3_lds_fits(n, n, item) and not geqp3_lds_fits(n + 1, n + 1, item)
    return n


SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (8, 8), (17, 9), (9, 17), (33, 20), (20, 33), (64, 64), (65, 65), (130, 67),
          (67, 130), (300, 40), (129, 129), (40, 300), (600, 3), (5000, 3)]
ALL_MODES_AT = {(17, 9), (9, 17), (65, 65), (67, 130)}


def _parity_cases():
    out = []
    for family, dtype in (("graded", "float64"), ("graded", "float32"), ("gauss", "float64")):
        e = lds_edge(dtype)
        for shape in [*SHAPES, (e, e), (e + 1, e + 1)]:
            for mode in (MODES if shape in ALL_MODES_AT else ("economic",)):
                out.append(pytest.param(family, dtype, shape, mode, id=f"{family}-{dtype}-{shape[0]}x{shape[1]}-{mode}"))
    return out


def test_lds_edges_are_where_the_cases_say():
    assert lds_edge("float64") == 136 and lds_edge("float32") == 193


@pytest.mark.parametrize("family,dtype,shape,mode", _parity_cases())
def test_matches_lapack(hip, family, dtype, shape, mode):
    x, fac = case(family, *shape, dtype)
    want = lapack_outputs(x, mode, fac)
    gap = min_gap(np.triu(fac[0]))
    assert gap >= 4 * sqrt_eps(dtype), (gap, "the pivots of this case are not separated: the case is wrong")
    got = qr_exe(mode, dtype)(x)
    ratio = worst_ratio(got, want, x)
    print(f"{family} {dtype} {shape} {mode}: min gap {gap:.3e}, worst |a-b|/bar = {ratio:.3e}")
    assert ratio <= 1.0
    check_invariants(x, got, mode)


@pytest.mark.parametrize("m,pairs", [(12, 3), (40, 8), (16, 8)])
def test_recomputed_norms_decide_the_pivots(hip, m, pairs):
    x = parallel(m, pairs, m + pairs)
    qr, tau, jpvt = lapack_factor(x)
    gap = min_gap(np.triu(qr))
    assert gap >= 4 * sqrt_eps("float64"), gap
    got = qr_exe("economic", "float64")(x)
    assert np.array_equal(got[-1], jpvt), (got[-1], jpvt)
    check_invariants(x, got, "economic")


# ---- degenerate inputs ----------------------------------------------------------------------------
def test_all_zero_matrix_is_lapack_bit_for_bit(hip):
    z = np.zeros((4, 3))
    got, want = qr_exe("raw", "float64")(z), lapack_outputs(z, "raw")
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (a, b)
    assert np.array_equal(got[3], np.arange(3)) and np.array_equal(got[1], np.zeros(3))
    check_invariants(z, qr_exe("economic", "float64")(z), "economic")


def test_equal_largest_columns_take_the_lower_position(hip):
    x = gauss(9, 6, "float64", 3)
    x[:, 4] = x[:, 1] = 5.0 * x[:, 1]
    got = qr_exe("economic", "float64")(x)
    assert got[-1][0] == 1, got[-1]
    check_invariants(x, got, "economic")


def test_rank_two_product(hip):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((12, 2)) @ rng.standard_normal((2, 7))
    got = qr_exe("economic", "float64")(x)
    check_invariants(x, got, "economic")
    d = np.abs(np.diag(got[1]))
    assert (d[2:] <= 1e-12 * d[0]).all(), d


def test_integer_operand_gives_float64(hip):
    x = np.random.default_rng(4).integers(-9, 10, size=(7, 5))
    got = qr_exe("economic", "float64", 0, "int64")(x)
    want = lapack_outputs(x.astype("float64"), "economic")
    assert [a.dtype for a in got] == [np.float64, np.float64, np.int32]
    assert worst_ratio(got, want, x.astype("float64")) <= 1.0
    check_invariants(x.astype("float64"), got, "economic")


@pytest.mark.parametrize("shape", [(0, 3), (3, 0)])
@pytest.mark.parametrize("mode", MODES)
def test_empty_operands_do_what_the_reference_does(hip, shape, mode):
    """QR.perform on an empty operand is LAPACK's own argument check: with SciPy 1.15, (3, 0) returns empty factors
    (and the identity for the full Q) while (0, 3) raises f2py's ``_flapack.error`` from the second geqp3 call"""
    x = np.zeros(shape)
    try:
        want = lapack_outputs(x, mode)
    except Exception as e:  # noqa: BLE001 (the class has no public name)
        with pytest.raises(type(e)):
            qr_exe(mode, "float64")(x)
        return
    got = qr_exe(mode, "float64")(x)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (a, b)


# ---- batches through Blockwise --------------------------------------------------------------------
def _stack(shape, items, dtype):
    return np.stack([graded(*shape, dtype, 1000 + 7 * k + sum(shape)) for k in range(items)])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("items", [1, 3, 67])
@pytest.mark.parametrize("shape", [(8, 8), (33, 20), (67, 130)])
def test_stack_equals_the_items_bit_for_bit(hip, shape, items, dtype):
    xs = _stack(shape, items, dtype)
    got = qr_exe("economic", dtype, 1)(xs)
    one = qr_exe("economic", dtype)
    for k in range(items):
        for a, b in zip(got, one(xs[k])):
            assert a[k].dtype == b.dtype and np.array_equal(a[k], b), (k, shape)
    check_invariants(xs[-1], [a[-1] for a in got], "economic")


def test_two_batch_dimensions_and_every_mode(hip):
    xs = _stack((9, 17), 6, "float64").reshape(2, 3, 9, 17)
    for mode in MODES:
        got = qr_exe(mode, "float64", 2)(xs)
        one = qr_exe(mode, "float64")
        for i in range(2):
            for j in range(3):
                ref = one(xs[i, j])
                assert len(ref) == len(got)
                for a, b in zip(got, ref):
                    assert a.shape[:2] == (2, 3) and np.array_equal(a[i, j], b), (mode, i, j)


def test_zero_and_rank_deficient_items_leave_the_others_alone(hip):
    xs = _stack((33, 20), 5, "float64")
    alone = qr_exe("economic", "float64", 1)(xs)
    rng = np.random.default_rng(8)
    mixed = xs.copy()
    mixed[1] = 0.0
    mixed[3] = rng.standard_normal((33, 2)) @ rng.standard_normal((2, 20))
    got = qr_exe("economic", "float64", 1)(mixed)
    for k in (0, 2, 4):
        for a, b in zip(got, alone):
            assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(got[2][1], np.arange(20)) and not got[1][1].any()
    for k in (1, 3):
        check_invariants(mixed[k], [a[k] for a in got], "economic")


def test_global_form_forced_by_the_environment(hip, tmp_path):
    """PTHIP_QR_NO_LDS is read when the library loads: a fresh child process factors the (64, 64) graded case with
    it set, and the parent holds the result to the same bar"""
    x, fac = case("graded", 64, 64, "float64")
    np.save(tmp_path / "x.npy", x)
    env = dict(os.environ, PTHIP_QR_NO_LDS="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_rrqr_worker.py"), str(tmp_path / "x.npy"), str(tmp_path / "out.npz")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(tmp_path / "out.npz")
    got = [z[f"out{k}"] for k in range(3)]
    ratio = worst_ratio(got, lapack_outputs(x, "economic", fac), x)
    print(f"global form, graded float64 (64, 64): worst |a-b|/bar = {ratio:.3e}")
    assert ratio <= 1.0
    check_invariants(x, got, "economic")


# ---- frozen plan ----------------------------------------------------------------------------------
def test_frozen_plan_replays_bit_identically(hip):
    exe = qr_exe("economic", "float64")
    xa, xb = graded(33, 20, "float64", 1), graded(33, 20, "float64", 2)
    ea, eb = exe(xa), exe(xb)
    plan = exe.freeze(xa)
    try:
        for _ in range(2):
            for x, e in ((xa, ea), (xb, eb)):
                for a, b in zip(plan(x), e):
                    assert np.array_equal(a, b)
    finally:
        plan.close()


# ---- end to end -----------------------------------------------------------------------------------
def test_end_to_end_against_the_c_linker(hip):
    import e2e_util as E

    pytensor = E.activate()
    import pytensor.tensor as ptt

    for var, val in ((ptt.dmatrix("x"), graded(33, 20, "float64", 53)), (ptt.dtensor3("x"), _stack((33, 20), 3, "float64"))):
        outs = list(ptt.linalg.qr(var, mode="economic", pivoting=True))
        f_hip = pytensor.function([var], outs, mode="hip")
        f_ref = pytensor.function([var], outs, mode=E.reference_mode())
        nodes = E.hip_executable(f_hip).graph.nodes
        assert not any(nd.op == "HostPerform" for nd in nodes), [nd.op for nd in nodes]
        want = f_ref(val)
        for call in range(3):  # eager, capture, replay
            got = f_hip(val)
            items = [(val, got, want)] if val.ndim == 2 else [(val[k], [a[k] for a in got], [b[k] for b in want]) for k in range(len(val))]
            for x, g, w in items:
                assert worst_ratio(g, w, x) <= 1.0, call
