"""GPU: batched general solves and inverses of small matrices in one launch (csrc/lu_batched.hip through
``dispatch/lu.py::solve_tier``), the composed tier above n = 64, and the batched generalised ``eigh``.

The yardstick is NumPy / SciPy on the host in float64.  The bar of every comparison, per item:
``max|x - x_ref| <= tol * max|x_ref|`` with tol = 1e-12 (float64) / 1e-5 (float32), the project's parity tolerances;
the parity inputs ``A = G + n I`` keep cond(A) <= 100 (float64) / 10 (float32), which the tests assert.
"""
import numpy as np
import pytest

from pytensor_amd.ir import Graph

pytestmark = pytest.mark.gpu

TOL = {"float64": 1e-12, "float32": 1e-5}
CHUNK = 8  # right-hand-side columns per pass of the kernel (csrc/lu_batched.hip CH)


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


def solve_exe(dtype, a_nd, b_nd, b_ndim, assume_a="gen", lower=False):
    from pytensor_amd.executor import HipExecutable

    p = {"assume_a": assume_a, "lower": lower, "b_ndim": b_ndim}
    out_nd = max(a_nd - 2, b_nd - b_ndim) + b_ndim
    if a_nd == 2 and b_nd == b_ndim:
        g = one_node("Solve", p, [(dtype, 2), (dtype, b_nd)], [(dtype, out_nd)])
    else:
        sig = "(m,m),(m)->(m)" if b_ndim == 1 else "(m,m),(m,k)->(m,k)"
        g = one_node("Blockwise", {"core_op": "Solve", "core_params": p, "signature": sig}, [(dtype, a_nd), (dtype, b_nd)], [(dtype, out_nd)])
    return HipExecutable(g)


def inv_exe(dtype, nd):
    from pytensor_amd.executor import HipExecutable

    if nd == 2:
        return HipExecutable(one_node("MatrixInverse", {}, [(dtype, 2)], [(dtype, 2)]))
    return HipExecutable(one_node("Blockwise", {"core_op": "MatrixInverse", "core_params": {}, "signature": "(m,m)->(m,m)"}, [(dtype, nd)], [(dtype, nd)]))


def well_conditioned(n, batch, dtype, seed):
    """A = G + n I, G standard normal; the bound on cond(A) is asserted, never repaired"""
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((batch, n, n)) + n * np.eye(n)).astype(dtype)
    cond = np.linalg.cond(A.astype("float64")).max()
    assert cond <= (100 if dtype == "float64" else 10), (n, batch, dtype, seed, cond)
    return A, rng


def assert_bar(x, ref, dtype, what=""):
    """the bar, per item along the leading axis"""
    assert x.shape == ref.shape and str(x.dtype) == dtype, (what, x.shape, ref.shape, x.dtype)
    err = np.abs(x.astype("float64") - ref).reshape(ref.shape[0], -1).max(axis=1)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1)
    print(f"{what}: worst max|x - ref| / max|ref| over {ref.shape[0]} items = {np.nanmax(err / scale):.3e}")
    bad = np.nonzero(~(err <= TOL[dtype] * scale))[0]
    assert bad.size == 0, (what, [(int(k), err[k], scale[k]) for k in bad[:5]])


# (n, right-hand sides, batch, dtype, seed): every lane-group width and both sides of it, both template edges, every
# kind of right-hand side and every batch size, pruned from the full product
PARITY = [
    (1, "vec", 65, "float64", 0), (1, 3, 2, "float32", 0), (2, 1, 257, "float64", 2), (2, "n", 2, "float32", 0),
    (3, 3, 1, "float64", 0), (3, 9, 2, "float32", 0), (5, "n", 2, "float64", 0), (5, "vec", 1, "float32", 0),
    (8, 9, 65, "float64", 0), (8, 1, 2, "float32", 0), (9, "vec", 257, "float64", 0), (9, 3, 65, "float32", 0),
    (16, 1, 1, "float64", 0), (16, "n", 257, "float32", 0), (17, 3, 2, "float64", 0), (17, 9, 1, "float32", 0),
    (32, "n", 65, "float64", 0), (32, "vec", 2, "float32", 0), (33, 9, 257, "float64", 0), (33, 1, 65, "float32", 0),
    (63, "vec", 1, "float64", 0), (63, 3, 257, "float32", 0), (64, 1, 2, "float64", 0), (64, "n", 1, "float32", 0),
    (64, "n", 65, "float64", 0), (64, 9, 257, "float32", 0), (8, "n", 257, "float64", 0), (4, 9, 257, "float64", 0),
    (16, "vec", 257, "float32", 0), (3, 9, 1, "float64", 0),
]


@pytest.mark.parametrize("n,rhs,batch,dtype,seed", PARITY)
def test_parity(hip, n, rhs, batch, dtype, seed):
    assert CHUNK + 1 == 9
    A, rng = well_conditioned(n, batch, dtype, seed)
    b_ndim = 1 if rhs == "vec" else 2
    core = (n,) if rhs == "vec" else (n, n if rhs == "n" else rhs)
    b = rng.standard_normal((batch, *core)).astype(dtype)
    ref = np.linalg.solve(A.astype("float64"), b.astype("float64")[..., None] if b_ndim == 1 else b.astype("float64"))
    ref = ref[..., 0] if b_ndim == 1 else ref
    (x,) = solve_exe(dtype, 3, 1 + b_ndim, b_ndim)(A, b)
    assert_bar(x, ref, dtype, f"solve n={n} rhs={rhs} batch={batch}")
    if batch == 1:  # the unbatched node (what a Scan step holds) takes the same kernel
        (x1,) = solve_exe(dtype, 2, b_ndim, b_ndim)(A[0], b[0])
        assert np.array_equal(x1, x[0])


@pytest.mark.parametrize("n", [4, 16, 64])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pivoting_is_real(hip, n, dtype):
    rng = np.random.default_rng(100 + n)
    batch = 67
    D = 0.01 * rng.standard_normal((batch, n, n)) + np.eye(n) * (1.0 + rng.random((batch, n, 1)))
    A = np.stack([D[k][rng.permutation(n)] for k in range(batch)]).astype(dtype)
    # (without row interchanges the first pivots are ~0.01 against column maxima of ~1)
    assert np.median(np.abs(np.diagonal(A, axis1=1, axis2=2)) / np.abs(A).max(axis=1)) < 0.1
    b = rng.standard_normal((batch, n, 3)).astype(dtype)
    ref = np.linalg.solve(A.astype("float64"), b.astype("float64"))
    (x,) = solve_exe(dtype, 3, 3, 2)(A, b)
    assert_bar(x, ref, dtype, f"pivot n={n}")


@pytest.mark.parametrize("n", [4, 8])
def test_singular_and_nan_items_stay_isolated(hip, n):
    batch = 130
    A, rng = well_conditioned(n, batch, "float64", 7)
    A = A.copy()
    singular, nan_item = [0, 65, batch - 1], 77
    for k in singular:
        A[k, k % n, :] = 0.0  # an exactly zero row
    A[nan_item, 1, 0] = np.nan
    b = rng.standard_normal((batch, n))
    (x,) = solve_exe("float64", 3, 2, 1)(A, b)
    dead = np.zeros(batch, bool)
    dead[singular + [nan_item]] = True
    assert np.isnan(x[dead]).all()
    ref = np.linalg.solve(A[~dead], b[~dead][..., None])[..., 0]
    assert_bar(x[~dead], ref, "float64", f"isolation n={n}")


@pytest.mark.parametrize("n,seed", [(3, 1), (16, 0), (64, 0)])
def test_inverse_of_a_stack(hip, n, seed):
    A, _ = well_conditioned(n, 257, "float64", seed)
    (x,) = inv_exe("float64", 3)(A)
    assert_bar(x, np.linalg.inv(A), "float64", f"inv n={n}")


def test_inverse_singular_item_raises(hip):
    A, _ = well_conditioned(8, 257, "float64", 0)
    exe = inv_exe("float64", 3)
    S = A.copy()
    S[100, 3, :] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        exe(S)
    assert_bar(exe(A)[0], np.linalg.inv(A), "float64", "inv after the flag was cleared")
    # the composed tier raises the same way, and the single matrix still does
    B, _ = well_conditioned(96, 3, "float64", 0)
    assert_bar(exe(B)[0], np.linalg.inv(B), "float64", "inv n=96")
    B[1, 5, :] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        exe(B)
    with pytest.raises(np.linalg.LinAlgError):
        inv_exe("float64", 2)(S[100])


def test_composed_tier_shared_operands_and_wide_right_hand_sides(hip):
    """n = 96 is past the wave tier: one factorisation handed on with a batch stride of 0, a shared block of
    right-hand sides, and a stack against a multi-column stack"""
    n = 96
    A, rng = well_conditioned(n, 3, "float64", 0)
    b = rng.standard_normal((3, n, 2))
    (x,) = solve_exe("float64", 2, 3, 2)(A[0], b)  # A (96, 96) against b (3, 96, 2)
    assert_bar(x, np.linalg.solve(A[0], b), "float64", "shared A, n=96")
    (x,) = solve_exe("float64", 3, 2, 2)(A, b[0])  # A (3, 96, 96) against b (96, 2)
    assert_bar(x, np.linalg.solve(A, b[0]), "float64", "shared b, n=96")
    b5 = rng.standard_normal((3, n, 5))
    (x,) = solve_exe("float64", 3, 3, 2)(A, b5)
    assert_bar(x, np.linalg.solve(A, b5), "float64", "stack against a 5-column stack, n=96")


@pytest.fixture(scope="module")
def pt(hip):
    from e2e_util import activate

    pytensor = activate()
    import pytensor.tensor as ptt

    return pytensor, ptt


@pytest.mark.parametrize("n", [8, 33])
def test_broadcast_batch_dims_and_strided_operands(hip, pt, n):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve

    A1, rng = well_conditioned(n, 1, "float64", 0)
    A2, A3, A4 = ptt.matrix("A2"), ptt.tensor3("A3"), ptt.tensor4("A4")
    b2, b3, b4 = ptt.matrix("b2"), ptt.tensor3("b3"), ptt.tensor4("b4")
    # A (n, n) with b (65, n)
    bv = rng.standard_normal((65, n))
    x = pytensor.function([A2, b2], solve(A2, b2, b_ndim=1), mode="hip")(A1[0], bv)
    assert_bar(x, np.linalg.solve(A1[0], bv.T).T.copy(), "float64", "A (n,n), b (65,n)")
    # A (5, 1, n, n) with b (1, 7, n, 3)
    Av, _ = well_conditioned(n, 5, "float64", 0)
    bw = rng.standard_normal((1, 7, n, 3))
    x = pytensor.function([A4, b4], solve(A4, b4), mode="hip")(Av[:, None], bw)
    ref = np.linalg.solve(Av[:, None], bw)
    assert x.shape == (5, 7, n, 3)
    assert_bar(x.reshape(35, n, 3), ref.reshape(35, n, 3), "float64", "A (5,1,n,n), b (1,7,n,3)")
    # a transposed view, and every second matrix of a larger stack
    As, _ = well_conditioned(n, 10, "float64", 0)
    bs = rng.standard_normal((5, n, 2))
    xt, xs = pytensor.function([A3, b3], [solve(A3[:5].transpose(0, 2, 1), b3), solve(A3[::2], b3)], mode="hip")(As, bs)
    assert_bar(xt, np.linalg.solve(As[:5].transpose(0, 2, 1), bs), "float64", "transposed view")
    assert_bar(xs, np.linalg.solve(As[::2], bs), "float64", "every second matrix")


@pytest.mark.parametrize("lower", [True, False])
def test_symmetric_solve_reads_one_triangle(hip, lower):
    n, batch = 9, 65
    G, rng = well_conditioned(n, batch, "float64", 0)
    S = (G + G.transpose(0, 2, 1)) / 2
    assert np.linalg.cond(S).max() <= 100
    half = S.copy()
    iu = np.triu_indices(n, 1)
    if lower:
        half[:, iu[0], iu[1]] = np.nan
    else:
        half[:, iu[1], iu[0]] = np.nan
    b = rng.standard_normal((batch, n, 2))
    (x,) = solve_exe("float64", 3, 3, 2, assume_a="sym", lower=lower)(half, b)
    assert_bar(x, np.linalg.solve(S, b), "float64", f"sym lower={lower}")


def test_gradient_of_a_batched_solve(hip, pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve

    A, rng = well_conditioned(8, 33, "float64", 0)
    b, w = rng.standard_normal((33, 8)), rng.standard_normal((33, 8))
    A3, b2, w2 = ptt.tensor3("A"), ptt.matrix("b"), ptt.matrix("w")
    cost = (solve(A3, b2, b_ndim=1) * w2).sum()
    gA, gb = pytensor.function([A3, b2, w2], pytensor.grad(cost, [A3, b2]), mode="hip")(A, b, w)
    x = np.linalg.solve(A, b[..., None])[..., 0]
    gb_ref = np.linalg.solve(A.transpose(0, 2, 1), w[..., None])[..., 0]
    gA_ref = -gb_ref[:, :, None] * x[:, None, :]
    assert_bar(gb, gb_ref, "float64", "gb")
    assert_bar(gA, gA_ref, "float64", "gA")


def _launches(hip, exe, *ins):
    exe(*ins)  # warm-up: allocations, module loads
    lib = hip.lib()
    c0 = lib.pthip_launch_count()
    out = exe(*ins)
    return lib.pthip_launch_count() - c0, out


def _stack(n, batch):
    rng = np.random.default_rng(n)
    return rng.standard_normal((batch, n, n)) + n * np.eye(n), rng.standard_normal((batch, n))


def test_launch_count_does_not_grow_with_the_batch(hip):
    counts = {}
    for n in (8, 96):
        exe = solve_exe("float64", 3, 2, 1)
        for batch in (2, 257):
            A, b = _stack(n, batch)
            counts[n, batch], (x,) = _launches(hip, exe, A, b)
            assert_bar(x, np.linalg.solve(A, b[..., None])[..., 0], "float64", f"n={n} batch={batch}")
        assert counts[n, 257] == counts[n, 2], counts
    inv = {}
    for batch in (2, 257):
        A, _ = _stack(8, batch)
        inv[batch], _ = _launches(hip, inv_exe("float64", 3), A)
    assert inv[257] == inv[2], inv
    A, b = _stack(8, 1)
    small, _ = _launches(hip, solve_exe("float64", 2, 1, 1), A[0], b[0])
    assert small < counts[96, 2], (small, counts)


def test_frozen_plan_replays_bit_identically(hip):
    A, b = _stack(8, 257)
    exe = solve_exe("float64", 3, 2, 1)
    (e1,), (e2,) = exe(A, b), exe(A, b)
    assert np.array_equal(e1, e2)
    plan = exe.freeze(A, b)
    try:
        for _ in range(3):
            (r,) = plan(A, b)
            assert np.array_equal(r, e1)
    finally:
        plan.close()


def test_generalised_eigh_of_a_stack(hip):
    import scipy.linalg

    from pytensor_amd.executor import HipExecutable

    rng = np.random.default_rng(9)
    nb, n = 9, 6
    A = rng.standard_normal((nb, n, n))
    A = A + A.transpose(0, 2, 1)
    M = rng.standard_normal((nb, n, n))
    B = M @ M.transpose(0, 2, 1) + 6 * np.eye(n)
    assert np.linalg.cond(B).max() <= 10  # (the reduction C = L^-1 A L^-T loses a factor cond(B))
    g = one_node("Blockwise", {"core_op": "Eigh", "core_params": {"lower": True}, "signature": "(m,m),(m,m)->(m),(m,m)"},
                 [("float64", 3), ("float64", 3)], [("float64", 2), ("float64", 3)])
    w, v = HipExecutable(g)(A, B)
    for k in range(nb):
        wr = scipy.linalg.eigh(A[k], B[k], eigvals_only=True)
        assert np.abs(w[k] - wr).max() <= 1e-10 * np.abs(wr).max(), (k, w[k], wr)
        assert np.abs(v[k].T @ B[k] @ v[k] - np.eye(n)).max() <= 1e-10, k
