"""CPU self-test of tests/blas_cases.py: the bound of the dense-BLAS sweep is attainable by a correct product (NumPy's own
float32 / float64 ``A @ B``, a different summation order, passes on every row of the table), every mutation a wrong kernel
could produce fails it, and the table's branch names agree with a Python restatement of the dispatch of csrc/gemm.hip.
A checker that cannot fail is worth nothing: this is the test of that."""
import numpy as np
import pytest

import blas_cases as bc


@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            cache[name, dt] = bc.GemmData(bc.GEMM_BY_NAME[name], dt)
        return cache[name, dt]

    return get


def _numpy_result(d, alpha, beta):
    """the product in the operand dtype throughout, as a correct kernel would form it"""
    T = d.dt.type
    out = T(alpha) * np.matmul(d.A, d.B)
    if beta != 0:
        out = out + T(beta) * d.C
    assert out.dtype == d.dt
    return out


@pytest.mark.parametrize("dt", bc.DTYPES)
@pytest.mark.parametrize("row", bc.GEMM_ROWS, ids=lambda r: r.name)
def test_table_routes_match_the_dispatch(row, dt):
    branch, nslabs, launches = bc.plan_route(dt, *row.shape)
    assert branch == row.branch(dt)
    assert (nslabs > 1) == (row.branch(dt) in bc.SPLIT_BRANCHES or row.name == "t64_for_split")
    assert launches == (2 if row.branch(dt) in bc.SPLIT_BRANCHES else 1)
    # none of these is taken by csrc/gemm_skinny.hip, and the long-double reference stays cheap
    assert row.M < 8192 and row.K < 8192
    assert row.batch * row.M * row.N * row.K <= 10 ** 8


def test_table_covers_every_branch_in_both_dtypes():
    for dt, want in (("float64", {"skinny_short", "skinny_long", "skinny_split", "plain", "split", "t64"}),
                     ("float32", {"skinny_short", "skinny_long", "skinny_split", "plain", "split", "persistent", "s256"})):
        assert {r.branch(dt) for r in bc.GEMM_ROWS} == want
    plans = {r.name: bc.split_plan(*r.shape) for r in bc.GEMM_ROWS}
    assert plans["skinny_split_4steps"] == (2, 64)
    assert plans["skinny_split_ragged"] == (4, 80) and 300 - 3 * 80 == 60
    assert plans["skinny_split_52"] == (52, 80)
    assert plans["skinny_split_m1"] == (2, 80)
    assert plans["split_ragged"] == (2, 80) and 131 - 80 == 51
    assert plans["t64_for_split"] == (3, 80)
    tiles = {r.name: -(-r.M // 128) * -(-r.N // 128) * r.batch for r in bc.GEMM_ROWS}
    assert tiles["remap_on"] % 8 == 0 and tiles["remap_off"] % 8 != 0
    assert tiles["persistent"] % 8 == 0 and tiles["persistent_k33"] % 8 != 0
    assert all(tiles[n] > 512 for n in ("persistent", "persistent_k33", "persistent_k17", "persistent_interior"))
    assert set(bc.PARTIALS_ROWS) >= {"skinny_split_ragged", "split", "t64_for_split", "plain"}


@pytest.mark.parametrize("dt", bc.DTYPES)
@pytest.mark.parametrize("row", bc.GEMM_ROWS, ids=lambda r: r.name)
def test_numpy_product_passes_on_every_row(data, row, dt):
    d = data(row.name, dt)
    for alpha, beta in ((1.0, 0.0), (bc.ALPHA, bc.BETA)):
        want, bound = d.expect(alpha, beta, d.C)
        bc.check(_numpy_result(d, alpha, beta), want, bound, dt, row.name)
    # a shared (batch stride 0) operand
    if row.batch > 1:
        want, bound = d.expect(1.0, 0.0, share_a=True)
        bc.check(np.matmul(d.A[:1], d.B), want, bound, dt, row.name)
    # the operands come back unchanged from their NaN-padded parents, in every layout
    for trans in (False, True):
        for lay in (bc.ALIGNED, dict(ptr=1, pitch="aligned", bstride="aligned"), dict(ptr=0, pitch="odd", bstride="odd")):
            op = bc.embed(d.A, trans=trans, **lay)
            np.testing.assert_array_equal(op.view(), d.A)
            assert int(np.isnan(op.parent).sum()) == op.parent.size - d.A.size
            assert (op.s0 == 1) if trans else (op.s1 == 1)
            assert (op.off % bc.vec_elems(dt) == 0) == (lay["ptr"] == 0)


def _must_fail(got, want, bound, dt):
    with pytest.raises(AssertionError):
        bc.check(got, want, bound, dt, "mutation")


@pytest.mark.parametrize("dt", bc.DTYPES)
@pytest.mark.parametrize("name", ["skinny_short", "skinny_split_ragged", "skinny_split_52", "split_ragged", "t64_for_split", "persistent_k33", "s256"])
def test_mutations_of_a_correct_result_fail(data, name, dt):
    d = data(name, dt)
    row = d.row
    nb, M, N, K = row.shape
    T = d.dt.type
    good = _numpy_result(d, bc.ALPHA, bc.BETA)
    want, bound = d.expect(bc.ALPHA, bc.BETA, d.C)
    bc.check(good, want, bound, dt, name)
    b, i, j = nb - 1, M // 2, N // 2
    # one k term dropped from one element (the SMALLEST term of that element: the hardest to see)
    terms = d.A[b, i, :].astype(np.float64) * d.B[b, :, j].astype(np.float64)
    k = int(np.argmin(np.abs(terms)))
    if abs(terms[k]) * abs(bc.ALPHA) > 2 * float(bound[b, i, j]):
        bad = good.copy()
        bad[b, i, j] = T(bad[b, i, j] - T(bc.ALPHA) * T(terms[k]))
        _must_fail(bad, want, bound, dt)
    k = int(np.argmax(np.abs(terms)))
    bad = good.copy()
    bad[b, i, j] = T(bad[b, i, j] - T(bc.ALPHA) * T(terms[k]))
    _must_fail(bad, want, bound, dt)
    # one element taken from the neighbouring 16-wide tile column
    if N > 16:
        bad = good.copy()
        bad[b, i, j] = good[b, i, j - 16]
        _must_fail(bad, want, bound, dt)
    # one NaN pad value let into a sum
    bad = good.copy()
    bad[b, i, j] = bad[b, i, j] + T(np.nan)
    _must_fail(bad, want, bound, dt)
    # beta * C applied twice
    _must_fail(good + T(bc.BETA) * d.C, want, bound, dt)
    # a slab added twice
    nsplit, kchunk = bc.split_plan(*row.shape)
    slab = np.matmul(d.A[:, :, :min(kchunk, K)], d.B[:, :min(kchunk, K), :])
    _must_fail(good + T(bc.ALPHA) * slab, want, bound, dt)
    # K = 0 with beta = 0: anything but an exact zero fails
    z, zb = np.zeros((2, 3), dt), np.zeros((2, 3), bc.hp_type(dt))
    bc.check(z, zb, zb, dt)
    bc.check(-z, zb, zb, dt)
    z[1, 2] = np.finfo(dt).tiny
    _must_fail(z, zb, zb, dt)


@pytest.mark.parametrize("dt", bc.DTYPES)
def test_gemv_finish_and_ger_references(dt):
    T = np.dtype(dt).type
    for case in bc.GEMV_CASES:
        if case.only and case.only != dt:
            continue
        d = bc.gemv_data(case, dt)
        it = d.dt.itemsize
        Av = np.lib.stride_tricks.as_strided(d.a_parent[d.a_off:], (case.M, case.N), (d.sA0 * it, d.sA1 * it))
        np.testing.assert_array_equal(Av, d.A)
        assert {"row": d.sA1 == 1 or case.N == 1, "col": d.sA0 == 1, "gen": d.sA0 != 1 and d.sA1 != 1}[case.kind]
        if case.N:
            np.testing.assert_array_equal(d.x_parent[d.x_off + case.sx * np.arange(case.N)], d.x)
        assert int(np.isnan(d.x_parent).sum()) == d.x_parent.size - case.N
        want, bound = bc.gemv_expect(d.A, d.x, bc.ALPHA, bc.BETA, d.y, dt)
        good = T(bc.ALPHA) * (d.A @ d.x) + T(bc.BETA) * d.y
        bc.check(good, want, bound, dt, case.name)
        if case.N:
            bad = good.copy()
            bad[case.M // 2] -= T(bc.ALPHA) * d.A[case.M // 2, -1] * d.x[-1]  # the last column dropped
            if abs(float(d.A[case.M // 2, -1]) * float(d.x[-1])) * 0.75 > 2 * float(bound[case.M // 2]):
                _must_fail(bad, want, bound, dt)
        if np.any(np.abs(bc.BETA * d.y.astype(np.float64)) > 2 * bound):  # (the worst-case bound grows with N: 16400 columns hide one y)
            _must_fail(good + T(bc.BETA) * d.y, want, bound, dt)
    rng = np.random.default_rng(5)
    part = rng.standard_normal((65, 7)).astype(dt)
    y = rng.standard_normal(7).astype(dt)
    want, bound = bc.finish_expect(part, bc.ALPHA, bc.BETA, y, dt)
    good = T(bc.ALPHA) * part.sum(axis=0, dtype=dt) + T(bc.BETA) * y
    bc.check(good, want, bound, dt)
    _must_fail(good + T(bc.ALPHA) * part[64], want, bound, dt)
    A, x, yy = rng.standard_normal((5, 9)).astype(dt), rng.standard_normal(5).astype(dt), rng.standard_normal(9).astype(dt)
    want, bound = bc.ger_expect(A, x, yy, bc.ALPHA, dt)
    good = A + (T(bc.ALPHA) * x)[:, None] * yy[None, :]
    bc.check(good, want, bound, dt)
    _must_fail(A + (T(bc.ALPHA) * x)[:, None] * yy[None, ::-1], want, bound, dt)
    _must_fail(good * (1 + 8 * T(np.finfo(dt).eps)), want, bound, dt)
