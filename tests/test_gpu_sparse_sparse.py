"""GPU: ``true_dot`` of two sparse operands under ``mode="hip"`` (csrc/spgemm.hip) against scipy on the host.

Integer-valued data make every product and sum exact, so structure and values are compared bit for bit with scipy's
``x @ y`` after ``sort_indices()`` (the device result is always sorted).  Standard-normal data are held to the bound
|got - want| <= (t + 1) u (|A| |B|)_ij around a long-double dense product, t the products on the entry and u the unit
roundoff: the running-sum bound gamma_t with a fused or an unfused multiply-add, derived, not measured.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import e2e_util as E
from pytensor_amd.dispatch.sparse import SPGEMM_PIECE, SPGEMM_WAVE_UB, SPGEMM_WG_UB

pytestmark = pytest.mark.gpu

FORMATS = [("csr", "csr"), ("csr", "csc"), ("csc", "csr"), ("csc", "csc")]


@pytest.fixture(scope="module")
def pt():
    pytensor = E.activate()
    if not E.have_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import pytensor.sparse as ps

    return pytensor, ps


@functools.lru_cache(maxsize=None)
def _true_dot(fx, fy, dt):
    import pytensor
    import pytensor.sparse as ps

    x, y = ps.matrix(fx, "x", dtype=dt), ps.matrix(fy, "y", dtype=dt)
    return pytensor.function([x, y], ps.true_dot(x, y), mode="hip")


def _same(got, want, what=""):
    want = want.copy()
    want.sort_indices()
    assert sp.issparse(got) and (got.format, got.shape, got.dtype) == (want.format, want.shape, want.dtype), f"{what}: {got!r} vs {want!r}"
    for attr in ("indptr", "indices", "data"):
        np.testing.assert_array_equal(getattr(got, attr), getattr(want, attr), err_msg=f"{what}: {attr}")


def _designed(a, ub, n, dt, normal=False):
    """A (6 x a) whose row 0 has ``a`` entries and meets exactly ``ub`` entries of B (a x n); row 1 of A and column 2
    of B are empty, the other rows of A are short (the wave tier runs next to whatever tier row 0 is in).  Indices are
    unsorted.  Data: small non-zero integers, or standard normal."""
    rng = np.random.default_rng(a + ub)
    val = rng.standard_normal if normal else (lambda k: rng.integers(1, 4, k) * rng.choice([-1, 1], k))
    lens = ub // a + (np.arange(a) < ub % a)
    free = np.delete(np.arange(n), 2)
    b_ind = np.concatenate([rng.choice(free, k, replace=False) for k in lens])
    B = sp.csr_matrix((val(ub).astype(dt), b_ind.astype(np.int32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)), shape=(a, n))
    a_ind = np.concatenate([rng.permutation(a), *[rng.choice(a, 3, replace=False) for _ in range(4)]])
    A = sp.csr_matrix((val(a + 12).astype(dt), a_ind.astype(np.int32), np.array([0, a, a, a + 3, a + 6, a + 9, a + 12], np.int32)), shape=(6, a))
    return A, B


# (entries of A's row 0, its products, columns of B): both sides of every tier bound and of a chunk, and A rows longer
# than the LDS prefix array of the wave, workgroup and dense-row tiers
DESIGNED = {
    "chunk": (8, 64, 50), "chunk+1": (8, 65, 50),
    "wave_ub": (32, SPGEMM_WAVE_UB, 300), "wave_ub+1": (32, SPGEMM_WAVE_UB + 1, 300),
    "wg_ub": (32, SPGEMM_WG_UB, 2000), "wg_ub+1": (32, SPGEMM_WG_UB + 1, 2000),
    "wave_pieces": (SPGEMM_PIECE["wave"] + 36, 200, 40),
    "wg_pieces": (SPGEMM_PIECE["workgroup"] + 44, 3000, 500),
    "dense_pieces": (SPGEMM_PIECE["workgroup"] + 44, 6000, 700),
}
SMALL = {
    "nnz0": lambda dt: (sp.csr_matrix((5, 4), dtype=dt), sp.csr_matrix(np.arange(24, dtype=dt).reshape(4, 6))),
    "rows0": lambda dt: (sp.csr_matrix((0, 4), dtype=dt), sp.csr_matrix(np.arange(24, dtype=dt).reshape(4, 6))),
    "cancellation": lambda dt: (sp.csr_matrix(np.array([[1, 1]], dt)), sp.csr_matrix(np.array([[1, 3], [-1, 0]], dt))),
    "nan": lambda dt: (sp.csr_matrix(np.array([[1, 2], [0, 3]], dt)), sp.csr_matrix(np.array([[np.nan, 1], [1, 0]], dt))),
}


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("fx,fy", FORMATS)
@pytest.mark.parametrize("case", [*DESIGNED, *SMALL])
def test_exact_against_scipy(pt, case, fx, fy, dt):
    A, B = _designed(*DESIGNED[case], dt) if case in DESIGNED else SMALL[case](dt)
    if case in DESIGNED:
        assert (abs(A[0]) @ abs(B)).sum() > 0 and np.diff(B.indptr)[A[0].indices].sum() == DESIGNED[case][1]
    A, B = A.asformat(fx), B.asformat(fy)
    want = A @ B
    if case == "cancellation":
        assert want.nnz == 1  # (the structural entry (0, 0) sums to exactly 0 and must vanish)
    _same(_true_dot(fx, fy, dt)(A, B), want, case)


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("fx,fy,second", [("csr", "csr", "Y"), ("csc", "csc", "Y"), ("csr", "csc", "X"), ("csc", "csr", "X")])
def test_unsorted_indices_and_duplicates(pt, fx, fy, second, dt):
    pytensor, ps = pt
    import pytensor.sparse.basic as sb
    import pytensor.tensor as ptt

    # X: 4 x 5 as csr (5 x 4 as csc), major 1 empty, (0, 3) stored twice; Y: 5 x 4 as csr (4 x 5 as csc), major 2 empty,
    # (0, 2) and (3, 1) stored twice; both unsorted
    X = (np.array([1, -2, 3, 2, 7, -1, 2], dt), np.array([3, 0, 3, 1, 0, 4, 2], np.int32), np.array([0, 3, 3, 5, 7], np.int32), (4, 5))
    Y = (np.array([2, 1, -3, 4, 1, 5, -2, 3], dt), np.array([2, 0, 2, 3, 1, 1, 0, 3], np.int32), np.array([0, 3, 4, 4, 6, 8], np.int32), (5, 4))
    ins, mats, host = [], [], []
    for fmt, (data, ind, ptr, shape) in ((fx, X), (fy, Y if second == "Y" else X)):
        shape = shape if fmt == "csr" else shape[::-1]
        d, i, p, s = ptt.vector(dtype=dt), ptt.ivector(), ptt.ivector(), ptt.ivector()
        ins += [d, i, p, s]
        mats.append(sb.CSM(fmt)(d, i, p, s))
        host.append((sp.csr_matrix if fmt == "csr" else sp.csc_matrix)((data, ind, ptr), shape=shape))
    vals = [v for m in host for v in (m.data, m.indices, m.indptr, np.array(m.shape, np.int32))]
    got = pytensor.function(ins, ps.true_dot(*mats), mode="hip")(*vals)
    np.testing.assert_array_equal(got.toarray(), (host[0] @ host[1]).toarray())
    for r in range(len(got.indptr) - 1):
        assert np.all(np.diff(got.indices[got.indptr[r]:got.indptr[r + 1]]) > 0), f"major {r}"


ROUNDED = {"wave": (32, 200, 300), "workgroup": (32, 2000, 1500), "dense_row": (32, 6000, 2500)}


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("tier", list(ROUNDED))
def test_rounded_within_the_running_sum_bound(pt, tier, dt):
    A, B = _designed(*ROUNDED[tier], dt, normal=True)
    f = _true_dot("csr", "csr", dt)
    got, again = f(A, B), f(A, B)
    for attr in ("indptr", "indices", "data"):  # two calls: identical bytes
        assert getattr(got, attr).tobytes() == getattr(again, attr).tobytes(), attr
    want = A @ B
    want.sort_indices()
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    Ad, Bd = A.toarray().astype(np.longdouble), B.toarray().astype(np.longdouble)
    rows = np.repeat(np.arange(got.shape[0]), np.diff(got.indptr))
    t = ((Ad != 0).astype(np.int64) @ (Bd != 0).astype(np.int64))[rows, got.indices]
    assert t.min() >= 1 and t.max() > 1  # (no structural entry was dropped for these seeds, and sums do occur)
    u = np.longdouble(np.finfo(dt).eps) / 2
    err = np.abs(got.data.astype(np.longdouble) - (Ad @ Bd)[rows, got.indices])
    bound = (t + 1) * u * (np.abs(Ad) @ np.abs(Bd))[rows, got.indices]
    assert np.all(err <= bound), f"worst error / bound = {np.max(err / bound)}"


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_the_two_products_of_the_pullback(pt, dt):
    pytensor, ps = pt
    A, B = _designed(32, 300, 200, dt)  # x: 6 x 32, y: 32 x 200
    G = (A @ B).astype(dt)  # a gradient with the structure of the result: integer-valued
    x, y, gz = ps.csr_matrix("x", dtype=dt), ps.csr_matrix("y", dtype=dt), ps.csr_matrix("gz", dtype=dt)
    f = pytensor.function([x, y, gz], [ps.true_dot(gz, ps.transpose(y)), ps.true_dot(ps.transpose(x), gz)], mode="hip")
    gx, gy = f(A, B, G)
    _same(gx, G @ B.T.tocsc(), "gz y^T")
    _same(gy, A.T.tocsc() @ G, "x^T gz")


def test_column_index_of_a_out_of_range(pt):
    pytensor, ps = pt
    import pytensor.sparse.basic as sb
    import pytensor.tensor as ptt

    d, i, p, s = ptt.dvector(), ptt.ivector(), ptt.ivector(), ptt.ivector()
    y = ps.csr_matrix("y", dtype="float64")
    f = pytensor.function([d, i, p, s, y], ps.true_dot(sb.CSM("csr")(d, i, p, s), y), mode="hip")
    B = sp.csr_matrix(np.arange(1.0, 13.0).reshape(3, 4))
    args = [np.array([1.0, 2.0]), None, np.array([0, 1, 2], np.int32), np.array([2, 3], np.int32), B]
    args[1] = np.array([0, 3], np.int32)  # 3 >= k = 3
    with pytest.raises(IndexError):
        f(*args)
    args[1] = np.array([0, 2], np.int32)
    _same(f(*args), sp.csr_matrix(([1.0, 2.0], [0, 2], [0, 1, 2]), shape=(2, 3)) @ B, "after the error")
