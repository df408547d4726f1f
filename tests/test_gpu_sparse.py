"""GPU: pytensor.sparse csr / csc under ``mode="hip"`` against the reference's C linker (``FAST_RUN`` under the CVM,
with its C sparse ops) on the same inputs.

Structural ops and gathers are bit-exact (data, indices and indptr); products and sums are held to the tolerances
below, which belong to this file, norm-wise: |got - want| <= rtol * (|want| + max|want|) — the summation order differs
from the reference's, so an element where terms cancel is only as exact as the largest one.  The structured unaries
apply the generated Elemwise to ``data`` and share its tolerances (e2e_util.assert_close).  Inputs cover empty rows and columns, nnz = 0, a 0 x n matrix, one row of 1e5
entries, unsorted indices and duplicate entries (built through ``CSM``), and k in {1, 3, 8, 64}.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import e2e_util as E

pytestmark = pytest.mark.gpu

RTOL = {"float64": 1e-12, "float32": 1e-5}


@pytest.fixture(scope="module")
def pt():
    pytensor = E.activate()
    if not E.have_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import pytensor.sparse as ps
    import pytensor.tensor as ptt

    return pytensor, ptt, ps


def _fns(pytensor, ins, outs):
    f_hip = pytensor.function(ins, outs, mode="hip", on_unused_input="ignore")
    f_ref = pytensor.function(ins, outs, mode=E.reference_mode(), on_unused_input="ignore")
    return f_hip, f_ref


def _same(got, want, what, rtol=None):
    """sparse: format, shape and the three arrays; exact unless rtol is given (then data to rtol, structure exact)"""
    if sp.issparse(want):
        assert sp.issparse(got) and got.format == want.format and got.shape == want.shape, f"{what}: {got!r} vs {want!r}"
        np.testing.assert_array_equal(got.indptr, want.indptr, err_msg=what)
        np.testing.assert_array_equal(got.indices, want.indices, err_msg=what)
        assert got.data.dtype == want.data.dtype, what
        if rtol is None:
            np.testing.assert_array_equal(got.data, want.data, err_msg=what)
        else:
            _close(got.data, want.data, what, rtol)
        return
    if rtol is None:
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == want.dtype and got.shape == want.shape, what
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        _close(np.asarray(got), want, what, rtol)


def _close(got, want, what, rtol):
    want = np.asarray(want)
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    E.assert_close(got, want, what, rtol=rtol, atol=rtol * scale)


def _check(pytensor, ins, outs, vals, rtol=None, calls=2):
    f_hip, f_ref = _fns(pytensor, ins, outs)
    want = f_ref(*vals)
    for c in range(calls):
        got = f_hip(*vals)
        for k, (a, b) in enumerate(zip(got, want)):
            _same(a, b, f"output {k}, call {c}", rtol)
    return f_hip


def _rand(m, n, density, fmt, dt, seed):
    rng = np.random.default_rng(seed)
    a = sp.random(m, n, density=density, format="csr", random_state=rng, dtype=np.float64)
    if m > 2:
        a = a.tolil()
        a[1, :] = 0  # an empty row
        a = a.tocsr()
    if n > 3:
        a = a.tocsc()
        a[:, 2] = 0  # an empty column
    a = a.asformat(fmt)
    a.eliminate_zeros()
    return a.astype(dt)


def _messy(fmt, dt):
    """unsorted indices, a duplicate entry, an empty row (and column), built the way CSM takes them"""
    data = np.array([1.5, -2.0, 3.25, 0.5, 7.0, -1.0, 2.5], dtype=dt)
    indices = np.array([3, 0, 3, 1, 0, 4, 2], dtype=np.int32)
    indptr = np.array([0, 3, 3, 5, 7], dtype=np.int32)  # major 1 is empty; (0, 3) is stored twice
    shape = np.array([4, 5] if fmt == "csr" else [5, 4], dtype=np.int32)
    return data, indices, indptr, shape


MATS = {
    "random": lambda fmt, dt: _rand(37, 29, 0.15, fmt, dt, 1),
    "nnz0": lambda fmt, dt: sp.csr_matrix((6, 5), dtype=dt).asformat(fmt),
    "rows0": lambda fmt, dt: sp.csr_matrix((0, 7), dtype=dt).asformat(fmt),
}


def _one_long_row(fmt, dt):
    rng = np.random.default_rng(7)
    n = 120_000
    cols = np.sort(rng.choice(n, 100_000, replace=False)).astype(np.int32)
    a = sp.csr_matrix((rng.standard_normal(cols.size).astype(dt), cols, np.array([0, 0, cols.size, cols.size, cols.size], np.int32)),
                      shape=(4, n))
    return a.asformat(fmt)


# ---------------------------------------------------------------------------------------------------------------
# structural ops and gathers: bit-exact
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("mat", list(MATS))
def test_structural_ops_bit_exact(pt, mat, fmt, dt):
    pytensor, ptt, ps = pt
    import pytensor.sparse.basic as sb
    import pytensor.sparse.math as sm

    A = MATS[mat](fmt, dt)
    m, n = A.shape
    x = ps.matrix(fmt, "x", dtype=dt)
    b = ptt.matrix("b", dtype=dt)
    vc, vr = ptt.vector("vc", dtype=dt), ptt.vector("vr", dtype=dt)
    rng = np.random.default_rng(3)
    B = rng.standard_normal((m, n)).astype(dt)
    B[:1, :] = 0  # (a zero row: SparseFromDense drops it)
    VC, VR = rng.standard_normal(n).astype(dt), rng.standard_normal(m).astype(dt)
    other = "float32" if dt == "float64" else "float64"
    outs = [ps.transpose(x), ps.dense_from_sparse(x), sb.SparseFromDense(fmt)(b), sb.cast(x, other),
            sm.mul_s_d(x, b), sm.mul_s_v(x, vc), sm.structured_add_s_v(x, vc), sm.add_s_d(x, b), *sb.csm_properties(x)[:3]]
    if fmt == "csc":
        outs += [sb.ColScaleCSC()(x, vc), sb.RowScaleCSC()(x, vr)]
    _check(pytensor, [x, b, vc, vr], outs, [A, B, VC, VR])
    # the structured unary: the structure exactly, the data within the Elemwise tolerances
    f_hip, f_ref = _fns(pytensor, [x], [ps.structured_exp(x)])
    (got,), (want,) = f_hip(A), f_ref(A)
    assert got.format == want.format
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.indptr, want.indptr)
    E.assert_close(got.data, want.data, "structured_exp")


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_unsorted_duplicates_through_csm(pt, fmt, dt):
    pytensor, ptt, ps = pt
    import pytensor.sparse.basic as sb
    import pytensor.sparse.math as sm

    d, i, p, s = ptt.vector("d", dtype=dt), ptt.ivector("i"), ptt.ivector("p"), ptt.ivector("s")
    x = sb.CSM(fmt)(d, i, p, s)
    b = ptt.matrix("b", dtype=dt)
    vals = _messy(fmt, dt)
    m, n = int(vals[3][0]), int(vals[3][1])
    B = np.random.default_rng(0).standard_normal((m, n)).astype(dt)
    Bk = np.random.default_rng(1).standard_normal((n, 3)).astype(dt)
    bk = ptt.matrix("bk", dtype=dt)
    # structure-preserving: the caller's arrays come back exactly
    _check(pytensor, [d, i, p, s, b], [x, ps.transpose(x), sm.mul_s_d(x, b)], [*vals, B])
    # duplicates are summed, as toarray() sums them
    _check(pytensor, [d, i, p, s, b], [ps.dense_from_sparse(x)], [*vals, B])
    # AddSD: the reference's Python perform (scipy x + y) sums duplicates; its C AddSD_ccode, which FAST_RUN picks,
    # keeps the last one.  The hip linker sums them, consistently with DenseFromSparse: compared with scipy here.
    f = pytensor.function([d, i, p, s, b], sm.add_s_d(x, b), mode="hip")
    cls = sp.csr_matrix if fmt == "csr" else sp.csc_matrix
    want = cls(vals[:3], shape=tuple(vals[3])) + B
    np.testing.assert_array_equal(f(*vals, B), np.asarray(want))
    _check(pytensor, [d, i, p, s, bk], [ps.structured_dot(x, bk), sm.sp_sum(x, 0), sm.sp_sum(x, 1), sm.sp_sum(x)],
           [*vals, Bk], rtol=RTOL[dt])
    g = pytensor.grad((ps.structured_dot(x, bk) ** 2).sum(), d)
    _check(pytensor, [d, i, p, s, bk], [g], [*vals, Bk], rtol=RTOL[dt])


# ---------------------------------------------------------------------------------------------------------------
# products and sums
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("mat", [*MATS, "long_row"])
def test_products_and_sums(pt, mat, fmt, dt):
    pytensor, ptt, ps = pt
    import pytensor.sparse.math as sm

    A = _one_long_row(fmt, dt) if mat == "long_row" else MATS[mat](fmt, dt)
    m, n = A.shape
    x = ps.matrix(fmt, "x", dtype=dt)
    rng = np.random.default_rng(5)
    for k in (1, 3, 8, 64):
        if mat == "long_row" and k == 64:
            continue  # (k = 8 already runs the long-row pass with packed B rows)
        b, c, y = ptt.matrix("b", dtype=dt), ptt.matrix("c", dtype=dt), ptt.matrix("y", dtype=dt)
        B = rng.standard_normal((n, k)).astype(dt)
        C = rng.standard_normal((k, m)).astype(dt)
        Y = rng.standard_normal((m, k)).astype(dt)
        outs = [ps.structured_dot(x, b), sm.dot(x, b), sm.dot(c, x), sm.sampling_dot(y, b, x)]
        _check(pytensor, [x, b, c, y], outs, [A, B, C, Y], rtol=RTOL[dt])
    v = ptt.vector("v", dtype=dt)
    V = rng.standard_normal(m).astype(dt)
    _check(pytensor, [x, v], [sm.sp_sum(x), sm.sp_sum(x, 0), sm.sp_sum(x, 1), sm.dot(v, x)], [A, V], rtol=RTOL[dt])
    b = ptt.matrix("b", dtype=dt)
    _check(pytensor, [x, b], [sm.true_dot(x, b)], [A, rng.standard_normal((n, 2)).astype(dt)], rtol=RTOL[dt])


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_gradients(pt, fmt):
    pytensor, ptt, ps = pt
    import pytensor.sparse.basic as sb
    import pytensor.sparse.math as sm

    dt = "float64"
    A = _rand(31, 23, 0.2, fmt, dt, 11)
    m, n = A.shape
    x = ps.matrix(fmt, "x", dtype=dt)
    b = ptt.dmatrix("b")
    c = ptt.dmatrix("c")
    rng = np.random.default_rng(2)
    B, C = rng.standard_normal((n, 4)), rng.standard_normal((4, m))
    cost = (ps.structured_dot(x, b) ** 2).sum() + (sm.dot(c, x) ** 2).sum() + (sm.sp_sum(x, 0) ** 2).sum()
    gx, gb, gc = pytensor.grad(cost, [x, b, c])
    _check(pytensor, [x, b, c], [gx, gb, gc], [A, B, C], rtol=1e-12)
    for sparse_grad in (True, False):
        for axis in (None, 0, 1):
            g = pytensor.grad((sm.sp_sum(x, axis, sparse_grad=sparse_grad) ** 2).sum(), x)
            _check(pytensor, [x], [g], [A], rtol=1e-12)
    d, i, p, s = ptt.dvector("d"), ptt.ivector("i"), ptt.ivector("p"), ptt.ivector("s")
    M = sb.CSM(fmt)(d, i, p, s)
    gd = pytensor.grad((ps.structured_dot(M, b) ** 2).sum(), d)
    _check(pytensor, [d, i, p, s, b], [gd], [A.data, A.indices, A.indptr, np.array(A.shape, np.int32), B], rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------
# CAR logp + grad, as PyMC writes it: sparse constant W
# ---------------------------------------------------------------------------------------------------------------

def _grid_adjacency(r, c):
    n = r * c
    idx = np.arange(n).reshape(r, c)
    rows = np.concatenate([idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()])
    cols = np.concatenate([idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()])
    return sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))


def _car(pytensor, ptt, ps, W, eigen):
    import pytensor.sparse.math as sm

    Wc = ps.as_sparse_variable(W)
    phi, tau, alpha = ptt.dvector("phi"), ptt.dscalar("tau"), ptt.dscalar("alpha")
    D = sm.sp_sum(Wc, axis=0)  # (PyMC CAR.logp)
    Wphi = ps.structured_dot(Wc, phi[:, None])[:, 0]
    delta = phi * D - alpha * Wphi
    logp = 0.5 * phi.shape[0] * ptt.log(tau) - 0.5 * tau * (phi * delta).sum()
    logp = logp + 0.25 * tau * ps.dot(delta[None, :], Wc)[0].dot(phi) / phi.shape[0]
    if eigen:
        Dm = ps.dense_from_sparse(Wc).sum(axis=0)
        dinv = 1.0 / ptt.sqrt(Dm)
        DWD = dinv[:, None] * ps.dense_from_sparse(Wc) * dinv[None, :]
        lam = ptt.linalg.eigvalsh(DWD, ptt.eye(phi.shape[0]))
        logp = logp + 0.5 * ptt.log1p(-alpha * lam).sum()
    return [phi, tau, alpha], [logp, *pytensor.grad(logp, [phi, tau, alpha])]


def test_car_small_with_eigen_term(pt):
    pytensor, ptt, ps = pt
    W = _grid_adjacency(20, 20)
    ins, outs = _car(pytensor, ptt, ps, W, eigen=True)
    phi = np.random.default_rng(0).standard_normal(400)
    # (eager: the generalised Eigvalsh synchronises the stream mid-graph, which a hipGraph capture cannot hold)
    with pytensor.config.change_flags(hip__auto_freeze=False):
        f = _check(pytensor, ins, outs, [phi, 1.7, 0.6], rtol=1e-9, calls=3)
    assert "HostPerform" not in [n.op for n in f.maker.linker.last_ir.nodes]


def test_car_million_freezes_and_replays(pt):
    pytensor, ptt, ps = pt
    W = _grid_adjacency(1000, 1000)
    ins, outs = _car(pytensor, ptt, ps, W, eigen=False)
    phi = np.random.default_rng(1).standard_normal(W.shape[0])
    f = _check(pytensor, ins, outs, [phi, 1.3, 0.9], rtol=1e-9, calls=3)
    exe = E.hip_executable(f)
    assert exe._auto_plan is not None and exe.stats["replays"] >= 1, exe.stats
    assert not exe.has_sparse_io
    # W is a constant: uploaded once, its transpose (if any kernel needed it) built once and kept with it
    consts = [v for v in exe._const_cache.values() if type(v).__name__ == "DeviceSparse"]
    assert consts and all(c.data.buf.ptr for c in consts)


# ---------------------------------------------------------------------------------------------------------------
# determinism and sparse inputs
# ---------------------------------------------------------------------------------------------------------------

def _transpose_on_device(A):
    """pthip_csr_transpose of a scipy csr matrix: the csc arrays of the same matrix"""
    from pytensor_amd import ffi
    from pytensor_amd.device import DeviceArray

    m, n = A.shape
    d, i, p = (DeviceArray.from_host(np.ascontiguousarray(a)) for a in (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)))
    od, oi, op = DeviceArray.empty((A.nnz,), A.dtype), DeviceArray.empty((A.nnz,), "int32"), DeviceArray.empty((n + 1,), "int32")
    ffi.check(ffi.lib().pthip_csr_transpose(ffi.np_dtype_code(A.dtype), m, n, A.nnz, d.ptr, i.ptr, p.ptr, od.ptr, oi.ptr, op.ptr))
    return od.to_host(), oi.to_host(), op.to_host()


def test_bit_reproducible(pt):
    pytensor, ptt, ps = pt
    import pytensor.sparse.math as sm

    rng = np.random.default_rng(4)
    n = 1_000_000
    A = sp.random(n, n, density=8 / n, format="csr", random_state=rng)
    x = ps.csr_matrix("x", dtype="float64")
    v, g, b = ptt.dvector("v"), ptt.dmatrix("g"), ptt.dmatrix("b")
    V = rng.standard_normal(n)
    G, B = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    # SpMV, SpMV through the transpose (dense x sparse), SDDMM
    f = pytensor.function([x, v, g, b], [sm.dot(x, v), sm.dot(v, x), sm.sampling_dot(g, b, x)], mode="hip")
    r1, r2 = f(A, V, G, B), f(A, V, G, B)
    np.testing.assert_array_equal(r1[0], r2[0])
    np.testing.assert_array_equal(r1[1], r2[1])
    for attr in ("data", "indices", "indptr"):
        np.testing.assert_array_equal(getattr(r1[2], attr), getattr(r2[2], attr))
    _close(r1[0], A @ V, "SpMV", 1e-12)
    _close(r1[1], A.T @ V, "SpMV through the transpose", 1e-12)
    # the transpose itself: twice bit-identical, and scipy's tocsc() ordering for sorted input
    t1, t2 = _transpose_on_device(A), _transpose_on_device(A)
    want = A.tocsc()
    for a, c, w in zip(t1, t2, (want.data, want.indices, want.indptr)):
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(a, w)


def test_sparse_inputs_with_changing_nnz_stay_eager(pt):
    pytensor, ptt, ps = pt
    x = ps.csr_matrix("x", dtype="float64")
    b = ptt.dmatrix("b")
    f = pytensor.function([x, b], ps.structured_dot(x, b), mode="hip")
    exe = E.hip_executable(f)
    assert exe.has_sparse_io and not exe.auto_freeze  # documented: sparse inputs keep the graph eager
    B = np.random.default_rng(0).standard_normal((50, 4))
    for k, dens in enumerate((0.05, 0.2, 0.05, 0.0, 0.5)):
        A = sp.random(40, 50, density=dens, format="csr", random_state=k)
        _close(f(A, B), A @ B, f"call {k}", 1e-12)
    assert exe._auto_plan is None and exe.stats["replays"] == 0
