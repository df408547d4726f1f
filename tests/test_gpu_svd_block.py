"""GPU: the whole-chip block Jacobi SVD (``pthip_svd_block``, csrc/eigh.hip) through its C ABI at the smallest shapes
that reach each of its paths, and through ``svd_device`` (``SVD``, ``MatrixPinv``, ``Lstsq``, ``Blockwise(SVD)``) with
``SVD_ROWS_MAX`` lowered, and once at the size from which the tier is routed to: 2049 x 2049.

The yardstick is NumPy in float64 on the host and the bars are the project's SVD bars
(``tests/test_gpu_svd_batched.py::check_svd``, restated in ``bars`` so that a reference can be shared), per item, with
tol = 1e-12 (float64) / 2e-5 (float32):

- ``max|s - s_ref| <= tol * s_ref[0]``;
- ``max|U diag(s) Vt - x| <= 50 tol max|x|``; ``U^T U`` and ``Vt Vt^T`` within ``50 tol`` of the identity.

The C-ABI factors of a wide x (r x c) are ``U = Pt^T``, ``Vt = Wt``.
"""
import ctypes

import numpy as np
import pytest

from pytensor_amd.dispatch import decomp
from test_gpu_svd_batched import TOL, check_pinv, cond2_stack, gaussian_stack, one_node

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def status_word(hip):
    w = ctypes.c_int(0)
    hip.check(hip.lib().pthip_check_status(ctypes.byref(w)))
    return w.value


def svd_block(hip, x, vectors, rows_out=None):
    """``pthip_svd_block`` on a stack x (batch, r, c), r <= c: (S, Wt, Pt, status word) on the host"""
    from pytensor_amd.device import DeviceArray

    nb, r, c = x.shape
    rows_out = r if rows_out is None else rows_out
    X = DeviceArray.from_host(np.ascontiguousarray(x))
    S = DeviceArray.empty((nb, r), x.dtype)
    Wt = DeviceArray.empty((nb, rows_out, c), x.dtype) if vectors else None
    Pt = DeviceArray.empty((nb, r, r), x.dtype) if vectors else None
    hip.check(hip.lib().pthip_svd_block(hip.np_dtype_code(x.dtype), nb, r, c, int(vectors), rows_out, X.ptr, S.ptr,
                                        Wt.ptr if vectors else None, Pt.ptr if vectors else None))
    word = status_word(hip)
    assert np.array_equal(X.to_host(), x, equal_nan=True), "the input is read, not destroyed"
    if not vectors:
        return S.to_host(), None, None, word
    return S.to_host(), Wt.to_host(), Pt.to_host(), word


def bars(x, U, s, Vt, dtype, what, s_ref=None):
    """the bars of the module docstring for every item of the stack x (batch, m, n); U (batch, m, k or m), Vt (batch,
    k or n, n) or both None"""
    nb, m, n = x.shape
    k = min(m, n)
    tol = TOL[dtype]
    x64 = x.astype("float64")
    if s_ref is None:
        s_ref = np.linalg.svd(x64, compute_uv=False)
    assert s.shape == (nb, k) and str(s.dtype) == dtype, (what, s.shape, s.dtype)
    smax = np.maximum(s_ref[:, 0], 1e-300)
    ratios = {"s": (np.abs(s.astype("float64") - s_ref).max(axis=1, initial=0.0) / (tol * smax)).max()}
    if U is not None:
        assert str(U.dtype) == dtype and str(Vt.dtype) == dtype
        U64, V64, s64 = U.astype("float64"), Vt.astype("float64"), s.astype("float64")
        rec = (U64[:, :, :k] * s64[:, None, :]) @ V64[:, :k, :]
        scale = np.maximum(np.abs(x64).reshape(nb, -1).max(axis=1), 1e-300)
        ratios["rec"] = (np.abs(rec - x64).reshape(nb, -1).max(axis=1) / (50 * tol * scale)).max()
        ratios["UtU"] = np.abs(U64.transpose(0, 2, 1) @ U64 - np.eye(U.shape[2])).max() / (50 * tol)
        ratios["VVt"] = np.abs(V64 @ V64.transpose(0, 2, 1) - np.eye(Vt.shape[1])).max() / (50 * tol)
    print(f"{what}: ratios to the bars {({k_: float(f'{v:.3e}') for k_, v in ratios.items()})}")
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


def abi_case(hip, x, dtype, what, rows_out=None):
    """vectors 0 and 1 on the stack x (batch, r, c): status 0, the bars, S of the two jobs within tol s_max"""
    nb, r, c = x.shape
    s_ref = np.linalg.svd(x.astype("float64"), compute_uv=False)
    s0, _, _, w0 = svd_block(hip, x, 0)
    assert w0 == 0, (what, w0)
    bars(x, None, s0, None, dtype, f"S {what}", s_ref)
    s1, Wt, Pt, w1 = svd_block(hip, x, 1, rows_out)
    assert w1 == 0, (what, w1)
    assert Wt.shape == (nb, r if rows_out is None else rows_out, c) and Pt.shape == (nb, r, r)
    bars(x, Pt.transpose(0, 2, 1), s1, Wt, dtype, f"factors {what}", s_ref)
    assert (np.diff(s1.astype("float64"), axis=1) <= 0).all(), what
    assert np.abs(s0.astype("float64") - s1).max() <= TOL[dtype] * max(s_ref.max(), 1e-300), what
    return s1, Wt, Pt


# (r, c): the smallest item; one pair padded / full; two pairs with 63 padding rows; no padding and a partial column
# chunk; three pairs (the first real tournament); three pairs with long rows; few rows, long rows
F64_SHAPES = [(1, 1), (33, 33), (64, 64), (65, 65), (128, 200), (129, 129), (192, 500), (70, 1000)]
F32_SHAPES = [(65, 65), (129, 300)]


@pytest.mark.parametrize("kind", ["cond2", "gauss"])
@pytest.mark.parametrize("r,c,dtype", [(r, c, "float64") for r, c in F64_SHAPES] + [(r, c, "float32") for r, c in F32_SHAPES])
def test_entry_parity(hip, r, c, dtype, kind):
    x = cond2_stack(r, c, 1, dtype) if kind == "cond2" else gaussian_stack(r, c, 1, dtype)
    abi_case(hip, np.array(x), dtype, f"{kind} {r}x{c} {dtype}")


@pytest.mark.parametrize("kind", ["cond2", "gauss"])
def test_batch_items_are_the_items_alone(hip, kind):
    x = np.array(cond2_stack(65, 65, 2, "float64") if kind == "cond2" else gaussian_stack(65, 65, 2, "float64"))
    whole = abi_case(hip, x, "float64", f"{kind} 65x65 batch=2")
    for vectors in (0, 1):
        both = svd_block(hip, x, vectors)
        for k in range(2):
            alone = svd_block(hip, x[k : k + 1], vectors)
            for a, b in zip(both[:3], alone[:3]):
                assert (a is None and b is None) or np.array_equal(a[k], b[0]), (kind, vectors, k)
    assert np.array_equal(whole[0], svd_block(hip, x, 1)[0])


@pytest.mark.parametrize("r,c", [(65, 130), (70, 200)])  # the completion's Eigh in the LDS kernel / in the block tier
@pytest.mark.parametrize("dtype", ["float64"])
def test_full_matrices(hip, r, c, dtype):
    x = gaussian_stack(r, c, 1, dtype)
    _, Wt, _ = abi_case(hip, x, dtype, f"full {r}x{c}", rows_out=c)  # (bars: all c rows of Wt orthonormal, the first r rebuild x)
    assert Wt.shape == (1, c, c)


def _orthonormal(a, tol, what):
    a = a.astype("float64")
    err = np.abs(a @ a.T - np.eye(a.shape[0])).max()
    print(f"{what}: orthonormality {err:.3e} (bar {50 * tol:.1e})")
    assert err <= 50 * tol, (what, err)


def test_rank_deficient_and_zero_inputs(hip):
    rng = np.random.default_rng(11)
    low = rng.standard_normal((129, 40)) @ rng.standard_normal((40, 200))
    holes = rng.standard_normal((100, 150))
    holes[[3, 64, 99], :] = 0.0
    holes[:, :10] = 0.0
    for what, x in (("rank 40 of 129", low), ("zero rows and columns", holes)):
        s, Wt, Pt = abi_case(hip, x[None], "float64", what)
        _orthonormal(Wt[0], 1e-12, f"Wt {what}")
        _orthonormal(Pt[0], 1e-12, f"Pt {what}")
    assert (s[0, -3:] == 0.0).all() and (s[0, :-3] > 0.0).all()  # the three zero rows: real rows, not padding
    z = np.zeros((1, 65, 70))
    for vectors in (0, 1):
        s, Wt, Pt, word = svd_block(hip, z, vectors)
        assert word == 0 and s.shape == (1, 65) and not s.any()
    _orthonormal(Wt[0], 1e-12, "Wt of zeros")
    _orthonormal(Pt[0], 1e-12, "Pt of zeros")


def test_graded_input_keeps_both_factors_orthonormal(hip):
    """the case that fails when the inner solver keeps its absolute threshold: rows 1e-10 of the largest are never
    orthogonalised against each other"""
    rng = np.random.default_rng(12)
    Q1 = np.linalg.qr(rng.standard_normal((96, 96)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((96, 96)))[0]
    sv = np.logspace(0, -12, 96)
    x = ((Q1 * sv) @ Q2)[None]
    s, Wt, Pt = abi_case(hip, x, "float64", "graded 96x96")
    np.testing.assert_allclose(s[0, :8], sv[:8], rtol=1e-8)
    _orthonormal(Wt[0], 1e-12, "Wt graded")
    _orthonormal(Pt[0], 1e-12, "Pt graded")


def _svd_exe(full, uv, nd=2, **kw):
    from pytensor_amd.executor import HipExecutable

    params = {"full_matrices": full, "compute_uv": uv}
    outs = [("float64", nd), ("float64", nd - 1), ("float64", nd)] if uv else [("float64", nd - 1)]
    if nd == 2:
        return HipExecutable(one_node("SVD", params, [("float64", 2)], outs), **kw)
    sig = "(m,n)->(m,k),(k),(k,n)" if uv else "(m,n)->(k)"
    return HipExecutable(one_node("Blockwise", {"core_op": "SVD", "core_params": params, "signature": sig}, [("float64", nd)], outs), **kw)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input(hip, monkeypatch, bad):
    x = np.array(gaussian_stack(65, 65, 1, "float64"))
    good = x.copy()
    x[0, 17, 40] = bad
    for vectors in (0, 1):
        s, Wt, Pt, word = svd_block(hip, x, vectors)
        assert word & 4, word
        assert np.isnan(s).all() and (not vectors or (np.isnan(Wt).all() and np.isnan(Pt).all()))
        assert hip.lib().pthip_svd_block_sweeps() == 0
    monkeypatch.setattr(decomp, "SVD_ROWS_MAX", 64)
    exe = _svd_exe(False, True)
    with pytest.raises(np.linalg.LinAlgError, match="SVD did not converge"):
        exe(x[0])
    U, s, Vt = exe(good[0])
    bars(good, U[None], s[None], Vt[None], "float64", "finite call after a non-finite one")
    assert svd_block(hip, good, 0)[3] == 0


@pytest.mark.parametrize("m,n", [(130, 70), (70, 130)])
def test_public_path_with_the_bound_lowered(hip, monkeypatch, m, n):
    from pytensor_amd.executor import HipExecutable

    monkeypatch.setattr(decomp, "SVD_ROWS_MAX", 64)
    assert decomp.svd_tier(m, n, 1) == "block"
    x = np.array(gaussian_stack(m, n, 1, "float64"))
    s_ref = np.linalg.svd(x, compute_uv=False)
    k = min(m, n)
    for full in (False, True):
        U, s, Vt = _svd_exe(full, True)(x[0])
        assert U.shape == ((m, m) if full else (m, k)) and Vt.shape == ((n, n) if full else (k, n))
        bars(x, U[None], s[None], Vt[None], "float64", f"SVD full={full} {m}x{n}", s_ref)
    (s,) = _svd_exe(False, False)(x[0])
    bars(x, None, s[None], None, "float64", f"SVD S alone {m}x{n}", s_ref)
    xc = np.array(cond2_stack(m, n, 1, "float64"))
    (X,) = HipExecutable(one_node("MatrixPinv", {"hermitian": False}, [("float64", 2)], [("float64", 2)]))(xc[0])
    check_pinv(xc, X[None], "float64", f"pinv {m}x{n}")
    # auto-freeze on, as under pytensor.function(mode="hip"): the tier reads the device every sweep, so the capture is
    # given up quietly, every call runs eagerly and the stream stays usable
    exe = _svd_exe(False, True, auto_freeze=True)
    for _ in range(3):
        U, s, Vt = exe(x[0])
        bars(x, U[None], s[None], Vt[None], "float64", f"repeated call {m}x{n}", s_ref)
    print(f"auto-freeze stats {exe.stats}")
    assert exe.stats["replays"] == 0, exe.stats
    exe = _svd_exe(False, True)
    for _ in range(3):
        U, s, Vt = exe(x[0])
    bars(x, U[None], s[None], Vt[None], "float64", f"repeated call, default executable {m}x{n}", s_ref)
    assert exe.stats["replays"] == 0


def test_public_lstsq_and_blockwise(hip, monkeypatch):
    from pytensor_amd.executor import HipExecutable

    monkeypatch.setattr(decomp, "SVD_ROWS_MAX", 64)
    rng = np.random.default_rng(13)
    a, b = rng.normal(size=(130, 70)), rng.normal(size=(130, 3))
    got = HipExecutable(_lstsq_graph())(a, b)
    want = np.linalg.lstsq(a, b, rcond=-1.0)
    for k, (u, v) in enumerate(zip(got, want)):
        assert np.shape(u) == np.shape(v), (k, np.shape(u), np.shape(v))
        np.testing.assert_allclose(u, v, rtol=1e-10, atol=1e-13, err_msg=f"lstsq out{k}")
    x = np.array(gaussian_stack(130, 70, 2, "float64"))
    U, s, Vt = _svd_exe(False, True, nd=3)(x)
    assert U.shape == (2, 130, 70) and Vt.shape == (2, 70, 70)
    bars(x, U, s, Vt, "float64", "Blockwise(SVD) 2x130x70")
    (s0,) = _svd_exe(False, False, nd=3)(x)
    bars(x, None, s0, None, "float64", "Blockwise(SVD) S alone 2x130x70")


def _lstsq_graph():
    from pytensor_amd.ir import Graph

    g = Graph(name="one_Lstsq")
    ins = [g.new_var("float64", (None, None)), g.new_var("float64", (None, None))]
    rc = np.asarray(-1.0)
    cs = [g.new_var(str(rc.dtype), rc.shape, const=rc)]
    outs = [g.new_var(dt, (None,) * nd) for dt, nd in [("float64", 2), ("float64", 1), ("int32", 0), ("float64", 1)]]
    g.add_node("Lstsq", {}, [*ins, *cs], outs)
    g.inputs, g.outputs = ins, outs
    return g


def test_the_bound_itself_2049(hip):
    """the only test at the workload's own size: below min(m, n) = 2049 nothing is routed to the tier without a patch"""
    n = 2049
    assert decomp.SVD_ROWS_MAX == 2048 and decomp.svd_tier(n, n, 1) == "block"
    x = np.random.default_rng(2049).standard_normal((1, n, n))
    s_ref = np.linalg.svd(x, compute_uv=False)
    (s,) = _svd_exe(False, False)(x[0])
    print(f"2049 x 2049 S alone: {hip.lib().pthip_svd_block_sweeps()} sweeps")
    bars(x, None, s[None], None, "float64", "2049x2049 S alone", s_ref)
    U, s, Vt = _svd_exe(False, True)(x[0])
    print(f"2049 x 2049 economic: {hip.lib().pthip_svd_block_sweeps()} sweeps")
    bars(x, U[None], s[None], Vt[None], "float64", "2049x2049 economic", s_ref)
