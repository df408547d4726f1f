"""GPU: ``Blockwise(SVD)``, ``Blockwise(MatrixPinv)`` and ``Blockwise(QR)`` over a whole stack — the one-launch Jacobi
tier (csrc/svd_batched.hip through ``dispatch/decomp.py::svd_tier``) and the batched kernels above it.

The yardstick is NumPy in float64 on the host.  The bars are those of ``tests/test_gpu_decomp.py::_check_svd``, per item,
with tol = 1e-12 (float64) / 2e-5 (float32):

- ``max|s - s_ref| <= tol * s_ref[0]`` (relative to the largest singular value: LAPACK's own small singular values are
  only accurate to eps * s_max);
- ``max|U diag(s) Vt - x| <= 50 tol max|x|``; ``U^T U`` and ``Vt Vt^T`` within ``50 tol`` of the identity;
- pinv: ``max|X - pinv_ref| <= tol max|pinv_ref|`` with tol = 1e-12 / 1e-5 on inputs of cond <= 2.01.

The parity inputs ``Q1[:, :k] diag(linspace(1, 2, k)) Q2[:k, :]`` have cond <= 2.01, which the tests assert from NumPy
and never repair; Gaussian stacks are used as well for the SVD bars, none of which depends on the condition number.
"""
import numpy as np
import pytest

from pytensor_amd.dispatch.decomp import SVD_WAVE_MAX, svd_tier
from pytensor_amd.ir import Graph

pytestmark = pytest.mark.gpu

TOL = {"float64": 1e-12, "float32": 2e-5}
PINV_TOL = {"float64": 1e-12, "float32": 1e-5}


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


def _blockwise(core, cp, sig, dtype, nd, out_nds):
    from pytensor_amd.executor import HipExecutable

    return HipExecutable(one_node("Blockwise", {"core_op": core, "core_params": cp, "signature": sig}, [(dtype, nd)], [(dtype, k) for k in out_nds]))


def svd_exe(dtype, nd, job):
    """job as in csrc/svd_batched.hip: 0 = S alone, 1 = economic, 2 = full"""
    if job == 0:
        return _blockwise("SVD", {"full_matrices": False, "compute_uv": False}, "(m,n)->(k)", dtype, nd, [nd - 1])
    return _blockwise("SVD", {"full_matrices": job == 2, "compute_uv": True}, "(m,n)->(m,k),(k),(k,n)", dtype, nd, [nd, nd - 1, nd])


def pinv_exe(dtype, nd):
    return _blockwise("MatrixPinv", {"hermitian": False}, "(m,n)->(n,m)", dtype, nd, [nd])


QR_OUTS = {"economic": 2, "full": 2, "r": 1, "raw": 3}


def qr_exe(dtype, nd, mode):
    from pytensor_amd.executor import HipExecutable

    outs = {"economic": [nd, nd], "full": [nd, nd], "r": [nd], "raw": [nd, nd - 1, nd]}[mode]
    if nd == 2:
        return HipExecutable(one_node("QR", {"mode": mode, "pivoting": False}, [(dtype, 2)], [(dtype, k) for k in outs]))
    return _blockwise("QR", {"mode": mode, "pivoting": False}, "(m,n)->(m,k),(k,n)", dtype, nd, outs)


_STACKS = {}


def cond2_stack(m, n, batch, dtype, seed=0):
    """x = Q1[:, :k] diag(linspace(1, 2, k)) Q2[:k, :]; cond <= 2.01 is asserted, never repaired.  Computed once per
    key and handed out read-only."""
    key = (m, n, batch, dtype, seed)
    if key not in _STACKS:
        rng = np.random.default_rng(1000 * m + 10 * n + seed)
        k = min(m, n)
        Q1 = np.linalg.qr(rng.standard_normal((batch, m, m)))[0]
        Q2 = np.linalg.qr(rng.standard_normal((batch, n, n)))[0]
        x = ((Q1[:, :, :k] * np.linspace(1.0, 2.0, k)) @ Q2[:, :k, :]).astype(dtype)
        s = np.linalg.svd(x.astype("float64"), compute_uv=False)
        assert (s[:, 0] / s[:, -1]).max() <= 2.01, key
        x.setflags(write=False)
        _STACKS[key] = x
    return _STACKS[key]


def gaussian_stack(m, n, batch, dtype, seed=0):
    x = np.random.default_rng(77 + 1000 * m + 10 * n + seed).standard_normal((batch, m, n)).astype(dtype)
    return x


def report(what, ratios):
    print(f"{what}: worst ratio to the bar = {np.nanmax(ratios) if len(ratios) else 0.0:.3e}")


def check_svd(x, U, s, Vt, full, dtype, what):
    """the bars of the module docstring for every item of the stack x (batch, m, n)"""
    nb, m, n = x.shape
    k = min(m, n)
    tol = TOL[dtype]
    x64 = x.astype("float64")
    s_ref = np.linalg.svd(x64, compute_uv=False)
    assert s.shape == (nb, k) and str(s.dtype) == dtype, (what, s.shape, s.dtype)
    smax = np.maximum(s_ref[:, :1], 1e-300)
    r_s = np.abs(s.astype("float64") - s_ref).max(axis=1, initial=0.0) / (tol * smax[:, 0])
    ratios = [r_s.max(initial=0.0)]
    if U is not None:
        assert U.shape == ((nb, m, m) if full else (nb, m, k)) and Vt.shape == ((nb, n, n) if full else (nb, k, n)), (what, U.shape, Vt.shape)
        assert str(U.dtype) == dtype and str(Vt.dtype) == dtype
        U64, V64, s64 = U.astype("float64"), Vt.astype("float64"), s.astype("float64")
        rec = (U64[:, :, :k] * s64[:, None, :]) @ V64[:, :k, :]
        scale = np.maximum(np.abs(x64).reshape(nb, -1).max(axis=1), 1e-300)
        ratios.append((np.abs(rec - x64).reshape(nb, -1).max(axis=1) / (50 * tol * scale)).max())
        ratios.append(np.abs(U64.transpose(0, 2, 1) @ U64 - np.eye(U.shape[2])).max() / (50 * tol))
        ratios.append(np.abs(V64 @ V64.transpose(0, 2, 1) - np.eye(Vt.shape[1])).max() / (50 * tol))
    report(what, ratios)
    assert all(r <= 1.0 for r in ratios), (what, ratios)


def check_pinv(x, X, dtype, what):
    nb, m, n = x.shape
    ref = np.linalg.pinv(x.astype("float64"))
    assert X.shape == (nb, n, m) and str(X.dtype) == dtype, (what, X.shape, X.dtype)
    err = np.abs(X.astype("float64") - ref).reshape(nb, -1).max(axis=1)
    scale = np.abs(ref).reshape(nb, -1).max(axis=1)
    ok = err <= PINV_TOL[dtype] * scale
    report(what, err[scale > 0] / (PINV_TOL[dtype] * scale[scale > 0]))
    assert ok.all(), (what, [(int(i), err[i], scale[i]) for i in np.nonzero(~ok)[0][:5]])


# (m, n, batch): every lane-group width and both sides of it, tall and wide, batches that do and do not fill a wave
WAVE_SHAPES = [
    (1, 1, 65), (1, 7, 2), (7, 1, 257), (2, 2, 257), (3, 3, 1), (3, 3, 257), (6, 3, 257),
    (8, 8, 65), (9, 4, 257), (4, 9, 2), (9, 9, 65),
    (16, 8, 65), (16, 16, 1), (17, 17, 2), (33, 8, 65), (8, 33, 2), (32, 32, 65), (33, 33, 2),
    (64, 16, 257), (64, 32, 65), (32, 64, 65), (64, 64, 1), (64, 64, 257),
]
ROWS_SHAPES = [(65, 3, 65), (3, 65, 65), (100, 60, 3), (257, 31, 2)]
PARITY = [(m, n, b, "float64") for m, n, b in WAVE_SHAPES + ROWS_SHAPES] + [(m, n, b, "float32") for m, n, b in (WAVE_SHAPES + ROWS_SHAPES)[::2]]


@pytest.mark.parametrize("m,n,batch,dtype", PARITY)
def test_parity_all_jobs(hip, m, n, batch, dtype):
    assert svd_tier(m, n, batch) == ("wave" if max(m, n) <= SVD_WAVE_MAX else "rows")
    what = f"{m}x{n} batch={batch} {dtype}"
    for kind, x in (("cond2", cond2_stack(m, n, batch, dtype)), ("gauss", gaussian_stack(m, n, batch, dtype))):
        (s,) = svd_exe(dtype, 3, 0)(x)
        check_svd(x, None, s, None, False, dtype, f"S {kind} {what}")
        for job in (1, 2):
            U, s1, Vt = svd_exe(dtype, 3, job)(x)
            check_svd(x, U, s1, Vt, job == 2, dtype, f"job {job} {kind} {what}")
        if kind == "cond2":
            (X,) = pinv_exe(dtype, 3)(x)
            check_pinv(x, X, dtype, f"pinv {what}")


def test_rotation_threshold_converges_on_the_benchmark_stack(hip):
    """the 256 Gaussian 64 x 64 float64 matrices tools/bench_svd_batched.py draws (seed 0, in its sweep order): with a
    rotation threshold of the bare eps item 233 ran into the 60-sweep cap in the instance with vectors ("SVD did not
    converge"); with gesvj's eps * sqrt(c) the whole stack converges and meets the bars"""
    rng = np.random.default_rng(0)
    x = None
    for m, n in [(3, 3), (8, 8), (16, 16), (32, 32), (64, 64)]:
        for b in (1, 16, 256, 4096):
            draw = rng.standard_normal((b, m, n))
            if (m, n, b) == (64, 64, 256):
                x = draw
    U, s, Vt = svd_exe("float64", 3, 1)(x)
    check_svd(x, U, s, Vt, False, "float64", "benchmark stack 64x64 batch=256")
    (X,) = pinv_exe("float64", 3)(x[232:235])
    assert np.isfinite(X).all()


def test_four_dimensional_batch(hip):
    x = cond2_stack(9, 5, 6, "float64").reshape(3, 2, 9, 5)
    U, s, Vt = svd_exe("float64", 4, 1)(x)
    assert U.shape == (3, 2, 9, 5) and s.shape == (3, 2, 5) and Vt.shape == (3, 2, 5, 5)
    check_svd(x.reshape(6, 9, 5), U.reshape(6, 9, 5), s.reshape(6, 5), Vt.reshape(6, 5, 5), False, "float64", "4-D economic")
    (X,) = pinv_exe("float64", 4)(x)
    assert X.shape == (3, 2, 5, 9)
    check_pinv(x.reshape(6, 9, 5), X.reshape(6, 5, 9), "float64", "4-D pinv")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pinv_structural_rank_deficiency(hip, dtype):
    """rank deficiency by structure only (a zero row, a zero column, the all-zero item): no computed singular value
    sits near the rcond cut-off"""
    x = np.array(cond2_stack(7, 5, 9, dtype))
    x[1, 3, :] = 0.0
    x[2, :, 1] = 0.0
    x[3] = 0.0
    x[8, 0, :] = 0.0
    (X,) = pinv_exe(dtype, 3)(x)
    assert not X[3].any()
    check_pinv(x, X, dtype, f"pinv of rank-deficient items {dtype}")
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))
    (Xt,) = pinv_exe(dtype, 3)(xt)
    check_pinv(xt, Xt, dtype, f"pinv of wide rank-deficient items {dtype}")


def _mixed_batch():
    rng = np.random.default_rng(5)
    m, n = 12, 8
    items = [cond2_stack(m, n, 3, "float64")[k] for k in range(3)]
    items.append(rng.standard_normal((m, 3)) @ rng.standard_normal((3, n)))  # 3: rank 3 of 8
    items.append(np.zeros((m, n)))  # 4: all zero
    Q1 = np.linalg.qr(rng.standard_normal((m, m)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    items.append((Q1[:, :n] * np.logspace(0, -12, 20)[:n]) @ Q2)  # 5: graded
    bad = rng.standard_normal((m, n))
    bad[5, 2] = np.nan
    items.append(bad)  # 6: NaN
    items += [cond2_stack(m, n, 3, "float64", seed=1)[k] for k in range(3)]
    return np.stack(items)


def test_mixed_batch_items_do_not_touch_each_other(hip):
    x = _mixed_batch()
    nb, m, n = x.shape
    exes = {job: svd_exe("float64", 3, job) for job in (0, 1, 2)}
    exes[3] = pinv_exe("float64", 3)
    for job, exe in exes.items():
        whole = exe(x)
        for k in range(nb):
            alone = exe(x[k : k + 1])
            for a, b in zip(whole, alone):
                assert np.array_equal(a[k], b[0], equal_nan=True), (job, k)
    U, s, Vt = exes[1](x)
    assert np.isnan(s[6]).all() and np.isnan(U[6]).all() and np.isnan(Vt[6]).all()
    assert np.isnan(exes[3](x)[0][6]).all() and np.isnan(exes[0](x)[0][6]).all()
    good = [0, 1, 2, 7, 8, 9]
    check_svd(x[good], U[good], s[good], Vt[good], False, "float64", "ordinary items of the mixed batch")
    eye = np.eye(n)
    for k in (3, 4, 5):  # factors stay orthonormal whatever the rank
        assert np.abs(U[k].T @ U[k] - eye).max() <= 50 * 1e-12 and np.abs(Vt[k] @ Vt[k].T - eye).max() <= 50 * 1e-12, k
        assert np.abs((U[k] * s[k]) @ Vt[k] - x[k]).max() <= 50 * 1e-12 * max(np.abs(x[k]).max(), 1e-300), k
    assert (s[3, 3:] <= 1e-13 * s[3, 0]).all() and not s[4].any()
    np.testing.assert_allclose(s[5], np.logspace(0, -12, 20)[:8], rtol=1e-8)
    Uf, sf, Vf = exes[2](x)
    for k in (3, 4, 5):
        assert np.abs(Uf[k].T @ Uf[k] - np.eye(m)).max() <= 50 * 1e-12 and np.abs(Vf[k] @ Vf[k].T - eye).max() <= 50 * 1e-12, k


@pytest.mark.parametrize("m,n", [(9, 5), (5, 9), (16, 16)])
def test_strided_and_broadcast_stacks(hip, m, n):
    """the kernel reads its operand through three strides: a transposed view of the stack, every second matrix of a
    larger stack and one matrix shared across a broadcast batch dimension give the bits of the contiguous copy"""
    from pytensor_amd.device import DeviceArray
    from pytensor_amd.dispatch.decomp import gesvj_device

    env = type("_Env", (), {"lib": hip.lib()})
    big = np.array(gaussian_stack(m, n, 10, "float64"))
    dev = DeviceArray.from_host(big)
    views = {
        "transposed": (dev.view((10, n, m), (m * n, 1, n)), np.ascontiguousarray(big.transpose(0, 2, 1))),
        "every second": (dev.view((5, m, n), (2 * m * n, n, 1)), np.ascontiguousarray(big[::2])),
        "shared": (dev.view((4, m, n), (0, n, 1), 3 * m * n), np.ascontiguousarray(np.broadcast_to(big[3], (4, m, n)))),
        "outer and shared": (dev.view((2, 3, m, n), (5 * m * n, 0, n, 1)), np.ascontiguousarray(np.broadcast_to(big[::5][:, None], (2, 3, m, n)))),
    }
    for what, (view, host) in views.items():
        for job in (0, 1, 2, 3):
            got = [o.to_host() for o in gesvj_device(env, view, job, 1e-15)]
            want = [o.to_host() for o in gesvj_device(env, DeviceArray.from_host(host), job, 1e-15)]
            for a, b in zip(got, want):
                assert a.shape == b.shape and np.array_equal(a, b), (what, job)
    s_ref = np.linalg.svd(big[::2], compute_uv=False)
    (s,) = gesvj_device(env, views["every second"][0], 0)
    assert np.abs(s.to_host() - s_ref).max() <= 1e-12 * s_ref.max()


def _launches(hip, exe, *ins):
    exe(*ins)  # warm-up: allocations, module loads
    lib = hip.lib()
    c0 = lib.pthip_launch_count()
    out = exe(*ins)
    return lib.pthip_launch_count() - c0, out


def test_launch_count_does_not_grow_with_the_batch(hip):
    from pytensor_amd.device import DeviceArray
    from pytensor_amd.dispatch.decomp import gesvj_device

    lib = hip.lib()
    env = type("_Env", (), {"lib": lib})
    for (m, n) in ((8, 8), (6, 3), (3, 6), (SVD_WAVE_MAX + 6, 9), (9, SVD_WAVE_MAX + 6)):
        tier = svd_tier(m, n, 2)
        counts = {}
        for job in (0, 1, 2, 3):
            exe = pinv_exe("float64", 3) if job == 3 else svd_exe("float64", 3, job)
            for batch in (2, 257):
                counts[job, batch], _ = _launches(hip, exe, cond2_stack(m, n, batch, "float64"))
            assert counts[job, 257] == counts[job, 2], (m, n, counts)
        print(f"{m}x{n} ({tier}): launches and copies per job {[counts[j, 2] for j in range(4)]}")
        if tier == "wave":
            # one input up, one output down on both sides: S alone and the pseudo-inverse cost the same, one kernel each
            assert counts[0, 2] == counts[3, 2], (m, n, counts)
            # and on an operand that is on the device already every job is exactly one launch, nothing else
            for batch in (2, 257):
                dev = DeviceArray.from_host(np.array(cond2_stack(m, n, batch, "float64")))
                for job in (0, 1, 2, 3):
                    c0 = lib.pthip_launch_count()
                    outs = gesvj_device(env, dev, job, 1e-15)
                    assert lib.pthip_launch_count() - c0 == 1, (m, n, batch, job)
                    del outs
    for mode in QR_OUTS:
        c = {batch: _launches(hip, qr_exe("float64", 3, mode), gaussian_stack(9, 5, batch, "float64"))[0] for batch in (2, 257)}
        assert c[257] == c[2], (mode, c)


@pytest.mark.parametrize("m,n", [(9, 5), (5, 9), (64, 64)])
@pytest.mark.parametrize("mode", list(QR_OUTS))
def test_batched_qr_is_the_unbatched_kernel(hip, m, n, mode):
    x = gaussian_stack(m, n, 5, "float64")
    whole = qr_exe("float64", 3, mode)(x)
    single = qr_exe("float64", 2, mode)
    assert len(whole) == QR_OUTS[mode]
    for k in range(x.shape[0]):
        for a, b in zip(whole, single(x[k])):
            assert a[k].shape == b.shape and np.array_equal(a[k], b), (mode, k)
    if mode in ("economic", "full"):
        Q, R = whole
        assert np.abs(Q @ R - x).max() <= 1e-13 * max(m, n)


@pytest.fixture(scope="module")
def pt(hip):
    from e2e_util import activate

    pytensor = activate()
    import pytensor.tensor as ptt

    return pytensor, ptt


@pytest.mark.parametrize("shape", [(7, 6, 5), (5, 4, 9)])
def test_end_to_end_against_the_c_linker(hip, pt, shape):
    pytensor, ptt = pt
    from e2e_util import compare_hip_and_cvm
    from pytensor.tensor.linalg import pinv, svd

    nb, m, n = shape
    x = np.array(cond2_stack(m, n, nb, "float64"))
    A3 = ptt.tensor3("A")
    compare_hip_and_cvm([A3], svd(A3, compute_uv=False), [x], calls=3, rtol=1e-12, atol=1e-12, must_freeze=True)
    compare_hip_and_cvm([A3], pinv(A3), [x], calls=3, rtol=0.0, atol=1e-12 * np.abs(np.linalg.pinv(x)).max(), must_freeze=True)
    U, s, Vt = svd(A3, full_matrices=False)
    rebuilt = (U * s[:, None, :]) @ Vt
    compare_hip_and_cvm([A3], rebuilt, [x], calls=3, rtol=0.0, atol=1e-12 * np.abs(x).max())
    # views in the graph: a transposed stack, every second matrix, one matrix shared across a broadcast batch dimension
    f = pytensor.function([A3], [svd(A3.transpose(0, 2, 1), compute_uv=False), svd(A3[::2], compute_uv=False), pinv(A3[::2])], mode="hip")
    st, s2, p2 = f(x)
    (s_plain,) = svd_exe("float64", 3, 0)(np.ascontiguousarray(x.transpose(0, 2, 1)))
    assert np.array_equal(st, s_plain)
    assert np.array_equal(s2, svd_exe("float64", 3, 0)(np.ascontiguousarray(x[::2]))[0])
    assert np.array_equal(p2, pinv_exe("float64", 3)(np.ascontiguousarray(x[::2]))[0])
    A2 = ptt.matrix("A2")
    shared = ptt.broadcast_to(A2, (4, m, n))
    sb = pytensor.function([A2], svd(shared, compute_uv=False), mode="hip")(x[0])
    # (the graph rewrites may factor the shared matrix once, with the single-matrix kernel, and broadcast the result: the
    #  bar here is the parity one; bit-equality of a stride-0 stack is test_strided_and_broadcast_stacks')
    s_ref = np.linalg.svd(x[0], compute_uv=False)
    assert sb.shape == (4, min(m, n)) and np.abs(sb - s_ref).max() <= 1e-12 * s_ref[0]


def test_gradients_against_the_c_linker(hip, pt):
    pytensor, ptt = pt
    from e2e_util import compare_hip_and_cvm
    from pytensor.tensor.linalg import svd

    nb, m, n = 7, 6, 5
    x = np.array(cond2_stack(m, n, nb, "float64"))  # singular values linspace(1, 2, 5): gap 0.25
    rng = np.random.default_rng(3)
    w, W = rng.standard_normal((nb, n)), rng.standard_normal((nb, m, m))
    A3, wv, Wv = ptt.tensor3("A"), ptt.matrix("w"), ptt.tensor3("W")
    g1 = pytensor.grad((wv * svd(A3, compute_uv=False)).sum(), A3)
    ref = pytensor.function([A3, wv], g1, mode="FAST_COMPILE")(x, w)
    compare_hip_and_cvm([A3, wv], g1, [x, w], calls=3, rtol=0.0, atol=1e-10 * np.abs(ref).max())
    U, s, Vt = svd(A3, full_matrices=False)
    U2 = U[..., :2]
    g2 = pytensor.grad(((U2 @ U2.mT) * Wv).sum(), A3)  # a projector: free of the sign ambiguity
    ref = pytensor.function([A3, Wv], g2, mode="FAST_COMPILE")(x, W)
    compare_hip_and_cvm([A3, Wv], g2, [x, W], calls=3, rtol=0.0, atol=1e-10 * np.abs(ref).max())


def test_empty_stacks_give_empty_outputs(hip):
    for shape in ((0, 4, 3), (5, 0, 3), (5, 4, 0)):
        x = np.zeros(shape)
        nb, m, n = shape
        k = min(m, n)
        (s,) = svd_exe("float64", 3, 0)(x)
        assert s.shape == (nb, k)
        U, s, Vt = svd_exe("float64", 3, 1)(x)
        assert U.shape == (nb, m, k) and s.shape == (nb, k) and Vt.shape == (nb, k, n)
        (X,) = pinv_exe("float64", 3)(x)
        assert X.shape == (nb, n, m)
        Q, R = qr_exe("float64", 3, "economic")(x)
        assert Q.shape == (nb, m, k) and R.shape == (nb, k, n)
