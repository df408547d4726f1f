"""GPU: float16 products (csrc/hgemm.hip) through the C ABI and through ``pytensor.function(mode="hip")``.

Reference: operands converted exactly to a wider type, ``A @ B`` there (long double via ``blas_cases.hp_matmul``).  A
product of two halves is exact in fp32, so the only errors are K fp32 additions in some order and ONE rounding to half:

    |out - exact| <= 2^-11 |exact| + K 2^-23 sum_k |a_k b_k| + 2^-25

(2^-25: half the smallest half subnormal — subnormal results must come out gradually).  Where |exact| exceeds
65504 (1 + 2^-12) the output must be the infinity of that sign; within the bound of that threshold 65504 passes too.
Operands are views into NaN-filled parents and outputs sit between sentinels (tests/blas_cases.py,
tests/_blas_tiers_worker.py), so an element read or written out of range fails the case.
"""
import numpy as np
import pytest

import _blas_tiers_worker as dev
import blas_cases as bc
from e2e_util import activate, hip_executable

pytestmark = pytest.mark.gpu
H = np.longdouble
OVER = H(65504) * (1 + H(2) ** -12)
ORIENT = ((False, False), (False, True), (True, False), (True, True))
OFF = dict(ptr=1, pitch="odd", bstride="odd")
# one tile; M, N, K tails; a full 128-tile with half a stage; two tiles each way; skinny; just past skinny; long K;
# the stage depth (64) - 1, exact, + 1
SHAPES = [(1, 1, 1), (33, 31, 17), (128, 128, 32), (129, 130, 65), (64, 200, 1000), (65, 40, 96), (5, 37, 8200), (40, 50, 63), (40, 50, 64),
          (40, 50, 65)]


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def check(got, A, B, what):
    """hold ``got`` (float16, (batch, M, N)) to the bound for operands A (., M, K), B (., K, N); returns the worst ratio"""
    A, B = np.asarray(A).astype(H), np.asarray(B).astype(H)
    exact, mag = bc.hp_matmul(A, B), bc.hp_matmul(np.abs(A), np.abs(B))
    assert got.dtype == np.float16 and got.shape == exact.shape, (what, got.dtype, got.shape, exact.shape)
    bound = H(2) ** -11 * np.abs(exact) + A.shape[-1] * H(2) ** -23 * mag + H(2) ** -25
    must_inf, may_inf = np.abs(exact) - bound > OVER, np.abs(exact) + bound >= OVER
    assert np.array_equal(got[must_inf].astype(H), np.sign(exact[must_inf]) * np.inf), f"{what}: overflow must give inf"
    band = may_inf & ~must_inf & np.isinf(got)
    assert np.array_equal(np.sign(got[band]), np.sign(exact[band])), what
    rest = ~(must_inf | band)
    ratio = bc.worst_ratio(got[rest], exact[rest], bound[rest])
    print(f"{what}: worst |err| / bound = {ratio:.3g}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


def run_hgemm(hip, opA, opB, shape):
    """``pthip_hgemm`` on blas_cases Operand views; asserts one launch; returns out (batch, M, N)"""
    nb, M, N, K = shape
    (dA, pA), (dB, pB) = dev.upload(opA.parent, opA.off), dev.upload(opB.parent, opB.off)
    out = dev.Out(nb * M * N, np.float16)
    lib = hip.lib()
    before = lib.pthip_launch_count()
    hip.check(lib.pthip_hgemm(nb, M, N, K, pA, opA.sb, opA.s0, opA.s1, pB, opB.sb, opB.s0, opB.s1, out.ptr))
    assert lib.pthip_launch_count() - before == 1, shape
    return out.fetch((nb, M, N))


_OPS = {}


def operands(shape, seed=0):
    if shape not in _OPS:
        nb, M, N, K = shape
        rng = np.random.default_rng([seed, *shape])
        _OPS[shape] = rng.standard_normal((nb, M, K)).astype(np.float16), rng.standard_normal((nb, K, N)).astype(np.float16)
    return _OPS[shape]


@pytest.mark.parametrize("tA,tB", ORIENT)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hgemm_shapes_orientations(hip, shape, tA, tB):
    A, B = operands((1, *shape))
    got = run_hgemm(hip, bc.embed(A, trans=tA), bc.embed(B, trans=tB), (1, *shape))
    check(got, A, B, f"hgemm {shape} A{'T' if tA else 'N'} B{'T' if tB else 'N'}")


@pytest.mark.parametrize("tA,tB", ORIENT)
def test_hgemm_misaligned(hip, tA, tB):
    """pointer off by one half, odd leading dimension, odd batch stride: the 2-byte staging path, tails in M, N, K"""
    shape = (2, 70, 131, 75)
    A, B = operands(shape)
    check(run_hgemm(hip, bc.embed(A, trans=tA, **OFF), bc.embed(B, trans=tB, **OFF), shape), A, B, f"misaligned {tA} {tB}")


# batch 3; more tiles than resident workgroups (520 > 512: a workgroup walks two tiles, the second one's first stage is
# fetched behind the first one's last), with two stages / remapped tile ids and with one stage / plain ids
@pytest.mark.parametrize("shape", [(3, 33, 40, 70), (520, 5, 7, 70), (515, 3, 4, 40)], ids=lambda s: "x".join(map(str, s)))
def test_hgemm_batched(hip, shape):
    A, B = operands(shape)
    a = run_hgemm(hip, bc.embed(A), bc.embed(B, trans=True), shape)
    check(a, A, B, f"batched {shape}")
    assert np.array_equal(a.view(np.uint16), run_hgemm(hip, bc.embed(A), bc.embed(B, trans=True), shape).view(np.uint16)), "two runs differ"
    got = run_hgemm(hip, bc.embed(A, trans=True), bc.embed(B[:1], bstride="zero"), shape)
    check(got, A, B[:1], f"broadcast B {shape}")


def test_hgemm_k0_overflow_subnormal(hip):
    rng = np.random.default_rng(5)
    got = run_hgemm(hip, bc.embed(np.zeros((2, 65, 0), np.float16)), bc.embed(np.zeros((2, 0, 130), np.float16)), (2, 65, 130, 0))
    assert got.shape == (2, 65, 130) and not got.view(np.uint16).any(), "K = 0 must give +0"
    # overflow: |sum| ~ 64 * 64 * 32 = 2 * 65536, rows of either sign
    M, N, K = 40, 33, 32
    A = (np.where(np.arange(M) % 2, -64.0, 64.0)[:, None] * (1 + rng.random((M, K)) / 8)).astype(np.float16)[None]
    B = (64.0 * (1 + rng.random((K, N)) / 8)).astype(np.float16)[None]
    got = run_hgemm(hip, bc.embed(A), bc.embed(B), (1, M, N, K))
    check(got, A, B, "overflow")
    assert np.isinf(got).all() and (got[0, 0] > 0).all() and (got[0, 1] < 0).all()
    # normal inputs of magnitude 2^-10 .. 2^-9 and random sign: the 16-term sums are half subnormals
    K = 16
    A, B = ((rng.choice([-1.0, 1.0], s) * 2.0**-10 * (1 + rng.random(s))).astype(np.float16) for s in ((1, M, K), (1, K, N)))
    got = run_hgemm(hip, bc.embed(A), bc.embed(B), (1, M, N, K))
    check(got, A, B, "subnormal results")
    assert (np.abs(got.astype(np.float64)) < 2.0**-14).all() and (got != 0).mean() > 0.9


def test_hgemm_refuses_an_operand_without_unit_stride(hip):
    lib = hip.lib()
    A, B = operands((1, 8, 8, 8))
    (dA, pA), (dB, pB) = dev.upload(A.reshape(-1), 0), dev.upload(B.reshape(-1), 0)
    out = dev.Out(16, np.float16)
    before = lib.pthip_launch_count()
    assert lib.pthip_hgemm(1, 4, 4, 4, pA, 0, 16, 2, pB, 0, 8, 1, out.ptr) != 0 and b"(16, 2)" in lib.pthip_last_error()
    assert lib.pthip_launch_count() == before
    hip.check(lib.pthip_hgemm(1, 0, 4, 4, pA, 0, 4, 1, pB, 0, 4, 1, out.ptr))  # empty: nothing launched
    assert lib.pthip_launch_count() == before


@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("M,K", [(1, 7), (70, 33), (257, 4100)])
def test_hgemv(hip, M, K, layout):
    rng = np.random.default_rng([9, M, K])
    A, x = rng.standard_normal((M, K)).astype(np.float16), rng.standard_normal(K).astype(np.float16)
    lib = hip.lib()
    for tag, a_kw, sx, x_ptr in (("aligned", bc.ALIGNED, 1, 0), ("misaligned, strided x", dict(ptr=1, pitch="odd"), 3, 1)):
        op = bc.embed(A[None], trans=(layout == "col"), **a_kw)
        xp, xo = bc.embed_vec(x, sx, x_ptr)
        (dA, pA), (dx, px) = dev.upload(op.parent, op.off), dev.upload(xp, xo)
        runs = []
        for _ in range(2):
            out = dev.Out(M, np.float16)
            before = lib.pthip_launch_count()
            hip.check(lib.pthip_hgemv(M, K, pA, op.s0, op.s1, px, sx, out.ptr))
            assert lib.pthip_launch_count() - before == 1
            runs.append(out.fetch((1, M, 1)))
        check(runs[0], A[None], x[None, :, None], f"hgemv {M}x{K} {layout} {tag}")
        assert np.array_equal(runs[0].view(np.uint16), runs[1].view(np.uint16)), "two runs differ"


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pt(hip):
    pytensor = activate()
    import pytensor.tensor as ptt

    return pytensor, ptt


def _draw(*shapes):
    rng = np.random.default_rng(11)
    return [rng.standard_normal(s).astype(np.float16) for s in shapes]


def _launches(hip, f, *args):
    before = hip.lib().pthip_launch_count()
    out = f(*args)
    return out, hip.lib().pthip_launch_count() - before


@pytest.mark.parametrize("sx,sy", [((33, 20), (20, 70)), ((33, 20), (20,)), ((20,), (20, 70)), ((20,), (20,)), ((3, 17, 9), (3, 9, 5)),
                                   ((3, 17, 9), (9, 5)), ((2, 3, 17, 9), (3, 9, 5))], ids=str)
def test_dot_and_matmul_end_to_end(hip, pt, sx, sy):
    pytensor, ptt = pt
    x, y = (ptt.tensor(nm, dtype="float16", shape=(None,) * len(s)) for nm, s in (("x", sx), ("y", sy)))
    f = pytensor.function([x, y], ptt.matmul(x, y) if len(sx) > 2 else ptt.dot(x, y), mode="hip")
    assert "HostPerform" not in [n.op for n in f.maker.linker.last_ir.nodes]
    X, Y = _draw(sx, sy)
    got, n = _launches(hip, f, X, Y)
    assert got.shape == np.matmul(X, Y).shape
    Xm, Ym = X if X.ndim > 1 else X[None, :], Y if Y.ndim > 1 else Y[:, None]
    bshape = np.broadcast_shapes(Xm.shape[:-2], Ym.shape[:-2])
    A, B = (np.broadcast_to(v, bshape + v.shape[-2:]).reshape(-1, *v.shape[-2:]) for v in (Xm, Ym))
    check(got.reshape(A.shape[0], A.shape[1], B.shape[2]), A, B, f"{sx} @ {sy}")
    if sx == (3, 17, 9) and sy == (3, 9, 5):  # one product launch for the stack: as many launches as for one item
        _, n1 = _launches(hip, f, X[:1], Y[:1])
        assert n == n1, (n, n1)
    # the third call of one signature replays the frozen plan: the same bits
    outs = [f(X, Y) for _ in range(3)]
    assert hip_executable(f)._auto_plan is not None
    assert all(np.array_equal(got.view(np.uint16), o.view(np.uint16)) for o in outs)


def test_dense_layer_gradient(hip, pt):
    """d/dx, d/dw of tanh(x @ w).sum(): each of the three products held to the bound on the operands the device gave it"""
    pytensor, ptt = pt
    x, w = ptt.matrix("x", dtype="float16"), ptt.matrix("w", dtype="float16")
    y = ptt.dot(x, w)
    gy, gx, gw = pytensor.grad(ptt.tanh(y).sum(), [y, x, w])
    f = pytensor.function([x, w], [y, gy, gx, gw], mode="hip")
    assert "HostPerform" not in [n.op for n in f.maker.linker.last_ir.nodes]
    X, W = _draw((70, 33), (33, 130))
    Y, GY, GX, GW = f(X, W)
    check(Y[None], X[None], W[None], "y = x @ w")
    check(GX[None], GY[None], W.T[None], "gx = gy @ w.T")
    check(GW[None], X.T[None], GY[None], "gw = x.T @ gy")
