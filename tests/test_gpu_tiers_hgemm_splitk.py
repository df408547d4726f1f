"""GPU: split-K float16 products (csrc/hgemm.hip: few output tiles, deep K) through the C ABI and through
``pytensor.grad`` under ``mode="hip"``.

Reference, bound and leak guards are those of tests/test_gpu_tiers_hgemm.py (``check``: long double product,
``2^-11 |exact| + K 2^-23 sum|ab| + 2^-25``; NaN parents, sentinels around the output).  The additions inside the
splits and the S - 1 additions of the slabs are K - 1 fp32 additions in all, so the bound is the unsplit one.  A split
needs 8 stages of 64 per range: K > 960 here.
"""
import numpy as np
import pytest

import _blas_tiers_worker as dev
import blas_cases as bc
import test_gpu_tiers_hgemm as base
from e2e_util import hip_executable

pytestmark = pytest.mark.gpu
hip, pt = base.hip, base.pt
# one skinny tile, M / N / K tails, 129 stages over 16 splits (uneven, the last stage has 8 columns); four 128-tiles
# with different edge masks, each on its own ticket; 19 full stages over 2 splits (10 + 9); 17 stages, the last one a
# single column
SPLIT_SHAPES = [(5, 37, 8200), (129, 130, 1100), (40, 50, 1216), (33, 31, 1025)]


def bits(a):
    return a.view(np.uint16)


@pytest.mark.parametrize("tA,tB", base.ORIENT)
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_shapes_orientations(hip, shape, tA, tB):
    assert hip.lib().pthip_hgemm_splits(1, *shape) > 1
    A, B = base.operands((1, *shape))
    opA, opB = bc.embed(A, trans=tA), bc.embed(B, trans=tB)
    got = base.run_hgemm(hip, opA, opB, (1, *shape))  # (asserts one launch)
    base.check(got, A, B, f"split hgemm {shape} {tA} {tB}")
    assert np.array_equal(bits(got), bits(base.run_hgemm(hip, opA, opB, (1, *shape)))), "two runs differ"


@pytest.mark.parametrize("tA,tB", base.ORIENT)
def test_split_misaligned(hip, tA, tB):
    shape = (2, 70, 131, 1030)
    assert hip.lib().pthip_hgemm_splits(*shape) > 1
    A, B = base.operands(shape)
    base.check(base.run_hgemm(hip, bc.embed(A, trans=tA, **base.OFF), bc.embed(B, trans=tB, **base.OFF), shape), A, B, f"misaligned {tA} {tB}")


def test_split_more_units_than_workgroups(hip):
    """300 tiles x 2 splits on 512 workgroups: 88 of them walk two units, finishing the tile of one and not of the other;
    the shared B is read by every item"""
    shape = (300, 5, 7, 1024)
    assert shape[0] * hip.lib().pthip_hgemm_splits(*shape) > 512
    A, B = base.operands(shape)
    got = base.run_hgemm(hip, bc.embed(A), bc.embed(B, trans=True), shape)
    base.check(got, A, B, f"batched split {shape}")
    assert np.array_equal(bits(got), bits(base.run_hgemm(hip, bc.embed(A), bc.embed(B, trans=True), shape))), "two runs differ"
    base.check(base.run_hgemm(hip, bc.embed(A, trans=True), bc.embed(B[:1], bstride="zero"), shape), A, B[:1], "broadcast B")


@pytest.mark.parametrize("shape", [(1, *s) for s in base.SHAPES if s[2] <= 960] + [(520, 5, 7, 70), (512, 5, 7, 8200)], ids=str)
def test_shallow_or_full_grids_stay_unsplit(hip, shape):
    assert hip.lib().pthip_hgemm_splits(*shape) == 1


def test_split_overflow_in_one_rounding(hip):
    """four partial sums of about +-37000 each (finite as halves, too): only their fp32 sum, about +-148000, overflows"""
    rng = np.random.default_rng(5)
    M, N, K = 40, 33, 2048
    assert hip.lib().pthip_hgemm_splits(1, M, N, K) == 4
    A = (np.where(np.arange(M) % 2, -8.0, 8.0)[:, None] * (1 + rng.random((M, K)) / 8)).astype(np.float16)[None]
    B = (8.0 * (1 + rng.random((K, N)) / 8)).astype(np.float16)[None]
    got = base.run_hgemm(hip, bc.embed(A), bc.embed(B), (1, M, N, K))
    base.check(got, A, B, "overflow across splits")
    assert np.isinf(got).all() and (got[0, 0] > 0).all() and (got[0, 1] < 0).all()


# row layout: the inner product and three rows (one row per block), five rows (four per block); column layout
@pytest.mark.parametrize("M,layout", [(1, "row"), (3, "row"), (5, "row"), (70, "col")])
def test_hgemv_split(hip, M, layout):
    K = 50001
    rng = np.random.default_rng([9, M, K])
    A, x = rng.standard_normal((M, K)).astype(np.float16), rng.standard_normal(K).astype(np.float16)
    lib = hip.lib()
    for tag, a_kw, sx, x_ptr in (("aligned", bc.ALIGNED, 1, 0), ("misaligned, strided x", dict(ptr=1, pitch="odd"), 3, 1)):
        op = bc.embed(A[None], trans=(layout == "col"), **a_kw)
        xp, xo = bc.embed_vec(x, sx, x_ptr)
        (dA, pA), (dx, px) = dev.upload(op.parent, op.off), dev.upload(xp, xo)
        assert lib.pthip_hgemv_splits(M, K, op.s0, op.s1) > 1
        runs = []
        for _ in range(2):
            out = dev.Out(M, np.float16)
            before = lib.pthip_launch_count()
            hip.check(lib.pthip_hgemv(M, K, pA, op.s0, op.s1, px, sx, out.ptr))
            assert lib.pthip_launch_count() - before == 1
            runs.append(out.fetch((1, M, 1)))
        base.check(runs[0], A[None], x[None, :, None], f"split hgemv {M}x{K} {layout} {tag}")
        assert np.array_equal(bits(runs[0]), bits(runs[1])), "two runs differ"


def test_weight_gradient_of_a_deep_batch(hip, pt):
    """gw = x.T @ gy of a dense layer: M, N are the layer widths and K the batch, which is deep enough to split"""
    pytensor, ptt = pt
    x, w = ptt.matrix("x", dtype="float16"), ptt.matrix("w", dtype="float16")
    y = ptt.dot(x, w)
    gy, gw = pytensor.grad(ptt.tanh(y).sum(), [y, w])
    f = pytensor.function([x, w], [gy, gw], mode="hip")
    assert "HostPerform" not in [n.op for n in f.maker.linker.last_ir.nodes]
    X, W = base._draw((1100, 33), (33, 130))
    assert hip.lib().pthip_hgemm_splits(1, 33, 130, 1100) > 1
    GY, GW = f(X, W)
    base.check(GW[None], X.T[None], GY[None], "gw = x.T @ gy")
    outs = [f(X, W)[1] for _ in range(3)]  # the third call of one signature replays the frozen plan
    assert hip_executable(f)._auto_plan is not None
    assert all(np.array_equal(bits(GW), bits(o)) for o in outs)
