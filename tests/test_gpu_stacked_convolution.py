"""GPU: ``Blockwise(Convolve1d)`` and ``Blockwise(Convolve2d)`` over a whole broadcast stack in one launch
(csrc/conv_batched.hip through ``dispatch/misc.py::convolve1d_stack`` / ``convolve2d_stack``).

The yardstick is the direct sum in ``np.longdouble`` from seeded standard-normal inputs.  The bar is derived, not
measured: an output is a recursive sum of m products in working precision, m at most the size of the smaller operand, so

    |got - want| <= gamma_m * S + u * |want|,   gamma_m = m u / (1 - m u),   u = 2^-53 (float64) / 2^-24 (float32),

with S the same convolution of the absolute values (long double as well) and the last term the rounding of the
reference to the working type.  It holds with or without FMA contraction.  int64 results are compared exactly, and an
output the reference has as NaN or Inf must be the same NaN or Inf.  The shapes come from the module's constants.
"""
import numpy as np
import pytest

from pytensor_amd.dispatch.misc import (CONV1D_CHUNK as C, CONV1D_TILE as T, CONV2D_COL_CHUNK as KC, CONV2D_ROW_CHUNK as KR, CONV2D_TILE,
                                        CONV_STACK_LAUNCHES, conv_tier)
from pytensor_amd.ir import Graph

pytestmark = pytest.mark.gpu
TH, TW = CONV2D_TILE
U = {"float64": 2.0**-53, "float32": 2.0**-24}
DTYPES = ["float64", "float32", "int64"]


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def conv_exe(core_ndim, dta, nda, dtb, ndb, full, flip=False):
    """one ``Blockwise`` node with a constant ``full_mode``; flip: ``b[..., ::-1]`` (a ``Subtensor`` node) feeds it"""
    from pytensor_amd.executor import HipExecutable

    g = Graph(name=f"conv{core_ndim}d")
    a, b = g.new_var(dta, (None,) * nda), g.new_var(dtb, (None,) * ndb)
    mode = g.new_var("bool", (), const=np.asarray(bool(full)))
    kernel = b
    if flip:
        step = g.new_var("int64", (), const=np.asarray(-1))
        kernel = g.new_var(dtb, (None,) * ndb)
        g.add_node("Subtensor", {"idx_list": [slice(None, None, None)] * (ndb - 1) + [slice(None, None, 0)]}, [b, step], [kernel])
    dt = str(np.result_type(dta, dtb))
    out = g.new_var(dt, (None,) * (max(nda, ndb)))
    sig = "(n),(k),()->(o)" if core_ndim == 1 else "(m,n),(p,q),()->(o,r)"
    g.add_node("Blockwise", {"core_op": f"Convolve{core_ndim}d", "core_params": {}, "signature": sig}, [a, kernel, mode], [out])
    g.inputs, g.outputs = [a, b], [out]
    return HipExecutable(g)


def reference(a, b, full, core_ndim):
    """the broadcast stack of direct sums in long double"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    bshape = np.broadcast_shapes(a.shape[:-core_ndim], b.shape[:-core_ndim])
    A, B = np.broadcast_to(a, bshape + a.shape[-core_ndim:]), np.broadcast_to(b, bshape + b.shape[-core_ndim:])
    if core_ndim == 1:
        flat = [np.convolve(x, y, "full" if full else "valid") for x, y in zip(A.reshape(-1, A.shape[-1]), B.reshape(-1, B.shape[-1]))]
        return np.stack(flat).reshape(*bshape, -1)
    (ha, wa), (hb, wb) = A.shape[-2:], B.shape[-2:]
    out = np.zeros((*bshape, ha + hb - 1, wa + wb - 1), np.longdouble)
    for p in range(hb):
        for q in range(wb):
            out[..., p : p + ha, q : q + wa] += A * B[..., p : p + 1, q : q + 1]
    return out if full else out[..., min(ha, hb) - 1 : max(ha, hb), min(wa, wb) - 1 : max(wa, wb)]


def check(got, a, b, full, core_ndim, what):
    want = reference(a, b, full, core_ndim)
    dt = str(np.result_type(a.dtype, b.dtype))
    assert got.shape == want.shape and str(got.dtype) == dt, (what, got.shape, want.shape, got.dtype)
    if dt == "int64":
        assert np.array_equal(got, want.astype("int64")), what
        return
    m = min(int(np.prod(a.shape[-core_ndim:])), int(np.prod(b.shape[-core_ndim:])))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin].astype(dt), equal_nan=True), (what, "non-finite outputs")
    S = reference(np.abs(a), np.abs(b), full, core_ndim)
    bound = (m * U[dt] / (1 - m * U[dt])) * S + U[dt] * np.abs(want)
    err = np.abs(got[fin].astype(np.longdouble) - want[fin])
    ratio = float(np.max(err / np.maximum(bound[fin], np.finfo(np.longdouble).tiny), initial=0.0))
    print(f"{what}: worst |got - want| / bound = {ratio:.3e}")
    assert ratio <= 1.0, (what, ratio)


def draw(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-9, 10, size=shape) if dtype == "int64" else rng.standard_normal(shape).astype(dtype)


# (signal, taps, items): taps = 1; the swap; several tiles of one item; every side of the tap chunk with a signal of
# three chunks; items packed two and four to a workgroup with a last group that is not full
FULL_1D = [(40, 1, 3), (5, 12, 3), (T - 3, 3, 2), (T - 2, 3, 2), (T - 1, 3, 2), (2 * T + 1, 3, 2),
           (3 * C, C - 1, 2), (3 * C, C, 2), (3 * C, C + 1, 2), (3 * C + 7, 2 * C + 5, 2), (45, 6, 37), (T // 4 - 4, 6, 3)]
# (the same outputs counts in "valid" mode; equal lengths: one output)
VALID_1D = [(40, 1, 3), (5, 12, 3), (9, 9, 3), (T + 1, 3, 2), (T + 2, 3, 2), (T + 3, 3, 2), (2 * T + 5, 3, 2),
            (3 * C, C - 1, 2), (3 * C, C, 2), (3 * C, C + 1, 2), (4 * C, 2 * C + 5, 2), (55, 6, 37), (T // 4 + 6, 6, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,items,full", [(*c, True) for c in FULL_1D] + [(*c, False) for c in VALID_1D])
def test_convolve1d_stack(hip, n, k, items, full, dtype):
    a, b = draw((items, n), dtype, 1000 * n + k), draw((items, k), dtype, 7 + 1000 * n + k)
    assert conv_tier((items,)) == "stack"
    (got,) = conv_exe(1, dtype, 2, dtype, 2, full)(a, b)
    check(got, a, b, full, 1, f"1-d {n} * {k} x {items} {'full' if full else 'valid'} {dtype}")


# (image, kernel, items): kernels 1 x 1, 3 x 5, taller than a row chunk, wider than a column chunk; outputs of a tile
# +- 1 in each direction; the image smaller than the kernel; small images packed four and two to a workgroup
FULL_2D = [((9, 11), (1, 1), 3), ((TH - 3, TW - 3), (3, 5), 2), ((TH - 1, TW - 5), (3, 5), 2), ((20, 9), (KR + 3, 2), 3), ((4, 70), (2, KC + 3), 2),
           ((3, 4), (6, 9), 3), ((6, 7), (3, 3), 10), ((20, 10), (3, 3), 5), ((3, 10), (10, 3), 2)]
VALID_2D = [((9, 11), (1, 1), 3), ((TH + 1, TW + 5), (3, 5), 2), ((TH + 3, TW + 3), (3, 5), 2), ((30, 9), (KR + 3, 2), 3), ((5, 2 * KC), (2, KC + 3), 2),
            ((3, 4), (6, 9), 3), ((8, 9), (3, 3), 10), ((7, 7), (7, 7), 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("img,ker,items,full", [(*c, True) for c in FULL_2D] + [(*c, False) for c in VALID_2D])
def test_convolve2d_stack(hip, img, ker, items, full, dtype):
    a, b = draw((items, *img), dtype, 100 * img[0] + ker[1]), draw((items, *ker), dtype, 3 + 100 * img[0] + ker[1])
    (got,) = conv_exe(2, dtype, 3, dtype, 3, full)(a, b)
    check(got, a, b, full, 2, f"2-d {img} * {ker} x {items} {'full' if full else 'valid'} {dtype}")


# batch shapes of the two operands: dimensions that do not flatten, an unbatched operand on either side
BROADCAST = [((5, 1), (1, 3)), ((7,), ()), ((), (7,)), ((4, 5), (4, 1)), ((2, 1, 3, 1, 2, 1), (1, 2, 1, 3, 1, 2))]


@pytest.mark.parametrize("ba,bb", BROADCAST)
@pytest.mark.parametrize("full", [True, False])
def test_broadcast_batches(hip, ba, bb, full):
    a, b = draw((*ba, 70), "float64", 11), draw((*bb, 9), "float64", 12)
    (got,) = conv_exe(1, "float64", a.ndim, "float64", b.ndim, full)(a, b)
    check(got, a, b, full, 1, f"1-d batches {ba} and {bb}")
    a2, b2 = draw((*ba, 9, 12), "float32", 13), draw((*bb, 4, 3), "float64", 14)  # (and a promoted operand)
    (got,) = conv_exe(2, "float32", a2.ndim, "float64", b2.ndim, full)(a2, b2)
    check(got, a2, b2, full, 2, f"2-d batches {ba} and {bb}")


@pytest.mark.parametrize("full", [True, False])
def test_flipped_operand_of_the_gradient(hip, full):
    """``flip(...)`` of the pullback reaches the kernel as a negative stride, as the stack's kernel and as its signal"""
    for n, k in ((300, 12), (12, 300)):
        a, b = draw((6, n), "float64", 21), draw((6, k), "float64", 22)
        (got,) = conv_exe(1, "float64", 2, "float64", 2, full, flip=True)(a, b)
        check(got, a, b[:, ::-1], full, 1, f"1-d flipped {n} * {k}")
    a, b = draw((6, 20, 30), "float64", 23), draw((6, 3, 5), "float64", 24)
    (got,) = conv_exe(2, "float64", 3, "float64", 3, full, flip=True)(a, b)
    check(got, a, b[:, :, ::-1], full, 2, "2-d flipped")


@pytest.mark.parametrize("full", [True, False])
def test_nan_and_inf_stay_in_their_item(hip, full):
    """a NaN in one item's signal, an Inf in one tap of another (which the zero padding of a "full" end must not meet)"""
    a, b = draw((5, 90), "float64", 31), draw((5, 7), "float64", 32)
    a[1, 40], b[3, 2] = np.nan, np.inf
    (got,) = conv_exe(1, "float64", 2, "float64", 2, full)(a, b)
    check(got, a, b, full, 1, "1-d NaN / Inf")
    assert np.isfinite(got[[0, 2, 4]]).all() and np.isnan(got[1]).any()
    a2, b2 = draw((5, 12, 14), "float64", 33), draw((5, 3, 4), "float64", 34)
    a2[1, 5, 5], b2[3, 1, 2] = np.nan, np.inf
    (got,) = conv_exe(2, "float64", 3, "float64", 3, full)(a2, b2)
    check(got, a2, b2, full, 2, "2-d NaN / Inf")
    assert np.isfinite(got[[0, 2, 4]]).all() and np.isnan(got[1]).any()


def test_valid_mode_of_matrices_neither_of_which_holds_the_other(hip):
    with pytest.raises(ValueError, match="one must be at least as large as the other in every dimension"):
        conv_exe(2, "float64", 3, "float64", 3, False)(np.ones((3, 5, 3)), np.ones((3, 3, 5)))


def test_one_launch_whatever_the_batch(hip):
    """the route: the launches and copies of a call (the kernel, the result's download, a cast where an operand is
    promoted) do not grow with the stack; on the per-item loop they do"""
    lib = hip.lib()
    for core_ndim, sa, sb in ((1, (60,), (7,)), (2, (9, 12), (3, 4))):
        for dta, shared, extra in (("float64", False, 0), ("float64", True, 0), ("float32", False, 1)):
            exe = conv_exe(core_ndim, dta, core_ndim + 1, "float64", core_ndim + (0 if shared else 1), True)
            counts = {}
            for items in (3, 48):
                a, b = draw((items, *sa), dta, 41), draw(sb if shared else (items, *sb), "float64", 42)
                exe(a, b)  # warm-up: allocations, module loads, the constant's upload
                c0 = lib.pthip_launch_count()
                exe(a, b)
                counts[items] = lib.pthip_launch_count() - c0
            print(f"{core_ndim}-d {dta} shared={shared}: launches and copies {counts}")
            assert counts[3] == counts[48] <= CONV_STACK_LAUNCHES + extra + 1, (core_ndim, dta, shared, counts)
