"""GPU: float16 ``Softmax`` / ``LogSoftmax`` (csrc/softmax.hip ``hsoftmax_kernel``) through the C ABI and through graphs.

Reference: the exact softmax of the half input (long double).  The kernel computes max, exp, sum and quotient in fp32
and rounds once, so with e = the exact value

    softmax:      |out - e| <= (2^-11 + (cols + 16) 2^-23) |e| + 2^-25
    log-softmax:  |out - e| <= 2^-11 |e| + 2^-22 (|x - max| + |log sum|) + (cols + 16) 2^-23 + 2^-25

(2^-25: half the smallest half subnormal).  Where |e| is beyond the largest half the result must be that infinity.
"""
import numpy as np
import pytest

import _blas_tiers_worker as dev
import blas_cases as bc
from e2e_util import activate, reference_mode

pytestmark = pytest.mark.gpu
H = np.longdouble
OVER = H(65504) * (1 + H(2) ** -12)
# tier switches of hsoftmax(): cols <= 64 eight rows per wave | a wave per row (64 | 65); a workgroup per row when
# rows < 512 and cols >= 4096 (4095 | 4096 at 3 rows, 511 | 512 rows at 4096); 16-byte packs when cols % 8 == 0
# (64, 72, 4096, 8200) | single halves (7, 65, 4095, 5000); (2, 5000) and (3, 8200) are longer than one pass of the
# workgroup tier over a row (256 single halves, 2048 halves in packs)
SHAPES = [(1, 1), (3, 7), (5, 64), (2, 65), (4, 72), (3, 4095), (3, 4096), (511, 4096), (512, 4096), (2, 5000), (3, 8200)]


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def exact(x, log):
    x = np.asarray(x).astype(H)
    d = x - x.max(-1, keepdims=True)
    ls = np.log(np.exp(d).sum(-1, keepdims=True))
    return (d - ls, d, ls) if log else (np.exp(d - ls), d, ls)


def bound(e, d, ls, log):
    cols = e.shape[-1]
    if log:
        return H(2) ** -11 * np.abs(e) + H(2) ** -22 * (np.abs(d) + np.abs(ls)) + (cols + 16) * H(2) ** -23 + H(2) ** -25
    return (H(2) ** -11 + (cols + 16) * H(2) ** -23) * np.abs(e) + H(2) ** -25


def run(hip, x, log):
    rows, cols = x.shape
    d, p = dev.upload(x.reshape(-1), 0)
    out = dev.Out(x.size, np.float16)
    lib = hip.lib()
    before = lib.pthip_launch_count()
    hip.check(lib.pthip_softmax(hip.np_dtype_code("float16"), int(log), rows, cols, p, out.ptr))
    assert lib.pthip_launch_count() - before == 1
    return out.fetch(x.shape)


def hold(got, x, log, what):
    e, d, ls = exact(x, log)
    b = bound(e, d, ls, log)
    assert got.dtype == np.float16 and got.shape == e.shape
    over = np.abs(e) - b > OVER
    assert np.array_equal(got[over].astype(H), np.sign(e[over]) * np.inf), f"{what}: beyond the largest half must be inf"
    ratio = bc.worst_ratio(got[~over], e[~over], b[~over])
    print(f"{what}: worst |err| / bound = {ratio:.3g}")
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("log", [False, True], ids=["softmax", "log_softmax"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_softmax_rows(hip, shape, log):
    x = (3 * np.random.default_rng([3, *shape]).standard_normal(shape)).astype(np.float16)
    hold(run(hip, x, log), x, log, f"{shape} log={log}")


@pytest.mark.parametrize("log", [False, True], ids=["softmax", "log_softmax"])
def test_half_softmax_extreme_rows(hip, log):
    """one 60000 among -60000s (zeros; the log form overflows to -inf), and a row whose small terms are half subnormals"""
    x = np.full((2, 100), -60000.0, np.float16)
    x[0, 37] = 60000.0
    x[1] = np.linspace(0, -19, 100)
    got = run(hip, x, log)
    hold(got, x, log, f"extreme rows log={log}")
    if not log:
        assert got[0, 37] == 1 and not np.delete(got[0], 37).any() and ((got[1] > 0) & (got[1] < 2.0**-14)).any()


@pytest.fixture(scope="module")
def pt(hip):
    pytensor = activate()
    import pytensor.tensor as ptt

    return pytensor, ptt


def test_softmax_over_axis_0_through_a_graph(hip, pt):
    pytensor, ptt = pt
    x = ptt.matrix("x", dtype="float16")
    f = pytensor.function([x], [ptt.special.softmax(x, axis=0), ptt.special.log_softmax(x, axis=0)], mode="hip")
    X = np.random.default_rng(4).standard_normal((70, 33)).astype(np.float16)
    for got, log in zip(f(X), (False, True)):
        hold(np.ascontiguousarray(got.T), np.ascontiguousarray(X.T), log, f"axis=0 log={log}")


def test_classifier_head_log_softmax_of_a_product(hip, pt):
    """log_softmax(x @ W) against the float64 value: the product y is rounded to half once (hgemm's bound dy), and a
    log-softmax moves by at most 2 max_i |dy_i| when its input moves by dy; then the log-softmax bound itself"""
    pytensor, ptt = pt
    x, W = ptt.matrix("x", dtype="float16"), ptt.matrix("W", dtype="float16")
    f = pytensor.function([x, W], ptt.special.log_softmax(ptt.dot(x, W), axis=-1), mode="hip")
    rng = np.random.default_rng(5)
    X, Wm = rng.standard_normal((33, 40)).astype(np.float16), rng.standard_normal((40, 70)).astype(np.float16)
    got = f(X, Wm)
    y, mag = X.astype(H) @ Wm.astype(H), np.abs(X).astype(H) @ np.abs(Wm).astype(H)
    dy = (H(2) ** -11 * np.abs(y) + 40 * H(2) ** -23 * mag + H(2) ** -25).max(-1, keepdims=True)
    e, d, ls = exact(y, True)
    ratio = bc.worst_ratio(got, e, 2 * dy + bound(e, d, ls, True))
    print(f"log_softmax(x @ W): worst |err| / bound = {ratio:.3g}")
    assert got.dtype == np.float16 and ratio <= 1.0, ratio


def test_attention_gradient_evaluates_and_is_as_close_as_the_reference(hip, pt):
    """d sum(attention * w) / d(q, k, v): float16 outputs of the right shapes; against the float64 gradient the largest
    error is at most twice the largest error of the reference's own float16 evaluation of the same gradient graph (both
    round every op to half, in different orders)"""
    pytensor, ptt = pt

    def grads(dtype, mode):
        q, k, v, w = (ptt.tensor(n, dtype=dtype, shape=(None,) * 3) for n in "qkvw")
        att = ptt.matmul(ptt.special.softmax(ptt.matmul(q, k.swapaxes(1, 2)) * ptt.constant(0.25, dtype=dtype), axis=-1), v)
        return pytensor.function([q, k, v, w], pytensor.grad((att * w).sum(), [q, k, v]), mode=mode)

    rng = np.random.default_rng(6)
    args = [rng.standard_normal(s).astype(np.float16) for s in ((2, 33, 16), (2, 65, 16), (2, 65, 24), (2, 33, 24))]
    got = grads("float16", "hip")(*args)
    ref16 = grads("float16", reference_mode())(*args)
    ref64 = grads("float64", reference_mode())(*[a.astype(np.float64) for a in args])
    for name, g, r16, r64, a in zip("qkv", got, ref16, ref64, args):
        assert g.dtype == np.float16 and g.shape == a.shape, (name, g.dtype, g.shape)
        mine, theirs = np.abs(g.astype(np.float64) - r64).max(), np.abs(r16.astype(np.float64) - r64).max()
        print(f"d/d{name}: hip max error {mine:.3g}, reference float16 max error {theirs:.3g}, ratio {mine / theirs:.3g}")
        assert mine <= 2 * theirs, (name, mine, theirs)
