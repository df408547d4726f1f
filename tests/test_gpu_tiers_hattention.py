"""GPU: float16 attention (csrc/hattention.hip) through the C ABI and through ``pytensor.function(mode="hip")``.

Reference: operands converted exactly to long double; ``s = scale q k^T``, ``p = exp(s - max)``, ``l = sum p``,
``o = p v / l`` there.  The kernel keeps s, p's sum and o in fp32 and rounds p to half for the second product, so

    |out - o| <= 2^-11 |o| + (2^-11 + 2 d + (T + 8) 2^-23) (p |v|) / l + 2^-25 sum_t |v_t| / l + 2^-25
    d = D 2^-23 max_t sum_d |scale q k| + 2^-22 max_t |s|

(final rounding; p as a half, relatively, and 2^-25 for its subnormal range; the fp32 score error entering numerator
and denominator through exp; the fp32 accumulation; a subnormal half result).  The unfused chain (D > 128, the 4-D
form) rounds the scores to half twice and the softmax once: d grows by 2^-10 max |s| + 2^-24 and 2^-11 becomes 2 2^-11.
Operands are views into NaN-filled parents and the output sits between sentinels (tests/blas_cases.py,
tests/_blas_tiers_worker.py), so an element read or written out of range fails the case.
"""
import numpy as np
import pytest

import _blas_tiers_worker as dev
import blas_cases as bc
from e2e_util import activate, hip_executable

pytestmark = pytest.mark.gpu
H = np.longdouble
RAMP = lambda T: np.linspace(0.1, 3.0, T)[None, :, None]
TIGHT = dict(pitch="tight", bstride="odd")
# (batch, S, T, D, Dv), scale (how, value), q/k multiplier, key ramp, operand placement
CASES = {
    "single row and key": ((1, 1, 1, 8, 8), None, 1, False, {}),
    "exact tiles": ((1, 32, 64, 16, 32), None, 1, False, {}),
    "one past a wave, one past a key tile": ((2, 33, 65, 16, 16), ("mul", 0.25), 1, False, {}),
    "one past the workgroup, 2-byte rows": ((1, 129, 130, 20, 40), ("div", 8.0), 1, False, TIGHT),
    "moving maximum, scores to 100": ((3, 40, 193, 72, 40), ("mul", 0.125), 3, True, {}),
    "Dv = 128": ((1, 129, 64, 64, 128), None, 2, True, {}),
    "largest D, five key tiles": ((2, 64, 257, 128, 128), ("mul", 0.0884), 1, False, {}),
    "shared K and V": ((4, 16, 100, 64, 64), None, 1, False, dict(shared=True)),
    "misaligned base": ((2, 33, 65, 16, 16), ("mul", 0.25), 1, False, dict(ptr=1)),
}


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def reference(q, k, v, scale):
    """(o, bound pieces) in long double for halves q (., S, D), k (., T, D), v (., T, Dv) and the factor ``scale``"""
    q, k, v = (np.asarray(x).astype(H) for x in (q, k, v))
    kT = k.transpose(0, 2, 1)
    s, mag = scale * bc.hp_matmul(q, kT), abs(scale) * bc.hp_matmul(np.abs(q), np.abs(kT))
    p = np.exp(s - s.max(-1, keepdims=True))
    l = p.sum(-1, keepdims=True)
    return bc.hp_matmul(p, v) / l, dict(pv=bc.hp_matmul(p, np.abs(v)) / l, vl=np.abs(v).sum(1, keepdims=True) / l,
                                        mag=mag.max(-1, keepdims=True), smax=np.abs(s).max(-1, keepdims=True), D=q.shape[-1], T=k.shape[1])


def bound(o, r, unfused=False):
    d = r["D"] * H(2) ** -23 * r["mag"] + H(2) ** -22 * r["smax"]
    u = H(2) ** -11
    if unfused:
        d, u = d + H(2) ** -10 * r["smax"] + H(2) ** -24, 2 * u
    return u * np.abs(o) + (u + 2 * d + (r["T"] + 8) * H(2) ** -23) * r["pv"] + H(2) ** -25 * r["vl"] + H(2) ** -25


def hold(got, q, k, v, scale, what, unfused=False):
    o, r = reference(q, k, v, H(scale))
    assert got.dtype == np.float16 and got.shape == o.shape, (what, got.dtype, got.shape, o.shape)
    ratio = bc.worst_ratio(got, o, np.broadcast_to(bound(o, r, unfused), o.shape))
    print(f"{what}: worst |err| / bound = {ratio:.3g}")
    assert ratio <= 1.0, (what, ratio)


def draw(shape, mul=1, ramp=False, seed=0):
    nb, S, T, D, Dv = shape
    rng = np.random.default_rng([seed, *shape])
    q, k, v = (rng.standard_normal(s) for s in ((nb, S, D), (nb, T, D), (nb, T, Dv)))
    k = k * RAMP(T) if ramp else k
    return (q * mul).astype(np.float16), (k * mul).astype(np.float16), v.astype(np.float16)


@pytest.mark.parametrize("name", CASES)
def test_hattention_c_abi(hip, name):
    shape, scale, mul, ramp, place = CASES[name]
    nb, S, T, D, Dv = shape
    q, k, v = draw(shape, mul, ramp)
    place = dict(place)
    if place.pop("shared", False):
        k, v = k[:1], v[:1]
    ops = [bc.embed(q, **place)] + [bc.embed(x, **place, **(dict(bstride="zero") if len(x) < nb else {})) for x in (k, v)]
    keep, ptrs = zip(*(dev.upload(op.parent, op.off) for op in ops))
    sc = dev.upload(np.array([scale[1]], np.float16), 0) if scale else (None, None)
    lib, runs = hip.lib(), []
    for _ in range(2):
        out = dev.Out(nb * S * Dv, np.float16)
        before = lib.pthip_launch_count()
        hip.check(lib.pthip_hattention(nb, S, T, D, Dv, ptrs[0], ops[0].sb, ops[0].s0, ptrs[1], ops[1].sb, ops[1].s0, ptrs[2], ops[2].sb,
                                       ops[2].s0, sc[1], int(bool(scale) and scale[0] == "div"), out.ptr))
        assert lib.pthip_launch_count() - before == 1, name
        runs.append(out.fetch((nb, S, Dv)))
    factor = 1 if not scale else (H(np.float16(scale[1])) if scale[0] == "mul" else 1 / H(np.float16(scale[1])))
    hold(runs[0], q, k, v, factor, name)
    assert np.array_equal(runs[0].view(np.uint16), runs[1].view(np.uint16)), "two runs differ"


def test_hattention_refuses_what_it_cannot_run(hip):
    lib = hip.lib()
    assert lib.pthip_hattention_max_d() == 128
    before = lib.pthip_launch_count()
    assert lib.pthip_hattention(1, 4, 4, 136, 8, None, 0, 136, None, 0, 136, None, 0, 8, None, 0, None) != 0 and b"136" in lib.pthip_last_error()
    assert lib.pthip_hattention(1, 4, 0, 8, 8, None, 0, 8, None, 0, 8, None, 0, 8, None, 0, None) != 0
    assert lib.pthip_launch_count() == before


# ---- through the graph ------------------------------------------------------------------------------------------------
# form -> (ndim, shape, how the scale enters, fused?)
FORMS = {
    "3-D, constant scale": (3, (2, 33, 65, 16, 24), "const", True),
    "2-D, Dot22Scalar": (2, (1, 70, 40, 24, 16), "const", True),
    "3-D, runtime divisor": (3, (2, 33, 65, 16, 24), "div", True),
    "D = 136: the unfused chain": (3, (2, 33, 65, 136, 24), "const", False),
    "4-D stack": (4, (6, 33, 65, 16, 16), "const", False),
}


@pytest.mark.parametrize("form", FORMS)
def test_attention_through_the_graph(hip, form):
    pytensor = activate()
    import pytensor.tensor as ptt

    nd, shape, how, fused = FORMS[form]
    q, k, v = (ptt.tensor(n, dtype="float16", shape=(None,) * nd) for n in "qkv")
    c = ptt.scalar("c", dtype="float16")
    s = ptt.matmul(q, k.swapaxes(-1, -2)) if nd > 2 else ptt.dot(q, k.T)
    s = s / c if how == "div" else s * ptt.constant(0.25, dtype="float16")
    p = ptt.special.softmax(s, axis=-1)
    f = pytensor.function([q, k, v] + ([c] if how == "div" else []), ptt.matmul(p, v) if nd > 2 else ptt.dot(p, v), mode="hip")
    ops = [n.op for n in hip_executable(f).graph.nodes]
    if nd < 4:
        assert ops.count("Attention") == 1 and "Softmax" not in ops, ops
    Q, K, V = draw(shape, seed=1)
    lead = {2: (), 3: shape[:1], 4: (2, 3)}[nd]
    args = [x.reshape(*lead, *x.shape[1:]) for x in (Q, K, V)] + ([np.float16(4.0)] if how == "div" else [])
    before = hip.lib().pthip_launch_count()
    got = f(*args)
    launches = hip.lib().pthip_launch_count() - before
    assert (launches > 1) if not fused else True, launches
    hold(got.reshape(shape[0], shape[1], shape[4]), Q, K, V, 0.25, form, unfused=not fused)
    assert np.array_equal(got.view(np.uint16), f(*args).view(np.uint16)) and np.array_equal(got.view(np.uint16), f(*args).view(np.uint16))


def test_masked_attention_is_not_fused_and_evaluates(hip):
    pytensor = activate()
    import pytensor.tensor as ptt

    q, k, v, m = (ptt.tensor(n, dtype="float16", shape=(None,) * 3) for n in "qkvm")
    f = pytensor.function([q, k, v, m], ptt.matmul(ptt.special.softmax(ptt.matmul(q, k.swapaxes(1, 2)) + m, axis=-1), v), mode="hip")
    ops = [n.op for n in hip_executable(f).graph.nodes]
    assert "Attention" not in ops and "Softmax" in ops, ops
    Q, K, V = draw((2, 33, 65, 16, 24), seed=2)
    mask = np.where(np.arange(65)[None, None, :] > np.arange(33)[None, :, None] + 32, -np.inf, 0).astype(np.float16)
    got = f(Q, K, V, np.broadcast_to(mask, (2, 33, 65)))
    # keys behind the mask carry no weight: the same as attention over the keys in front of it, row by row
    assert got.shape == (2, 33, 24) and got.dtype == np.float16 and np.isfinite(got).all()
    hold(got[:, :1], Q[:, :1], K[:, :33], V[:, :33], 1, "masked, first row", unfused=True)
