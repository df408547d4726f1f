"""GPU: jv / ive / kve / owens_t (and iv, kv, kn, their gradients) under ``mode="hip"``.

The device values are held to the mpmath fixtures at the bars of tests/test_special_bessel_host.py, to SciPy's
special values bit for bit, and to the reference's C linker (which evaluates these ops through SciPy) on graphs:
grad(i1), log(iv) / log(kv) where the unscaled forms overflow, kn, a jv inside a Scan step and a many-term
graph.  Two calls, and a replayed plan against eager execution, give the same bits.
"""
import numpy as np
import pytest

import e2e_util as E
from test_special_bessel_host import BARS, FAR, GOLDEN, special_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    pytensor = E.activate()
    if not E.have_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import pytensor.tensor as ptt

    return pytensor, ptt


def _binary(pytensor, ptt, name, dtype="float64"):
    a, b = ptt.vector("a", dtype=dtype), ptt.vector("b", dtype=dtype)
    return pytensor.function([a, b], getattr(ptt, name)(a, b), mode="hip")


@pytest.mark.parametrize("name", ["jv", "ive", "kve", "owens_t"])
def test_fixtures_fp64(pt, name):
    pytensor, ptt = pt
    d = np.load(GOLDEN)[name]
    got = _binary(pytensor, ptt, name)(d[:, 0], d[:, 1])
    err = np.abs(got - d[:, 2]) / d[:, 3]
    far = np.abs(d[:, 1]) > 1e4 if name != "owens_t" else np.zeros(len(d), bool)
    assert np.isfinite(got).all()
    assert err[~far].max() <= BARS[name], d[~far][np.argmax(err[~far])]
    if far.any():
        assert err[far].max() <= FAR


@pytest.mark.parametrize("name", ["jv", "ive", "kve", "owens_t"])
def test_fixtures_fp32_within_one_ulp_of_scipy(pt, name):
    import scipy.special as sp

    pytensor, ptt = pt
    d = np.load(GOLDEN)[name]
    ok = (np.abs(d[:, :2]) < 1e38).all(axis=1)
    ok[ok] = (d[ok, :2].astype(np.float32).astype(np.float64) == d[ok, :2]).all(axis=1)
    a, b = d[ok, 0].astype(np.float32), d[ok, 1].astype(np.float32)
    got = _binary(pytensor, ptt, name, "float32")(a, b)
    assert got.dtype == np.float32
    ref = getattr(sp, name)(a, b)
    fin = np.isfinite(ref) & (np.abs(ref) > np.finfo(np.float32).tiny)
    assert (np.abs(got[fin] - ref[fin]) <= np.spacing(np.abs(ref[fin]).astype(np.float32))).all()


def test_special_values_bit_for_bit(pt):
    pytensor, ptt = pt
    table = special_table()
    for name in ("jv", "ive", "kve", "owens_t"):
        rows = [r for r in table if r[0] == name]
        a = np.array([r[1] for r in rows])
        b = np.array([r[2] for r in rows])
        want = np.array([r[3] for r in rows])
        got = _binary(pytensor, ptt, name)(a, b)
        same = (np.isnan(got) & np.isnan(want)) | ((got == want) & (np.signbit(got) == np.signbit(want)))
        assert same.all(), [(r, g) for r, g, s in zip(rows, got, same) if not s]


def _inputs(rng, n=4096, xmax=50.0):
    v = rng.uniform(-10, 10, n)
    x = rng.uniform(1e-3, xmax, n)
    return v, x


def test_grad_i1_against_the_c_linker(pt):
    pytensor, ptt = pt
    x = ptt.dvector("x")
    # x > 0: the existing I0 / I1 lowering (the device library's cyl_bessel_i0 / i1) gives NaN for x < 0
    xv = np.random.default_rng(0).uniform(1e-3, 30, 4096)
    E.compare_hip_and_cvm([x], [ptt.i1(x), pytensor.grad(ptt.i1(x).sum(), x)], [xv], rtol=1e-12)


def test_log_iv_and_log_kv_with_gradients_where_unscaled_overflows(pt):
    pytensor, ptt = pt
    v, x = ptt.dvector("v"), ptt.dvector("x")
    rng = np.random.default_rng(1)
    vv = rng.uniform(0, 20, 2048)
    xv = np.concatenate([rng.uniform(1e-2, 50, 1024), rng.uniform(700, 1000, 1024)])
    liv, lkv = ptt.log(ptt.iv(v, x)), ptt.log(ptt.kv(v, x))
    outs = [liv, lkv, pytensor.grad(liv.sum(), x), pytensor.grad(lkv.sum(), x)]
    E.compare_hip_and_cvm([v, x], outs, [vv, xv], rtol=1e-11)


def test_kn_against_the_c_linker(pt):
    pytensor, ptt = pt
    n, x = ptt.lvector("n"), ptt.dvector("x")
    rng = np.random.default_rng(2)
    E.compare_hip_and_cvm([n, x], [ptt.kn(n, x)], [rng.integers(-20, 20, 4096), rng.uniform(1e-2, 60, 4096)], rtol=1e-12)


def test_jv_inside_a_scan_step(pt):
    pytensor, ptt = pt
    x = ptt.dvector("x")
    ys, _ = pytensor.scan(lambda k, acc: acc + ptt.jv(k - 2.5, x), sequences=[ptt.arange(6.0)], outputs_info=[ptt.zeros_like(x)])
    xv = np.random.default_rng(3).uniform(0.1, 40, 1024)
    E.compare_hip_and_cvm([x], [ys[-1]], [xv], rtol=1e-10, atol=1e-12)


def test_many_term_graph_with_owens_t_and_ive(pt):
    pytensor, ptt = pt
    v, x, h = ptt.dvector("v"), ptt.dvector("x"), ptt.dvector("h")
    rng = np.random.default_rng(4)
    vv, xv = _inputs(rng)
    hv = rng.uniform(-5, 5, vv.size)
    terms = [ptt.owens_t(h, x / 10).sum(), ptt.ive(v, x).sum(), (ptt.log(ptt.kve(v, x))).sum(), ptt.jv(v, x).sum(),
             (h * x).sum(), ptt.exp(-x).sum()]
    logp = sum(terms)
    outs = [logp, *pytensor.grad(logp, [x, h])]
    E.compare_hip_and_cvm([v, x, h], outs, [vv, xv, hv], rtol=1e-10)


def test_bits_reproduce_and_replay_matches_eager(pt):
    pytensor, ptt = pt
    v, x, h = ptt.dvector("v"), ptt.dvector("x"), ptt.dvector("h")
    rng = np.random.default_rng(5)
    vv, xv = _inputs(rng, 1 << 16)
    hv = rng.uniform(-5, 5, vv.size)
    outs = [ptt.jv(v, x), ptt.ive(v, x), ptt.kve(v, x), ptt.owens_t(h, x / 10), (ptt.jv(v, x) * ptt.owens_t(h, v)).sum()]
    f = pytensor.function([v, x, h], outs, mode="hip")
    runs = [f(vv, xv, hv) for _ in range(3)]  # eager, capture, replay
    with pytensor.config.change_flags(hip__auto_freeze=False):
        g = pytensor.function([v, x, h], outs, mode="hip")
    eager = [g(vv, xv, hv) for _ in range(2)]
    for r in runs[1:] + eager:
        for a, b in zip(runs[0], r):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
