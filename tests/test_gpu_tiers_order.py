"""GPU: the order- and index-defined kernels through the C ABI, bit for bit against NumPy: ``pthip_sort`` (both tiers, one
to three far phases, several rows), ``pthip_cumulative``, ``pthip_argmax``, ``pthip_nonzero`` (the carry across the scan
kernel's 256-count chunks) and ``pthip_searchsorted`` (every comparison type, the grid-stride loop's second pass).

Inputs lie inside poisoned parents, outputs between sentinels with all-ones bytes in between (the guarded buffers of
tests/_softmax_tiers_worker.py); every call's launch count is held to what the host code makes.
"""
import numpy as np
import pytest

import order_cases as oc
import reduce_cases as rc
import _softmax_tiers_worker as dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from pytensor_amd import ffi

    if ffi.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ffi.init(0)
    return ffi


def gin(x, off=0):
    """upload ``x`` behind ``LEAD + off`` poisoned elements, 8 more behind it: (keepalive, pointer)"""
    x = np.ascontiguousarray(x)
    lead = rc.LEAD + off
    parent = np.full(lead + x.size + 8, rc.poison(x.dtype), dtype=x.dtype)
    parent[lead:lead + x.size] = x.reshape(-1)
    return dev.upload(parent, lead)


def launches_of(lib, fn):
    before = lib.pthip_launch_count()
    r = fn()
    return r, int(lib.pthip_launch_count() - before)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape}, expected {want.dtype}{want.shape}"
    ne = rc.bits(got) != rc.bits(want)
    if ne.any():
        i = tuple(int(v) for v in np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {got.size} differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


# ---------------------------------------------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------------------------------------------
def _sort_call(hip, x, vals=True, idx=True, off=0):
    lib = hip.lib()
    rows, n = x.shape
    keep, px = gin(x, off)
    ov = dev.Out(rows * n, x.dtype, off) if vals else None
    oi = dev.Out(rows * n, np.int64) if idx else None
    r, launches = launches_of(lib, lambda: lib.pthip_sort(hip.np_dtype_code(x.dtype), rows, n, px, ov.ptr if ov else None, oi.ptr if oi else None))
    hip.check(r)
    assert launches == oc.sort_launches(rows, n), f"{launches} launches for {rows} x {n}"
    del keep
    return (ov.fetch((rows, n)) if ov else None), (oi.fetch((rows, n)) if oi else None)


def _sort_check(hip, x, what, **kw):
    want_i = np.argsort(x, axis=1, kind="stable").astype(np.int64)
    want_v = np.take_along_axis(x, want_i, axis=1)
    got_v, got_i = _sort_call(hip, x, **kw)
    if got_i is not None:
        same_bits(got_i, want_i, f"{what}: indices")
    if got_v is not None:
        same_bits(got_v, want_v, f"{what}: values")
        if x.dtype.kind != "f":
            assert np.array_equal(got_v, np.sort(x, axis=1))


@pytest.mark.parametrize("dt", oc.SORT_DTYPES)
@pytest.mark.parametrize("n", oc.SORT_N_LDS + oc.SORT_N_LONG)
def test_sort(hip, n, dt):
    for rows in ((2,) if n <= oc.SORT_TILE else (1, 3)):
        for j, kind in enumerate(oc.sort_kinds(dt)):
            x = oc.sort_data(kind, dt, rows, n)
            _sort_check(hip, x, f"sort {dt} {rows} x {n} {kind}", off=j % 2)
            if j == 0:
                _sort_check(hip, x, f"sort {dt} {rows} x {n} {kind}, values only", idx=False)
                _sort_check(hip, x, f"sort {dt} {rows} x {n} {kind}, indices only", vals=False)


def test_sort_empty(hip):
    lib = hip.lib()
    for rows, n in ((0, 5), (3, 0)):
        out = dev.Out(8, np.float64)
        r, launches = launches_of(lib, lambda: lib.pthip_sort(hip.np_dtype_code("float64"), rows, n, out.ptr, out.ptr, None))
        hip.check(r)
        assert launches == 0
        out.fetch()
    r, launches = launches_of(lib, lambda: lib.pthip_sort(hip.np_dtype_code("float16"), 1, 4, None, None, None))
    assert r != 0 and launches == 0 and b"pthip_sort: unsupported dtype" in lib.pthip_last_error()


# ---------------------------------------------------------------------------------------------------------------
# cumulative
# ---------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = ((1, 1000, 1), (3, 17, 257), (257, 5, 1), (2, 1, 300))


def _scan_data(dt, shape, mul, special):
    dt = np.dtype(dt)
    rng = np.random.default_rng([shape[0], shape[1], shape[2], dt.itemsize, mul])
    if dt.kind == "f":
        x = (rng.uniform(0.5, 1.5, shape) * np.where(rng.random(shape) < 0.3, -1, 1) if mul else rng.standard_normal(shape)).astype(dt)
        if special and x.size:
            # NaN and infinities enter part way down some lines and are carried from there
            x[0, shape[1] // 2, 0] = np.nan
            x[-1, shape[1] // 3, -1] = np.inf
            if shape[1] > 3:
                x[-1, shape[1] - 1, -1] = -np.inf if not mul else 0.0
        return x
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)  # narrow sums and every product wrap


@pytest.mark.parametrize("dt", oc.SCAN_DTYPES)
@pytest.mark.parametrize("shape", SCAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cumulative(hip, shape, dt):
    lib = hip.lib()
    for mul in (0, 1):
        for special in ((False, True) if np.dtype(dt).kind == "f" else (False,)):
            x = _scan_data(dt, shape, mul, special)
            with np.errstate(all="ignore"):
                want = (np.cumprod if mul else np.cumsum)(x, axis=1, dtype=x.dtype)
            for off in (0, 1):
                keep, px = gin(x, off)
                out = dev.Out(x.size, dt, off)
                r, launches = launches_of(lib, lambda: lib.pthip_cumulative(hip.np_dtype_code(dt), mul, *shape, px, out.ptr))
                hip.check(r)
                assert launches == 1
                rc.check_exact(out.fetch(shape), want, f"cumulative {dt} {shape} mul={mul} special={special}")
                del keep
            if special:
                assert np.isnan(want).any() and np.isinf(want).any()


def test_cumulative_empty(hip):
    lib = hip.lib()
    for shape in ((0, 5, 3), (3, 0, 4), (3, 5, 0)):
        out = dev.Out(8, np.float64)
        r, launches = launches_of(lib, lambda: lib.pthip_cumulative(hip.np_dtype_code("float64"), 0, *shape, out.ptr, out.ptr))
        hip.check(r)
        assert launches == 0
        out.fetch()
    r, launches = launches_of(lib, lambda: lib.pthip_cumulative(hip.np_dtype_code("bool"), 0, 1, 1, 1, None, None))
    assert r != 0 and launches == 0 and b"pthip_cumulative: unsupported dtype" in lib.pthip_last_error()


# ---------------------------------------------------------------------------------------------------------------
# argmax
# ---------------------------------------------------------------------------------------------------------------
def _argmax_cases(dt, rows, R):
    dt = np.dtype(dt)
    rng = np.random.default_rng([rows, R, dt.itemsize, dt.kind == "u"])
    if dt.kind == "f":
        lowest, base = -np.inf, np.round(rng.standard_normal((rows, R)) * 2).astype(dt)  # (rounded: ties)
    else:
        lowest = np.iinfo(dt).min
        base = rng.integers(max(lowest, -3), 4, (rows, R)).astype(dt)
    yield "ties", base
    yield "lowest everywhere", np.full((rows, R), lowest, dtype=dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        yield "extremes", np.array([info.min, info.max, info.max - 1, info.min + 1], dtype=dt)[rng.integers(0, 4, (rows, R))]
    if dt == np.uint64:
        yield "above 2^63", (rng.integers(0, 4, (rows, R), dtype=np.uint64) + np.uint64((1 << 63) - 2))
    if dt.kind == "f":
        yield "all -inf but one", np.where(np.arange(R)[None, :] == (np.arange(rows)[:, None] % R), dt.type(-1e30), dt.type(-np.inf)).astype(dt)
        x = base.copy()
        top = x.argmax(axis=1)
        for r_ in range(rows):  # NaN at position 0, behind the maximum, in front of it, none: by row
            where = (0, min(top[r_] + 1, R - 1), max(top[r_] - 1, 0), None)[r_ % 4]
            if where is not None:
                x[r_, where] = np.nan
        yield "nan", x


@pytest.mark.parametrize("dt", oc.SCAN_DTYPES)
@pytest.mark.parametrize("R", (1, 2, 1000))
@pytest.mark.parametrize("rows", (1, 255, 256, 257))
def test_argmax(hip, rows, R, dt):
    lib = hip.lib()
    for j, (kind, x) in enumerate(_argmax_cases(dt, rows, R)):
        keep, px = gin(x, j % 2)
        out = dev.Out(rows, np.int64)
        r, launches = launches_of(lib, lambda: lib.pthip_argmax(hip.np_dtype_code(dt), rows, R, px, out.ptr))
        hip.check(r)
        assert launches == 1
        same_bits(out.fetch(), np.argmax(x, axis=1).astype(np.int64), f"argmax {dt} {rows} x {R} {kind}")
        del keep


def test_argmax_refusals(hip):
    lib = hip.lib()
    out = dev.Out(4, np.int64)
    r, launches = launches_of(lib, lambda: lib.pthip_argmax(hip.np_dtype_code("float64"), 4, 0, out.ptr, out.ptr))
    assert r != 0 and launches == 0 and b"pthip_argmax: attempt to get argmax of an empty sequence" in lib.pthip_last_error()
    r, launches = launches_of(lib, lambda: lib.pthip_argmax(hip.np_dtype_code("float64"), 0, 3, out.ptr, out.ptr))
    hip.check(r)
    assert launches == 0
    out.fetch()


# ---------------------------------------------------------------------------------------------------------------
# nonzero
# ---------------------------------------------------------------------------------------------------------------
def _masks(n):
    rng = np.random.default_rng(n)
    yield "all true", np.ones(n, np.uint8)
    yield "all false", np.zeros(n, np.uint8)
    last = np.zeros(n, np.uint8)
    last[n - 1:] = 1
    yield "last byte", last
    yield "1 %", (rng.random(n) < 0.01).astype(np.uint8)
    yield "99 %", (rng.random(n) < 0.99).astype(np.uint8)
    yield "bytes other than 1", np.where(rng.random(n) < 0.5, rng.integers(2, 256, n), 0).astype(np.uint8)


@pytest.mark.parametrize("n", (0, 1, 15, 16, 17, 4095, 4096, 4097, 256 * 4096 + 1))
def test_nonzero(hip, n):
    lib = hip.lib()
    for j, (kind, mask) in enumerate(_masks(n)):
        keep, pm = gin(mask, j % 2)  # (the bytes around the mask are non-zero)
        idx, count = dev.Out(n, np.int64), dev.Out(1, np.int64)
        r, launches = launches_of(lib, lambda: lib.pthip_nonzero(n, pm, idx.ptr, count.ptr))
        hip.check(r)
        assert launches == (3 if n > 0 else 1), f"{launches} launches"  # count, scan, write; the count word alone is cleared for n = 0
        want = np.flatnonzero(mask).astype(np.int64)
        k = int(count.fetch()[0])
        assert k == want.size, f"nonzero {n} {kind}: count {k}, expected {want.size}"
        got = idx.fetch()
        same_bits(got[:k], want, f"nonzero {n} {kind}")
        assert np.all(got[k:] == -1), f"nonzero {n} {kind}: idx_out behind the count was written"
        del keep


# ---------------------------------------------------------------------------------------------------------------
# searchsorted
# ---------------------------------------------------------------------------------------------------------------
def _search(hip, x, v, right, sorter=None, off=0):
    lib = hip.lib()
    kx, px = gin(x, off)
    kv, pv = gin(v, off)
    ks, ps = gin(sorter.astype(np.int64)) if sorter is not None else (None, None)
    out = dev.Out(v.size, np.int64)
    r, launches = launches_of(lib, lambda: lib.pthip_searchsorted(hip.np_dtype_code(x.dtype), x.size, px, ps, hip.np_dtype_code(v.dtype), v.size, pv,
                                                                  int(right), out.ptr))
    hip.check(r)
    assert launches == (1 if v.size else 0)
    got = out.fetch()
    del kx, kv, ks
    return got


@pytest.mark.parametrize("xdt,vdt", oc.SEARCH_PAIRS, ids=lambda d: d)
def test_searchsorted(hip, xdt, vdt):
    rng = np.random.default_rng([len(xdt), len(vdt), np.dtype(xdt).itemsize, np.dtype(vdt).itemsize])
    for n, m in ((1000, 300), (1, 40), (2, 40), (0, 7), (5, 0), (77, 1)):
        x = oc.search_values(xdt, n, rng, sort=True)
        v = oc.search_values(vdt, m, rng)
        if np.dtype(vdt).kind == "f" and m > 3:
            v[::7] = np.nan  # NaN keys go behind everything
        if np.dtype(xdt).kind == "f" and n > 10:
            x[-5:] = np.nan  # NaNs at the end of x, as np.sort leaves them
        perm = rng.permutation(n)
        shuffled = x[perm]
        sorter = np.argsort(shuffled, kind="stable")
        for side in ("left", "right"):
            what = f"searchsorted {xdt} x {vdt} n={n} m={m} {side}"
            want = np.searchsorted(x, v, side=side).astype(np.int64)
            same_bits(_search(hip, x, v, side == "right", off=(side == "right")), want, what)
            want = np.searchsorted(shuffled, v, side=side, sorter=sorter).astype(np.int64)
            same_bits(_search(hip, shuffled, v, side == "right", sorter), want, what + " through a sorter")


def test_searchsorted_uint64_above_2_63(hip):
    """the cases of the defect: keys and array values from 2^63 on compared as negative numbers"""
    x = np.array([1, 2 ** 63 + 5], dtype=np.uint64)
    v = np.array([2 ** 63, 0, 2 ** 63 + 5, 2 ** 63 + 6, 2 ** 64 - 1, 1], dtype=np.uint64)
    for side in ("left", "right"):
        same_bits(_search(hip, x, v, side == "right"), np.searchsorted(x, v, side=side).astype(np.int64), f"uint64 {side}")
    assert _search(hip, x, v[:1], False)[0] == 1
    # uint64 with a signed integer: NumPy compares the pair as float64
    vi = np.array([-1, 0, 2, 2 ** 62, -2 ** 63, 2 ** 63 - 1], dtype=np.int64)
    for side in ("left", "right"):
        same_bits(_search(hip, x, vi, side == "right"), np.searchsorted(x, vi, side=side).astype(np.int64), f"uint64 x int64 {side}")
    xi = np.array([-2 ** 63, -2 ** 63, -1, 0, 2 ** 63 - 1, 2 ** 63 - 1], dtype=np.int64)
    for vv in (np.array([-2 ** 63, 2 ** 63 - 1, 0, -1, -2 ** 63 + 1, 2 ** 63 - 2], dtype=np.int64), v):
        for side in ("left", "right"):
            same_bits(_search(hip, xi, vv, side == "right"), np.searchsorted(xi, vv, side=side).astype(np.int64), f"int64 extremes x {vv.dtype} {side}")


def test_searchsorted_second_pass_of_the_grid(hip):
    m = 8192 * 256 + 1
    rng = np.random.default_rng(5)
    x = np.sort(np.round(rng.standard_normal(1000) * 50))
    v = np.round(rng.standard_normal(m) * 60)
    v[-1] = 1e9  # the one key of the second pass
    same_bits(_search(hip, x, v, False), np.searchsorted(x, v).astype(np.int64), "2 M keys")
