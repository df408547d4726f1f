"""Shapes, data and the restated host decisions of the order kernels: ``pthip_sort`` (csrc/sort.hip), ``pthip_cumulative``
and ``pthip_argmax`` (csrc/scanops.hip), ``pthip_nonzero`` (csrc/nonzero.hip), ``pthip_searchsorted`` (csrc/misc.hip).

Pure NumPy: imported by tests/test_gpu_tiers_order.py (GPU) and tests/test_reduce_cases.py (the CPU checks).  All of
these kernels are index- or order-defined: every comparison with NumPy is bit for bit.
"""
import numpy as np

SORT_DTYPES = ("float64", "float32", "int64", "int32", "int16", "int8", "uint8", "bool", "uint16", "uint32", "uint64")
SCAN_DTYPES = tuple(d for d in SORT_DTYPES if d != "bool")
SORT_TILE = 4096
SORT_N_LDS = (1, 2, 3, 255, 256, 257, 4095, 4096)
SORT_N_LONG = (4097, 8193, 16385)  # one, two and three far phases


def sort_padded(n):
    P = 2
    while P < n:
        P <<= 1
    return P


def sort_far_phases(n):
    P, k, c = sort_padded(n), 2 * SORT_TILE, 0
    while k <= P:
        c, k = c + 1, k << 1
    return c


def sort_launches(rows, n):
    """one launch in LDS; else the copy, the first tile pass, per far phase its far steps and a tile pass, the store"""
    if rows == 0 or n == 0:
        return 0
    P = sort_padded(n)
    if P <= SORT_TILE:
        return 1
    count, k = 2, 2 * SORT_TILE
    while k <= P:
        j = k >> 1
        while j >= SORT_TILE:
            count, j = count + 1, j >> 1
        count, k = count + 1, k << 1
    return count + 1


def _nan_bits(rng, dt, size):
    """NaNs of differing payload and sign"""
    if dt == np.float64:
        b = np.uint64(0x7FF0000000000000) | rng.integers(1, 1 << 52, size, dtype=np.uint64) | (rng.integers(0, 2, size, dtype=np.uint64) << np.uint64(63))
        return b.view(np.float64)
    b = np.uint32(0x7F800000) | rng.integers(1, 1 << 23, size, dtype=np.uint32) | (rng.integers(0, 2, size, dtype=np.uint32) << np.uint32(31))
    return b.view(np.float32)


def sort_kinds(dt):
    dt = np.dtype(dt)
    kinds = ["four", "sorted", "reversed", "equal", "extremes"]
    if dt.kind in "if":
        kinds.append("negative")
    if dt == np.uint64:
        kinds.append("high")
    if dt.kind == "f":
        kinds += ["nan", "infzero"]
    return kinds


def sort_data(kind, dt, rows, n, seed=0):
    dt = np.dtype(dt)
    rng = np.random.default_rng([seed, rows, n, dt.itemsize, sum(map(ord, kind + dt.kind))])
    shape = (rows, n)
    if dt.kind == "b":
        x = rng.integers(0, 2, shape).astype(bool)
        return {"sorted": np.sort(x, axis=1), "reversed": np.sort(x, axis=1)[:, ::-1].copy(), "equal": np.ones(shape, bool)}.get(kind, x)
    if dt.kind == "f":
        lo, hi = np.finfo(dt).min, np.finfo(dt).max
        wide = rng.standard_normal(shape).astype(dt)
    else:
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        wide = rng.integers(lo, hi, shape, dtype=dt, endpoint=True)
    if kind == "four":
        vals = np.array([lo, hi, 3, 100], dtype=dt) if dt.kind != "f" else np.array([-1.5, 0.25, 2.0, 1e30], dtype=dt)
        return vals[rng.integers(0, 4, shape)]
    if kind == "sorted":
        return np.sort(wide, axis=1)
    if kind == "reversed":
        return np.sort(wide, axis=1)[:, ::-1].copy()
    if kind == "equal":
        return np.full(shape, wide.flat[0] if wide.size else 0, dtype=dt)
    if kind == "extremes":
        near = [lo, hi, np.nextafter(dt.type(lo), dt.type(0)), np.nextafter(dt.type(hi), dt.type(0))] if dt.kind == "f" else [lo, hi, lo + 1, hi - 1]
        return np.array(near + [1], dtype=dt)[rng.integers(0, 5, shape)]
    if kind == "negative":
        return (-np.abs(wide) - 1).astype(dt) if dt.kind == "f" else rng.integers(lo, -1, shape, dtype=dt, endpoint=True)
    if kind == "high":
        return (rng.integers(0, 1 << 62, shape, dtype=np.uint64) * np.uint64(2) + np.uint64(1 << 63)).astype(dt)
    if kind == "nan":
        x = wide.copy()
        m = rng.random(shape) < 0.2
        x[m] = _nan_bits(rng, dt, int(m.sum()))
        return x
    assert kind == "infzero"
    return np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0], dtype=dt)[rng.integers(0, 6, shape)]


# ---- searchsorted: the (x, v) dtype pairs and the comparison type the kernel must choose for them ----
SEARCH_PAIRS = (
    ("float64", "float64"), ("float32", "float64"), ("float16", "float16"), ("float16", "int32"), ("int64", "float32"), ("float64", "int64"),
    ("float32", "uint64"),
    ("int64", "int64"), ("int32", "int8"), ("uint8", "int16"), ("uint32", "int64"), ("bool", "int8"),
    ("uint64", "uint64"), ("uint64", "uint32"), ("uint16", "uint64"), ("bool", "uint64"), ("uint64", "bool"),
    ("uint64", "int64"), ("uint64", "int8"), ("int64", "uint64"), ("int32", "uint64"),
)


def search_path(xdt, vdt):
    """``pthip_searchsorted`` restated: "float" (compare as float64), "signed" (as int64) or "unsigned" (as uint64)"""
    kx, kv = np.dtype(xdt), np.dtype(vdt)
    if "f" in (kx.kind, kv.kind):
        return "float"
    if np.uint64 in (kx, kv):
        return "float" if "i" in (kx.kind, kv.kind) else "unsigned"
    return "signed"


def search_values(dt, size, rng, sort=False):
    """values of ``dt`` that collide often (long runs of ties) and sit at the type's edges; uint64 around 2^63"""
    dt = np.dtype(dt)
    if dt.kind == "b":
        x = rng.integers(0, 2, size).astype(bool)
    elif dt.kind == "f":
        x = np.round(rng.standard_normal(size) * 4).astype(dt) / dt.type(2)
    else:
        info = np.iinfo(dt)
        mid = (1 << 63) if dt == np.uint64 else 0
        pool = [info.min, info.min + 1, info.max - 1, info.max] + [mid + d for d in range(-6, 7) if info.min <= mid + d <= info.max]
        x = np.array(pool, dtype=dt)[rng.integers(0, len(pool), size)]
    return np.sort(x) if sort else x
