"""Sparse kernels on the device (csrc/sparse.hip): SpMV / SpMM (k = 1, 8) and the CSR transpose, plus a CAR
logp+grad evaluation against the reference's C linker.

Matrices: the 5-point 2-D grid Laplacian at 1e6 and 1e7 rows (5 nnz per row) and a power-law row-length matrix
(Zipf row lengths, mean ~8).  Cold HBM: each operand set is replicated until the rotation covers >= 1.5 GiB, so
the 256 MiB Infinity Cache serves nothing; the reported time is the mean over the rotation (HIP events around
the whole rotation, no host sync inside).  Roofline in algorithmic bytes:
  SpMV / SpMM: nnz*(sizeof(dtype)+4) + (m+1)*4 + n*k*sizeof(dtype) (B, gathered at least once) + m*k*sizeof(dtype)
  transpose:   2 * nnz*(sizeof(dtype)+4) + (m+1)*4 + (n+1)*4
fraction = bytes / time / 8 TB/s.  One JSON line per case.   usage: python tools/bench_sparse.py [--quick]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from pytensor_amd import ffi  # noqa: E402
from pytensor_amd.device import DeviceArray  # noqa: E402

HBM = 8e12
ROTATE = 1.5 * 2**30


def laplacian(side):
    n = side * side
    idx = np.arange(n).reshape(side, side)
    r = [idx.ravel()]
    c = [idx.ravel()]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:, 1:], idx[:, :-1]), (idx[:-1, :], idx[1:, :]), (idx[1:, :], idx[:-1, :])):
        r.append(a.ravel())
        c.append(b.ravel())
    r, c = np.concatenate(r), np.concatenate(c)
    v = np.where(r == c, 4.0, -1.0)
    return sp.csr_matrix((v, (r, c)), shape=(n, n))


def power_law(n, seed=0):
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.zipf(1.8, n), 20000).astype(np.int64)
    lens = (lens * (8.0 / lens.mean())).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cols = rng.integers(0, n, int(indptr[-1]), dtype=np.int32)
    return sp.csr_matrix((rng.standard_normal(cols.size), cols, indptr), shape=(n, n))


def upload(A):
    return [DeviceArray.from_host(np.ascontiguousarray(a)) for a in (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32))]


def timed(lib, fns, reps=3):
    e0, e1 = C.c_void_p(), C.c_void_p()
    ffi.check(lib.pthip_event_create(C.byref(e0)))
    ffi.check(lib.pthip_event_create(C.byref(e1)))
    for f in fns:  # warm: code loaded, pool filled
        f()
    ffi.check(lib.pthip_synchronize())
    ffi.check(lib.pthip_event_record(e0))
    for _ in range(reps):
        for f in fns:
            f()
    ffi.check(lib.pthip_event_record(e1))
    ffi.check(lib.pthip_event_synchronize(e1))
    ms = C.c_float()
    ffi.check(lib.pthip_event_elapsed_ms(e0, e1, C.byref(ms)))
    lib.pthip_event_destroy(e0)
    lib.pthip_event_destroy(e1)
    return ms.value / (reps * len(fns))


def bench_matrix(lib, name, A):
    m, n = A.shape
    nnz = A.nnz
    lens = np.diff(A.indptr)
    lanes = 1 if nnz / m <= 6 else 4 if nnz / m <= 24 else 16 if nnz / m <= 96 else 64
    has_long = int(lens.max() > 1024)
    mat_bytes = nnz * 12 + (m + 1) * 4
    for k in (1, 8):
        per = mat_bytes + (n + m) * k * 8
        copies = max(1, min(32, int(np.ceil(ROTATE / per))))
        sets = []
        for c in range(copies):
            d, i, p = upload(A)
            B = DeviceArray.from_host(np.random.default_rng(c).standard_normal((n, k)))
            out = DeviceArray.empty((m, k), "float64")
            sets.append((d, i, p, B, out))

        def mk(s):
            d, i, p, B, out = s
            return lambda: ffi.check(lib.pthip_csr_spmm(7, m, n, k, nnz, d.ptr, i.ptr, p.ptr, B.ptr, k, 1, out.ptr, k, 1, lanes, has_long))

        ms = timed(lib, [mk(s) for s in sets])
        got = sets[0][4].to_host()
        Bh = sets[0][3].to_host()
        err = float(np.max(np.abs(got - A @ Bh)) / max(np.max(np.abs(A @ Bh)), 1e-300))
        print(json.dumps({"case": f"spmm k={k}", "matrix": name, "rows": m, "nnz": nnz, "copies": copies, "us": round(ms * 1e3, 1),
                          "GB/s": round(per / ms / 1e6, 1), "frac_8TBs": round(per / (ms * 1e-3) / HBM, 3), "relerr": err}), flush=True)
        del sets
    per = 2 * nnz * 12 + (m + 1) * 4 + (n + 1) * 4
    copies = max(1, min(16, int(np.ceil(ROTATE / per))))
    sets = []
    for c in range(copies):
        d, i, p = upload(A)
        sets.append((d, i, p, DeviceArray.empty((nnz,), "float64"), DeviceArray.empty((nnz,), "int32"), DeviceArray.empty((n + 1,), "int32")))

    def mkt(s):
        d, i, p, od, oi, op = s
        return lambda: ffi.check(lib.pthip_csr_transpose(7, m, n, nnz, d.ptr, i.ptr, p.ptr, od.ptr, oi.ptr, op.ptr))

    ms = timed(lib, [mkt(s) for s in sets], reps=2)
    want = A.tocsc()
    ok = bool(np.array_equal(sets[0][5].to_host(), want.indptr) and np.array_equal(sets[0][4].to_host(), want.indices)
              and np.array_equal(sets[0][3].to_host(), want.data))
    print(json.dumps({"case": "transpose", "matrix": name, "rows": m, "nnz": nnz, "copies": copies, "us": round(ms * 1e3, 1),
                      "GB/s": round(per / ms / 1e6, 1), "frac_8TBs": round(per / (ms * 1e-3) / HBM, 3), "equals_tocsc": ok}), flush=True)


def bench_car(side, reps):
    import e2e_util as E

    pytensor = E.activate()
    import pytensor.sparse as ps
    import pytensor.tensor as ptt
    from test_gpu_sparse import _car, _grid_adjacency

    W = _grid_adjacency(side, side)
    ins, outs = _car(pytensor, ptt, ps, W, eigen=False)
    vals = [np.random.default_rng(0).standard_normal(W.shape[0]), 1.3, 0.9]
    res = {}
    for mode, label in (("hip", "hip"), (E.reference_mode(), E.reference_mode_name())):
        f = pytensor.function(ins, outs, mode=mode)
        for _ in range(3):
            f(*vals)
        t0 = time.perf_counter()
        for _ in range(reps):
            f(*vals)
        res[label] = reps / (time.perf_counter() - t0)
    print(json.dumps({"case": "CAR logp+grad", "d": side * side, "evals_per_s": {k: round(v, 1) for k, v in res.items()}}), flush=True)


def main():
    quick = "--quick" in sys.argv
    ffi.init(0)
    lib = ffi.lib()
    mats = [("laplacian_1e6", lambda: laplacian(1000)), ("power_law_1e6", lambda: power_law(1_000_000))]
    if not quick:
        mats.insert(1, ("laplacian_1e7", lambda: laplacian(3163)))
    for name, make in mats:
        bench_matrix(lib, name, make())
    bench_car(1000, 20 if quick else 50)


if __name__ == "__main__":
    main()
