"""Call time of the two SVD tiers that take one large matrix — ``pthip_svd_rows`` (one workgroup, r <= 2048) and
``pthip_svd_block`` (the whole chip, any r) — through the C ABI on the same device-resident input, next to
``np.linalg.svd`` on the host.

Sweep: one square matrix at n = 256, 512, 1024, 2048, 3072, 4096 and one 1024 x 8192 matrix (Gaussian, seed 0), float64
and float32, ``S`` alone and the economic factors.  Per point: a host clock around one call that ends in a synchronise
(the input is on the device already; the rows tier destroys its input, so it gets a fresh device copy before the clock
starts), after one warm-up call, the two tiers alternately in one process, the median of ``--reps`` (>= 5) calls and
the spread (max - min) / median; where the first call took over a second, the median of two.  ``sweeps`` is the number of
outer sweeps the block tier took (``pthip_svd_block_sweeps``), ``status`` the device error word after the call (0:
converged).  ``host_ms`` is one ``np.linalg.svd`` call (median of three below n = 2048).

``--jsonl`` appends, so a sweep can be split over several runs; ``--rows-max`` leaves the rows tier out above a size.

usage: python tools/bench_svd_block.py [--jsonl FILE] [--sizes 256,512,...] [--dtypes float64,float32] [--wide] [--rows-max R]
       python tools/bench_svd_block.py --summary FILE.jsonl"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [256, 512, 1024, 2048, 3072, 4096]
WIDE = (1024, 8192)
ROWS_MAX = 2048  # pthip_svd_rows's own bound


def _calls(ffi, x, vectors, rows_max=ROWS_MAX):
    """{tier: function that runs one call and returns (seconds, status word)}"""
    from pytensor_amd.device import DeviceArray

    lib = ffi.lib()
    r, c = x.shape
    code = ffi.np_dtype_code(x.dtype)
    X = DeviceArray.from_host(x)
    S = DeviceArray.empty((r,), x.dtype)
    Wt = DeviceArray.empty((r, c), x.dtype) if vectors else None
    Pt = DeviceArray.empty((r, r), x.dtype) if vectors else None
    work = DeviceArray.empty((r, r) if vectors else (1,), x.dtype)
    word = ctypes.c_int(0)

    def finish(t0):
        ffi.check(lib.pthip_check_status(ctypes.byref(word)))  # synchronises
        return time.perf_counter() - t0, word.value

    def block():
        ffi.check(lib.pthip_synchronize())
        t0 = time.perf_counter()
        ffi.check(lib.pthip_svd_block(code, 1, r, c, vectors, r, X.ptr, S.ptr, Wt.ptr if vectors else None, Pt.ptr if vectors else None))
        return finish(t0)

    def rows():
        Xc = X.contiguous_copy()
        ffi.check(lib.pthip_synchronize())
        t0 = time.perf_counter()
        ffi.check(lib.pthip_svd_rows(code, 1, r, c, vectors, Xc.ptr, work.ptr, S.ptr, (Wt if vectors else work).ptr, (Pt if vectors else work).ptr))
        return finish(t0)

    return {"block": block, "rows": rows} if r <= min(rows_max, ROWS_MAX) else {"block": block}


def measure_point(ffi, x, vectors, reps, rows_max=ROWS_MAX):
    calls = _calls(ffi, x, vectors, rows_max)
    first = {k: f()[0] for k, f in calls.items()}  # warm-up: code objects, the pool
    n = {k: (2 if first[k] > 1.0 else reps) for k in calls}
    ts, words = {k: [] for k in calls}, {k: 0 for k in calls}
    sweeps = None
    for i in range(max(n.values())):
        for k, f in calls.items():  # alternately
            if i < n[k]:
                t, w = f()
                ts[k].append(t)
                words[k] |= w
                if k == "block":
                    sweeps = ffi.lib().pthip_svd_block_sweeps()
    out = {}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"ms": round(med * 1e3, 3), "spread": round((max(ts[k]) - min(ts[k])) / med, 3), "calls": n[k], "status": words[k]}
    out["block"]["sweeps"] = sweeps
    return out


def host_ms(x, vectors):
    f = (lambda: np.linalg.svd(x, full_matrices=False)) if vectors else (lambda: np.linalg.svd(x, compute_uv=False))
    ts = []
    for _ in range(3 if min(x.shape) < 2048 else 1):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def measure(args):
    from pytensor_amd import ffi

    ffi.init(0)
    shapes = [(n, n) for n in args.sizes] + ([WIDE] if args.wide else [])
    out = open(args.jsonl, "a") if args.jsonl else None
    for dtype in args.dtypes:
        for r, c in shapes:
            x = np.random.default_rng(0).standard_normal((r, c)).astype(dtype)
            for vectors in (0, 1):
                row = {"dtype": dtype, "r": r, "c": c, "job": "econ" if vectors else "s"}
                row.update(measure_point(ffi, x, vectors, args.reps, args.rows_max))
                if not args.no_host:
                    row["host_ms"] = host_ms(x, vectors)
                print(json.dumps(row), flush=True)
                if out:
                    out.write(json.dumps(row) + "\n")
                    out.flush()


def summary(path):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    lines = ["| dtype | job | r x c | rows ms (spread) | block ms (spread) | sweeps | rows / block | host ms |", "|" + "---|" * 8]
    for w in rows:
        b, ro = w["block"], w.get("rows")
        lines.append(f"| {w['dtype']} | {w['job']} | {w['r']} x {w['c']} | " + (f"{ro['ms']:.1f} ({ro['spread']:.2f})" if ro else "-") +
                     f" | {b['ms']:.1f} ({b['spread']:.2f}) | {b['sweeps']} | " + (f"{ro['ms'] / b['ms']:.2f}" if ro else "-") + f" | {w.get('host_ms', '-')} |")
    # the smallest measured square size from which the block tier is faster, by more than both spreads, at every larger
    # measured size for both dtypes and both jobs
    sizes = sorted({w["r"] for w in rows if w["r"] == w["c"] and "rows" in w})
    faster = lambda w: w["rows"]["ms"] * (1 - w["rows"]["spread"]) > w["block"]["ms"] * (1 + w["block"]["spread"])
    cross = None
    for n in reversed(sizes):
        at = [w for w in rows if w["r"] == n and w["c"] == n and "rows" in w]
        if at and all(faster(w) for w in at):
            cross = n
        else:
            break
    lines.append("")
    lines.append(f"Recorded crossover (square, both dtypes, both jobs, beyond the spread, at every larger measured size): n = {cross}")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jsonl")
    ap.add_argument("--sizes", type=lambda s: [int(v) for v in s.split(",") if v], default=SIZES)
    ap.add_argument("--dtypes", type=lambda s: s.split(","), default=["float64", "float32"])
    ap.add_argument("--wide", action="store_true", help="the 1024 x 8192 matrix as well")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--rows-max", type=int, default=ROWS_MAX, help="time the rows tier only up to this r (a call at r = 2048 takes a minute)")
    ap.add_argument("--summary", metavar="JSONL")
    args = ap.parse_args()
    if args.summary:
        summary(args.summary)
    else:
        measure(args)


if __name__ == "__main__":
    main()
