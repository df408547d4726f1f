"""Call time of ``Blockwise(SVD)``, ``Blockwise(MatrixPinv)`` and ``Blockwise(QR)`` on stacks of small matrices, next
to NumPy's time for the same stack on the host.

Everything goes through ``HipExecutable`` on one ``Blockwise`` node, so this file runs unchanged on a commit from
before the batched tiers (where the stack is walked on the host, one item at a time) and on one after: run it on both
and put the two ``--jsonl`` files side by side with ``--compare``.

Sweep: shapes 3x3, 8x8, 16x16, 32x32, 64x64, 64x16, 100x60; batches 1, 16, 256, 4096 (a stack above 1 GiB is skipped);
float64 and float32; SVD with S alone, economic SVD, pinv; economic QR at 16x16 and 64x16.  Per point: the median
host-clock time of a whole executable call — upload of the stack, the device work, download of the results, ending in
the synchronise of the download — over ``--reps`` calls after ``--warmup`` (fewer where one call takes over a second).  A stack the commit under test raises ``LinAlgError`` for is recorded
with its message instead of a time.
``host_us`` is ``np.linalg.svd`` / ``pinv`` / ``qr`` on the same stack, median of three.

usage: python tools/bench_svd_batched.py [--jsonl FILE] [--tag NAME] [--quick]
       python tools/bench_svd_batched.py --compare PARENT.jsonl CHANGE.jsonl [--out FILE.md]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(3, 3), (8, 8), (16, 16), (32, 32), (64, 64), (64, 16), (100, 60)]
BATCHES = [1, 16, 256, 4096]
QR_SHAPES = [(16, 16), (64, 16)]
MAX_BYTES = 1 << 30


def one_node(op, params, in_specs, out_specs):
    from pytensor_amd.ir import Graph

    g = Graph(name=f"one_{op}")
    ins = [g.new_var(dt, (None,) * nd) for dt, nd in in_specs]
    outs = [g.new_var(dt, (None,) * nd) for dt, nd in out_specs]
    g.add_node(op, params, ins, outs)
    g.inputs, g.outputs = ins, outs
    return g


def executable(mode, dtype):
    from pytensor_amd.executor import HipExecutable

    if mode == "svd_s":
        core, cp, sig, outs = "SVD", {"full_matrices": False, "compute_uv": False}, "(m,n)->(k)", [2]
    elif mode == "svd_econ":
        core, cp, sig, outs = "SVD", {"full_matrices": False, "compute_uv": True}, "(m,n)->(m,k),(k),(k,n)", [3, 2, 3]
    elif mode == "pinv":
        core, cp, sig, outs = "MatrixPinv", {"hermitian": False}, "(m,n)->(n,m)", [3]
    else:
        core, cp, sig, outs = "QR", {"mode": "economic", "pivoting": False}, "(m,n)->(m,k),(k,n)", [3, 3]
    return HipExecutable(one_node("Blockwise", {"core_op": core, "core_params": cp, "signature": sig}, [(dtype, 3)], [(dtype, k) for k in outs]))


HOST = {
    "svd_s": lambda x: np.linalg.svd(x, compute_uv=False),
    "svd_econ": lambda x: np.linalg.svd(x, full_matrices=False),
    "pinv": np.linalg.pinv,
    "qr_econ": np.linalg.qr,
}


def timed(fn, warmup, reps):
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    if first > 1.0:  # (a host loop over thousands of items: one more call is the measurement)
        warmup, reps = 0, 2
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts)


def measure(args):
    from pytensor_amd import ffi

    ffi.init(0)
    rows = []
    rng = np.random.default_rng(0)
    shapes, batches = (SHAPES[:2] + SHAPES[4:5], BATCHES[:3]) if args.quick else (SHAPES, BATCHES)
    for dtype in ("float64", "float32"):
        exes = {mode: executable(mode, dtype) for mode in HOST}
        for m, n in shapes:
            for batch in batches:
                if batch * m * n * np.dtype(dtype).itemsize > MAX_BYTES:
                    continue
                x = rng.standard_normal((batch, m, n)).astype(dtype)
                for mode in HOST:
                    if mode == "qr_econ" and (m, n) not in QR_SHAPES:
                        continue
                    th, _ = timed(lambda: HOST[mode](x), 0, 3)
                    row = {"tag": args.tag, "dtype": dtype, "mode": mode, "m": m, "n": n, "batch": batch}
                    try:
                        t, spread = timed(lambda: exes[mode](x), args.warmup, args.reps)
                        row.update(call_us=round(t * 1e6, 1), spread=round(spread, 2))
                    except np.linalg.LinAlgError as e:  # (a stack the commit under test cannot factor: recorded, not timed)
                        row.update(call_us=None, spread=None, error=str(e))
                    row["host_us"] = round(th * 1e6, 1)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.jsonl:
        os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
        with open(args.jsonl, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def compare(parent, change, out):
    key = lambda r: (r["dtype"], r["mode"], r["m"], r["n"], r["batch"])
    load = lambda p: {key(r): r for r in map(json.loads, open(p)) if "mode" in r}
    a, b = load(parent), load(change)
    lines = ["| dtype | mode | m x n | batch | parent_us | change_us | parent / change | host_us (NumPy) | change vs host |", "|" + "---|" * 9]
    for k in a:
        if k not in b:
            continue
        pa, ch = a[k]["call_us"], b[k]["call_us"]
        host = statistics.median([a[k]["host_us"], b[k]["host_us"]])
        if pa is None or ch is None:
            show = lambda r: "raised: " + r.get("error", "") if r["call_us"] is None else f"{r['call_us']:.1f}"
            lines.append(f"| {k[0]} | {k[1]} | {k[2]} x {k[3]} | {k[4]} | {show(a[k])} | {show(b[k])} | - | {host:.1f} | {'-' if ch is None else f'{host / ch:.2f}'} |")
            continue
        lines.append(f"| {k[0]} | {k[1]} | {k[2]} x {k[3]} | {k[4]} | {pa:.1f} | {ch:.1f} | {pa / ch:.1f} | {host:.1f} | {host / ch:.2f} |")
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jsonl")
    ap.add_argument("--tag", default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="3x3, 8x8 and 64x64 at batch 1, 16, 256")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "CHANGE"))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare, args.out)
    else:
        measure(args)


if __name__ == "__main__":
    main()
