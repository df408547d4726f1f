"""Device time of ``Solve(assume_a="banded")`` against ``Solve(assume_a="gen")`` on the same band matrices (frozen
plans with resident operands, launches between HIP events; warm, several repetitions, the median).

usage: python tools/bench_banded.py [--out FILE.md] [--max-gib G] [--reps R] [n,kl,ku,batch ...]

Without shapes: float64, nrhs = 1, n in {256, 1024, 4096} x (kl, ku) in {(1,1), (8,8), (64,64)} at batch 1 and 256, and
n = 8192 at batch 1.  A shape whose matrices alone exceed ``--max-gib`` (default 4) is listed as skipped.  One JSON
line per shape; ``--out`` also writes the table."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytensor_amd import ffi  # noqa: E402
from pytensor_amd.executor import HipExecutable  # noqa: E402
from pytensor_amd.ir import Graph  # noqa: E402


def solve_graph(assume_a, batched):
    g = Graph(name=f"solve_{assume_a}")
    nd = 3 if batched else 2
    a, b, x = g.new_var("float64", (None,) * nd), g.new_var("float64", (None,) * (nd - 1)), g.new_var("float64", (None,) * (nd - 1))
    p = {"assume_a": assume_a, "lower": False, "b_ndim": 1}
    if batched:
        g.add_node("Blockwise", {"core_op": "Solve", "core_params": p, "signature": "(m,m),(m)->(m)"}, [a, b], [x])
    else:
        g.add_node("Solve", p, [a, b], [x])
    g.inputs, g.outputs = [a, b], [x]
    return g


def band_matrices(n, kl, ku, batch, rng):
    """0.01 G inside the band + a diagonal in [1, 2), built diagonal by diagonal; four distinct items, tiled"""
    base = np.zeros((min(batch, 4), n, n))
    for d in range(-kl, ku + 1):
        m = n - abs(d)
        if m <= 0:
            continue
        i = np.arange(m) + max(-d, 0)
        base[:, i, i + d] = 0.01 * rng.standard_normal((len(base), m)) + (1.0 + rng.random((len(base), m)) if d == 0 else 0.0)
    return np.ascontiguousarray(np.resize(base, (batch, n, n)))


def device_ms(plan, reps):
    """median over ``reps`` repetitions of the per-launch device time, each repetition sized to ~50 ms"""
    lib = ffi.lib()
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.pthip_event_create(C.byref(e0)); lib.pthip_event_create(C.byref(e1))
    ms = C.c_float()

    def timed(k):
        lib.pthip_event_record(e0)
        for _ in range(k):
            plan.launch_async()
        lib.pthip_event_record(e1); lib.pthip_event_synchronize(e1)
        lib.pthip_event_elapsed_ms(e0, e1, C.byref(ms))
        return ms.value / k

    timed(1)
    inner = int(min(50, max(1, 50.0 / max(timed(1), 1e-3))))
    return statistics.median(timed(inner) for _ in range(reps))


def measure(assume_a, A, b, reps):
    batched = A.ndim == 3
    exe = HipExecutable(solve_graph(assume_a, batched), resident=[0, 1])
    (x,) = exe(A, b)
    plan = exe.freeze(A, b, fetch_outputs=False)
    try:
        return device_ms(plan, reps), x
    finally:
        plan.close()


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    max_gib = float(argv[argv.index("--max-gib") + 1]) if "--max-gib" in argv else 4.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    shapes = [tuple(int(v) for v in a.split(",")) for a in argv if a[0].isdigit() and "," in a]
    if not shapes:
        shapes = [(n, k, k, batch) for n in (256, 1024, 4096) for k in (1, 8, 64) for batch in (1, 256)] + [(8192, k, k, 1) for k in (1, 8, 64)]
    ffi.init(0)
    rng = np.random.default_rng(0)
    rows = []
    for n, kl, ku, batch in shapes:
        rec = {"n": n, "kl": kl, "ku": ku, "batch": batch, "dtype": "float64", "nrhs": 1}
        if batch * n * n * 8 > max_gib * 2**30:
            rec["skipped"] = f"A alone is {batch * n * n * 8 / 2**30:.1f} GiB"
        else:
            A = band_matrices(n, kl, ku, batch, rng)
            b = rng.standard_normal((batch, n))
            if batch == 1:
                A, b = A[0], b[0]
            rec["banded_ms"], xb = measure("banded", A, b, reps)
            rec["gen_ms"], xg = measure("gen", A, b, reps)
            rec["gen_over_banded"] = round(rec["gen_ms"] / rec["banded_ms"], 2)
            rec["max_abs_diff"] = float(np.abs(xb - xg).max())
            rec["banded_ms"], rec["gen_ms"] = round(rec["banded_ms"], 4), round(rec["gen_ms"], 4)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("# Solve(assume_a=\"banded\") against Solve(assume_a=\"gen\") on the same matrices\n\n")
            f.write(f"`python tools/bench_banded.py` — float64, nrhs = 1, frozen plans with resident operands, device time per call in ms "
                    f"(median of {reps} repetitions after a warm-up).\n\n")
            f.write("| n | (kl, ku) | batch | banded ms | gen ms | gen / banded |\n|---|---|---|---|---|---|\n")
            for r in rows:
                if "skipped" in r:
                    f.write(f"| {r['n']} | ({r['kl']}, {r['ku']}) | {r['batch']} | not run: {r['skipped']} | | |\n")
                else:
                    f.write(f"| {r['n']} | ({r['kl']}, {r['ku']}) | {r['batch']} | {r['banded_ms']} | {r['gen_ms']} | {r['gen_over_banded']} |\n")


if __name__ == "__main__":
    main(sys.argv[1:])
