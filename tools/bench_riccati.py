"""Per-call time of ``solve_discrete_are`` through ``pytensor.function(mode="hip")`` against the reference's C
linker, one JSON line per configuration (default output: profiles/riccati_bench.jsonl).

Configurations: m in {2, 14, 64, 256, 1024} with n = 1 and n = m/4; a batch of 64 DAREs at m = 10; the
steady-state Kalman log-likelihood plus gradient of the seasonal model (m = 14, 96 observations).  Every
call includes the host upload of the operands and the download of X.  Each side is called until it has
run for about a second (at least 3 calls, fewer only for single calls over 10 s), after one warm-up call;
a warm-up call over 20 s (the reference's QZ at m = 1024) is the measurement itself.

Usage:  python tools/bench_riccati.py [--out PATH] [--max-m M]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def _time(f, args, budget=1.0):
    t0 = time.perf_counter()
    f(*args)  # warm-up (compilation, plan capture)
    first = time.perf_counter() - t0
    if first > 20.0:  # (the reference at m = 1024: one call is the measurement)
        return first, 1
    ts = []
    t_end = time.perf_counter() + budget
    while len(ts) < 3 or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        f(*args)
        ts.append(time.perf_counter() - t0)
        if ts[-1] > 10.0 or len(ts) >= 200:
            break
    return float(np.median(ts)), len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "riccati_bench.jsonl"))
    ap.add_argument("--max-m", type=int, default=1024)
    a = ap.parse_args()
    import make_ref

    make_ref.activate()
    import pytensor
    import pytensor.tensor as pt
    from pytensor.compile.mode import Mode
    from pytensor.tensor.linalg import solve_discrete_are

    import pytensor_amd
    import riccati_cases as rc
    from pytensor_amd import ffi

    pytensor_amd.register()
    cvm = Mode(linker="cvm", optimizer="fast_run")
    buf = ctypes.create_string_buffer(256)
    ffi.check(ffi.lib().pthip_device_name(buf, 256))
    device = buf.value.decode()
    rows = []

    def record(name, ins, outs, vals, **extra):
        f_hip = pytensor.function(ins, outs, mode="hip")
        f_ref = pytensor.function(ins, outs, mode=cvm)
        got, want = f_hip(*vals), f_ref(*vals)
        err = max(float(np.max(np.abs(np.asarray(g) - np.asarray(w))) / max(float(np.max(np.abs(np.asarray(w)))), 1e-300))
                  for g, w in zip(got, want))
        t_hip, n_hip = _time(f_hip, vals)
        t_ref, n_ref = _time(f_ref, vals)
        row = {"case": name, **extra, "hip_ms": round(t_hip * 1e3, 4), "ref_ms": round(t_ref * 1e3, 4),
               "speedup": round(t_ref / t_hip, 2), "max_rel_diff": err, "calls": [n_hip, n_ref],
               "device": device}
        print(json.dumps(row), flush=True)
        rows.append(row)

    for m in (2, 14, 64, 256, 1024):
        if m > a.max_m:
            continue
        for n in sorted({1, max(m // 4, 1)}):
            ins = [pt.dmatrix(nm) for nm in "ABQR"]
            record(f"dare_m{m}_n{n}", ins, [solve_discrete_are(*ins)], list(rc.random_case(m, n, 42 + m + n)), m=m, n=n)
    items = [rc.random_case(10, 2, 9000 + k) for k in range(64)]
    ins = [pt.dtensor3(nm) for nm in "ABQR"]
    record("dare_batch64_m10", ins, [solve_discrete_are(*ins)], [np.stack([it[j] for it in items]) for j in range(4)], m=10, n=2,
           batch=64)
    kins, logp = rc.kalman_graph(pt, solve_discrete_are, pytensor.scan)
    rng = np.random.default_rng(3)
    y = np.cumsum(rng.normal(size=96)) * 0.3 + np.tile(np.sin(np.arange(12)), 8)
    record("kalman_logp_grad_m14", kins, [logp, pytensor.grad(logp, kins[0])], [np.log(np.array([0.5, 0.2, 0.4, 0.3, 1.0])), y],
           m=14, n=1, T=96)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
